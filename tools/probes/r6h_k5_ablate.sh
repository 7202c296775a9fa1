cd ${GRAFT_REPO_ROOT:-.}
export CONV_BENCH_STORE16=1 CONV_BENCH_ROTATE=3
for e in 0 1501 1502 1504 1503 1505 1506 1507; do PWS_EXPERIMENT=$e python tools/conv_bench.py CONV_K5S1 64 256 256 32 64 bf16 2>&1 | grep -v amdgpu; done
