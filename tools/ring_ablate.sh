#!/bin/bash
# Timing-only ablations of the ring kernel (results are meaningless): 1501 = DMA pieces fetch nothing, 1502 = no matrix phase,
# 1504 = no epilogue, and their sums (1503, 1505, 1506, 1507): 1500 + mask, EXP_RING_ABLATE in csrc/experiments.h.
export CONV_BENCH_STORE16=1 CONV_BENCH_ROTATE=3
for e in 0 1501 1502 1504 1503 1506 1507; do
  export PWS_EXPERIMENT=$e
  python tools/conv_bench.py CONVT_K4S2 64 128 128 256 64 bf16
  python tools/conv_bench.py CONV_K3S1 64 128 128 128 128 bf16
  python tools/conv_bench.py CONV_K3S1 64 256 256 64 64 bf16
done 2>&1 | grep -v amdgpu.ids
