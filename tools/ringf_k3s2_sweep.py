#!/usr/bin/env python3
"""The headline's stride-2 launches of conv_ringf_kernel under PWS_OPT_EXPERIMENT ids, in one process:
python tools/ringf_k3s2_sweep.py 2216,2217,2218,2220,2222,2221,2223,0,2232 (ids: ringf_plan, csrc/conv_ring_f32.hip:
2200 + 16 v + mask; v = 1 full workgroups, the parent commit's launches, with the ablation masks; 0 the product; 2232 half workgroups
also for 16 x 32 tiles)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("CONV_BENCH_ROTATE", "3")
import conv_bench as cb  # noqa: E402

SHAPES = [("down1", 8, 256, 256, 64, 64), ("down2", 8, 128, 128, 64, 128), ("down3", 8, 64, 64, 128, 256),
          ("dbot2", 8, 128, 128, 128, 128), ("dbot3", 16, 64, 64, 256, 256)]

if __name__ == "__main__":
    exps = [int(e) for e in sys.argv[1].split(",")]
    for name, n, h, w, ci, co in SHAPES:
        for e in exps:
            os.environ["PWS_EXPERIMENT"] = str(e)
            print(name, end=" ", flush=True)
            cb.bench("CONV_K3S2", n, h, w, ci, co, False)
