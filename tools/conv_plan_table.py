"""Which kernel runs each conv layer of a generator forward: layer -> kernel / variant / grid / K split, read off the dispatch ladder
(csrc/conv_dispatch.hip) through pws_netg_forward_plan.  Needs the built library, no GPU.

    python tools/conv_plan_table.py --n 8 --ngf 64 --math bf16 --store bf16 [--train] [--cus 256] [--experiment ID]
    python tools/conv_plan_table.py --check      # the pinned configurations against tests/golden/conv_dispatch.json
    python tools/conv_plan_table.py --write      # regenerate that file (a threshold moved: show the diff in the pull request)

A row's `follow` says what is issued behind the launch: 1 = the split-K reduce, 2 = the sign-bit pass, 3 = both."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_dispatch.json")
GOLDEN_CUS = 256
# name -> (n, ngf, math, store, is_training)
PINNED = {
    "inference fp32 n8 ngf64": (8, 64, "fp32", "fp32", 0),
    "inference bf16 n8 ngf64": (8, 64, "bf16", "bf16", 0),
    "training fp32 n2 ngf16": (2, 16, "fp32", "fp32", 1),
    "training bf16 n8 ngf64": (8, 64, "bf16", "bf16", 1),
    "inference fp32 n16 ngf64": (16, 64, "fp32", "fp32", 0),
}


def forward_plan(n, ngf, math, store, is_training, cus=GOLDEN_CUS, input_nc=31):
    """The conv launches of one forward in issue order, as dicts (hipabi.PwsConvChoice.as_dict)."""
    from pwstablenet_amd import hipabi as A
    L = A.lib()
    opts = A.PwsNetgOpts(A.MATH_BF16 if math == "bf16" else A.MATH_FP32, A.STORE_BF16 if store == "bf16" else A.STORE_FP32, 1, 0, 0)
    buf = (A.PwsConvChoice * 256)()
    cnt = L.pws_netg_forward_plan(n, input_nc, ngf, is_training, ctypes.byref(opts), cus, buf, 256)
    if cnt < 0 or cnt > 256:
        raise RuntimeError("pws_netg_forward_plan: %d: %s" % (cnt, L.pws_last_error().decode()))
    return [buf[i].as_dict(L) for i in range(cnt)]


def pinned_table():
    return {"_meta": {"compute_units": GOLDEN_CUS, "input_nc": 31, "what": "pws_netg_forward_plan per configuration; tools/conv_plan_table.py --write"},
            "configs": {name: forward_plan(*cfg) for name, cfg in PINNED.items()}}


def show(rows):
    print("%-5s %-24s %-18s %-16s %7s %6s %6s %s" % ("layer", "kernel", "variant", "grid", "threads", "LDS", "ksplit", "follow"))
    for r in rows:
        print("%-5d %-24s %-18s %-16s %7d %6d %6d %d" % (r["tag"], r["kernel"], ",".join(map(str, r["variant"])), "x".join(map(str, r["grid"])),
                                                        r["threads"], r["lds_bytes"], r["ksplit"], r["follow"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--ngf", type=int, default=64)
    ap.add_argument("--math", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--store", choices=("fp32", "bf16"), default=None)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--cus", type=int, default=GOLDEN_CUS)
    ap.add_argument("--experiment", type=int, default=0)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.write or a.check:
        table = pinned_table()
        if a.write:
            with open(GOLDEN, "w") as f:   # one launch per line: a moved threshold shows as the lines it moves
                f.write('{"_meta": %s,\n "configs": {\n' % json.dumps(table["_meta"]))
                f.write(",\n".join('  "%s": [\n%s\n  ]' % (name, ",\n".join("   " + json.dumps(r) for r in rows)) for name, rows in table["configs"].items()))
                f.write("\n }}\n")
            return print("wrote", GOLDEN)
        with open(GOLDEN) as f:
            same = json.load(f) == table
        print("identical" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    from pwstablenet_amd import hipabi as A
    with A.experiment(a.experiment):
        show(forward_plan(a.n, a.ngf, a.math, a.store or a.math, int(a.train), a.cus))


if __name__ == "__main__":
    main()
