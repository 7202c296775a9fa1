"""A/B of the generator's backward between two builds of the library: same gradient bits, same launches in the same order.

    python tools/ab_netg_backward.py --parent-lib /path/to/parent/libpwstable_hip.so [--out profiles/netg_backward_ab.json]

runs every case below once with the library of this tree and once with the other one (PWS_LIB_PATH), each in a child process of
its own under `timeout`, stops at the first non-zero status, and compares per case
  * the SHA-256 of the gradient slab (use_BN: of the unpacked parameter gradients, which hold the slab and dbn), and
  * the ordered (kernel name, tag) list pws_prof_collect reports for the backward.
All cases run with PWS_NETG_DETERMINISTIC, so equal launches give equal bits.  Cases: fp32 and bf16 at batch 8 (ngf 64) and batch 2
(ngf 16) with all six upstream gradients (nparts 1 and 4), with grids[2] alone and with the three residuals alone (ops without a
gradient are skipped and deferred weight-gradient pairs stay unpaired), and the use_BN path once."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UPSTREAM = {"all": ([0, 1, 2], [0, 1, 2]), "grids2": ([2], []), "resid": ([], [0, 1, 2])}
CASES = [(math, n, ngf, which, nparts) for math in ("fp32", "bf16") for n, ngf in ((8, 64), (2, 16))
         for which, nparts in (("all", 1), ("all", 4), ("grids2", 1), ("resid", 1))]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def launches(A):
    return [[name, tag] for name, tag, _, _, _ in A.prof_collect(8192)]


def run_cases(out_path):
    import torch
    from pwstablenet_amd import hipabi as A
    from pwstablenet_amd import synth
    from pwstablenet_amd.lib.networks_cascading import UnetGenerator, define_G
    L = A.lib()
    res = {}
    nets = {}
    for math, n, ngf, which, nparts in CASES:
        if (math, ngf) not in nets:
            net = define_G(31, 2, ngf, "normal", 0.02)
            net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=ngf)})
            nets[(math, ngf)] = net.cuda().module
            nets[(math, ngf)].set_math(math)
            nets[(math, ngf)].deterministic = True
        net = nets[(math, ngf)]
        x = torch.from_numpy(synth.make_window(n, 31, 256, seed=4)).cuda()
        gen = torch.Generator().manual_seed(7)
        up = [torch.randn(n, 256, 256, 2, generator=gen).cuda() for _ in range(6)]
        sv = {}
        net._run(x, True, train_ctx=sv)
        gi, ri = UPSTREAM[which]
        g_grids = (ctypes.c_void_p * 3)(*[up[k].data_ptr() if k in gi else None for k in range(3)])
        g_resid = (ctypes.c_void_p * 3)(*[up[3 + k].data_ptr() if k in ri else None for k in range(3)])
        dpacked = torch.empty(L.pws_netg_grad_floats(31, ngf), device="cuda", dtype=torch.float32)
        opts = net._opts(sv["math"], sv["store"])
        masks = []
        torch.cuda.synchronize()
        L.pws_prof_enable(1)
        for part in range(nparts):
            mask = (ctypes.c_ubyte * 46)()
            A.check(L.pws_netg_backward_lists(A.ptr(sv["packed"]), A.ptr(net.packed_dgrad_weights()), A.ptr(sv["x"]), n, 31, ngf, sv["ac"],
                                              ctypes.c_void_p(sv["ws_ptr"]), sv["ws_bytes"], A.ptr(sv["resid"]), A.ptr(sv["thetas"]), g_grids,
                                              g_resid, A.ptr(dpacked), part, nparts, mask, ctypes.byref(opts), A.current_stream()),
                    "pws_netg_backward_lists")
            masks.append(list(mask))
        torch.cuda.synchronize()
        rec = launches(A)
        L.pws_prof_enable(0)
        res["%s n%d ngf%d %s nparts%d" % (math, n, ngf, which, nparts)] = {"slab_sha256": sha(dpacked), "final_masks": masks, "launches": rec}
    # use_BN once: through autograd (the BatchNorm forward keeps what its backward needs there)
    torch.manual_seed(0)
    bn = UnetGenerator(31, 2, 16, use_BN=True).cuda().train()
    bn.deterministic = True
    x = torch.from_numpy(synth.make_window(2, 31, 256, seed=4)).cuda()
    gen = torch.Generator().manual_seed(7)
    up = [torch.randn(2, 256, 256, 2, generator=gen).cuda() for _ in range(6)]
    grids, resid = bn(x)
    torch.cuda.synchronize()
    L.pws_prof_enable(1)
    sum((o * u).sum() for o, u in zip(list(grids) + list(resid), up)).backward()
    torch.cuda.synchronize()
    rec = [r for r in launches(A)]
    L.pws_prof_enable(0)
    h = hashlib.sha256()
    for p in bn.parameters():
        h.update(p.grad.detach().cpu().contiguous().numpy().tobytes())
    res["use_BN fp32 n2 ngf16 all"] = {"grads_sha256": h.hexdigest(), "launches": rec}
    with open(out_path, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "netg_backward_ab.json"))
    ap.add_argument("--child")
    ap.add_argument("--timeout", type=int, default=400)
    a = ap.parse_args()
    if a.child:
        return run_cases(a.child)
    from pwstablenet_amd import build
    sides = {}
    for side, lib in (("parent", os.path.abspath(a.parent_lib)), ("change", None)):
        tmp = a.out + "." + side + ".tmp"
        env = dict(os.environ)
        env.pop("PWS_LIB_PATH", None)
        if lib:
            env["PWS_LIB_PATH"] = lib
        rc = subprocess.call(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", tmp], env=env)
        if rc != 0:
            sys.exit("ab_netg_backward: the %s side ended with status %d: stopping" % (side, rc))
        with open(tmp) as f:
            sides[side] = json.load(f)
        os.remove(tmp)
    out = {"_meta": {"source_hash": build.source_hash(), "what": "backward of the generator, this tree against --parent-lib; PWS_NETG_DETERMINISTIC"},
           "cases": {}}
    ok = True
    for name, c in sides["change"].items():
        p = sides["parent"][name]
        key = "slab_sha256" if "slab_sha256" in c else "grads_sha256"
        same_order = c["launches"] == p["launches"]
        same_set = sorted(map(tuple, c["launches"])) == sorted(map(tuple, p["launches"]))
        row = {key: c[key], "parent_" + key: p[key], "bits_identical": c[key] == p[key], "launches": len(c["launches"]),
               "launch_order_identical": same_order, "launch_multiset_identical": same_set,
               "final_masks_identical": c.get("final_masks") == p.get("final_masks")}
        if not same_order:   # the flushed unpaired weight gradients may change places among themselves: show where
            row["order_differs_at"] = [[i, u, v] for i, (u, v) in enumerate(zip(c["launches"], p["launches"])) if u != v]
        ok = ok and row["bits_identical"] and same_set and row["final_masks_identical"]
        out["cases"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if "sha256" not in k}))
    out["all_identical"] = ok
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
