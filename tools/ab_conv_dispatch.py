"""A/B of the conv dispatch between two builds of the library: same launches in the same order with the same work, same bits.

    python tools/ab_conv_dispatch.py --parent-lib /path/to/parent/libpwstable_hip.so [--out profiles/conv_dispatch_ab.json]
    python tools/ab_conv_dispatch.py --parent-lib ... --host-time [--out profiles/conv_dispatch_host_time.json]

Runs every case below once with the library of this tree and once with the other one (PWS_LIB_PATH), each side in a child process of
its own under `timeout`, stops at the first non-zero status, and compares per case
  * the ordered (kernel name, tag, flops, bytes) list pws_prof_collect reports, and
  * the SHA-256 of the fields (and residuals), and of the gradient slab for the training cases (PWS_NETG_DETERMINISTIC).
Cases: the eager inference forward at batch 8, ngf 64, in fp32 and in bf16 math + storage; a training forward + backward at batch 2,
ngf 16, fp32 (where the bf16 kernels' fall-through rungs run); a training forward + backward at batch 8, ngf 64, bf16.

--mode trace (a child by itself, the program behind `rocprofv3 --kernel-trace --output-format csv -d DIR --`): the two inference
forwards once each, nothing else traced in that run; --trace-compare PARENT_DIR CHANGE_DIR then reads both kernel traces, writes the
ordered (kernel name with template arguments, grid, workgroup, LDS) lists to profiles/conv_dispatch_trace_{parent,change}.json and
compares them.

--host-time: the host side of an eager pws_netg_forward_opts call (issue until return, batch 8, median of 200 calls after a warm-up),
three runs per side, alternating; the change must not exceed the parent's slowest run by more than the parent's spread."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name -> (n, ngf, math, training)
CASES = {"inference fp32 n8 ngf64": (8, 64, "fp32", False), "inference bf16 n8 ngf64": (8, 64, "bf16", False),
         "training fp32 n2 ngf16": (2, 16, "fp32", True), "training bf16 n8 ngf64": (8, 64, "bf16", True)}
NEW_ENTRIES = ("pws_conv2d_fwd_plan", "pws_conv2d_bwd_data_plan", "pws_netg_forward_plan")   # not in a parent built before them


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().float().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def load():
    from pwstablenet_amd import hipabi as A
    if os.environ.get("PWS_LIB_PATH"):
        for name in NEW_ENTRIES:
            A.SIGNATURES.pop(name, None)
    return A


def make_net(A, ngf, math):
    import torch
    from pwstablenet_amd import synth
    from pwstablenet_amd.lib.networks_cascading import define_G
    net = define_G(31, 2, ngf, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=ngf)})
    net = net.cuda().module
    net.set_math(math)
    net.deterministic = True
    return net


def run_cases(out_path):
    import torch
    A = load()
    from pwstablenet_amd import synth
    L = A.lib()
    res = {}
    for name, (n, ngf, math, training) in CASES.items():
        net = make_net(A, ngf, math)
        x = torch.from_numpy(synth.make_window(n, 31, 256, seed=4)).cuda()
        net.packed_weights(train=training)
        torch.cuda.synchronize()
        L.pws_prof_enable(1)
        if not training:
            with torch.no_grad():
                grid = net._run(x, False)
            torch.cuda.synchronize()
            row = {"fields_sha256": sha(grid)}
        else:
            sv = {}
            grids, resid = net._run(x, True, train_ctx=sv)
            gen = torch.Generator().manual_seed(7)
            up = [torch.randn(n, 256, 256, 2, generator=gen).cuda() for _ in range(6)]
            g_grids = (ctypes.c_void_p * 3)(*[up[k].data_ptr() for k in range(3)])
            g_resid = (ctypes.c_void_p * 3)(*[up[3 + k].data_ptr() for k in range(3)])
            dpacked = torch.empty(L.pws_netg_grad_floats(31, ngf), device="cuda", dtype=torch.float32)
            opts = net._opts(sv["math"], sv["store"])
            mask = (ctypes.c_ubyte * 46)()
            A.check(L.pws_netg_backward_lists(A.ptr(sv["packed"]), A.ptr(net.packed_dgrad_weights()), A.ptr(sv["x"]), n, 31, ngf, sv["ac"],
                                              ctypes.c_void_p(sv["ws_ptr"]), sv["ws_bytes"], A.ptr(sv["resid"]), A.ptr(sv["thetas"]), g_grids,
                                              g_resid, A.ptr(dpacked), 0, 1, mask, ctypes.byref(opts), A.current_stream()), "pws_netg_backward_lists")
            torch.cuda.synchronize()
            row = {"fields_sha256": sha(*grids, *resid), "slab_sha256": sha(dpacked)}
        row["launches"] = [[k, tag, flops, nbytes] for k, tag, flops, nbytes, _ in A.prof_collect(16384)]
        L.pws_prof_enable(0)
        res[name] = row
    with open(out_path, "w") as f:
        json.dump(res, f)


def run_host_time(out_path):
    import torch
    A = load()
    L, st = A.lib(), A.current_stream()
    res = {}
    for math in ("fp32", "bf16"):
        n, ngf = 8, 64
        net = make_net(A, ngf, math)
        packed = net.packed_weights()
        x = torch.zeros((n, 31, 256, 256), device="cuda")
        ws_bytes = L.pws_netg_workspace_bytes(n, 31, ngf, 0)
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
        ws_ptr = (ws.data_ptr() + 255) // 256 * 256
        grids = torch.empty((n, 256, 256, 2), device="cuda")
        opts = net._opts()
        times = []
        for i in range(220):
            t0 = time.perf_counter()
            rc = L.pws_netg_forward_opts(A.ptr(packed), A.ptr(x), n, 31, ngf, 0, 0, ctypes.c_void_p(ws_ptr), ws_bytes, A.ptr(grids), None, None,
                                         ctypes.byref(opts), st)
            t1 = time.perf_counter()
            A.check(rc, "pws_netg_forward_opts")
            torch.cuda.synchronize()   # (outside the timed span: the queue never backs up into the next call's issue)
            if i >= 20:
                times.append((t1 - t0) * 1e6)
        times.sort()
        res[math] = {"median_us": times[len(times) // 2], "min_us": times[0], "p90_us": times[int(len(times) * 0.9)]}
    with open(out_path, "w") as f:
        json.dump(res, f)


def run_trace_target():
    import torch
    A = load()
    from pwstablenet_amd import synth
    for math in ("fp32", "bf16"):
        net = make_net(A, 64, math)
        x = torch.from_numpy(synth.make_window(8, 31, 256, seed=4)).cuda()
        with torch.no_grad():
            net._run(x, False)
        torch.cuda.synchronize()


def trace_list(d):
    """[kernel name, grid, workgroup, LDS bytes] per dispatch of the library's kernels, in dispatch order, from rocprofv3's kernel_trace.csv under d."""
    import csv
    import glob
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        sys.exit("ab_conv_dispatch: expected one kernel_trace.csv under %s, found %d" % (d, len(files)))
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    return [[r["Kernel_Name"], [int(r["Grid_Size_" + a]) for a in "XYZ"], [int(r["Workgroup_Size_" + a]) for a in "XYZ"], int(r["LDS_Block_Size"])]
            for r in rows if "pws::" in r["Kernel_Name"]]


def trace_compare(parent_dir, change_dir):
    lists = {"parent": trace_list(parent_dir), "change": trace_list(change_dir)}
    for side, rows in lists.items():
        with open(os.path.join(ROOT, "profiles", "conv_dispatch_trace_%s.json" % side), "w") as f:
            json.dump({"what": "rocprofv3 --kernel-trace of the eager inference forwards at batch 8, ngf 64, fp32 then bf16: [kernel, grid, workgroup, "
                               "LDS bytes] per dispatch of the library, in dispatch order", "dispatches": rows}, f, indent=0)
            f.write("\n")
    same = lists["parent"] == lists["change"]
    print("kernel traces: %d / %d dispatches, %s" % (len(lists["parent"]), len(lists["change"]), "identical" if same else "DIFFERENT"))
    if not same:
        for i, (u, v) in enumerate(zip(lists["parent"], lists["change"])):
            if u != v:
                print(i, u, v)
                break
    sys.exit(0 if same and lists["parent"] else 1)


def child(mode, lib, tmp, timeout):
    env = dict(os.environ)
    env.pop("PWS_LIB_PATH", None)
    if lib:
        env["PWS_LIB_PATH"] = lib
    rc = subprocess.call(["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), "--child", tmp, "--mode", mode], env=env)
    if rc != 0:
        sys.exit("ab_conv_dispatch: the %s side ended with status %d: stopping" % ("parent" if lib else "change", rc))
    with open(tmp) as f:
        out = json.load(f)
    os.remove(tmp)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--host-time", action="store_true")
    ap.add_argument("--child")
    ap.add_argument("--mode", default="cases")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--trace-compare", nargs=2, metavar=("PARENT_DIR", "CHANGE_DIR"))
    a = ap.parse_args()
    if a.trace_compare:
        return trace_compare(*a.trace_compare)
    if a.mode == "trace":
        return run_trace_target()
    if a.child:
        return run_host_time(a.child) if a.mode == "host" else run_cases(a.child)
    from pwstablenet_amd import build
    parent = os.path.abspath(a.parent_lib)
    if a.host_time:
        out_path = a.out or os.path.join(ROOT, "profiles", "conv_dispatch_host_time.json")
        runs = {"parent": [], "change": []}
        for i in range(3):
            for side, lib in (("parent", parent), ("change", None)):
                runs[side].append(child("host", lib, out_path + ".tmp", a.timeout))
        out = {"_meta": {"source_hash": build.source_hash(), "what": "host time of one eager pws_netg_forward_opts call, batch 8, ngf 64: median of 200 "
                         "calls per run, three runs per side, alternating"}, "runs": runs, "verdict": {}}
        ok = True
        for math in ("fp32", "bf16"):
            p = [r[math]["median_us"] for r in runs["parent"]]
            c = [r[math]["median_us"] for r in runs["change"]]
            limit = max(p) + (max(p) - min(p))
            out["verdict"][math] = {"parent_median_us": p, "change_median_us": c, "limit_us": limit, "within": max(c) <= limit}
            ok = ok and max(c) <= limit
            print(math, json.dumps(out["verdict"][math]))
    else:
        out_path = a.out or os.path.join(ROOT, "profiles", "conv_dispatch_ab.json")
        sides = {"parent": child("cases", parent, out_path + ".tmp", a.timeout), "change": child("cases", None, out_path + ".tmp", a.timeout)}
        out = {"_meta": {"source_hash": build.source_hash(), "what": "conv dispatch, this tree against --parent-lib: ordered (kernel, tag, flops, bytes) "
                         "per launch and output bits; PWS_NETG_DETERMINISTIC"}, "cases": {}}
        ok = True
        for name, c in sides["change"].items():
            p = sides["parent"][name]
            row = {"launches": len(c["launches"]), "launches_identical": c["launches"] == p["launches"]}
            for key in ("fields_sha256", "slab_sha256"):
                if key in c:
                    row[key], row["parent_" + key] = c[key], p[key]
            row["bits_identical"] = all(c[k] == p[k] for k in ("fields_sha256", "slab_sha256") if k in c)
            if not row["launches_identical"]:
                row["differs_at"] = [[i, u, v] for i, (u, v) in enumerate(zip(c["launches"], p["launches"])) if u != v][:8]
            ok = ok and row["launches_identical"] and row["bits_identical"]
            out["cases"][name] = row
            print(name, json.dumps({k: v for k, v in row.items() if "sha256" not in k}))
    out["all_identical" if not a.host_time else "all_within"] = ok
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
