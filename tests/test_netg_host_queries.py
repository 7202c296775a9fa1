"""The generator's host-only queries (packed sizes, gradient-slab layout, arena sizes, the nparts plan of the backward) return
exactly what the commit named in tests/golden/netg_host_queries.json returned: a Python host sizes its arena and cuts its
all-reduce from these integers, and the forward and the backward must agree on every address derived from them.

`python tests/test_netg_host_queries.py --record <commit>` rewrites the fixture from the library that is built in the tree."""
import ctypes
import json
import os
import sys

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "netg_host_queries.json")
SHAPES = [(31, 64), (31, 16), (3, 32)]
BATCHES = [1, 2, 8, 64]
NPARTS = [1, 2, 3, 4, 5, 6, 7, 8, 46]
NL = 46


def _lib():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pwstablenet_amd import hipabi
    return hipabi.lib()


def _plan(L, input_nc, ngf, nparts):
    out = (ctypes.c_ubyte * NL)(*([0xEE] * NL))
    return L.pws_netg_backward_plan(input_nc, ngf, nparts, out), list(out)


def _layout(L, input_nc, ngf):
    first, count = (ctypes.c_size_t * NL)(), (ctypes.c_size_t * NL)()
    return L.pws_netg_grad_layout(input_nc, ngf, first, count), list(first), list(count)


def collect(L):
    cases = {}
    for input_nc, ngf in SHAPES:
        c = {"packed_floats": L.pws_netg_packed_floats(input_nc, ngf),
             "packed_dgrad_floats": L.pws_netg_packed_dgrad_floats(input_nc, ngf),
             "grad_floats": L.pws_netg_grad_floats(input_nc, ngf),
             "bn_floats": L.pws_netg_bn_floats(input_nc, ngf),
             "grad_layout": _layout(L, input_nc, ngf),
             "backward_plan": {str(p): _plan(L, input_nc, ngf, p) for p in NPARTS},
             "workspace_bytes": {str(n): [L.pws_netg_workspace_bytes(n, input_nc, ngf, t) for t in (0, 1)] for n in BATCHES},
             "train_workspace_bytes": {str(n): L.pws_netg_train_workspace_bytes(n, input_nc, ngf) for n in BATCHES},
             "train_workspace_bytes_bn": {str(n): L.pws_netg_train_workspace_bytes_bn(n, input_nc, ngf) for n in BATCHES}}
        cases["%d,%d" % (input_nc, ngf)] = c
    null_z = ctypes.POINTER(ctypes.c_size_t)()
    null_b = ctypes.POINTER(ctypes.c_ubyte)()
    some = (ctypes.c_size_t * NL)()
    bad = {"ngf17": [L.pws_netg_packed_floats(31, 17), L.pws_netg_packed_dgrad_floats(31, 17), L.pws_netg_grad_floats(31, 17),
                     L.pws_netg_bn_floats(31, 17), L.pws_netg_workspace_bytes(2, 31, 17, 0), L.pws_netg_workspace_bytes(2, 31, 17, 1),
                     L.pws_netg_train_workspace_bytes(2, 31, 17), L.pws_netg_train_workspace_bytes_bn(2, 31, 17),
                     _layout(L, 31, 17)[0], _plan(L, 31, 17, 4)],
           "input_nc0": [L.pws_netg_packed_floats(0, 64), L.pws_netg_grad_floats(0, 64), L.pws_netg_workspace_bytes(2, 0, 64, 1),
                         L.pws_netg_train_workspace_bytes(2, 0, 64), _layout(L, 0, 64)[0], _plan(L, 0, 64, 4)],
           "n0": [L.pws_netg_workspace_bytes(0, 31, 64, 0), L.pws_netg_workspace_bytes(0, 31, 64, 1),
                  L.pws_netg_train_workspace_bytes(0, 31, 64), L.pws_netg_train_workspace_bytes_bn(0, 31, 64)],
           "nparts0": _plan(L, 31, 64, 0),
           "nparts256": _plan(L, 31, 64, 256),
           "plan_null": L.pws_netg_backward_plan(31, 64, 4, null_b),
           "layout_null": [L.pws_netg_grad_layout(31, 64, null_z, some), L.pws_netg_grad_layout(31, 64, some, null_z)]}
    return json.loads(json.dumps({"cases": cases, "bad_arguments": bad}))   # (tuples -> lists, as the fixture reads back)


def test_host_queries_equal_the_recorded_ones():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = collect(_lib())
    assert sorted(got["cases"]) == sorted(want["cases"])
    for shape, c in want["cases"].items():
        for query, value in c.items():
            assert got["cases"][shape][query] == value, (shape, query)
    assert got["bad_arguments"] == want["bad_arguments"]
    # the bad-argument returns are errors, not sizes: 0 for the size queries, PWS_EINVAL (non-zero) for the two that return a status,
    # and a refused plan leaves the caller's buffer alone
    bad = want["bad_arguments"]
    assert all(v == 0 for v in bad["ngf17"][:8] + bad["n0"]) and bad["ngf17"][8] != 0
    for rc, out in (bad["ngf17"][9], bad["nparts0"], bad["nparts256"]):
        assert rc != 0 and out == [0xEE] * NL
    assert bad["plan_null"] != 0 and all(bad["layout_null"])


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    doc = {"_recorded_from": "commit %s: every value below is an integer that commit's library returned" % sys.argv[2]}
    doc.update(collect(_lib()))
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE)
