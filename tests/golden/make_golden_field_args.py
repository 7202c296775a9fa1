#!/usr/bin/env python3
"""Writes tests/golden/field_args_errors.json: what the six field-domain entries (pws_field_zoom, pws_field_compose, pws_field_compose_rows,
pws_field_rigid, pws_field_wobble, pws_field_reach) and their four Python wrappers answer to bad arguments, as the commit BEFORE
csrc/field_lattice.h answered -- return code, message and precedence are what tests/test_field_args_cpu.py and tests/test_hip_field_args.py
hold the shared checks to.

    python tests/golden/make_golden_field_args.py /path/to/a/built/checkout/of/that/commit                       # no device: "c", "python" (CPU)
    python tests/golden/make_golden_field_args.py /path/to/... --device --out somewhere.json                      # on a GPU: "python" (device)

Section "c".  Pointers are made-up integers: every case is rejected by a check or has n == 0, so none is used, and the run must be on a
machine WITHOUT a device (the generator refuses otherwise: a case that slipped through would launch on them).  Every PWS_REQUIRE of every
entry is reached (REQUIRES below lists them by a phrase of their message; the generator refuses to write a fixture that leaves one out),
pairs of faults pin the order, and cases that END at "too large" show what the earlier checks let pass: out == field for pws_field_rigid, an
out that starts where the fields end.
Section "python".  The errors of zoom_fields, compose_fields, rigid_fields and wobble_fields: those raised before a tensor is looked at and
those about host tensors are recorded without a device; the others (--device) with 1 x 2 x 2 x 2 fields on the device.  Every case is a
rejection: no kernel is launched.  tests/field_args.py describes the rows."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

F, O, A, B, C, R = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000   # 256 MB apart
FAR = 1 << 41
BIGW, IMAX = 128 * 65536, 2 ** 31 - 1   # 65536 chunks of columns; with 2 row groups a frame, 2^31 blocks and more
BIG = {"fh": 2, "fw": BIGW}             # (128 MB of field: "too large" by its chunks, past every other check)
NAN = float("nan")

ORDER = {
    "pws_field_zoom": "field n fh fw coef out h0 w0 ac margin unc stream",
    "pws_field_compose": "field n fh fw d out h0 w0 ac margin unc stream",
    "pws_field_compose_rows": "field n fh fw d rates r out h0 w0 ac margin unc stream",
    "pws_field_rigid": "field n fh fw m rigidity h0 w0 out s0 s1 stream",
    "pws_field_wobble": "field n fh fw m sigma h0 w0 out s0 s1 stream",
    "pws_field_reach": "field n fh fw table levels rates r i0 i1 j0 j1 h0 w0 ac margin counts stream",
}
BASE = {"field": F, "n": 1, "fh": 4, "fw": 4, "coef": A, "d": A, "m": A, "table": A, "out": O, "h0": 8, "w0": 8, "ac": 0, "margin": 0, "unc": B,
        "s0": B, "s1": C, "counts": B, "rates": R, "r": 0.5, "rigidity": 0.5, "sigma": 1.0, "levels": 4, "i0": 0, "i1": 3, "j0": 0, "j1": 3,
        "stream": None}
# entry -> the phrases of its PWS_REQUIRE messages, in the order of the checks
REQUIRES = {
    "pws_field_zoom": ["bad shape", "at least 2 x 2 nodes", "bad frame size", "NULL pointer", "8-byte aligned", "must not overlap field",
                       "field or batch too large"],
    "pws_field_compose": ["bad shape", "at least 2 x 2 nodes", "at least 2 x 2 pixels", "bad margin", "NULL pointer", "8-byte aligned",
                          "must not overlap field", "field or batch too large"],
    "pws_field_compose_rows": ["r must lie", "rates must be non-NULL", "bad shape", "at least 2 x 2 nodes", "at least 2 x 2 pixels", "bad margin",
                               "NULL pointer", "8-byte aligned", "must not overlap field", "field or batch too large"],
    "pws_field_rigid": ["bad shape", "at least 2 x 2 nodes", "bad frame size", "rigidity must lie", "NULL pointer", "8-byte aligned",
                        "out must be field itself or must not overlap it", "field or batch too large"],
    "pws_field_wobble": ["bad shape", "at least 2 x 2 nodes", "bad frame size", "sigma must lie", "NULL pointer", "8-byte aligned",
                         "it cannot run in place", "field or scene too large"],
    "pws_field_reach": ["bad shape", "at least 2 x 2 nodes", "at least 2 x 2 pixels", "bad margin", "levels must lie", "r must lie",
                        "is empty or leaves", "NULL pointer", "8-byte aligned", "field or batch too large"],
}


def c_cases():
    """(entry, changed arguments, the phrase expected in the message -- None: the call returns 0)"""
    out = []
    for entry in ORDER:
        def add(phrase, **kw):
            out.append((entry, kw, phrase))
        reach = entry == "pws_field_reach"
        aux = {"pws_field_zoom": "coef", "pws_field_reach": "table"}.get(entry, "d" if "compose" in entry else "m")
        dest = "counts" if reach else "out"
        stats = {"pws_field_zoom": ["unc"], "pws_field_reach": ["counts"]}.get(entry, ["unc"] if "compose" in entry else ["s0", "s1"])
        frame = "bad frame size" if entry in ("pws_field_zoom", "pws_field_rigid", "pws_field_wobble") else "at least 2 x 2 pixels"
        big = dict(BIG, i1=1, j1=BIGW - 1) if reach else BIG
        # ---- the shape, the frame and the entry's own options
        add("bad shape", n=-1)
        add("at least 2 x 2 nodes", fh=1)
        add("at least 2 x 2 nodes", fw=1)
        add(frame, h0=1 if frame.startswith("at") else 0)
        add(frame, w0=1 if frame.startswith("at") else 0)
        add("bad shape", n=-1, fh=1)          # pairs: the earlier check speaks
        add("at least 2 x 2 nodes", fw=1, h0=0)
        add(frame, h0=0, field=None)
        if entry == "pws_field_zoom":
            add("bad frame size", margin=-1)
            add(None, n=0, h0=0, unc=None)    # (the frame size is checked for the count only)
            add("NULL pointer", h0=0, unc=None, field=None)
        if "compose" in entry or reach:
            add("bad margin", margin=-1)
            add(frame, w0=1, margin=-1)
            add("bad margin", margin=-1, field=None)
        if "compose" in entry:
            add(None, n=0, margin=-1, unc=None)   # (the margin is checked for the count only)
        if entry == "pws_field_compose_rows":
            for r in (1.5, -1.5, NAN):
                add("r must lie", r=r)
            add("rates must be non-NULL", rates=None)
            add("rates must be non-NULL", rates=R + 4)
            add("r must lie", r=2.0, rates=None)
            add("rates must be non-NULL", rates=None, fh=1)         # (before the shared checks)
            add("bad shape", n=-1, rates=None)                      # (rates are not looked at without frames)
            add("NULL pointer", r=0.0, field=None)
        if entry == "pws_field_rigid":
            for v in (-0.5, 1.5, NAN):
                add("rigidity must lie", rigidity=v)
            add("bad frame size", h0=0, rigidity=2.0)
            add("rigidity must lie", rigidity=2.0, field=None)
        if entry == "pws_field_wobble":
            for v in (0.0, 5.5, -1.0, NAN):
                add("sigma must lie", sigma=v)
            add("bad frame size", h0=0, sigma=0.0)
            add("sigma must lie", sigma=0.0, field=None)
        if reach:
            for v in (-1, 65):
                add("levels must lie", levels=v)
            for v in (1.5, NAN):
                add("r must lie", r=v)
            for kw in ({"i0": -1}, {"i0": 3, "i1": 2}, {"i1": 4}, {"j0": -1}, {"j0": 3, "j1": 2}, {"j1": 4}):
                add("is empty or leaves", **kw)
            add("bad margin", margin=-1, levels=65)
            add("levels must lie", levels=65, r=2.0)
            add("r must lie", r=2.0, i1=4)
            add("is empty or leaves", i1=4, field=None)
        # ---- no frames: nothing else is looked at
        add(None, n=0, **{k: None for k in ["field", aux, dest] + stats})
        add(None, n=0, field=F + 4)
        # ---- the pointers
        for k in ["field", aux, dest]:
            add("NULL pointer", **{k: None})
        add("NULL pointer", field=None, **{dest: O + 2})
        eight = ["field", aux] + (["rates"] if reach else ["out"])
        if entry == "pws_field_zoom":
            eight.remove("coef")
            add("8-byte aligned", coef=A + 2)
            add("field or batch too large", coef=A + 4, **big)   # (4 bytes are enough for coef)
        for k in eight:
            add("8-byte aligned", **{k: BASE[k] + 4})
        for k in stats:
            add("8-byte aligned", **{k: BASE[k] + 2})
        if reach:
            add("field or batch too large", rates=None, **big)   # (rates may be NULL)
        else:
            add("field or batch too large" if entry != "pws_field_wobble" else "field or scene too large", **dict(big, **{k: None for k in stats}))
        # ---- out against field
        if not reach:
            place = REQUIRES[entry][-2]
            for o in (F + 8, F - 8, F + 4 * 4 * 2 * 4 - 8):
                add(place, out=o)
            if entry != "pws_field_rigid":
                add(place, out=F)
            add("8-byte aligned", field=F + 4, out=F + 12)
            add(place, out=F + 8, **big)
        # ---- the grid, and what the checks before it let pass
        large = REQUIRES[entry][-1]
        add(large, **big)
        if not reach:
            add(large, out=F + 2 * BIGW * 2 * 4, **big)    # (out starts where the fields end)
            add(large, out=F - 2 * BIGW * 2 * 4, **big)
        if entry == "pws_field_rigid":
            add(large, out=F, **big)                       # (in place is allowed)
        if entry == "pws_field_wobble":
            add(large, n=32 * 65536, fh=2, fw=2)           # (65536 segments)
        elif reach:
            add(large, n=IMAX, fh=5, fw=2, i1=4, j1=1)
        else:
            add(large, n=IMAX, fh=5, fw=2, out=FAR)        # (2 row groups a frame)
    return out


T = {"t": [1, 2, 2, 2], "dtype": "float32"}
T64 = dict(T, dtype="float64")
D, D32, M = {"t": [1, 6], "dtype": "float64"}, {"t": [1, 6], "dtype": "float32"}, {"t": [1, 9], "dtype": "float64"}
RATES = {"t": [1, 2, 4], "dtype": "float64"}
WIN, HW = [0, 8, 0, 8], [8, 8]
NAMES = {"zoom_fields": ["field", "windows", "frame_hw"], "compose_fields": ["field", "d", "frame_hw"],
         "rigid_fields": ["field", "m", "frame_hw"], "wobble_fields": ["field", "m", "frame_hw", "sigma"]}


def host(t):
    return dict(t, host=True)


# (fn, positional arguments, keyword arguments): raised before a tensor is looked at, or about a tensor that is not on the device
PY_CPU = [
    ("zoom_fields", [host(T), WIN, HW], {"mode": "cubic"}),
    ("zoom_fields", [host(T), WIN, HW], {}),
    ("zoom_fields", [[1.0], WIN, HW], {}),
    ("compose_fields", [host(T), host(D), HW], {"mode": "cubic"}),
    ("compose_fields", [host(T), host(D), HW], {"rolling_shutter": "fast"}),
    ("compose_fields", [host(T), host(D), HW], {"rolling_shutter": 1.5}),
    ("compose_fields", [host(T), host(D), HW], {"rolling_shutter": NAN}),
    ("compose_fields", [host(T), host(D), HW], {"mode": "cubic", "rolling_shutter": 1.5}),
    ("compose_fields", [host(T), host(D), HW], {}),
    ("compose_fields", [[1.0], host(D), HW], {}),
    ("rigid_fields", [host(T), host(M), HW], {"rigidity": "stiff"}),
    ("rigid_fields", [host(T), host(M), HW], {"rigidity": 1.5}),
    ("rigid_fields", [host(T), host(M), HW], {"rigidity": NAN}),
    ("rigid_fields", [host(T), host(M), HW], {}),
    ("rigid_fields", [None, host(M), HW], {}),
    ("wobble_fields", [host(T), host(M), HW, "slow"], {}),
    ("wobble_fields", [host(T), host(M), HW, 0.0], {}),
    ("wobble_fields", [host(T), host(M), HW, 5.5], {}),
    ("wobble_fields", [host(T), host(M), HW, NAN], {}),
    ("wobble_fields", [host(T), host(M), HW, 1.0], {}),
]
STRIDED = dict(T, strided=True)
T3, T1 = {"t": [1, 2, 2], "dtype": "float32"}, {"t": [1, 1, 2, 2], "dtype": "float32"}
OUT3 = {"t": [1, 2, 3, 2], "dtype": "float32"}
# on the device, 1 x 2 x 2 x 2 fields; where two rules are violated the comment names the one that speaks
PY_DEVICE = [
    ("zoom_fields", [T64, WIN, HW], {}),
    ("zoom_fields", [T3, WIN, HW], {}),
    ("zoom_fields", [T1, WIN, HW], {}),
    ("zoom_fields", [T, "abcd", HW], {}),
    ("zoom_fields", [T, [[0, 8, 0, 8]] * 2, HW], {}),
    ("zoom_fields", [T, [0, 9, 0, 8], HW], {}),
    ("zoom_fields", [T, [0, 8, 0, 1], [1, 8]], {}),
    ("zoom_fields", [T, WIN, HW], {"out": T64}),
    ("zoom_fields", [T, WIN, HW], {"out": host(T)}),
    ("zoom_fields", [T, WIN, HW], {"out": OUT3}),
    ("zoom_fields", [T, WIN, HW], {"out": STRIDED, "return_uncovered": True}),
    ("zoom_fields", [T3, [0, 9, 0, 8], HW], {"out": OUT3}),         # the field's shape
    ("zoom_fields", [T, [0, 9, 0, 8], HW], {"out": T64}),           # the window
    ("compose_fields", [T64, D, HW], {}),
    ("compose_fields", [T, D32, HW], {}),
    ("compose_fields", [T, host(D), HW], {}),
    ("compose_fields", [T, [1.0] * 6, HW], {}),
    ("compose_fields", [T, D, HW], {"out": T64}),
    ("compose_fields", [T, D, HW], {"rates": dict(RATES, dtype="float32"), "rolling_shutter": 0.5}),
    ("compose_fields", [T, D, HW], {"rates": [0.0] * 8, "rolling_shutter": 0.5}),
    ("compose_fields", [T3, D, HW], {}),
    ("compose_fields", [T1, D, HW], {}),
    ("compose_fields", [T, {"t": [2, 6], "dtype": "float64"}, HW], {}),
    ("compose_fields", [T, D, HW], {"rates": {"t": [1, 8], "dtype": "float64"}, "rolling_shutter": 0.5}),
    ("compose_fields", [T, D, [1, 8]], {}),
    ("compose_fields", [T, D, HW], {"out": OUT3}),
    ("compose_fields", [T, D, HW], {"out": STRIDED, "return_uncovered": True}),
    ("compose_fields", [T3, D32, HW], {}),                          # d's dtype
    ("compose_fields", [T3, {"t": [2, 6], "dtype": "float64"}, HW], {}),   # the field's shape
    ("compose_fields", [T, {"t": [2, 6], "dtype": "float64"}, [1, 8]], {}),   # d's shape
    ("compose_fields", [T, D, [1, 8]], {"out": OUT3}),              # the frame
    ("compose_fields", [T, D, HW], {"out": T64, "rates": [0.0] * 8, "rolling_shutter": 0.5}),   # out before rates
    ("rigid_fields", [T64, M, HW], {}),
    ("rigid_fields", [T, dict(M, dtype="float32"), HW], {}),
    ("rigid_fields", [T, M, HW], {"out": T64}),
    ("rigid_fields", [T3, M, HW], {}),
    ("rigid_fields", [T, {"t": [1, 8], "dtype": "float64"}, HW], {}),
    ("rigid_fields", [T, {"t": [2, 3, 3], "dtype": "float64"}, HW], {}),
    ("rigid_fields", [T, M, [0, 8]], {}),
    ("rigid_fields", [T, M, HW], {"out": OUT3}),
    ("rigid_fields", [T, M, HW], {"out": STRIDED, "return_stats": True}),
    ("rigid_fields", [{"alias": "out"}, M, HW], {"out": T}),
    ("rigid_fields", [T3, dict(M, dtype="float32"), HW], {}),       # m's dtype
    ("rigid_fields", [T, {"t": [1, 8], "dtype": "float64"}, [0, 8]], {}),   # m's shape
    ("rigid_fields", [T, M, [0, 8]], {"out": OUT3}),                # the frame
    ("wobble_fields", [T64, M, HW, 1.0], {}),
    ("wobble_fields", [T, dict(M, dtype="float32"), HW, 1.0], {}),
    ("wobble_fields", [T, M, HW, 1.0], {"out": T64}),
    ("wobble_fields", [T1, M, HW, 1.0], {}),
    ("wobble_fields", [T, {"t": [1, 8], "dtype": "float64"}, HW, 1.0], {}),
    ("wobble_fields", [T, M, [8, 0], 1.0], {}),
    ("wobble_fields", [T, M, HW, 1.0], {"out": OUT3}),
    ("wobble_fields", [T, M, HW, 1.0], {"out": STRIDED, "return_stats": True}),
    ("wobble_fields", [T, M, HW, 1.0], {"scene_cuts": [5]}),
    ("wobble_fields", [T, M, HW, 1.0], {"out": {"same": "field"}}),
    ("wobble_fields", [T, M, [8, 0], 1.0], {"out": OUT3}),          # the frame
    ("wobble_fields", [T, M, HW, 1.0], {"out": OUT3, "scene_cuts": [5]}),   # out's shape
    ("wobble_fields", [T, M, HW, 1.0], {"out": {"same": "field"}, "scene_cuts": [5]}),   # the cuts
]


def record_c(lib):
    import field_args
    rows, seen = [], {e: set() for e in ORDER}
    for entry, kw, phrase in c_cases():
        unknown = set(kw) - set(ORDER[entry].split())
        assert not unknown, (entry, unknown)
        case = {"entry": entry, "args": [kw.get(k, BASE[k]) for k in ORDER[entry].split()]}
        rc, message = field_args.call_c(lib, case)
        if (phrase is None) != (rc == 0) or (phrase is not None and (rc != -22 or phrase not in message or not message.startswith(entry + ": "))):
            raise SystemExit("%s %r: expected %r, got %d %r" % (entry, kw, phrase, rc, message))
        seen[entry].add(phrase)
        rows.append(dict(case, rc=rc, message=message))
    for entry, phrases in REQUIRES.items():
        missing = set(phrases) - seen[entry]
        if missing or None not in seen[entry]:
            raise SystemExit("%s: no case reaches %r" % (entry, missing or "n == 0"))
    return rows


def record_python(PF, cases, device):
    import field_args
    rows = []
    for fn, args, kwargs in cases:
        case = {"fn": fn, "names": NAMES[fn], "args": args, "kwargs": kwargs}
        exc, message = field_args.call_python(PF, case, device)
        if exc is None:
            raise SystemExit("no exception: %r" % (case,))
        rows.append(dict(case, exc=exc, message=message))
    return rows


def main(argv):
    parent = os.path.abspath(argv[1])
    device = "--device" in argv
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(HERE, "field_args_errors.json")
    sys.path.insert(0, parent)
    import torch
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd import hipabi
    assert os.path.abspath(PF.__file__).startswith(parent + os.sep), PF.__file__
    fixture = {}
    if os.path.exists(out):
        with open(out) as f:
            fixture = json.load(f)
    if device:
        fixture["python_device"] = record_python(PF, PY_DEVICE, "cuda")
    else:
        if torch.cuda.is_available():
            raise SystemExit('section "c" calls the entries with made-up pointers: record it on a machine without a device')
        fixture["c"] = record_c(hipabi.lib())
        fixture["python_cpu"] = record_python(PF, PY_CPU, "cpu")
    with open(out, "w") as f:   # (a row a line)
        f.write("{\n%s\n}\n" % ",\n".join(' "%s": [\n%s\n ]' % (k, ",\n".join("  " + json.dumps(r) for r in v)) for k, v in sorted(fixture.items())))
    print("wrote", out, {k: len(v) for k, v in fixture.items()})


if __name__ == "__main__":
    main(sys.argv)
