#!/usr/bin/env python3
"""Writes tests/golden/stream_plan_errors.json: the ValueErrors that VideoStabilizer.run_video and run raise before they touch the device, as the
commit BEFORE the plan record raised them -- message and precedence are what tests/test_stream_plan_cpu.py holds VideoStabilizer._plan to.

    python tests/golden/make_golden_stream_plan.py /path/to/a/checkout/of/that/commit

No GPU: the stabiliser is built on device="cpu" around torch.nn.Identity() and the frames are CPU tensors; every error below fires before the first
device call.  (With valid arguments that commit goes on to the device and fails there, which is why the positive cases need the plan.)

A row: "covers" -- the raise statement it reaches, as file:line of that commit (rows that violate two rules name the winner, and "loses" the
other) --, "call", the constructor's "ctor" kwargs, "attrs" set after construction, the frames' "shape" and "dtype" (run: "gray", the planes'
count), the call's "kwargs" and the "message".  STATEMENTS lists every raise statement that run_video's prologue, run's and the checkers they
call can reach; the generator refuses to write a fixture that leaves one without a row."""
import json
import os
import sys

S = (8, 300, 600, 3)        # bgr24, the lattice's smallest frame
SMALL = (8, 64, 64, 3)      # below the lattice
NV12 = (8, 450, 600)
I422 = (8, 600, 600)
SM = {"smooth": 2.0}

# (covers, call, ctor, attrs, shape, dtype, kwargs[, loses])
CASES = [
    ("stream.py:1266", "run_video", {}, {}, S, "uint8", {"halo_left": 16}),
    ("stream.py:1270", "run_video", {}, {}, (3, 300, 600, 3), "uint8", {"halo_left": 2, "halo_right": 2}),
    ("functional.py:283", "run_video", {}, {}, S, "uint8", {"pixel_format": "yuv9"}),
    ("functional.py:308", "run_video", {}, {}, S, "uint16", {}),
    ("functional.py:195", "run_video", {}, {}, (8, 300, 600), "uint8", {}),
    ("functional.py:200", "run_video", {}, {}, S, "uint8", {"pixel_format": "nv12"}),
    ("functional.py:204", "run_video", {}, {}, (8, 451, 600), "uint8", {"pixel_format": "nv12"}),
    ("functional.py:207", "run_video", {}, {}, (8, 450, 602), "uint8", {"pixel_format": "nv12"}),
    ("stream.py:1278", "run_video", {}, {}, NV12, "uint8", {"pixel_format": "nv12", "frames_are_rgb": True}),
    ("stream.py:1280", "run_video", {}, {}, S, "uint8", {"output_size": [300, 150], "half_size_output": True}),
    ("stream.py:1284", "run_video", {}, {}, S, "uint8", {"output_size": [700, 150]}),
    ("stream.py:1289", "run_video", {}, {}, NV12, "uint8", {"pixel_format": "nv12", "output_size": [300, 151]}),
    ("stream.py:1290", "run_video", {}, {}, I422, "uint8", {"pixel_format": "i422", "output_size": [299, 150]}),
    ("stream.py:1294", "run_video", {}, {}, S, "uint8", {"crop": "best"}),
    ("stream.py:1296", "run_video", {}, {}, S, "uint8", {"crop": "auto", "halo_left": 1}),
    ("stream.py:1299", "run_video", {"borders": "keep"}, {}, S, "uint8", {"crop": "auto"}),
    ("stream.py:200", "run_video", {}, {}, SMALL, "uint8", {"crop": "auto"}),
    ("stream.py:1307", "run_video", {"edge": "mirror"}, {}, S, "float32", {}),
    ("stream.py:1311", "run_video", {"borders": "mosaic"}, {}, S, "float32", {}),
    ("stream.py:1313", "run_video", {"borders": "mosaic"}, {}, S, "uint8", {"in_flight": 2}),
    ("stream.py:1316", "run_video", {"borders": "mosaic"}, {}, S, "uint8", {"chunk": 4}),
    ("stream.py:200", "run_video", {"rigidity": 0.5}, {}, SMALL, "uint8", {}),
    ("stream.py:1323", "run_video", {}, {}, S, "uint8", {"zoom": 0.9, "crop": [0, 600, 0, 300]}),
    ("stream.py:1325", "run_video", {"borders": "keep"}, {}, S, "uint8", {"zoom": 0.9}),
    ("stream.py:1328", "run_video", {}, {}, S, "uint8", {"zoom": "x"}),
    ("stream.py:1330", "run_video", {}, {}, S, "uint8", {"zoom": "auto", "halo_right": 1}),
    ("stream.py:200", "run_video", {}, {}, SMALL, "uint8", {"zoom": "adaptive"}),
    ("stream.py:1338", "run_video", {}, {}, S, "uint8", {"zoom": [1]}),
    ("stream.py:1340", "run_video", {}, {}, S, "uint8", {"zoom": 1.5}),
    ("stream.py:428", "run_video", SM, {"rolling_shutter": "x"}, S, "uint8", {}),
    ("functional.py:646", "run_video", SM, {"rolling_shutter": [1]}, S, "uint8", {}),
    ("functional.py:648", "run_video", SM, {"rolling_shutter": 2.0}, S, "uint8", {}),
    ("stream.py:438", "run_video", {}, {"shutter_max_se": "x"}, S, "uint8", {}),
    ("stream.py:440", "run_video", {}, {"shutter_max_se": -1.0}, S, "uint8", {}),
    ("stream.py:1349", "run_video", {"smooth": 2.0, "rolling_shutter": 0.3}, {"smooth": 0.0}, S, "uint8", {}),
    ("stream.py:451", "run_video", SM, {"max_crop": "x"}, S, "uint8", {}),
    ("stream.py:453", "run_video", SM, {"max_crop": 0.7}, S, "uint8", {}),
    ("stream.py:460", "run_video", SM, {"limit_levels": 2.5}, S, "uint8", {}),
    ("stream.py:462", "run_video", SM, {"limit_levels": 100}, S, "uint8", {}),
    ("stream.py:469", "run_video", SM, {"limit_relax": "x"}, S, "uint8", {}),
    ("stream.py:471", "run_video", SM, {"limit_relax": 2.0}, S, "uint8", {}),
    ("stream.py:1353", "run_video", {"smooth": 2.0, "max_crop": 0.1}, {"smooth": 0.0}, S, "uint8", {}),
    ("stream.py:1356", "run_video", SM, {}, S, "uint8", {"halo_left": 1}),
    ("stream.py:1358", "run_video", {"smooth": 2.0, "borders": "keep"}, {}, S, "uint8", {}),
    ("functional.py:769", "run_video", {}, {"wobble": "x"}, S, "uint8", {}),
    ("functional.py:771", "run_video", {}, {"wobble": 9.0}, S, "uint8", {}),
    ("stream.py:1363", "run_video", {"wobble": 1.0}, {}, S, "uint8", {"halo_right": 2}),
    ("stream.py:1365", "run_video", {"wobble": 1.0, "borders": "mosaic"}, {}, S, "uint8", {}),
    ("stream.py:200", "run_video", {"wobble": 1.0}, {}, SMALL, "uint8", {}),
    ("stream.py:1371", "run_video", {}, {}, S, "uint8", {"scene_cuts": "x"}),
    ("stream.py:639", "run_video", {}, {}, S, "uint8", {"scene_cuts": ["a"]}),
    ("stream.py:641", "run_video", {}, {}, S, "uint8", {"scene_cuts": [9]}),
    ("stream.py:1379", "run_video", {}, {}, S, "uint8", {"crop": [0, 10]}),
    ("stream.py:1383", "run_video", {}, {}, S, "uint8", {"crop": [0, 700, 0, 300]}),
    ("stream.py:1386", "run_video", {}, {}, NV12, "uint8", {"pixel_format": "nv12", "crop": [1, 301, 0, 150]}),
    ("stream.py:1387", "run_video", {}, {}, I422, "uint8", {"pixel_format": "i422", "crop": [1, 301, 0, 150]}),
    # run()'s own checks (frames (T, C, H, W) float32 are its float frames)
    ("stream.py:949", "run", {"borders": "keep"}, {}, S, "uint8", {"zoom": [0, 600, 0, 300]}),
    ("stream.py:951", "run", {"borders": "mosaic"}, {}, S, "uint8", {"zoom": [0, 600, 0, 300]}),
    ("stream.py:953", "run", {"borders": "mosaic"}, {}, (8, 3, 300, 600), "float32", {}),
    ("stream.py:957", "run", {"borders": "keep"}, {}, (8, 3, 300, 600), "float32", {}),
    ("stream.py:960", "run", {"edge": "clamp"}, {}, (8, 3, 300, 600), "float32", {}),
    ("functional.py:308", "run", {}, {}, S, "uint16", {}),
    ("functional.py:283", "run", {}, {}, S, "uint8", {"pixel_format": "yuv9"}),
    ("stream.py:963", "run", {}, {}, S, "uint8", {"halo_left": 16, "gray": 24}),
    ("stream.py:966", "run", {}, {}, S, "uint8", {"gray": 5}),
    ("stream.py:641", "run", {}, {}, S, "uint8", {"scene_cuts": [9]}),
    ("stream.py:200", "run", {"rigidity": 1.0}, {}, SMALL, "uint8", {}),
    ("functional.py:561", "run", {}, {}, S, "uint8", {"zoom": "abcd"}),
    ("functional.py:563", "run", {}, {}, S, "uint8", {"zoom": [[0, 1, 0, 1]]}),
    ("functional.py:566", "run", {}, {}, S, "uint8", {"zoom": [0, 700, 0, 300]}),
    ("stream.py:963", "run", {}, {}, (0, 300, 600, 3), "uint8", {"halo_right": -1, "gray": 0}),   # (T == 0 is checked like any clip)
    ("stream.py:966", "run", {}, {}, (0, 300, 600, 3), "uint8", {"gray": 3}),
    # two rules violated at once: the one checked first speaks
    ("stream.py:1323", "run_video", {}, {}, S, "uint8", {"zoom": "x", "crop": [0, 600, 0, 300]}, "stream.py:1328"),
    ("stream.py:1296", "run_video", {"borders": "keep"}, {}, S, "uint8", {"crop": "auto", "halo_left": 1}, "stream.py:1299"),
    ("stream.py:1356", "run_video", {"smooth": 2.0, "borders": "mosaic"}, {}, S, "uint8", {"halo_left": 1}, "stream.py:1358"),
    ("stream.py:1284", "run_video", {}, {}, S, "uint8", {"output_size": [700, 150], "crop": [0, 900, 0, 300]}, "stream.py:1383"),
    ("stream.py:1266", "run_video", {}, {}, S, "uint8", {"halo_left": 16, "pixel_format": "yuv9"}, "functional.py:283"),
    ("stream.py:1294", "run_video", {}, {}, S, "uint8", {"crop": "best", "zoom": "x"}, "stream.py:1328"),
    ("stream.py:1307", "run_video", {"edge": "mirror", "borders": "mosaic"}, {}, S, "float32", {}, "stream.py:1311"),
    ("stream.py:428", "run_video", SM, {"rolling_shutter": "x", "max_crop": 0.7}, S, "uint8", {}, "stream.py:453"),
    ("functional.py:771", "run_video", {}, {"wobble": 9.0}, S, "uint8", {"scene_cuts": "x"}, "stream.py:1371"),
    ("stream.py:641", "run_video", {}, {}, S, "uint8", {"scene_cuts": [9], "crop": [0, 700, 0, 300]}, "stream.py:1383"),
    ("stream.py:200", "run_video", {"rigidity": 0.5}, {}, SMALL, "uint8", {"zoom": "auto"}, "stream.py:200 (zoom)"),
    ("stream.py:1278", "run_video", {}, {}, NV12, "uint8", {"pixel_format": "nv12", "frames_are_rgb": True, "output_size": [300, 151]}, "stream.py:1289"),
    ("stream.py:1313", "run_video", {"borders": "mosaic"}, {}, S, "uint8", {"in_flight": 2, "chunk": 4, "zoom": 0.9}, "stream.py:1316, 1325"),
    ("stream.py:949", "run", {"borders": "keep"}, {}, (8, 3, 300, 600), "float32", {"zoom": [0, 600, 0, 300]}, "stream.py:957"),
    ("stream.py:963", "run", {}, {}, S, "uint8", {"halo_left": 16, "gray": 5}, "stream.py:966"),
]

# every raise statement that the prologue of run_video (stream.py:1264-1394, crop_window included), run (stream.py:944-984) and the checkers they
# call -- _check_shutter, _check_max_se, _check_limit, functional._check_rolling_shutter, _check_wobble, _zoom_windows, _check_cuts,
# frame_format / FrameFormat.frame_shape, _check_lattice -- can reach with some argument
STATEMENTS = sorted({c[0] for c in CASES})
EXPECTED_STATEMENTS = 63


def main(parent):
    sys.path.insert(0, os.path.abspath(parent))
    import torch
    from pwstablenet_amd.stream import VideoStabilizer
    assert len(STATEMENTS) == EXPECTED_STATEMENTS, len(STATEMENTS)
    rows = []
    for case in CASES:
        covers, call, ctor, attrs, shape, dtype, kwargs = case[:7]
        vs = VideoStabilizer(torch.nn.Identity(), device="cpu", **ctor)
        for k, v in attrs.items():
            setattr(vs, k, v)
        frames = torch.zeros(shape, dtype=getattr(torch, dtype))
        kw = dict(kwargs)
        try:
            if call == "run":
                gray = torch.zeros((kw.pop("gray", shape[0]), 256, 256))
                vs.run(gray, frames, out=torch.empty(0), **kw)   # (an `out`: no pinned allocation on the way to the later checks)
            else:
                vs.run_video(frames, **kw)
        except ValueError as e:
            message, tb = str(e), e.__traceback__
            while tb.tb_next is not None:
                tb = tb.tb_next
            where = "%s:%d" % (os.path.basename(tb.tb_frame.f_code.co_filename), tb.tb_lineno)
            if where != covers:
                raise SystemExit("%r was raised at %s" % (case, where))
        else:
            raise SystemExit("no ValueError: %r" % (case,))
        row = {"covers": covers, "call": call, "ctor": ctor, "attrs": attrs, "shape": list(shape), "dtype": dtype, "kwargs": kwargs, "message": message}
        if len(case) > 7:
            row["loses"] = case[7]
        rows.append(row)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_plan_errors.json")
    with open(out, "w") as f:
        f.write('{"statements": %s,\n "rows": [\n%s\n]}\n' % (json.dumps(STATEMENTS), ",\n".join(json.dumps(r) for r in rows)))   # (a row a line)
    print("wrote", out, len(rows), "rows,", len(STATEMENTS), "statements")


if __name__ == "__main__":
    main(sys.argv[1])
