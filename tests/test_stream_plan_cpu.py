"""VideoStabilizer._plan without a GPU: every ValueError that run_video and run raised before they touched the device, word for word and in
the precedence that the commit before the plan record had (tests/golden/stream_plan_errors.json, written from that commit by
tests/golden/make_golden_stream_plan.py); a failed call leaves the object as it was; and the plans of valid calls, with the values worked
out by hand from that commit's run_video in the comments."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pwstablenet_amd.stream import VideoStabilizer  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "stream_plan_errors.json")) as _f:
    FIXTURE = json.load(_f)
ROWS = FIXTURE["rows"]
# what a call leaves on the object: every result attribute, and the call's cuts and wait
RESULTS = ("zoom_windows", "zoom_uncovered", "rigid_residual", "rigid_unfit", "mosaic_unfilled", "motion_in", "motion_out", "motion_inliers_in",
           "motion_inliers_out", "_report", "smooth_motion", "smooth_inliers", "smooth_path", "smooth_correction", "smooth_uncovered",
           "shutter_rates", "shutter_estimate", "rolling_shutter_used", "limit_strength", "limit_need", "limit_uncovered",
           "smooth_correction_unlimited", "wobble_removed", "wobble_unfit", "scene_cuts", "scene_wait_s")


def _stab(**ctor):
    return VideoStabilizer(torch.nn.Identity(), device="cpu", **ctor)


def _call(row, device):
    """The row's call on frames of the row's shape and dtype on ``device``; returns the stabiliser and the ValueError's message."""
    vs = _stab(**row["ctor"])
    for k, v in row["attrs"].items():
        setattr(vs, k, v)
    sentinels = {k: object() for k in RESULTS}
    for k, v in sentinels.items():
        setattr(vs, k, v)
    frames = torch.zeros(row["shape"], dtype=getattr(torch, row["dtype"]), device=device)
    kw = dict(row["kwargs"])
    with pytest.raises(ValueError) as err:
        if row["call"] == "run":
            gray = torch.zeros((kw.pop("gray", row["shape"][0]), 256, 256), device=device)
            vs.run(gray, frames, out=torch.empty(0), **kw)
        else:
            vs.run_video(frames, **kw)
    return vs, sentinels, str(err.value)


def test_every_reachable_raise_statement_has_a_row():
    covered = {r["covers"] for r in ROWS if "loses" not in r}
    assert covered == set(FIXTURE["statements"]) and len(covered) == 63
    assert sum("loses" in r for r in ROWS) >= 10   # two rules violated at once


@pytest.mark.parametrize("device", ["cpu", "meta"])
@pytest.mark.parametrize("k", range(len(ROWS)), ids=lambda k: "%s-%s-%d" % (ROWS[k]["call"], ROWS[k]["covers"], k))
def test_message_precedence_and_no_side_effects(k, device):
    row = ROWS[k]
    vs, sentinels, message = _call(row, device)
    assert message == row["message"]
    for name, v in sentinels.items():   # the failed call changed nothing
        assert getattr(vs, name) is v, name
    for name, v in row["attrs"].items():
        assert getattr(vs, name) == v


def _frames(shape, dtype=torch.uint8, device="meta"):
    return torch.empty(shape, dtype=dtype, device=device)


def test_plan_makes_no_device_call_and_changes_nothing():
    vs = _stab(smooth=2.0, rolling_shutter="auto", wobble=1.0, max_crop=0.1, metrics=True)
    before = dict(vars(vs))
    for device in ("cpu", "meta"):
        p = vs._plan(_frames((40, 300, 600, 3), device=device), chunk=16, crop="auto", scene_cuts="auto")
        assert p.on_host and p.T == 40 and p.detect and p.cuts == () and p.crop == "auto" and p.shutter == "auto" and p.metrics
    assert vars(vs) == before
    with pytest.raises(AttributeError):
        p.T = 1   # an immutable record


@pytest.mark.parametrize("ctor, kwargs, two_pass", [
    ({}, {}, False), ({}, {"crop": (0, 600, 0, 300)}, False), ({}, {"zoom": 0.9}, False), ({"rigidity": 1.0}, {}, False),
    ({"borders": "keep"}, {}, False), ({"borders": "mosaic"}, {}, False), ({"metrics": True}, {}, False),
    ({}, {"crop": "auto"}, True), ({}, {"zoom": "auto"}, True), ({}, {"zoom": "adaptive"}, True), ({"smooth": 0.5}, {}, True),
    ({"wobble": 0.5}, {}, True), ({"smooth": 2.0, "wobble": 1.0}, {"zoom": 0.9}, True)])
def test_two_pass(ctor, kwargs, two_pass):
    """run_video: ``two_pass = auto or zmode in ("auto", "adaptive") or smoothing or wob > 0.0`` and nothing else."""
    assert _stab(**ctor)._plan(_frames((8, 300, 600, 3)), **kwargs).two_pass is two_pass


def test_chunks_with_and_without_halos():
    """run_video: ``[(s if s > halo_left else 0, min(halo_left + T, s + chunk) if s + chunk < halo_left + T else n_all) for s in
    range(halo_left, halo_left + T, chunk)]``.  40 frames, chunk 16, no halos: s = 0, 16, 32 -> (0, 16), (16, 32), (32, 40).
    Halos (3, 2): T = 35, s = 3, 19, 35: s = 3 is not > 3 -> start 0, 19 < 38 -> stop 19; (19, 35); s = 35: 51 >= 38 -> stop n_all = 40."""
    vs = _stab()
    p = vs._plan(_frames((40, 300, 600, 3)), chunk=16)
    assert (p.T, p.n_all, p.chunks) == (40, 40, ((0, 16), (16, 32), (32, 40)))
    p = vs._plan(_frames((40, 300, 600, 3)), chunk=16, halo_left=3, halo_right=2)
    assert (p.T, p.n_all, p.halo_left, p.halo_right, p.chunks) == (35, 40, 3, 2, ((0, 19), (19, 35), (35, 40)))


def test_empty_and_single_frame_clips():
    """T = n_all - halos; range(h, h + 0, chunk) is empty; one frame is one chunk (0, 1)."""
    vs = _stab()
    p = vs._plan(_frames((0, 300, 600, 3)))
    assert (p.T, p.chunks, p.oh, p.ow, p.crop) == (0, (), 300, 600, None)
    p = vs._plan(_frames((5, 300, 600, 3)), halo_left=3, halo_right=2)   # a shard that holds halos only
    assert (p.T, p.n_all, p.chunks) == (0, 5, ())
    p = vs._plan(_frames((1, 300, 600, 3)))
    assert (p.T, p.chunks) == (1, ((0, 1),))
    # an empty clip returned before run_video read chunk or in_flight: whatever they hold is no error there
    p = vs._plan(_frames((0, 300, 600, 3)), chunk=0, in_flight="two")
    assert (p.T, p.chunks, p.in_flight) == (0, (), 1)


def test_output_shape_and_crop_window():
    vs = _stab()
    # bgr24, half_size_output: (oh, ow) = (h // 2, w // 2); no crop
    p = vs._plan(_frames((8, 720, 1280, 3)), half_size_output=True)
    assert (p.fmt.name, p.h, p.w, p.oh, p.ow, p.crop, p.half_size_output) == ("bgr24", 720, 1280, 360, 640, None, True)
    # nv12 (T, H * 3 // 2, W): 1080 rows are H = 720; output_size = (width, height); the crop (x0, x1, y0, y1, threshold 2) is the window
    # (cy0, cy1, cx0, cx1) = (y0 + 2, y1 - 2, x0 + 2, x1 - 2) = (10, 350, 6, 634): even edges, inside 640 x 360
    p = vs._plan(_frames((8, 1080, 1280)), pixel_format="nv12", output_size=(640, 360), crop=(4, 636, 8, 352, 2), in_flight=2)
    assert (p.fmt.name, p.h, p.w, p.oh, p.ow, p.crop, p.in_flight) == ("nv12", 720, 1280, 360, 640, (10, 350, 6, 634), 2)
    # i422 (T, 2 * H, W): x edges even, y edges free -- an odd y edge is allowed
    p = vs._plan(_frames((8, 600, 600)), pixel_format="i422", crop=(2, 598, 1, 299))
    assert (p.fmt.name, p.h, p.w, p.oh, p.ow, p.crop) == ("i422", 300, 600, 300, 600, (1, 299, 2, 598))
    # 10-bit frames keep their format; a device would be needed only to run them
    p = vs._plan(_frames((8, 450, 600), torch.uint16), pixel_format="p010", scene_cuts=[3, 6])
    assert (p.fmt.name, p.fmt.dtype, p.cuts, p.detect, p.lattice) == ("p010", torch.uint16, (3, 6), False, True)
    assert not vs._plan(_frames((8, 96, 128, 3))).lattice


def test_options_are_resolved():
    """_check_limit: limit_relax=None is 1 / ceil(3 sigma), resolved against the call's smooth; the zoom's window is _centred_window's."""
    p = _stab(smooth=2.5, max_crop=0.1)._plan(_frames((8, 300, 600, 3)))
    assert (p.smooth, p.max_crop, p.limit_levels) == (2.5, 0.1, 16) and p.limit_relax == 1.0 / math.ceil(3 * 2.5) == 0.125
    assert _stab(smooth=2.0, max_crop=0.1, limit_relax=0.5)._plan(_frames((8, 300, 600, 3))).limit_relax == 0.5
    vs = _stab(smooth=2.0, rolling_shutter=0.3, borders="black", edge="mirror", rigidity=0.5, mosaic_radius=4)
    vs.rolling_shutter, vs.wobble = -0.25, 1.5   # (set after construction: the plan reads them again)
    p = vs._plan(_frames((8, 300, 600, 3)), zoom=0.9, metrics=True, zoom_speed=0.01, zoom_min=0.6, scene_threshold=0.3, scene_min_len=8)
    assert (p.shutter, p.max_se, p.wobble, p.edge, p.rigid, p.keep, p.mosaic, p.radius, p.metrics) == (-0.25, 0.02, 1.5, "mirror", True, False, False, 4, True)
    # zoom=0.9 of 600 x 300: (0.5 w - 0.45 w, 0.5 w + 0.45 w, 0.5 h - 0.45 h, 0.5 h + 0.45 h)
    assert (p.zmode, p.zoom_speed, p.zoom_min, p.scene_threshold, p.scene_min_len) == ("fixed", 0.01, 0.6, 0.3, 8)
    assert p.zwin == (0.5 * 600 - 0.5 * 0.9 * 600, 0.5 * 600 + 0.5 * 0.9 * 600, 0.5 * 300 - 0.5 * 0.9 * 300, 0.5 * 300 + 0.5 * 0.9 * 300)
    p = _stab(borders="mosaic", mosaic_radius=4)._plan(_frames((8, 300, 600, 3)), chunk=4)
    assert (p.mosaic, p.radius, p.keep, p.two_pass) == (True, 4, False, False)
    assert _stab(borders="keep")._plan(_frames((8, 300, 600, 3))).keep


def test_functional_does_not_import_stream():
    code = "import sys; import pwstablenet_amd.functional; sys.exit(int('pwstablenet_amd.stream' in sys.modules))"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
