"""VideoStabilizer(smooth="l1") without a GPU: the plan takes the two-pass route and carries the path model, the reach and the weights;
everything that needs smooth > 0 takes "l1" as smoothing on; bad options are ValueErrors that leave the object as it was; a float smooth
plans as before."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pwstablenet_amd import stream  # noqa: E402
from pwstablenet_amd.stream import VideoStabilizer  # noqa: E402


def _stab(**ctor):
    return VideoStabilizer(torch.nn.Identity(), device="cpu", **ctor)


def _frames(shape=(8, 300, 600, 3), device="meta"):
    return torch.empty(shape, dtype=torch.uint8, device=device)


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_l1_plans_two_passes_and_carries_the_model(device):
    vs = _stab(smooth="l1")
    before = dict(vars(vs))
    p = vs._plan(_frames(device=device))
    assert p.two_pass is True and p.path_model == "l1" and p.smooth == 0.0
    assert (p.l1_reach, p.l1_weights) == (0.1, (10.0, 1.0, 100.0))
    assert vars(vs) == before and vs.smooth == "l1" and vs.smooth_l1_info is None
    p = _stab(smooth="l1", l1_reach=0.25, l1_weights=[1, 2, 3])._plan(_frames(device=device))
    assert (p.path_model, p.l1_reach, p.l1_weights) == ("l1", 0.25, (1.0, 2.0, 3.0))


def test_a_float_smooth_plans_as_before():
    p = _stab(smooth=2.5, max_crop=0.1)._plan(_frames())
    assert (p.smooth, p.path_model, p.two_pass, p.limit_relax) == (2.5, "gaussian", True, 0.125)
    p = _stab()._plan(_frames())
    assert (p.smooth, p.path_model, p.two_pass) == (0.0, None, False)
    assert _stab().smooth_l1_info is None


def test_limit_relax_resolves_to_the_generators_reach():
    """limit_relax=None under "l1": 1 / (period // 2) -- 1 / 15 at period 30; an explicit value stands."""
    assert _stab(smooth="l1", max_crop=0.1)._plan(_frames()).limit_relax == 1.0 / 15
    assert _stab(smooth="l1", max_crop=0.1, period=20)._plan(_frames()).limit_relax == 1.0 / 10
    assert _stab(smooth="l1", max_crop=0.1, limit_relax=0.5)._plan(_frames()).limit_relax == 0.5
    p = _stab(smooth="l1", max_crop=0.05, limit_levels=8)._plan(_frames())
    assert (p.max_crop, p.limit_levels) == (0.05, 8)


def test_what_needs_smoothing_takes_l1():
    p = _stab(smooth="l1", rolling_shutter=0.3)._plan(_frames())
    assert (p.shutter, p.path_model) == (0.3, "l1")
    assert _stab(smooth="l1", rolling_shutter="auto")._plan(_frames()).shutter == "auto"
    assert _stab(smooth="l1", max_crop=0.05)._plan(_frames()).max_crop == 0.05
    assert _stab(smooth="l1", wobble=1.0)._plan(_frames(), zoom="adaptive").two_pass
    # the halo and borders errors, with the messages that smooth > 0 has
    with pytest.raises(ValueError, match=r"run_video: smooth > 0 needs the whole clip \(a shard cannot see the scene's path\)"):
        _stab(smooth="l1")._plan(_frames((12, 300, 600, 3)), halo_left=2)
    for borders in ("keep", "mosaic"):
        with pytest.raises(ValueError, match="run_video: smooth > 0 warps in a second pass, which borders=\"%s\" does not have yet" % borders):
            _stab(smooth="l1", borders=borders)._plan(_frames())
    # and without smoothing the options that need it are still refused
    with pytest.raises(ValueError, match="needs smooth > 0"):
        _stab(rolling_shutter=0.3)
    with pytest.raises(ValueError, match="needs smooth > 0"):
        _stab(max_crop=0.1)


@pytest.mark.parametrize("kw, message", [
    ({"l1_reach": 0.0}, "VideoStabilizer: reach must lie in (0, 0.5], got 0.0"),
    ({"l1_reach": 0.6}, "VideoStabilizer: reach must lie in (0, 0.5], got 0.6"),
    ({"l1_reach": float("nan")}, "VideoStabilizer: reach must lie in (0, 0.5], got nan"),
    ({"l1_reach": "wide"}, "VideoStabilizer: reach must be a share of the frame in (0, 0.5], got 'wide'"),
    ({"l1_weights": (1.0, 2.0)}, "VideoStabilizer: weights must be three positive finite numbers (w1, w2, w3), got (1.0, 2.0)"),
    ({"l1_weights": (1.0, 0.0, 1.0)}, "VideoStabilizer: weights must be three positive finite numbers (w1, w2, w3), got (1.0, 0.0, 1.0)"),
    ({"l1_weights": (1.0, float("inf"), 1.0)}, "VideoStabilizer: weights must be three positive finite numbers (w1, w2, w3), got (1.0, inf, 1.0)"),
    ({"l1_weights": 3.0}, "VideoStabilizer: weights must be three positive finite numbers (w1, w2, w3), got 3.0"),
    ({"smooth": "l2"}, "VideoStabilizer: sigma must be a number of frames, got 'l2'"),
])
def test_bad_options_are_value_errors(kw, message):
    with pytest.raises(ValueError) as err:
        _stab(**dict({"smooth": "l1"}, **kw))
    assert str(err.value) == message


def test_options_set_later_are_checked_by_the_plan_and_nothing_changes():
    vs = _stab(smooth="l1")
    vs.l1_reach, vs.l1_weights = 0.7, (10.0, 1.0, 100.0)
    sentinel = object()
    vs.smooth_l1_info = vs.smooth_correction = vs.smooth_path = sentinel
    before = dict(vars(vs))
    with pytest.raises(ValueError) as err:
        vs.run_video(_frames())
    assert str(err.value) == "run_video: reach must lie in (0, 0.5], got 0.7"
    vs.l1_reach, vs.l1_weights = 0.2, (10.0, -1.0, 100.0)
    before["l1_reach"], before["l1_weights"] = 0.2, (10.0, -1.0, 100.0)
    with pytest.raises(ValueError) as err:
        vs.run_video(_frames())
    assert str(err.value) == "run_video: weights must be three positive finite numbers (w1, w2, w3), got (10.0, -1.0, 100.0)"
    assert vars(vs) == before and vs.smooth_l1_info is sentinel


def test_optimal_path_is_public_and_checks_before_the_device():
    assert stream.optimal_path is not None
    good = dict(frame_hw=(300, 600))
    with pytest.raises(ValueError, match="optimal_path: motion must be a \\(T, 4\\) float64 tensor on the device"):
        stream.optimal_path(torch.zeros(5, 4, dtype=torch.float64), **good)   # (a host tensor)
