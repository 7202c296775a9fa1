"""The instruments of tests/test_hip_homography_float64.py, pinned without a GPU: the lattice at odd frames, the margins of every entry
of the case table of tests/homography_ref.py (so that no decision of the fit is close in any of them), what two independent float64
solvers leave open per entry, the no-fit fields' reasons, the mutants the GPU gate must catch, and the float64 resize.

Measured here (printed by the tests, run with -s):
  fit entries (125)   smallest pivot ratio 0.59 .. 0.64; 1 .. 8 Gauss-Newton steps (the kernel caps at 20); spread ratio 1.0e5 .. 7.7e5
  spread              max |fit - fit_independent| 1.1e-16 .. 6.1e-14 (ten entries replaced for it, which had 1.0e-13 .. 1.5e-12 and up to
                      11 steps: homography_ref.REPLACED)
  no-fit              spread ratio 0 (constant), 6.8e-3 (spread 1e-8); pivot ratio -2.1e-16 (line), 0 (x-only, single row, single column),
                      3.6e-15 (parabola)
  near                spread 1e-5: spread ratio 6.8, pivot ratio 0.61; near-line: pivot ratio 5.0e-7
  mutants             two steps short: 2.8e-12 from the full fit at least; one point dropped: 4.3e-5 at least; the gate is 1e-12"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_ref as R  # noqa: E402

SPREAD_MAX = 1e-12 / 16      # below it, 16 x the spread stays under the gate's floor of 1e-12


def _round32(p):
    return p.astype(np.float32).astype(np.float64)      # the kernel's samples are float32


@functools.lru_cache(maxsize=None)
def _entry(frame_hw, field_hw):
    """[(family, p1, p2, M, info, spread)] of one launch of the table."""
    _, _, p2 = R.lattice(frame_hw)
    out = []
    for name, field in zip(R.FAMILIES, R.case_fields(frame_hw, field_hw)):
        p1 = _round32(R.sample64(field, frame_hw)[0])
        M, info = R.fit_info(p1, p2)
        out.append((name, p1, p2, M, info, R.spread(p1, p2) if M is not None else None))
    return out


@pytest.mark.parametrize("frame_hw", [(301, 601), (361, 641), (300, 600), (1081, 1920), (1080, 1921)])
def test_lattice_is_the_reference_formula_at_odd_frames(frame_hw):
    """main_new.py:556-563, evaluated term by term in Python's own arithmetic: the rows from H0 // 2, the columns from W0 // 2, p2's x from
    the float W0 / 2 and p2's y from the integer H0 // 2, both then rounded to float32 (:568)."""
    H0, W0 = frame_hw
    num_sample, stride_sample = 20, 15
    r, c, p2 = R.lattice(frame_hw)
    k = 0
    for sample_height in range(num_sample):
        for sample_width in range(num_sample):
            assert r[k] == H0 // 2 + (sample_height - num_sample // 2) * stride_sample
            assert c[k] == W0 // 2 + (sample_width - num_sample // 2) * stride_sample * 2
            assert p2[k, 0] == np.float32((W0 / 2 + (sample_width - num_sample / 2) * stride_sample * 2) / W0 * 2 - 1)
            assert p2[k, 1] == np.float32((H0 // 2 + (sample_height - num_sample // 2) * stride_sample) / H0 * 2 - 1)
            k += 1
    assert 0 <= r.min() and r.max() < H0 and 0 <= c.min() and c.max() < W0
    if W0 % 2:      # the column is half a pixel left of p2's x: the two halves differ, as in the reference
        assert np.all(np.abs((p2[:, 0] + 1) * W0 / 2 - c - 0.5) < 1e-4)


def test_replaced_entries_belong_to_the_table():
    for frame_hw, field_hw, name in R.REPLACED:
        assert (frame_hw, field_hw) in R.CASES and name in R.FAMILIES
    assert len(R.CASES) == 25 and len(R.FAMILIES) == 5


@pytest.mark.parametrize("frame_hw,field_hw", R.CASES)
def test_every_fit_entry_has_margins_and_a_small_spread(frame_hw, field_hw):
    """No Cholesky near refusal (pivot ratio >= 1e-3 against the test's 1e-12), convergence well inside the kernel's 20 steps (<= 15), a
    sample spread far from the no-spread test (ratio >= 100), and two solvers that share nothing agreeing to 1e-12 / 16."""
    for name, p1, p2, M, info, spread in _entry(frame_hw, field_hw):
        assert M is not None and np.array_equal(M, R.fit(p1, p2)), name
        print(frame_hw, field_hw, name, "steps %d pivot ratio %.3g spread ratio %.3g spread %.3g" % (
            info["steps"], info["pivot"], info["spread"], spread))
        assert info["pivot"] >= 1e-3 and info["steps"] <= 15 and info["spread"] >= 100, (name, info)
        assert spread <= SPREAD_MAX, (name, spread)
        assert M[2, 2] == 1.0 and R.fit_independent(p1, p2)[2, 2] == 1.0


def test_replaced_entries_as_first_built_keep_margins_and_a_gate_with_teeth():
    """The ten entries that REPLACED took out of the table, which the GPU file still runs: their spread is above 1e-12 / 16 (why they
    left), their margins are the table's, and 16 x their spread still lies below both mutants."""
    for frame_hw, field_hw, name in R.REPLACED:
        _, _, p2 = R.lattice(frame_hw)
        p1 = _round32(R.sample64(R.first_built(field_hw, name), frame_hw)[0])
        M, info = R.fit_info(p1, p2)
        spread, gate = R.spread(p1, p2), R.gate(p1, p2)
        short = float(np.abs(R.fit(p1, p2, iters=info["steps"] - 2) - M).max())
        drop = float(np.abs(R.fit(p1[1:], p2[1:]) - M).max())
        print(frame_hw, field_hw, name, "steps %d pivot ratio %.3g spread ratio %.3g spread %.3g gate %.3g two steps short %.3g one point "
              "dropped %.3g" % (info["steps"], info["pivot"], info["spread"], spread, gate, short, drop))
        assert info["pivot"] >= 1e-3 and info["steps"] <= 15 and info["spread"] >= 100, (name, info)
        assert SPREAD_MAX < spread and gate == 16.0 * spread and short > gate and drop > gate, (name, spread, short, drop)


def _nofit_samples():
    frame_hw = (360, 640)
    _, _, p2 = R.lattice(frame_hw)
    out = {name: _round32(R.sample64(f, frame_hw)[0]) for name, f in R.nofit_fields().items()}
    out["single row"] = _round32(R.sample64(R.family_field("identity", (1, 256)), frame_hw)[0])
    out["single column"] = _round32(R.sample64(R.family_field("identity", (256, 1)), frame_hw)[0])
    return p2, out


def test_every_nofit_entry_is_refused_for_a_clear_reason():
    """Either no spread (ratio <= 1e-2 against the test's 1) or no rank (a pivot ratio <= 1e-14 against the test's 1e-12): 100 times clear
    of the threshold, so the kernel, which sums in another order, decides alike."""
    p2, samples = _nofit_samples()
    for name, p1 in samples.items():
        M, info = R.fit_info(p1, p2)
        print("no fit:", name, info)
        assert M is None and R.fit(p1, p2) is None, name
        assert info["spread"] <= 1e-2 or (info["spread"] >= 100 and info["pivot"] <= 1e-14), (name, info)
    field = R.family_field("projective", (256, 256))
    node = sorted(R.sample64(field, (360, 640))[1])[777]
    for bad in (np.nan, np.inf, -np.inf):
        f = field.copy()
        f[node[0], node[1], 1] = bad
        with np.errstate(invalid="ignore"):
            p1 = _round32(R.sample64(f, (360, 640))[0])
            assert not np.isfinite(p1).all() and R.fit(p1, p2) is None, bad


def test_near_entries_are_fitted_clearly():
    """A spread of 1e-5 sits 6.8 times above the no-spread test: closer than the 100 times asked of the table, but md1 is a mean of 400
    float64 distances, which no summation order moves by more than 1e-13 of itself.  The near-line's smallest pivot ratio is 5e5 times
    the Cholesky test's."""
    frame_hw = (360, 640)
    _, _, p2 = R.lattice(frame_hw)
    for name, f in R.near_fields().items():
        p1 = _round32(R.sample64(f, frame_hw)[0])
        M, info = R.fit_info(p1, p2)
        print("near:", name, info, "spread", R.spread(p1, p2), "gate", R.gate(p1, p2))
        assert M is not None and info["pivot"] >= 1e-9 and info["spread"] >= 5 and info["steps"] <= 15, (name, info)


@pytest.mark.parametrize("frame_hw", R.FRAMES)
def test_the_gate_has_teeth(frame_hw):
    """Two mutants of the restatement miss the GPU test's gate against the full restatement, on every entry of this frame size whose fit
    takes at least three steps: Gauss-Newton stopped two steps before it converged, and the fit without lattice point 0."""
    short_min, drop_min, entries = np.inf, np.inf, 0
    for field_hw in R.FIELD_SIZES:
        for name, p1, p2, M, info, spread in _entry(frame_hw, field_hw):
            if info["steps"] < 3:
                continue
            gate = max(16.0 * spread, 1e-12)
            short = float(np.abs(R.fit(p1, p2, iters=info["steps"] - 2) - M).max())
            drop = float(np.abs(R.fit(p1[1:], p2[1:]) - M).max())
            assert short > gate and drop > gate, (field_hw, name, short, drop, gate)
            short_min, drop_min, entries = min(short_min, short), min(drop_min, drop), entries + 1
    print(frame_hw, "entries", entries, "two steps short: at least %.3g" % short_min, "one point dropped: at least %.3g" % drop_min)
    assert entries >= 15


@pytest.mark.parametrize("frame_hw,field_hw", R.CASES)
def test_sample64_is_the_align_corners_resize(frame_hw, field_hw):
    import torch
    f = np.random.RandomState(field_hw[0] + frame_hw[0]).uniform(-1, 1, field_hw + (2,))
    up = torch.nn.functional.interpolate(torch.from_numpy(f).permute(2, 0, 1)[None], size=frame_hw, mode="bilinear", align_corners=True)
    r, c, _ = R.lattice(frame_hw)
    want = up[0].permute(1, 2, 0).numpy()[r, c]
    got, nodes = R.sample64(f, frame_hw)
    assert got.shape == (400, 2) and np.abs(got - want).max() <= 1e-14
    assert all(0 <= y < field_hw[0] and 0 <= x < field_hw[1] for y, x in nodes)


@pytest.mark.parametrize("frame_hw", [(301, 601), (1080, 1920)])
def test_sample64_names_exactly_the_nodes_the_resize_reads(frame_hw):
    """One node of the (5, 7) field at a time is made NaN: torch's resize changes at the lattice exactly for the nodes of the set (a tap of
    weight zero still spreads a NaN), and so does sample64.  At 1080 x 1920 the lattice covers the centre only: 9 of the 35 nodes."""
    import torch
    f = R.family_field("projective", (5, 7)).astype(np.float64)
    r, c, _ = R.lattice(frame_hw)
    nodes = R.sample64(f, frame_hw)[1]
    read = set()
    for y in range(5):
        for x in range(7):
            g = f.copy()
            g[y, x] = np.nan
            up = torch.nn.functional.interpolate(torch.from_numpy(g).permute(2, 0, 1)[None], size=frame_hw, mode="bilinear",
                                                 align_corners=True)[0].permute(1, 2, 0).numpy()[r, c]
            assert np.array_equal(np.isnan(up), np.isnan(R.sample64(g, frame_hw)[0]))
            if np.isnan(up).any():
                read.add((y, x))
    assert read == nodes and len(nodes) == (35 if frame_hw[0] == 301 else 9)
