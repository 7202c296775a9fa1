"""GPU tests of the reach kernel (csrc/field_reach.hip; C: pws_field_reach): per frame and level, the nodes of a rectangle of the lattice
that the composition with that level's correction would leave uncovered.

Over the whole lattice the counts are ``compose_fields(..., return_uncovered=True)``'s EXACTLY, level by level -- the existing kernel is
the yardstick: both call one node function -- for both coordinate conventions, margins 0 and 1, without rates and with them at r = +-0.7.
Sub-rectangles are held to the float64 restatement's [lo, hi] per (frame, level) (tests/limit_ref.py reach_bounds: path_ref.compose64's
value tolerance 2^-22 W max|corner| + 2^-16 max|corner difference|, in pixels, plus one float32 rounding of the un-normalised coordinate,
as tests/test_hip_field_compose.py); the share of (frame, level) pairs that the reference leaves undecided is asserted below 1 % on the
reference alone.  Lattices (2, 2), (19, 37) (odd width, partial row group, one column chunk) and (256, 256) (two column chunks), a 640 x
360 frame."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limit_ref as L  # noqa: E402
import path_ref as P  # noqa: E402

FRAME = (360, 640)
EINVAL = -22
CAP = 0.01


def similarity(deg, scale, tx, ty):
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    return [c, -s, tx, s, c, ty]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def p(t):
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else None


@functools.lru_cache(maxsize=None)
def inputs(lat, n, seed):
    """(field (n, fh, fw, 2) float32 with one NaN node, d (n, 6) with a NaN row, an identity row and a shift of a million pixels when n allows,
    rates (n, 2, 4)); read-only."""
    rs = np.random.RandomState(seed)
    field = P.make_field((n,) + lat + (2,), seed, scale=0.98)
    d = np.array([similarity(rs.uniform(-2, 2), math.exp(rs.uniform(-0.04, 0.04)), rs.uniform(-50, 50), rs.uniform(-30, 30)) for _ in range(n)])
    if n >= 6:
        field[1, lat[0] // 2, lat[1] // 2, 0] = np.nan
        d[2, 4] = float("nan")
        d[3] = P.IDENTITY
        d[4] = [1.0, 0.0, 1e6, 0.0, 1.0, 0.0]
    rates = np.stack([rs.uniform(-0.003, 0.003, (n, 2)), rs.uniform(-0.004, 0.004, (n, 2)), rs.uniform(-6, 6, (n, 2)), rs.uniform(-4, 4, (n, 2))], -1)
    for a in (field, d, rates):
        a.setflags(write=False)
    return field, d, rates


def table_of(d, levels):
    """The levels' corrections; levels = 0: the rows themselves."""
    return L.levels_table(d, levels) if levels else np.asarray(d, np.float64)[:, None, :].copy()


def reach(hip, field, table, levels, rect, rates=None, r=0.0, ac=False, margin=0, frame=FRAME):
    n, fh, fw = field.shape[:3]
    counts = torch.full((n, levels + 1), -5, device="cuda", dtype=torch.int32)
    rc = hip.lib().pws_field_reach(p(field), n, fh, fw, p(table), levels, p(rates), r, rect[0], rect[1], rect[2], rect[3], frame[0], frame[1],
                                   int(ac), margin, p(counts), hip.current_stream())
    assert rc == 0, hip.lib().pws_last_error()
    return counts


WHOLE = [((2, 2), 6, 16), ((19, 37), 6, 16), ((19, 37), 6, 0), ((19, 37), 6, 1), ((19, 37), 70, 64), ((256, 256), 6, 16), ((256, 256), 1, 16)]


@pytest.mark.parametrize("lat,n,levels", WHOLE, ids=["%dx%d-n%d-l%d" % (c[0] + c[1:]) for c in WHOLE])
def test_the_whole_lattice_counts_are_the_composition_kernels(hip, lat, n, levels):
    from pwstablenet_amd import functional as PF
    field, d, rates = inputs(lat, n, lat[0] + n + levels)
    table = table_of(d, levels)
    field_d, table_d, rates_d = dev(field), dev(table), dev(rates)
    levels_d = [table_d[:, l].contiguous() for l in range(levels + 1)]
    rect = (0, lat[0] - 1, 0, lat[1] - 1)
    seen = 0
    for ac in (False, True):
        for mode, margin in (("bilinear", 0), ("bicubic", 1)):
            for r in (0.0, 0.7, -0.7):
                got = reach(hip, field_d, table_d, levels, rect, rates_d if r else None, r, ac, margin)
                want = torch.stack([PF.compose_fields(field_d, levels_d[l], FRAME, align_corners=ac, mode=mode, return_uncovered=True,
                                                      rates=rates_d if r else None, rolling_shutter=r)[1] for l in range(levels + 1)], 1)
                assert got.dtype == torch.int32 and torch.equal(got, want), (ac, margin, r, (got - want).abs().max())
                seen += int(got.sum())
                if n >= 6 and levels >= 1:
                    assert bool((got[4, 1:] == lat[0] * lat[1]).all())   # a million pixels away: every node, at every level >= 1
                    assert int(got[1].min()) >= 1                        # the NaN node is not covered at any level
                    assert bool((got[2] == got[2, 0]).all())             # a NaN row of d keeps the field at every level
    # rates with r = 0, and r without rates, are the affine kernel
    a = reach(hip, field_d, table_d, levels, rect, rates_d, 0.0)
    b = reach(hip, field_d, table_d, levels, rect, None, 0.7)
    assert torch.equal(a, reach(hip, field_d, table_d, levels, rect)) and torch.equal(a, b)
    assert seen > 0


# (lattice, n, levels, rectangle, seed): the seeds were picked on the CPU so that the float64 restatement decides every (frame, level) pair
# of every configuration below -- with one frame a single undecided pair is 6 % -- and counts something
SUB = [((19, 37), 70, 16, (5, 5, 9, 9), 1), ((19, 37), 70, 16, (7, 7, 0, 36), 1), ((19, 37), 6, 64, (2, 16, 3, 33), 4),
       ((19, 37), 6, 1, (0, 18, 0, 36), 1), ((2, 2), 6, 16, (1, 1, 0, 1), 2), ((256, 256), 1, 16, (12, 243, 12, 243), 4),
       ((256, 256), 1, 0, (100, 100, 0, 255), 1)]


@pytest.mark.parametrize("lat,n,levels,rect,seed", SUB, ids=["%dx%d-n%d-l%d-%s" % (c[0] + c[1:3] + ("_".join(map(str, c[3])),)) for c in SUB])
def test_sub_rectangles_against_float64(hip, lat, n, levels, rect, seed):
    field, d, rates = inputs(lat, n, seed)
    table = table_of(d, levels)
    field_d, table_d, rates_d = dev(field), dev(table), dev(rates)
    shares = []
    for ac, margin, r in ((False, 0, 0.0), (True, 1, 0.0), (False, 0, 0.7), (True, 0, -0.7)):
        lo, hi, share = L.reach_bounds(field, table, FRAME, rect, ac, margin, rates if r else None, r)
        shares.append(share)
        got = reach(hip, field_d, table_d, levels, rect, rates_d if r else None, r, ac, margin).cpu().numpy()
        nodes = (rect[1] - rect[0] + 1) * (rect[3] - rect[2] + 1)
        print("ac=%s margin=%d r=%g: counts up to %d of %d nodes, undecided pairs %.4f" % (ac, margin, r, got.max(), nodes, share))
        assert (lo <= got).all() and (got <= hi).all() and got.max() <= nodes, (ac, margin, r)
    assert max(shares) < CAP   # (the reference alone)


def test_two_runs_give_equal_counts(hip):
    field, d, rates = inputs((256, 256), 6, 11)
    field_d, table_d, rates_d = dev(field), dev(L.levels_table(d, 32)), dev(rates)
    rect = L.rectangle(0.9, FRAME, (256, 256))
    a = reach(hip, field_d, table_d, 32, rect, rates_d, 0.7)
    b = reach(hip, field_d, table_d, 32, rect, rates_d, 0.7)
    assert torch.equal(a, b) and int(a.sum()) > 0 and int(a[:, 0].sum()) < int(a[:, 32].sum())


def test_bad_arguments(hip):
    lib, s = hip.lib(), hip.current_stream()
    n, fh, fw, levels = 2, 8, 12, 4
    field = torch.zeros((n, fh, fw, 2), device="cuda")
    table = dev(L.levels_table(np.array([P.IDENTITY] * n), levels))
    rates = torch.zeros((n, 2, 4), device="cuda", dtype=torch.float64)
    counts = torch.full((n, levels + 1), -5, device="cuda", dtype=torch.int32)

    def call(field=field, n=n, fh=fh, fw=fw, table=table, levels=levels, rates=None, r=0.0, rect=(0, fh - 1, 0, fw - 1), h0=360, w0=640, margin=0,
             counts=counts):
        return lib.pws_field_reach(p(field), n, fh, fw, p(table), levels, p(rates), r, rect[0], rect[1], rect[2], rect[3], h0, w0, 0, margin, p(counts), s)
    assert call(field=None) == EINVAL and call(table=None) == EINVAL and call(counts=None) == EINVAL and b"NULL" in lib.pws_last_error()
    assert call(n=-1) == EINVAL and call(fh=1, rect=(0, 0, 0, 0)) == EINVAL and call(fw=1, rect=(0, 0, 0, 0)) == EINVAL
    assert call(h0=1) == EINVAL and call(w0=1) == EINVAL and call(margin=-1) == EINVAL
    assert call(levels=-1) == EINVAL and call(levels=65) == EINVAL and b"levels" in lib.pws_last_error()
    for rect in ((3, 2, 0, 5), (0, 5, 4, 3), (-1, 5, 0, 5), (0, fh, 0, 5), (0, 5, -1, 5), (0, 5, 0, fw)):   # empty, or leaving the lattice
        assert call(rect=rect) == EINVAL and b"rectangle" in lib.pws_last_error()
    for r in (1.5, -1.01, float("nan")):
        assert call(rates=rates, r=r) == EINVAL
    assert call(field=field.data_ptr() + 4) == EINVAL and b"aligned" in lib.pws_last_error()
    assert call(table=table.data_ptr() + 4) == EINVAL and call(rates=rates.data_ptr() + 4, r=0.5) == EINVAL
    assert call(counts=counts.data_ptr() + 2) == EINVAL
    # n = 0: nothing is launched, nothing is written (NULL pointers are fine)
    assert call(n=0) == 0 and call(n=0, field=None, table=None, counts=None) == 0
    torch.cuda.synchronize()
    assert bool((counts == -5).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((counts == 0).all())   # the identity field of zeros lies inside the frame: cleared, nothing counted
