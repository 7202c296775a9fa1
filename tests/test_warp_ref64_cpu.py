"""CPU tests of tests/warp_ref64.py, which tests/test_hip_warp_float64.py holds the fp32 warp kernels to:

  - the dispatch arithmetic, recomputed from the thresholds in the sources' text, for every row of the GPU file's case tables: each
    row reaches the kernel its comment names, the streaming rows sit on both sides of their thresholds, and a changed threshold
    breaks the claims;
  - the exactness claim: on every exact shape (at a CPU-sized batch) torch's fp32 forward and backward EQUAL torch's float64 and the
    float64 results are representable in fp32, so a bound of zero holds for the reference alone; the same for the exact resize and
    affine_grid cases;
  - the restated float64 functions against torch's float64 operators and autograd;
  - what the builders promise."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_ref64 as W  # noqa: E402
import test_hip_warp_float64 as G  # noqa: E402  (the case tables only; nothing of it runs here)
from pwstablenet_amd.hipabi import Exp  # noqa: E402

K = W.source_constants()
TOL = 1e-12


def _holds(got, claim, what):
    for key, want in claim.items():
        assert got[key] == want, (what, key, got[key], want)


def _representable(t):
    return bool((t.float().double() == t).all())


# ------------------------------------------------------------------------------------------------------------ dispatch
def test_thresholds_are_read_from_the_sources():
    assert K["fwd"] == ("(8.0 + 8.0 * c)", 256e6) and K["bwd"] == ("(16.0 + 8.0 * c)", 256e6) and K["fused"] == ("8.0 * c", 256e6)
    assert K["narrow"] == (np.float32(3), np.float32(0.999)) and K["kXcds"] == 8


@pytest.mark.parametrize("row,claim,bwd_kernel", G.EXACT_ROWS, ids=[G._x(r[0]) for r in G.EXACT_ROWS])
def test_exact_rows_reach_their_kernels(row, claim, bwd_kernel):
    n, c, h, w, ho, wo, _ = row
    _holds(W.dispatch_fwd(n, c, h, w, ho, wo, k=K), dict(claim, streaming=False), row)
    assert W.dispatch_bwd(n, c, h, w, ho, wo, ginput=False, k=K)["kernel"] == bwd_kernel
    assert W.dispatch_bwd(n, c, h, w, ho, wo, ginput=True, k=K)["kernel"] == G.GENERAL


def test_exact_table_is_the_issue_s():
    assert [r[0] for r in G.EXACT_ROWS] == [(2, 3, 64, 64, 64, 64, 0), (5, 3, 32, 32, 36, 52, 0), (3, 1, 16, 32, 5, 7, 0), (2, 3, 65, 257, 64, 64, 1),
                                            (2, 3, 65, 257, 5, 7, 1), (2, 3, 4, 2, 8, 8, 0), (2, 3, 8, 1, 4, 4, 0), (2, 3, 8, 1, 3, 3, 0), (2, 31, 8, 8, 16, 16, 0)]
    assert 5 * 36 * 52 // 4 == 2340


def test_alignment_and_experiment_rows_reach_their_kernels():
    n, c, h, w, ho, wo, _ = G.BASE_ROW
    assert W.dispatch_fwd(n, c, h, w, ho, wo, aligned=False, k=K)["kernel"] == G.UNALIGNED_CLAIM["fwd"]
    assert W.dispatch_bwd(n, c, h, w, ho, wo, ginput=False, aligned=False, k=K)["kernel"] == G.UNALIGNED_CLAIM["bwd_field_only"]
    for row, fwd, bwd in G.EXPERIMENT_ROWS:
        n, c, h, w, ho, wo, _ = row
        assert (ho, wo) == (64, 64)
        assert W.dispatch_fwd(n, c, h, w, ho, wo, exp=int(Exp.GS_ROWWIN), k=K)["kernel"] == fwd
        assert W.dispatch_bwd(n, c, h, w, ho, wo, ginput=False, exp=int(Exp.GS_BWD_GENERAL), k=K)["kernel"] == bwd


def test_streaming_rows_sit_on_both_sides_of_their_thresholds():
    c, h, w = G.STREAM_SHAPE
    assert [r[0] for r in G.STREAM_FWD] == [122, 123] and [r[0] for r in G.STREAM_BWD] == [97, 98] and [r[0] for r in G.FUSED_STREAM] == [11, 12]
    assert G.STREAM_N == 123
    for n, claim in G.STREAM_FWD:
        _holds(W.dispatch_fwd(n, c, h, w, h, w, k=K), claim, ("fwd", n))
    for n, claim in G.STREAM_BWD:
        _holds(W.dispatch_bwd(n, c, h, w, h, w, ginput=False, k=K), claim, ("bwd", n))
    (fh, fw), (fr_h, fr_w) = G.FUSED_720P
    for n, claim in G.FUSED_STREAM:
        _holds(W.dispatch_fused(n, 3, fr_h, fr_w, fh, fw, k=K), claim, ("fused", n))
    # the comparison runs of the streaming tests are never non-temporal, and the general backward never is
    general = int(Exp.GS_BWD_GENERAL)
    assert W.dispatch_fwd(123, c, h, w, h, w, exp=general, k=K)["kernel"] == G.FWD4
    assert W.dispatch_bwd(98, c, h, w, h, w, ginput=False, exp=general, k=K)["kernel"] == G.GENERAL
    assert W.dispatch_bwd(123, c, h, w, h, w, ginput=True, k=K) == dict(W._walk(123 * h * w, K), kernel=G.GENERAL, ppt=1, streaming=False)
    assert W.dispatch_fused(12, 3, fr_h, fr_w, fh, fw, exp=general, k=K)["kernel"] == G.NARROW


@pytest.mark.parametrize("which,table", [("fwd", "STREAM_FWD"), ("bwd", "STREAM_BWD"), ("fused", "FUSED_STREAM")])
def test_a_changed_threshold_breaks_the_claims(which, table):
    """the tables are tied to the constants: with any of the three limits moved by 10 % (a 720p frame is 8.6 % of the fused limit), a streaming row is on the wrong side"""
    c, h, w = G.STREAM_SHAPE
    (fh, fw), (fr_h, fr_w) = G.FUSED_720P
    for factor in (0.9, 1.1):
        k = dict(K)
        k[which] = (K[which][0], K[which][1] * factor)
        got = []
        for n, claim in getattr(G, table):
            d = {"fwd": lambda: W.dispatch_fwd(n, c, h, w, h, w, k=k), "bwd": lambda: W.dispatch_bwd(n, c, h, w, h, w, ginput=False, k=k),
                 "fused": lambda: W.dispatch_fused(n, 3, fr_h, fr_w, fh, fw, k=k)}[which]()
            got.append(d["streaming"] == claim["streaming"])
        assert not all(got), (which, factor)


@pytest.mark.parametrize("row,fwd,bwd", G.GENERAL_ROWS, ids=[G._x(r[0]) for r in G.GENERAL_ROWS])
def test_general_rows_reach_their_kernels(row, fwd, bwd):
    n, c, h, w, ho, wo = row
    assert W.dispatch_fwd(n, c, h, w, ho, wo, k=K)["kernel"] == fwd
    assert W.dispatch_bwd(n, c, h, w, ho, wo, ginput=False, k=K)["kernel"] == bwd
    assert not (W._pow2(h) and W._pow2(w))     # no exact builder for these with align_corners=False; the general fields' fractions are not dyadic in either convention
    assert [r[0] for r in G.GENERAL_ROWS] == [(1, 3, 37, 53, 37, 53), (2, 1, 40, 52, 24, 36), (3, 3, 17, 33, 8, 10)]


@pytest.mark.parametrize("row,claim", G.FUSED_ROWS + [G.FUSED_EXACT], ids=[str(r[0]) for r in G.FUSED_ROWS + [G.FUSED_EXACT]])
def test_fused_rows_reach_their_kernels(row, claim):
    n, (fh, fw), (h, w), off = row
    d = W.dispatch_fused(n, 3, h, w, fh, fw, aligned=not off, k=K)
    assert d["kernel"] == claim["kernel"] and not d["streaming"]
    three_rx = float(np.float32(3) * W.fused_rx(w, fw))
    assert abs(three_rx - claim["three_rx"]) < 1e-6, three_rx
    if claim["kernel"] == G.NARROW:
        assert three_rx < 0.999


def test_tightest_narrow_geometry():
    """no frame width up to 4096 with a field up to 512 wide comes closer to the NARROW limit from below than 5 x 331 -> 8 x 992 does
    by more than 1e-5"""
    limit = float(K["narrow"][1])
    got = float(np.float32(3) * W.fused_rx(992, 331))
    assert got < limit and limit - got < 1e-5, got


def test_every_kernel_of_the_family_is_reached():
    reached = {c["kernel"] for _, c, _ in G.EXACT_ROWS} | {b for _, _, b in G.EXACT_ROWS} | {c["kernel"] for _, c in G.STREAM_FWD + G.STREAM_BWD + G.FUSED_STREAM}
    reached |= {c["kernel"] for _, c in G.FUSED_ROWS} | {G.FUSED_EXACT[1]["kernel"]}
    want = {"grid_sample_fwd2_kernel<4, false>", "grid_sample_fwd2_kernel<4, true>", "grid_sample_fwd2_kernel<1, false>", "grid_sample_fwd_kernel<4>",
            "grid_sample_fwd_kernel<1>", "grid_sample_bwd_field_kernel<false>", "grid_sample_bwd_field_kernel<true>", "grid_sample_bwd_kernel",
            "upsample_grid_sample_fwd_kernel<4, true, true>", "upsample_grid_sample_fwd_kernel<4, true, false>",
            "upsample_grid_sample_fwd_kernel<4, false, false>", "upsample_grid_sample_fwd_kernel<1, false, false>"}
    assert want <= reached, want - reached
    with open(os.path.join(W.ROOT, "pwstablenet_amd/csrc/grid_sample.hip")) as f:
        text = f.read()
    for name in want:   # every claimed instantiation is one the entry points launch
        base, _, args = name.partition("<")
        assert (base + ("<" + args if args else ",")).replace(" ", "") in text.replace(" ", ""), name


# ------------------------------------------------------------------------------------------------------------ the exactness claim
EXACT_CPU = sorted({(min(r[0][0], 3),) + r[0][1:] for r in G.EXACT_ROWS} | {(1, 3, 256, 256, 256, 256, 0), (2, 3, 64, 64, 64, 64, 0)})


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("row", EXACT_CPU, ids=G._x)
def test_torch_fp32_equals_float64_on_exact_cases(row, kind):
    """the bound of zero holds for the reference alone: fp32 == float64, and the float64 results are fp32 numbers"""
    n, c, h, w, ho, wo, ac = row
    img, grid, gout = W.exact_frames((n, c, h, w), 1), W.exact_field(n, ho, wo, h, w, ac, kind, 2), W.exact_grads((n, c, ho, wo), 3)
    r64 = W.grid_sample64(img, grid, gout, ac)
    r32 = W.grid_sample32(img, grid, gout, ac)
    for key in ("out", "ginput", "ggrid"):
        assert _representable(r64[key]), key
        assert bool((r32[key].double() == r64[key]).all()), key
        assert float(r64[key].abs().max()) > 0, key
    as32 = W.grid_sample64(img, grid, gout, ac, exact=True, chunk=1)     # the form the GPU tests use: chunked, asserted, stored as fp32
    for key in ("out", "ginput", "ggrid"):
        assert as32[key].dtype == torch.float32 and bool((as32[key].double() == r64[key]).all()), key


@pytest.mark.parametrize("src,dst", G.RESIZE_EXACT, ids=lambda s: G._x(s))
def test_torch_fp32_equals_float64_on_exact_resizes(src, dst):
    (h, w), (ho, wo) = src, dst
    assert W.resize_is_exact(h, w, ho, wo)
    x, gout = W.exact_grads((2, 3, h, w), 4), W.exact_grads((2, 3, ho, wo), 5)
    o64, g64 = W.resize(x, ho, wo, gout)
    o32, g32 = W.resize(x, ho, wo, gout, torch.float32)
    assert _representable(o64) and _representable(g64)
    assert bool((o32.double() == o64).all()) and bool((g32.double() == g64).all())
    assert not W.resize_is_exact(5, 7, 11, 9) and not W.resize_is_exact(256, 256, 720, 1280)


@pytest.mark.parametrize("n,h,w,ac", G.AFFINE_BWD_EXACT, ids=lambda v: str(v))
def test_fp32_equals_float64_on_exact_affine_grids(n, h, w, ac):
    """The base coordinates are dyadic, so the grid is representable and an fp32 evaluation of the same formula (numpy, one operation at
    a time) equals it; the adjoint's double sum of integers times dyadic coordinates is exact in any order.  torch's own affine_grid is
    NOT the yardstick here: it scales a linspace, whose steps are rounded (2 / 15 at w = 16), in either precision -- see
    test_affine_grid64_equals_torch_float64 for how close the two are."""
    theta, ggrid = W.exact_theta(n, 6), W.exact_grads((n, h, w, 2), 7)
    g64 = W.affine_grid64(theta, h, w, ac)
    assert _representable(g64)
    f = np.float32
    bx = (f(2) * np.arange(w, dtype=f)) / f(w - 1) - f(1) if ac else (f(2) * np.arange(w, dtype=f) + f(1)) / f(w) - f(1)
    by = (f(2) * np.arange(h, dtype=f)) / f(h - 1) - f(1) if ac else (f(2) * np.arange(h, dtype=f) + f(1)) / f(h) - f(1)
    t = theta.numpy().reshape(n, 6, 1, 1)
    gx = t[:, 0] * bx.reshape(1, 1, w) + t[:, 1] * by.reshape(1, h, 1) + t[:, 2]
    gy = t[:, 3] * bx.reshape(1, 1, w) + t[:, 4] * by.reshape(1, h, 1) + t[:, 5]
    assert gx.dtype == np.float32
    assert np.array_equal(np.stack([gx, gy], -1).astype(np.float64), g64.numpy())
    if ac and _representable(torch.linspace(-1, 1, w, dtype=torch.float64)) and _representable(torch.linspace(-1, 1, h, dtype=torch.float64)):
        for dt in (torch.float32, torch.float64):     # where its linspace is dyadic too (17 x 33), torch's operator gives the same numbers in both precisions
            assert bool((F.affine_grid(theta.to(dt).reshape(n, 2, 3), (n, 1, h, w), align_corners=True).double() == g64).all()), dt
    gt = W.affine_grid_bwd64(ggrid, ac)
    flipped = W.affine_grid_bwd64(ggrid.flip(1, 2), ac)     # another order of the same sum
    sign = torch.tensor([-1.0, -1.0, 1.0, -1.0, -1.0, 1.0], dtype=torch.float64)
    assert bool((flipped == gt * sign).all())               # (the base coordinates are antisymmetric: x -> -x, y -> -y)
    assert float(gt.abs().max()) < 2.0 ** 24                # far inside what a double sum of such terms holds exactly


# ------------------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("n,h,w", [(2, 16, 32), (3, 17, 33), (2, 33, 65), (1, 2, 5)])
def test_affine_grid64_equals_torch_float64(n, h, w, ac):
    rs = np.random.RandomState(h + ac)
    theta, ggrid = torch.from_numpy(rs.standard_normal((n, 6))), torch.from_numpy(rs.standard_normal((n, h, w, 2)))
    th = theta.reshape(n, 2, 3).clone().requires_grad_(True)
    g = F.affine_grid(th, (n, 1, h, w), align_corners=bool(ac))
    g.backward(ggrid)
    mine = W.affine_grid64(theta, h, w, ac)
    assert float((mine - g.detach()).abs().max()) <= TOL * float(g.detach().abs().max())
    gt = W.affine_grid_bwd64(ggrid, ac)
    assert float((gt - th.grad.reshape(n, 6)).abs().max()) <= TOL * float(ggrid.abs().sum((1, 2, 3)).max())


@pytest.mark.parametrize("ac", [0, 1])
def test_chunked_grid_sample64_equals_torch_float64(ac):
    n, c, h, w, ho, wo = 5, 2, 9, 12, 7, 10
    rs = np.random.RandomState(9 + ac)
    img, gout = torch.from_numpy(rs.standard_normal((n, c, h, w))), torch.from_numpy(rs.standard_normal((n, c, ho, wo)))
    grid = W.general_field(n, ho, wo, h, w, ac, 3)
    i, g = img.clone().requires_grad_(True), grid.double().requires_grad_(True)
    o = F.grid_sample(i, g, mode="bilinear", padding_mode="zeros", align_corners=bool(ac))
    o.backward(gout)
    got = W.grid_sample64(img, grid, gout, ac, chunk=2)
    assert torch.equal(got["out"], o.detach()) and torch.equal(got["ginput"], i.grad) and torch.equal(got["ggrid"], g.grad)
    only = W.grid_sample64(img, grid, gout, ac, need=("ggrid",), chunk=3)
    assert list(only) == ["ggrid"] and torch.equal(only["ggrid"], g.grad)


@pytest.mark.parametrize("ac", [0, 1])
def test_fused_is_the_composition(ac):
    n, fh, fw, h, w = 2, 6, 7, 10, 13
    img, field = W.exact_frames((n, 3, h, w), 1).double(), W.fused_field(n, fh, fw, h, w, "stabiliser", 2).double()
    up = torch.nn.UpsamplingBilinear2d(size=(h, w))(field.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    want = F.grid_sample(img, up, mode="bilinear", padding_mode="zeros", align_corners=bool(ac))
    assert torch.equal(W.fused(img, field, ac), want)
    assert W.fused(img, field, ac, torch.float32).dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------ builders
def _pixels(grid, h, w, ac):
    g = grid.double()
    if ac:
        return (g[..., 0] + 1) * 0.5 * (w - 1), (g[..., 1] + 1) * 0.5 * (h - 1)
    return ((g[..., 0] + 1) * w - 1) * 0.5, ((g[..., 1] + 1) * h - 1) * 0.5


@pytest.mark.parametrize("m,ho,wo,h,w,ac", [(2, 8, 8, 16, 32, 0), (3, 5, 7, 17, 33, 1), (2, 4, 4, 8, 1, 0), (1, 64, 64, 64, 64, 0)])
def test_exact_scatter_field(m, ho, wo, h, w, ac):
    px, py = _pixels(W.exact_field(m, ho, wo, h, w, ac, "scatter", 11), h, w, ac)
    for p in (px, py):
        k = (p - torch.floor(p)) * 64
        assert bool((k == torch.round(k)).all()) and float(k.min()) >= 7 and float(k.max()) <= 57
    far = min(8, ho * wo // 4)
    x0, y0 = torch.floor(px).long(), torch.floor(py).long()
    corners = [(-1, -1), (w - 1, h - 1), (0, 0), (-1, h - 1), (w - 1, -1), (0, -1)][:ho * wo - far]
    for k, (cx, cy) in enumerate(corners):
        assert (int(x0[0].reshape(-1)[-1 - k]), int(y0[0].reshape(-1)[-1 - k])) == (cx, cy)
    fx = x0[m - 1].reshape(-1)[:far]
    assert all(int(v) in (-5 * w, 6 * w) for v in fx)
    body = x0.reshape(m, -1)[:m - 1] if m > 1 else x0.reshape(m, -1)[:, far:]     # (the last sample's first pixels are the far ones)
    assert int(body.min()) >= -3 and int(body.max()) <= w + 2


def test_exact_smooth_field_reads_consecutive_columns_of_one_row_pair():
    m, ho, wo, h, w = 2, 64, 64, 64, 64
    px, py = _pixels(W.exact_field(m, ho, wo, h, w, 0, "smooth", 12), h, w, 0)
    assert bool((px[:, :, 1:] - px[:, :, :-1] == 1).all()) and bool((py[:, :, 1:] == py[:, :, :-1]).all())
    shift = px[:, :, 0]
    assert float(shift.abs().max()) <= 2 and bool(((shift * 64) == torch.round(shift * 64)).all()) and len(torch.unique(shift)) > 8


def test_exact_field_refuses_sizes_that_are_not_exact():
    for h, w, ac in ((37, 53, 0), (64, 64, 1), (65, 257, 0), (16, 33, 1)):
        with pytest.raises(ValueError):
            W.exact_field(1, 4, 4, h, w, ac, "scatter", 0)
    frames, grads = W.exact_frames((2, 3, 8, 8), 1), W.exact_grads((2, 3, 8, 8), 2)
    assert frames.dtype == torch.float32 and float(frames.min()) >= 0 and float(frames.max()) <= 255 and bool((frames == frames.round()).all())
    assert float(grads.min()) >= -8 and float(grads.max()) <= 8 and bool((grads == grads.round()).all())


@pytest.mark.parametrize("ac", [0, 1])
def test_general_field_keeps_its_distance(ac):
    for n, c, h, w, ho, wo in [r[0] for r in G.GENERAL_ROWS]:
        px, py = _pixels(W.general_field(n, ho, wo, h, w, ac, 5), h, w, ac)
        for p in (px, py):
            fr = p - torch.floor(p)
            assert float(fr.min()) > 0.09 and float(fr.max()) < 0.91
        assert float(px.min()) < -4 * w and float(px.max()) > w       # far outside, and past the right edge


def test_fused_fields():
    for h, w in ((12, 48), (720, 1280)):
        st = W.fused_field(2, 16, 16, h, w, "stabiliser", 1).double()
        ident = torch.stack(torch.meshgrid(torch.linspace(-1, 1, 16, dtype=torch.float64), torch.linspace(-1, 1, 16, dtype=torch.float64), indexing="ij")[::-1], -1)
        assert float((st - ident).abs().max()) < 0.15 + 4.0 / min(h, w) + 1e-6
        lv = W.fused_field(2, 16, 16, h, w, "leaves", 1)
        assert float(lv[..., 0].min()) < -1 and float(lv[..., 0].max()) > 1 and float(lv[..., 1].min()) < -1 and float(lv[..., 1].max()) > 1


def test_offset8_is_8_byte_aligned_only():
    t = W.offset8((2, 3, 4), "cpu", 1.5)
    assert t.data_ptr() % 16 == 8 and t.is_contiguous() and float(t.sum()) == 36.0
