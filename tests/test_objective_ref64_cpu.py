"""CPU tests of tests/objective_ref64.py, the float64 restatement tests/test_hip_objective_float64.py holds the objective's kernels to:
every function against torch's own float64 grid_sample / affine_grid / autograd composition and against oracle/objective_ref.py
evaluated in double, 1e-12 of each output's largest value, on small shapes that include fields leaving the frame; the guarantees of the
input builders; and the dispatch arithmetic of the launches, recomputed from the constants in the sources' text for every row of the
GPU file's case tables."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objective_ref64 as R  # noqa: E402
import test_hip_objective_float64 as G  # noqa: E402  (the case tables only; nothing of it runs here)

from oracle import objective_ref as O  # noqa: E402

TOL = 1e-12


def _close(got, want, what, mag=None):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    err, mag = float((got - want).abs().max()), float(want.abs().max()) if mag is None else mag
    assert err <= TOL * max(mag, 1e-300), (what, err, mag)


# ------------------------------------------------------------------------------------------------------------ warp + L1
@pytest.mark.parametrize("m,h,w,field", [(2, 9, 12, "builder"), (1, 2, 2, "builder"), (2, 3, 6, "builder"), (3, 16, 20, "normal"), (2, 7, 5, "wide")])
@pytest.mark.parametrize("use_t,use_g,scale,acc", [(True, True, None, False), (True, False, 0.5, False), (False, True, None, True), (True, True, 0.5, True)])
def test_warp_norm_equals_torch_float64(m, h, w, field, use_t, use_g, scale, acc):
    rs = np.random.RandomState(m * 100 + h)
    if field == "builder":
        grid = R.make_warp_field(m, h, w, 3)[0].double()
    else:   # anywhere, a good part outside the frame
        grid = torch.from_numpy(rs.standard_normal((m, h, w, 2)) * (0.8 if field == "normal" else 3.0))
    src = torch.from_numpy(rs.uniform(-1, 1, (m, 3, h, w)))
    tgt = torch.from_numpy(rs.uniform(-1, 1, (m, 3, h, w))) if use_t else None
    gex = torch.from_numpy(rs.standard_normal((m, 3, h, w))) if use_g else None
    base = torch.from_numpy(rs.standard_normal((m, h, w, 2))) if acc else None
    c_l1 = 0.7
    g = grid.clone().requires_grad_(True)
    fake = F.grid_sample((src + 1) * 127.5, g, mode="bilinear", padding_mode="zeros", align_corners=False) / 127.5 - 1
    loss = torch.zeros((), dtype=torch.float64)
    if use_t:
        loss = loss + c_l1 * (1.0 if scale is None else scale) * (tgt - fake).abs().sum()
    if use_g:
        loss = loss + (fake * gex).sum()
    loss.backward()
    out = R.warp_norm(src, grid, tgt, c_l1, scale, gex, base)
    _close(out["fake"], fake.detach(), "fake", 1.0)
    if use_t:
        _close(out["l1"], (tgt - fake).abs().sum().detach(), "l1")
        _close(out["d"], (tgt - fake).detach(), "d", 1.0)
    want = g.grad + base if acc else g.grad
    _close(out["ggrid"], want, "ggrid")
    assert float(want.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ temporal L1
@pytest.mark.parametrize("n,h,w", [(2, 16, 16), (3, 11, 14), (1, 5, 9)])
@pytest.mark.parametrize("kind", list(R.THETAS))
def test_temporal_l1_equals_torch_float64(n, h, w, kind):
    rs = np.random.RandomState(n + h)
    theta = R.make_theta(kind, n).double()
    f1, f2 = torch.from_numpy(rs.uniform(-1, 1, (n, 3, h, w))), torch.from_numpy(rs.uniform(-1, 1, (n, 3, h, w)))
    g1_0, g2_0 = torch.from_numpy(rs.standard_normal((n, 3, h, w))), torch.from_numpy(rs.standard_normal((n, 3, h, w)))
    c, scale = 0.37, 2.0
    grid = F.affine_grid(theta.view(-1, 2, 3), (n, 3, h, w), align_corners=False)
    gx, gy = R.affine_grid(theta, h, w)
    _close(torch.stack([gx, gy], -1), grid, "affine_grid")
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    o21 = F.grid_sample(b, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    s = (o21 - a).abs().sum()
    (s * c * scale).backward()
    out = R.temporal_l1(f1, f2, theta, c, scale, g1_0, g2_0)
    _close(out["o21"], o21.detach(), "o21", 1.0)
    _close(out["sum"], s.detach(), "sum")
    _close(out["gfake1"], g1_0 + a.grad, "gfake1")
    _close(out["gfake2"], g2_0 + b.grad, "gfake2")
    none = R.temporal_l1(f1, f2, theta, c)
    _close(none["gfake1"], a.grad / scale, "gfake1, no scale, nothing to add to")
    _close(none["gfake2"], b.grad / scale, "gfake2, no scale, nothing to add to")


# ------------------------------------------------------------------------------------------------------------ feature points, smoothness
def test_feat_index_is_the_kernels_rule():
    """truncation toward zero, ONE wrap of a negative index, then the clamp"""
    for size in (256, 100, 60):
        for coord in (-1.0, 0.999, -1.004, -1.02, 0.0, 0.5, -0.5, 0.96, -0.96, 1.0, -3.5, -2.9, 1.7):
            i = int((float(np.float32(coord)) + 1) * size / 2)       # Python's int() truncates toward zero
            if i < 0:
                i += size
            i = min(max(i, 0), size - 1)
            assert int(R.feat_index(torch.tensor([coord], dtype=torch.float32), size)[0]) == i, (size, coord)
    assert [int(R.feat_index(torch.tensor([c], dtype=torch.float32), 256)[0]) for c in (-1.0, 0.999, -1.004, -1.02)] == [0, 255, 0, 254]


@pytest.mark.parametrize("m,nf,size", [(3, 40, 32), (2, 9, 16), (1, 1, 8)])
def test_feature_and_smoothness_equal_the_oracle_in_double(m, nf, size):
    rs = np.random.RandomState(m + nf)
    grid = torch.from_numpy(rs.uniform(-1, 1, (m, size, size, 2)))
    feats = R.make_features(m, nf, size, size, seed=1).double()
    base = torch.from_numpy(rs.standard_normal((m, size, size, 2)))
    g = grid.clone().requires_grad_(True)
    fs, fu = feats[:, :, 0:3].permute(0, 2, 1), feats[:, :, 3:6].permute(0, 2, 1)
    zero = torch.zeros((m, 3, size, size), dtype=torch.float64)
    _, delta, feat = O.loss_calculate(g, fs, fu, zero, zero, m, size, nf)
    feat.backward()
    c, scale = 1.0 / (nf * m), 2.0
    out = R.feature_loss(grid, feats, c, scale, base)
    _close(out["sum"] * c, feat.detach(), "feature sum")
    _close(out["ggrid"], base + scale * g.grad, "feature ggrid")
    if nf >= 4:     # points that share a pixel add up
        pix = out["pixel"]
        assert all(len(set(row.tolist())) < nf for row in pix)
    s = R.field_smoothness(grid)
    _close((s["dx"] / (m * size * (size - 1) * 2) + s["dy"] / (m * (size - 1) * size * 2)) / 2, delta.detach(), "delta")
    one_row, one_col = R.field_smoothness(grid[:, :1]), R.field_smoothness(grid[:, :, :1])
    assert float(one_row["dy"]) == 0.0 and float(one_col["dx"]) == 0.0 and float(one_row["dx"]) > 0


def test_feature_loss_on_a_field_that_is_not_square():
    rs = np.random.RandomState(4)
    m, nf, h, w = 2, 30, 12, 20
    grid = torch.from_numpy(rs.uniform(-1, 1, (m, h, w, 2)))
    feats = R.make_features(m, nf, h, w, seed=2).double()
    out = R.feature_loss(grid, feats, 0.5)
    want, gg = 0.0, torch.zeros_like(grid)
    for n in range(m):
        for k in range(nf):
            ix, iy = int((float(feats[n, k, 0]) + 1) * w / 2), int((float(feats[n, k, 1]) + 1) * h / 2)
            d = feats[n, k, 3:5] - grid[n, iy, ix]                  # Python indexing wraps a negative index
            want += float((d * d).sum())
            gg[n, iy, ix] += -2 * 0.5 * d
    _close(out["sum"], want, "sum")
    _close(out["ggrid"], gg, "ggrid")


# ------------------------------------------------------------------------------------------------------------ shape loss, finalize
@pytest.mark.parametrize("m,block", [(3, 4), (2, 8), (1, 16)])
def test_shape_loss_equals_the_oracle_in_double(m, block):
    size = block * block
    _close(R.shape_basis(block), O.shape_basis(block), "basis")
    resid = R.make_shape_resid(m, size, seed=block, block=block)
    r = resid.double().requires_grad_(True)
    a = torch.from_numpy(O.shape_basis(block))
    b = r.reshape(m, block, block, block, block, 2).permute(1, 3, 0, 2, 4, 5).reshape(-1, block * block, 2)     # as loss_shape
    proj = a @ (torch.inverse(a.t() @ a) @ a.t())
    lp = torch.dist(proj @ b, b, 1)
    c, scale = 0.5, 2.0
    (lp * c * scale).backward()
    out = R.shape_loss(resid, block, c, scale)
    _close(out["sum"], lp.detach(), "sum")
    _close(out["gresid"], r.grad, "gresid")
    np.testing.assert_allclose(float(out["sum"]), float(O.loss_shape(resid, block, size)), rtol=1e-6)      # (it returns fp32)
    assert R.check_shape_resid(resid, block) > 1e-9


def test_finalize_is_the_linear_combination():
    rs = np.random.RandomState(0)
    slots, coef = rs.uniform(0, 10, (16, 64)), rs.standard_normal((6, 16))
    want = [sum(coef[j, q] * slots[q].sum() for q in range(16)) for j in range(6)]
    _close(R.finalize(torch.from_numpy(slots), torch.from_numpy(coef)), want, "finalize")


# ------------------------------------------------------------------------------------------------------------ the builders' guarantees
@pytest.mark.parametrize("m,h,w", [(2, 64, 64), (3, 70, 101), (2, 3, 6), (1, 2, 2)])
def test_warp_field_keeps_every_sample_inside_its_cell(m, h, w):
    grid, px, py = R.make_warp_field(m, h, w, seed=m + h)
    assert grid.dtype == torch.float32
    g = grid.double().numpy()
    ix, iy = ((g[..., 0] + 1) * w - 1) / 2, ((g[..., 1] + 1) * h - 1) / 2       # the fp32 field's coordinates, in double
    for coord, built in ((ix, px), (iy, py)):
        frac = coord - np.floor(coord)
        assert frac.min() >= R.FRAC_LO - 1e-3 and frac.max() <= R.FRAC_HI + 1e-3, (frac.min(), frac.max())
        assert np.array_equal(np.floor(coord), np.floor(built))                 # rounding to fp32 changed no cell
    x0, y0 = np.floor(ix).astype(int), np.floor(iy).astype(int)
    assert x0.min() <= -5 * w and (h * w < 8 or x0.max() >= 5 * w)                # the far samples (a frame of four pixels has one)
    if h * w >= 4096:
        near = (x0 >= R.INT_LO) & (x0 <= w + R.INT_PAST)
        assert x0[near].min() == -3 and x0[near].max() == w + 2
        for v in (-3, -2, -1, 0, w - 2, w - 1, w, w + 2):
            assert (x0 == v).any(), v
        for v in (-3, -1, 0, h - 1, h, h + 2):
            assert (y0 == v).any(), v
        xs = np.clip(x0, 0, w - 2)
        for sel in (-1, 0, 1):                                                   # every branch of the paired 8-byte loads
            assert ((x0 - xs) == sel).any(), sel
        taps_out = np.mean([(xx < 0) | (xx >= w) | (yy < 0) | (yy >= h) for xx in (x0, x0 + 1) for yy in (y0, y0 + 1)])
        assert 0.02 < taps_out < 0.5, taps_out                                   # the share of taps outside the frame
        assert (((x0 < -1) | (x0 >= w)) & ((y0 < -1) | (y0 >= h))).any()         # all four taps outside


@pytest.mark.parametrize("source", ["u8", "smooth"])
def test_warp_case_decides_every_l1_sign(source):
    c = R.make_warp_case(3, 32, 40, seed=1, source=source)
    src, tgt = c["frames"][:, 0:3], c["frames"][:, 3:6]
    assert c["frames"].dtype == torch.float32 and c["grid"].dtype == torch.float32
    assert float(c["d64"].abs().min()) >= 0.04
    fake32 = F.grid_sample((src + 1) * 127.5, c["grid"], align_corners=False) / 127.5 - 1
    assert torch.equal(torch.sign(tgt - fake32).double(), torch.sign(c["d64"]))          # torch-fp32's signs are float64's, on every element
    if source == "u8":
        assert set(np.unique(np.round((src.numpy() + 1) * 127.5)).tolist()) <= set(range(256))


@pytest.mark.parametrize("kind", list(R.THETAS))
def test_temporal_case_decides_every_sign(kind):
    n, h, w = 2, 16, 16
    c = R.make_temporal_case(n, h, w, kind, seed=2)
    d64 = R.temporal_l1(c["fake1"], c["fake2"], c["theta"])["d"]
    assert float(d64.abs().min()) >= 0.04
    grid = F.affine_grid(c["theta"].view(-1, 2, 3), (n, 3, h, w), align_corners=False)
    d32 = F.grid_sample(c["fake2"], grid, align_corners=False) - c["fake1"]
    assert torch.equal(torch.sign(d32).double(), torch.sign(d64))


@pytest.mark.parametrize("m,nf,h,w", [(3, 400, 256, 256), (2, 401, 60, 100), (1, 1, 256, 256)])
def test_features_are_stable_and_share_pixels(m, nf, h, w):
    f = R.make_features(m, nf, h, w, seed=3)
    assert f.dtype == torch.float32 and f.shape == (m, nf, 6)
    edges = 4 if nf >= 8 else 0
    for k, size in ((0, w), (1, h)):
        pos = (f[..., k].double().numpy() + 1) * size / 2
        body = pos.reshape(-1)[:m * nf - edges] if k == 0 else pos.reshape(-1)
        if k == 0 and edges:
            body = np.concatenate([pos[0, :nf - 4].reshape(-1), pos[1:].reshape(-1)])
        frac = body - np.floor(body)
        assert frac.min() >= R.FRAC_LO - 1e-3 and frac.max() <= R.FRAC_HI + 1e-3
        co = body * 2 / size - 1
        assert co.min() >= -0.96 - 1e-6 and co.max() <= 0.96 + 1e-6
        # the fp32 evaluation of the kernel gives the same index
        i32 = ((f[..., k] + np.float32(1)) * np.float32(size) / np.float32(2)).to(torch.int32).long()
        i32 = torch.where(i32 < 0, i32 + size, i32).clamp(0, size - 1)
        assert torch.equal(i32, R.feat_index(f[..., k], size))
    if nf >= 4:
        pix = R.feature_loss(torch.zeros((m, h, w, 2)), f)["pixel"]
        q = nf // 4
        assert torch.equal(pix[:, :q], pix[:, q:2 * q])                          # a quarter shares its pixel with another point
    if edges:
        got = [int(v) for v in R.feat_index(f[0, nf - 4:, 0], w)]
        assert got[:3] == [0, int(1.999 * w / 2), 0] and (w != 256 or got[3] == 254), got


def test_shape_resid_is_a_smooth_field_plus_noise():
    resid = R.make_shape_resid(2, 256, seed=1, block=16)
    assert resid.dtype == torch.float32 and float(resid.abs().max()) <= 0.05 + 1e-2 + 1e-6
    assert R.check_shape_resid(resid, 16) > R.SIGN_GAP == 1e-9
    # a draw that does land within 1e-9 of zero (33 samples: 4.3 M residuals) is drawn again there, and only there
    plain, fixed = R.make_shape_resid(33, 256, seed=33), R.make_shape_resid(33, 256, seed=33, block=16)
    assert float(R.shape_loss(plain, 16)["r"].abs().min()) <= R.SIGN_GAP < R.check_shape_resid(fixed, 16)
    assert 0 < int((plain != fixed).sum()) < 100
    rough = (resid[:, :, 1:] - resid[:, :, :-1]).abs().mean()
    assert 3e-3 < float(rough) < 2e-2                                            # the noise of amplitude 1e-2 is there


# ------------------------------------------------------------------------------------------------------------ dispatch arithmetic
def _holds(claim, got, what):
    for k, v in claim.items():
        assert got.get(k) == v, (what, k, v, got)


def test_constants_are_read_from_the_sources():
    k = R.source_constants()
    assert k["lanes"] == 256 and k["slots"] == 64 and k["kXcds"] == 8 and k["kLossGrid"] >= 1024


def test_case_tables_reach_the_paths_they_name():
    """nb, capped or not, nb % 8, a ragged last block, the kernel taken and g_pair of every row of the GPU file's tables, from
    kLossGrid / kXcds as the sources spell them today: if someone moves the cap, the tables stop claiming coverage they do not give."""
    k = R.source_constants()
    for shape, bwd, claim, bwd_kernel in G.WARP_CASES:
        _holds(claim, R.dispatch_warp_fwd(*shape, k=k), ("warp fwd", shape))
        assert R.dispatch_warp_bwd(*shape, k=k)["kernel"] == bwd_kernel, shape
    shapes = [r[0] for r in G.WARP_CASES]
    walks = {s: R.dispatch_warp_fwd(*s, k=k) for s in shapes if R.dispatch_warp_fwd(*s, k=k)["kernel"] != "refused"}
    assert any(d["nb"] == k["kLossGrid"] for d in walks.values()), "no row at the last uncapped block count"
    assert any(d["capped"] and d["nb"] - k["kLossGrid"] <= k["kLossGrid"] // 16 and not d["ragged"] for d in walks.values()), "no row just above the cap"
    assert any(d["capped"] and d["ragged"] and d["mod8"] != 0 for d in walks.values())
    assert any(R.dispatch_warp_bwd(*s, k=k)["kernel"] == "warp_norm_bwd_kernel" for s in shapes)
    for shape, claim in G.TEMPORAL_CASES:
        _holds(claim, R.dispatch_temporal(*shape, k=k), ("temporal", shape))
    t = [R.dispatch_temporal(*r[0], k=k) for r in G.TEMPORAL_CASES]
    assert any(d["nb"] == k["kLossGrid"] for d in t) and any(d["capped"] and d["ragged"] and d["mod8"] != 0 for d in t)
    assert any(d["g_pair"] == 1 and d["wave_spans_rows"] for d in t) and any(d["g_pair"] == 0 and d["ragged"] for d in t)
    for shape, one_pixel, claim in G.SMOOTH_CASES:
        _holds(claim, R.dispatch_smooth(*shape, one_pixel=one_pixel, k=k), ("smoothness", shape, one_pixel))
    s = [R.dispatch_smooth(*r[0], one_pixel=r[1], k=k) for r in G.SMOOTH_CASES]
    for kernel in ("field_smoothness4_kernel", "field_smoothness_kernel"):
        assert any(d["kernel"] == kernel and d["capped"] and d["ragged"] for d in s), kernel
    assert any(d["nb"] == k["kLossGrid"] for d in s)
    for shape, general, claim in G.SHAPE_CASES:
        _holds(claim, R.dispatch_shape(*shape, general=general, k=k), ("shape", shape, general))
    w = [R.dispatch_shape(*r[0], general=r[1], k=k) for r in G.SHAPE_CASES]
    assert any(d["kernel"] == "shape_loss16_kernel" and not d["capped"] and d["grid"] == k["kLossGrid"] for d in w)
    assert any(d["kernel"] == "shape_loss16_kernel" and d["capped"] and d["nb"] < 2 * d["waves"] and d["nb"] % d["waves"] != 0 for d in w)
    assert any(d["kernel"] == "shape_loss_kernel" and d["live"] < d["threads"] for d in w)
    for shape, field, claim in G.FEATURE_CASES:
        _holds(claim, R.dispatch_feature(*shape, k=k), ("feature", shape))
    # every temporal row the GPU file runs is one of the table's shapes or a tiles' shape; the gather's limits hold
    for n, h, w_, kind, modes in G.temporal_rows():
        assert (n, h, w_) in [r[0] for r in G.TEMPORAL_CASES] + G.TEMPORAL_TILED + [(2, 16, 16)]
        if kind == "degenerate":
            assert modes == ("det",) and (h, w_) == (16, 16)
        if "det" in modes and max(h, w_) > 64:
            assert kind == "near identity"


def test_the_composite_batch_is_the_smallest_that_caps_every_launch():
    k = R.source_constants()

    def all_capped(n):
        m = 2 * n
        return (R.dispatch_warp_fwd(m, 256, 256, k=k)["capped"] and R.dispatch_temporal(n, 256, 256, k=k)["capped"]
                and R.dispatch_smooth(m, 256, 256, k=k)["capped"] and R.dispatch_shape(m, 256, 16, k=k)["capped"])
    assert all_capped(17) and not all_capped(16)
