"""GPU tests of the bicubic fused warp (csrc/warp_bicubic.hip; functional.upsample_grid_sample*(mode="bicubic"), VideoStabilizer(interpolation=
"bicubic")) against the float64 restatement tests/bicubic_ref.py, which tests/test_bicubic_ref_cpu.py pins to torch-CPU float64.

Shapes are the smallest that reach every path of the kernels: 6 x 8 (one lane pair per row; chroma planes of 3 rows, fewer than the 4-row
footprint), 38 x 52 (rows that are no multiple of the 4-row group), 18 x 260 (260 crosses the 256-pixel chunk with a one-lane tail; chroma rows
of 130 = 2 mod 4 samples), 1 and 3 samples (the narrow loads at the buffer's end are taken in the last sample only), fields of 5 x 7 and 16 x 16
(field access per pixel and through the wave), and one 288 x 320 case with a 256 x 256 field.

Acceptance of the integer formats is the bilinear byte paths' (yuv16_ref.accept): never more than 1 LSB off, off only where the exact clamped
value lies within 0.05 of an integer, at most 6 % of the samples off.  The band holds at these sizes by derivation: an fp32 coordinate of a plane
<= 320 wide is good to ~1e-4 pixels, the cubic's slope is <= ~3 sample ranges per pixel, so <= 0.08 LSB of 8 bits on random bytes and far less
on the smooth frames used here; random bytes serve only where the result is exact (integer coordinates, everything outside)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bicubic_ref as B  # noqa: E402
import yuv16_ref as R16  # noqa: E402
import yuv_ref as R  # noqa: E402

from pwstablenet_amd import synth  # noqa: E402

SHAPES = [(6, 8), (38, 52), (18, 260)]
FIELD_SIZES = [(5, 7), (16, 16)]
CASES = ["identity", "zoom_in", "zoom_out", "smooth"]
FMTS8, FMTS16 = ["nv12", "i420"], ["p010", "i010"]
PAD8, PAD16 = (16, 128), (64, 512)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def field_case(case, n, fh, fw, seed):
    if case == "identity":   # (exact only at a plane's own power-of-two size: test_exact_identity; here a smooth near-identity)
        return B.affine_field(n, fh, fw)
    if case == "zoom_in":    # every 4 x 4 footprint inside every plane
        return B.affine_field(n, fh, fw, scale=0.45, noise=0.002, seed=seed)
    if case == "zoom_out":   # footprints that straddle every edge, and a band of pixels with all 16 taps outside
        return B.affine_field(n, fh, fw, scale=1.3, shift=(1.5, -1.4))
    if fh == fw:
        return R16.smooth_field(n, seed, size=fh)
    return B.affine_field(n, fh, fw, scale=1.02, shift=(0.01, 0.02), noise=0.01, seed=seed)


def smooth_bgr(n, h, w, seed):
    """(n, h, w, 3) uint8: three smooth planes (yuv_ref.random_yuv's Y) as the channels."""
    return np.stack([R.unpack(R.random_yuv(n, h + h % 2, w, "i420", seed=seed + 7 * k), "i420")[0][:, :h] for k in range(3)], -1)


def accept(got, ref, ref_f, vmax, fmt="i010"):
    """yuv16_ref.accept on the clamped exact value (8-bit words pass as "i010": samples = the words themselves)."""
    return R16.accept(got, ref, np.clip(ref_f, 0, vmax), fmt)


def configs():
    for n in (1, 3):
        for fsize in FIELD_SIZES:
            for ac in (False, True):
                yield n, fsize, ac


def check_case(case, field, planes_hw, ac):
    """The field case is what its name says, on every plane size it is applied to."""
    for h, w in planes_hw:
        out = B.all_outside(field, h, w, ac)
        if case == "zoom_in":
            ix, iy = B.coordinates(field, h, w, ac)
            assert (np.floor(ix) >= 1).all() and (np.floor(ix) + 2 <= w - 1).all() and (np.floor(iy) >= 1).all() and (np.floor(iy) + 2 <= h - 1).all()
        elif case == "zoom_out":
            assert 0.05 < out.mean() < 0.97, out.mean()
        else:
            assert not out.all()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("hw", SHAPES)
def test_bgr(hip, hw, case):
    from pwstablenet_amd import functional as PF
    h, w = hw
    worst = 0.0
    for n, (fh, fw), ac in configs():
        f, field = smooth_bgr(n, h, w, seed=h + n), field_case(case, n, fh, fw, seed=w + n)
        check_case(case, field, [(h, w)], ac)
        for swap in (False, True):
            got = PF.upsample_grid_sample_u8(dev(f), dev(field), swap_rb=swap, align_corners=ac, mode="bicubic")
            assert got.dtype == torch.uint8 and tuple(got.shape) == f.shape
            got = got.cpu().numpy()
            ref, ref_f = B.warp_bgr(f, field, ac, swap)
            worst = max(worst, accept(got, ref, ref_f, 255))
            out = B.all_outside(field, h, w, ac)
            assert (got[out] == 0).all()
    print("bgr %s %s: largest share of samples 1 LSB off %.2e" % (hw, case, worst))


@pytest.mark.parametrize("fmt", FMTS8 + FMTS16)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("hw", SHAPES)
def test_yuv(hip, hw, case, fmt):
    from pwstablenet_amd import functional as PF
    h, w = hw
    deep = fmt in FMTS16
    worst = 0.0
    for n, (fh, fw), ac in configs():
        field = field_case(case, n, fh, fw, seed=w + n)
        check_case(case, field, [(h, w), (h // 2, w // 2)] if case != "zoom_in" else [(h, w)], ac)
        if deep:
            f = R16.random_yuv16(n, h, w, fmt, seed=h + n)
            if fmt == "p010":   # junk in the low 6 bits of every word is ignored and does not reach the output
                f = f | np.random.RandomState(h).randint(0, 64, f.shape).astype(np.uint16)
            got = PF.upsample_grid_sample_yuv420_16(dev(f), dev(field), fmt, align_corners=ac, mode="bicubic")
            ref, ref_f = B.warp_yuv16(f, field, fmt, ac)
        else:
            f = R.random_yuv(n, h, w, fmt, seed=h + n)
            got = PF.upsample_grid_sample_yuv420(dev(f), dev(field), fmt, align_corners=ac, mode="bicubic")
            ref, ref_f = B.warp_yuv(f, field, fmt, ac)
        assert got.dtype == (torch.uint16 if deep else torch.uint8) and tuple(got.shape) == f.shape
        got = got.cpu().numpy()
        worst = max(worst, accept(got, ref, ref_f, 1023 if deep else 255, fmt if deep else "i010"))
        out = B.outside_yuv(field, h, w, fmt in ("nv12", "p010"), ac)
        py, pc = PAD16 if deep else PAD8
        black = np.concatenate([np.full((n, h, w), py), np.full((n, h // 2, w), pc)], 1)
        placed = R16.place(black, fmt) if deep else black
        assert (got[out] == placed[out]).all()
        if fmt == "p010":
            assert (got & 63 == 0).all()
        elif fmt == "i010":
            assert got.max() <= 1023
    print("%s %s %s: largest share of samples 1 LSB off %.2e" % (fmt, hw, case, worst))


@pytest.mark.parametrize("hw", SHAPES)
def test_everything_outside_is_pad_exactly(hip, hw):
    """A shift of +-3e4: every tap of every pixel is outside, on random bytes; huge coordinates are safe because tap addresses are clamped."""
    from pwstablenet_amd import functional as PF
    h, w = hw
    rs = np.random.RandomState(h)
    for n, (fh, fw), ac in configs():
        for shift in (3e4, -3e4):
            field = dev(B.affine_field(n, fh, fw, shift=(shift, -shift)))
            got = PF.upsample_grid_sample_u8(dev(rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)), field, align_corners=ac, mode="bicubic")
            assert int(got.max()) == 0
            x = torch.from_numpy(rs.uniform(0, 255, (n, 3, h, w)).astype(np.float32)).cuda()
            assert float(PF.upsample_grid_sample(x, field, align_corners=ac, mode="bicubic").abs().max()) == 0.0
            for fmt in FMTS8:
                got = PF.upsample_grid_sample_yuv420(dev(R.random_yuv(n, h, w, fmt, seed=h, smooth=False)), field, fmt, align_corners=ac, mode="bicubic")
                got = got.cpu().numpy()
                assert (got[:, :h] == 16).all() and (got[:, h:] == 128).all()
            for fmt in FMTS16:
                got = PF.upsample_grid_sample_yuv420_16(dev(R16.random_yuv16(n, h, w, fmt, seed=h, smooth=False)), field, fmt, align_corners=ac,
                                                        mode="bicubic").cpu().numpy()
                assert np.array_equal(got[:, :h], R16.place(np.full((n, h, w), 64), fmt))
                assert np.array_equal(got[:, h:], R16.place(np.full((n, h // 2, w), 512), fmt))


@pytest.mark.parametrize("hw", [(8, 16), (32, 512)])
def test_exact_identity(hip, hw):
    """A field at the plane's own power-of-two size (align_corners=False) has exact integer coordinates: t = 0, the weights are (0, 1, 0, 0),
    and the plane comes back byte for byte, on random bytes.  The chroma planes of a 4:2:0 frame get their own run, with the field at
    THEIR size (the luma plane's field resized to them is not exact)."""
    from pwstablenet_amd import functional as PF
    h, w = hw
    rs = np.random.RandomState(w)
    for n in (1, 3):
        fy, fc = dev(B.affine_field(n, h, w)), dev(B.affine_field(n, h // 2, w // 2))
        f = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
        assert np.array_equal(PF.upsample_grid_sample_u8(dev(f), fy, mode="bicubic").cpu().numpy(), f)
        assert np.array_equal(PF.upsample_grid_sample_u8(dev(f), fy, swap_rb=True, mode="bicubic").cpu().numpy(), f[..., ::-1])
        x = torch.from_numpy(rs.uniform(-300, 300, (n, 3, h, w)).astype(np.float32)).cuda()
        assert torch.equal(PF.upsample_grid_sample(x, fy, mode="bicubic"), x)
        for fmt in FMTS8:
            f = R.random_yuv(n, h, w, fmt, seed=w + n, smooth=False)
            assert np.array_equal(PF.upsample_grid_sample_yuv420(dev(f), fy, fmt, mode="bicubic").cpu().numpy()[:, :h], f[:, :h])
            assert np.array_equal(PF.upsample_grid_sample_yuv420(dev(f), fc, fmt, mode="bicubic").cpu().numpy()[:, h:], f[:, h:])
        for fmt in FMTS16:
            f = R16.random_yuv16(n, h, w, fmt, seed=w + n, smooth=False)   # any 16-bit words
            want = R16.place(R16.samples(f, fmt), fmt)   # P010's low bits come out zero, I010 words above 1023 come out 1023
            assert np.array_equal(PF.upsample_grid_sample_yuv420_16(dev(f), fy, fmt, mode="bicubic").cpu().numpy()[:, :h], want[:, :h])
            assert np.array_equal(PF.upsample_grid_sample_yuv420_16(dev(f), fc, fmt, mode="bicubic").cpu().numpy()[:, h:], want[:, h:])


@pytest.mark.parametrize("ac", [False, True])
def test_288x320_with_a_256x256_field(hip, ac):
    """The stabiliser's geometry in small: a 256 x 256 field (yuv16_ref.smooth_field: zooms out a little, with white noise) on 288 x 320 frames,
    every format."""
    from pwstablenet_amd import functional as PF
    n, h, w = 2, 288, 320
    field = R16.smooth_field(n, seed=5)
    fd = dev(field)
    f = smooth_bgr(n, h, w, seed=1)
    for swap in (False, True):
        got = PF.upsample_grid_sample_u8(dev(f), fd, swap_rb=swap, align_corners=ac, mode="bicubic").cpu().numpy()
        print("bgr swap=%s ac=%s: share 1 LSB off %.2e" % (swap, ac, accept(got, *B.warp_bgr(f, field, ac, swap), 255)))
    for fmt in FMTS8:
        f = R.random_yuv(n, h, w, fmt, seed=2)
        got = PF.upsample_grid_sample_yuv420(dev(f), fd, fmt, align_corners=ac, mode="bicubic").cpu().numpy()
        print("%s ac=%s: share 1 LSB off %.2e" % (fmt, ac, accept(got, *B.warp_yuv(f, field, fmt, ac), 255)))
    for fmt in FMTS16:
        f = R16.random_yuv16(n, h, w, fmt, seed=3)
        got = PF.upsample_grid_sample_yuv420_16(dev(f), fd, fmt, align_corners=ac, mode="bicubic").cpu().numpy()
        print("%s ac=%s: share 1 LSB off %.2e" % (fmt, ac, accept(got, *B.warp_yuv16(f, field, fmt, ac), 1023, fmt)))


def torch_fp32_bicubic(x, field, ac):
    """torch-CPU in float32 on the same inputs: UpsamplingBilinear2d(size)(field), then grid_sample(mode="bicubic")."""
    import torch.nn.functional as F
    x, field = torch.from_numpy(x), torch.from_numpy(field)
    grid = F.interpolate(field.permute(0, 3, 1, 2), size=x.shape[-2:], mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    return F.grid_sample(x, grid, mode="bicubic", padding_mode="zeros", align_corners=ac).numpy()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("hw", SHAPES + [(7, 10), (288, 320)])
def test_fp32(hip, hw, case):
    """The fp32 kernel's largest error against the float64 restatement is at most 4 x that of torch-CPU float32 bicubic on the same inputs
    (the factor covers fma contraction and the other order of the field's interpolation, both legitimate fp32 evaluations).  7 x 10: a width
    that is no multiple of 4 (one pixel per lane)."""
    from pwstablenet_amd import functional as PF
    h, w = hw
    pairs = []
    for n, (fh, fw), ac in configs():
        if hw == (288, 320):
            if (fh, fw) != FIELD_SIZES[0] or n != 1:
                continue
            fh = fw = 256
        field = field_case(case, n, fh, fw, seed=w + n)
        check_case(case, field, [(h, w)], ac)
        x = np.random.RandomState(h + n).uniform(0, 255, (n, 3, h, w)).astype(np.float32)
        got = PF.upsample_grid_sample(dev(x), dev(field), align_corners=ac, mode="bicubic")
        assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
        got = got.cpu().numpy()
        ref = B.warp_nchw(x, field, ac)
        e_kernel, e_torch = float(np.abs(got - ref).max()), float(np.abs(torch_fp32_bicubic(x, field, ac) - ref).max())
        pairs.append((e_kernel, e_torch))
        out = B.all_outside(field, h, w, ac)
        assert (got.transpose(0, 2, 3, 1)[out] == 0).all()
    print("fp32 %s %s: (kernel, torch fp32) max abs error vs float64: %s" % (hw, case, ", ".join("(%.2e, %.2e)" % p for p in pairs)))
    for e_kernel, e_torch in pairs:
        assert e_kernel <= 4 * e_torch, (e_kernel, e_torch)


def test_argument_checks(hip):
    from pwstablenet_amd import functional as PF
    field = torch.zeros((1, 4, 4, 2), device="cuda")
    with pytest.raises(RuntimeError):   # w % 4
        PF.upsample_grid_sample_u8(torch.zeros((1, 8, 6, 3), dtype=torch.uint8, device="cuda"), field, mode="bicubic")
    with pytest.raises(RuntimeError):   # every plane holds the 4-column window: w >= 8 for 4:2:0
        PF.upsample_grid_sample_yuv420(torch.zeros((1, 12, 4), dtype=torch.uint8, device="cuda"), field, "nv12", mode="bicubic")
    with pytest.raises(RuntimeError):
        PF.upsample_grid_sample_yuv420_16(torch.zeros((1, 12, 4), dtype=torch.uint16, device="cuda"), field, "i010", mode="bicubic")
    with pytest.raises(RuntimeError):
        PF.upsample_grid_sample(torch.zeros((1, 3, 8, 3), device="cuda"), field, mode="bicubic")
    with pytest.raises(ValueError):   # odd H, as the bilinear twin
        PF.upsample_grid_sample_yuv420(torch.zeros((1, 13, 8), dtype=torch.uint8, device="cuda"), field, "nv12", mode="bicubic")
    with pytest.raises(ValueError):
        PF.upsample_grid_sample_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda"), field, mode="lanczos")
    # the default is the bilinear kernel
    f = dev(smooth_bgr(1, 8, 8, 0))
    fld = dev(B.affine_field(1, 4, 4, scale=0.5))
    assert torch.equal(PF.upsample_grid_sample_u8(f, fld), PF.upsample_grid_sample_u8(f, fld, mode="bilinear"))
    assert not torch.equal(PF.upsample_grid_sample_u8(f, fld), PF.upsample_grid_sample_u8(f, fld, mode="bicubic"))


def make_net():
    from pwstablenet_amd.lib.networks_cascading import define_G
    net = define_G(31, 2, 16, "normal", 0.02)
    net.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in synth.make_weights("W1", seed=123, ngf=16)})
    return net.cuda()


@pytest.mark.parametrize("fmt", ["bgr24", "nv12"])
def test_stabilizer_interpolation(hip, fmt):
    """VideoStabilizer(interpolation="bicubic") warps with the bicubic kernel on the very fields run() forms -- bit for bit the functional call
    on VideoStabilizer._fields of the same window planes -- and nothing else changes: the default equals "bilinear", two chunks in flight
    equal one."""
    from pwstablenet_amd import functional as PF
    from pwstablenet_amd.stream import VideoStabilizer, window_planes, window_planes_yuv
    net = make_net()
    T, h, w = 8, 288, 320
    if fmt == "bgr24":
        d = dev(np.ascontiguousarray(synth.smooth_frames_u8(1, T, h, w, 3)[0][..., None].repeat(3, -1)))
        gray = window_planes(d)
        warp = lambda fields, vs, mode: PF.upsample_grid_sample_u8(d, fields, swap_rb=vs.swap_rb, align_corners=vs.align_corners, mode=mode)   # noqa: E731
    else:
        y = synth.smooth_frames_u8(1, T, h, w, 3)[0]
        _, u, v = R.unpack(R.random_yuv(T, h, w, "i420", seed=3), "i420")
        d = dev(R.pack(y, u, v, fmt))
        gray = window_planes_yuv(d, fmt)
        warp = lambda fields, vs, mode: PF.upsample_grid_sample_yuv420(d, fields, fmt, align_corners=vs.align_corners, mode=mode)   # noqa: E731
    cubic, linear, default = (VideoStabilizer(net, batch=16, interpolation="bicubic"), VideoStabilizer(net, batch=16, interpolation="bilinear"),
                              VideoStabilizer(net, batch=16))
    assert cubic.interpolation == "bicubic" and default.interpolation == "bilinear"
    fields = torch.empty((T, 256, 256, 2), device="cuda")
    with torch.no_grad():
        cubic._fields(gray, 0, 0, fields)
    got = cubic.run(gray, d, pixel_format=fmt)
    assert got.shape == d.shape and got.dtype == torch.uint8
    assert torch.equal(got, warp(fields, cubic, "bicubic"))
    got_lin = linear.run(gray, d, pixel_format=fmt)
    assert torch.equal(got_lin, warp(fields, linear, "bilinear")) and not torch.equal(got, got_lin)
    assert torch.equal(default.run(gray, d, pixel_format=fmt), got_lin)
    assert torch.equal(cubic.run_video(d, chunk=16, pixel_format=fmt), got)
    assert torch.equal(default.run_video(d, chunk=16, pixel_format=fmt), got_lin)
    host = d.cpu().pin_memory()
    two, one = cubic.run_video(host, chunk=4, in_flight=2, pixel_format=fmt), cubic.run_video(host, chunk=4, in_flight=1, pixel_format=fmt)
    assert not two.is_cuda and torch.equal(two, one)
