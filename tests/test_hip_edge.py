"""GPU tests of the edge modes' kernel (csrc/border_edge.hip; functional.edge_borders_, C: pws_border_edge_u8 / _yuv_u8 / _yuv_u16) against
the float64 restatement tests/edge_ref.py.

Both edges x both interpolations x both align_corners values x four fields (keep_ref.field_case: identity, a shift that uncovers a wedge on
two sides, everything ~3e4 plane widths outside, a smooth random field) for bgr24 (with and without swap_rb) and the ten packed YUV formats
at keep_ref.SHAPES -- 16 x 20 (chroma width 10 = 2 mod 4), 18 x 24 (odd chroma height), 12 x 520 (rows across wave boundaries) with 8 x 8
fields -- and one 720 x 1280 case per format with a 256 x 256 field (the wave-shared field modes); T = 4.  The sources are smooth frames
(edge_ref.source_of), ``warped`` holds random words, so an untouched sample is recognisable.

Check (edge_ref.check_case), per sample, with delta = keep_ref.FACTOR x the plane's fp32 coordinate error on the test's own field: covered
and decided -- the warp's word; uncovered and decided -- at most 1 LSB from the float64 value, a difference only where the float64 blend
lies within 0.05 of an integer, at most 6 % of a case's uncovered samples differing (yuv16_ref.accept's band and cap); undecided -- either;
a non-finite coordinate -- the warp's word.  tests/test_edge_ref_cpu.py holds the restatement itself, in float32, to the same acceptance on
the same inputs (measured there: at most 0.1 % differ).  "mirror" under the "outside" field is not compared (fp32's floor no longer decides the tap there):
the bilinear result must lie within the source plane's range.  Exact cases are compared with ``==``."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_ref  # noqa: E402
import edge_ref as E  # noqa: E402
import keep_ref as K  # noqa: E402


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the cached arrays are read-only)


def call(warped, src, field, fmt_name, edge, mode, ac):
    from pwstablenet_amd import functional as PF
    fmt, swap = E.split(fmt_name)
    buf = dev(warped)
    got = PF.edge_borders_(buf, dev(src), dev(field), edge, fmt, swap_rb=swap, align_corners=ac, mode=mode)
    assert got is buf   # in place
    return got.cpu().numpy()


def plane_range_ok(got, src, refs, fmt_name):
    """Every filled sample lies within the min .. max of its source plane and channel (a bilinear blend of samples of that plane)."""
    fmt, swap = E.split(fmt_name)
    for gp, vals, ref in zip(E.planes(got, fmt), E.source_planes(src, fmt, swap), refs):
        sel = ref["need"] & ~ref["cov"] & ref["decided"]
        g = E.values(gp, fmt)
        for t in range(g.shape[0]):
            for c in range(g.shape[3]):
                v = g[t, ..., c][sel[t]]
                if v.size and not (vals[t, ..., c].min() <= v.min() and v.max() <= vals[t, ..., c].max()):
                    return False
    return True


def run_case(fmt_name, h, w, fs, case, ac, mode, edge):
    src, field, refs = E.case_reference(fmt_name, h, w, fs, case, ac, mode, edge)
    warped = E.warped_of(fmt_name, h, w)
    got = call(warped, src, field, fmt_name, edge, mode, ac)
    tag = (fmt_name, h, w, case, ac, mode, edge)
    share, und = E.check_case(got, warped, refs, fmt_name, tag, E.compares(case, edge))
    if case == "identity" and mode == "bilinear":
        assert np.array_equal(got, warped), tag
    if case in ("shift", "smooth", "outside"):
        assert not np.array_equal(got, warped), tag
    if case == "outside":
        fmt, swap = E.split(fmt_name)
        if edge == "clamp":   # everything reads one corner of its plane, under the read rule: exactly
            for gp, vals in zip(E.planes(got, fmt), E.source_planes(src, fmt, swap)):
                # shift (3e4, -3e4): far to the right (ix > 0) and far up (iy < 0) -- the top right corner
                want = np.broadcast_to(E.place(vals[:, :1, -1:], fmt), gp.shape)
                assert np.array_equal(gp, want), tag
        elif mode == "bilinear":
            assert plane_range_ok(got, src, refs, fmt_name), tag
    return share, und


@pytest.mark.parametrize("hwf", E.SHAPES, ids=lambda s: "%dx%d" % (s[0], s[1]))
@pytest.mark.parametrize("fmt_name", E.FORMATS)
def test_edge_small(hip, fmt_name, hwf):
    h, w, fs = hwf
    worst, und = 0.0, 0.0
    for case, ac, mode, edge in E.small_cases():
        share, u = run_case(fmt_name, h, w, fs, case, ac, mode, edge)
        worst, und = max(worst, share), max(und, u)
    print("%s %dx%d: largest share of differing uncovered samples %.5f, of undecided positions %.5f" % (fmt_name, h, w, worst, und))


@pytest.mark.parametrize("fmt_name", E.FORMATS)
def test_edge_720p(hip, fmt_name):
    h, w, fs = E.BIG
    case, ac, mode, edge = E.BIG_CASE[fmt_name]
    share, und = run_case(fmt_name, h, w, fs, case, ac, mode, edge)
    print("%s 720p %s ac=%s %s %s: share of differing uncovered samples %.5f, of undecided positions %.5f" % (fmt_name, case, ac, mode, edge, share, und))


@pytest.mark.parametrize("fmt_name", E.FORMATS)
def test_constant_planes_come_out_exactly(hip, fmt_name):
    """Taps that all hold one value give that value: every uncovered sample of a constant source is the constant, the maxima included
    (the fp32 cubic weights do not sum to 1)."""
    fmt, swap = E.split(fmt_name)
    h, w, fs = E.SHAPES[1]
    deep = E.dtype(fmt) == np.uint16
    warped = E.warped_of(fmt_name, h, w)
    for v in ((0, 1, 517, 1023) if deep else (0, 1, 200, 255)):
        src = np.broadcast_to(E.place(np.int64(v), fmt), warped.shape).astype(E.dtype(fmt))
        for case in ("shift", "smooth", "outside"):
            field = E.field_of(case, fs, w)
            for mode in E.MODES:
                for edge in E.EDGES:
                    got = call(warped, src, field, fmt_name, edge, mode, True)
                    for gp, wp, vals in zip(E.planes(got, fmt), E.planes(warped, fmt), E.source_planes(src, fmt, swap)):
                        ref = E.plane_reference(vals, field, (case, fs, w), True, mode, edge, fmt)
                        filled = ref["need"] & ~ref["cov"] & ref["decided"]
                        assert filled.any() and (gp[filled] == E.place(np.int64(v), fmt)).all(), (fmt_name, v, case, mode, edge)
                        assert np.array_equal(gp[ref["stay"]], wp[ref["stay"]])


@pytest.mark.parametrize("fmt_name", E.FORMATS)
def test_read_and_write_rules_on_any_words(hip, fmt_name):
    """Noise sources -- junk in P010's low bits, I010 words above 1023 -- under "clamp" and the "outside" field: every sample of a plane is its
    top right corner under the read rule (swap_rb; word >> 6; min(word, 1023)), written as the warp writes it."""
    fmt, swap = E.split(fmt_name)
    h, w, fs = E.SHAPES[0]
    rs = np.random.RandomState(9)
    src = rs.randint(0, 65536 if E.dtype(fmt) == np.uint16 else 256, E.frame_shape(fmt, E.T, h, w)).astype(E.dtype(fmt))
    for mode in E.MODES:
        got = call(E.warped_of(fmt_name, h, w), src, E.field_of("outside", fs, w), fmt_name, "clamp", mode, False)
        for gp, vals in zip(E.planes(got, fmt), E.source_planes(src, fmt, swap)):
            assert np.array_equal(gp, np.broadcast_to(E.place(vals[:, :1, -1:], fmt), gp.shape)), (fmt_name, mode)


@pytest.mark.parametrize("fmt_name", ["bgr24", "nv12", "i010", "i444", "p210"])
def test_non_finite_coordinates_keep_the_warps_words(hip, fmt_name):
    fmt, swap = E.split(fmt_name)
    h, w, fs = E.SHAPES[1]
    field = E.nonfinite_field(fs)
    src, warped = E.source_of(fmt, h, w), E.warped_of(fmt_name, h, w)
    for mode in E.MODES:
        for edge in E.EDGES:
            for ac in (False, True):
                got = call(warped, src, field, fmt_name, edge, mode, ac)
                refs = [E.plane_reference(v, field, ("nonfinite", fs), ac, mode, edge, fmt) for v in E.source_planes(src, fmt, swap)]
                assert any((~r["finite"]).any() for r in refs) and any((r["need"] & ~r["cov"]).any() for r in refs)
                for gp, wp, ref in zip(E.planes(got, fmt), E.planes(warped, fmt), refs):
                    E.check_plane(gp, wp, ref, fmt, (fmt_name, mode, edge, ac))


def test_pad_returns_the_input_without_a_launch(hip):
    from pwstablenet_amd import functional as PF
    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    # (no launch: not even the field is looked at, and the source may be the frames themselves)
    assert PF.edge_borders_(frames, frames, None, "pad") is frames
    host = torch.zeros((2, 12, 8), dtype=torch.uint8)
    assert PF.edge_borders_(host, host, None, "pad", "nv12") is host


def test_argument_checks(hip):
    from pwstablenet_amd import functional as PF
    A = hip
    lib, st, p = A.lib(), A.current_stream(), A.ptr
    EINVAL = -22
    field = torch.zeros((2, 4, 4, 2), device="cuda")
    u8, s8 = (torch.zeros(2 * 16 * 16 * 3, dtype=torch.uint8, device="cuda") for _ in range(2))
    u16, s16 = (torch.zeros(2 * 16 * 16 * 3, dtype=torch.uint16, device="cuda") for _ in range(2))
    # (frames, source, field, n, h, w, fh, fw, swap_rb, align_corners, bicubic, edge, stream)
    bgr = lambda edge, h=8, w=8, fr=u8, src=s8, n=2, bic=0: lib.pws_border_edge_u8(p(fr), p(src), p(field), n, h, w, 4, 4, 0, 0, bic, edge, st)   # noqa: E731
    assert bgr(1) == 0 and bgr(2) == 0 and bgr(2, bic=1) == 0 and bgr(1, n=0) == 0
    assert bgr(0) == EINVAL and b"edge" in lib.pws_last_error()
    assert bgr(3) == EINVAL and bgr(-1) == EINVAL and bgr(3, n=0) == EINVAL
    assert bgr(1, w=6) == EINVAL and bgr(1, w=2) == EINVAL and bgr(1, h=0) == EINVAL      # w % 4, w < 4, an empty frame
    assert bgr(1, fr=u8[1:]) == EINVAL and bgr(1, src=s8[2:]) == EINVAL                   # alignment, of the source too
    assert bgr(1, src=u8) == EINVAL and b"overlap" in lib.pws_last_error()               # source is frames
    assert bgr(1, src=u8[8 * 8 * 3:]) == EINVAL and bgr(1, src=u8[2 * 8 * 8 * 3:]) == 0   # one frame on: still overlaps; two on: does not
    assert lib.pws_border_edge_u8(p(u8), None, p(field), 2, 8, 8, 4, 4, 0, 0, 0, 1, st) == EINVAL   # NULL source
    for fn, buf, src in ((lib.pws_border_edge_yuv_u8, u8, s8), (lib.pws_border_edge_yuv_u16, u16, s16)):
        # (frames, source, field, n, h, w, fh, fw, layout, chroma, align_corners, bicubic, edge, stream)
        yuv = lambda edge, h=8, w=8, lay=0, chroma=0, bic=0, s=src: fn(p(buf), p(s), p(field), 2, h, w, 4, 4, lay, chroma, 0, bic, edge, st)   # noqa: E731,B023
        assert yuv(1) == 0 and yuv(2, chroma=1) == 0 and yuv(2, lay=1, chroma=2) == 0 and yuv(1, bic=1) == 0
        assert yuv(0) == EINVAL and yuv(3) == EINVAL
        assert yuv(1, h=7) == EINVAL and yuv(1, w=6) == EINVAL and yuv(1, lay=2) == EINVAL
        assert yuv(1, chroma=3) == EINVAL and yuv(1, lay=0, chroma=2) == EINVAL          # interleaved 4:4:4 is not offered
        assert yuv(1, w=4) == 0 and yuv(1, w=4, bic=1) == EINVAL                         # w >= 8 with the bicubic margin
        assert yuv(1, w=4, lay=1, chroma=2, bic=1) == 0                                  # any valid w at 4:4:4
        assert yuv(1, s=buf) == EINVAL and b"overlap" in lib.pws_last_error()
        assert yuv(1, s=buf[8 * 12:]) == EINVAL                                          # one frame on: the second overlaps the first
    torch.cuda.synchronize()
    frames, source = (torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    for edge in ("wrap", "black", 1, None):
        with pytest.raises(ValueError, match="edge"):
            PF.edge_borders_(frames, source, field, edge)
    with pytest.raises(ValueError, match="mode"):
        PF.edge_borders_(frames, source, field, "clamp", mode="lanczos")
    with pytest.raises(ValueError, match="integer pixel formats"):   # float frames
        PF.edge_borders_(torch.zeros((2, 3, 8, 8), device="cuda"), torch.zeros((2, 3, 8, 8), device="cuda"), field, "clamp")
    with pytest.raises(ValueError, match="contiguous"):
        nc = torch.zeros((2, 8, 16, 3), dtype=torch.uint8, device="cuda")[:, :, ::2]
        PF.edge_borders_(nc, source, field, "mirror")
    with pytest.raises(ValueError, match="contiguous"):
        PF.edge_borders_(torch.zeros((4, 12, 8), dtype=torch.uint8, device="cuda")[::2], torch.zeros((2, 12, 8), dtype=torch.uint8, device="cuda"),
                         field, "mirror", "nv12")
    with pytest.raises(ValueError, match="source"):   # shape
        PF.edge_borders_(frames, source[:1], field, "clamp")
    with pytest.raises(ValueError, match="source"):   # dtype
        PF.edge_borders_(frames, source.to(torch.int8), field, "clamp")
    with pytest.raises(ValueError, match="field"):
        PF.edge_borders_(frames, source, field[:1], "clamp")
    with pytest.raises(ValueError):     # an unknown format
        PF.edge_borders_(frames, source, field, "clamp", "yuv444")
    with pytest.raises(ValueError):     # dtype / format mismatch
        PF.edge_borders_(torch.zeros((2, 12, 8), dtype=torch.uint8, device="cuda"), torch.zeros((2, 12, 8), dtype=torch.uint8, device="cuda"), field,
                         "clamp", "p010")
    with pytest.raises(RuntimeError):   # PWS_EINVAL through functional: w % 4
        PF.edge_borders_(torch.zeros((2, 8, 6, 3), dtype=torch.uint8, device="cuda"), torch.zeros((2, 8, 6, 3), dtype=torch.uint8, device="cuda"), field,
                         "clamp")
    with pytest.raises(RuntimeError):   # w >= 8 for 4:2:0 with the bicubic margin
        PF.edge_borders_(torch.zeros((2, 12, 4), dtype=torch.uint8, device="cuda"), torch.zeros((2, 12, 4), dtype=torch.uint8, device="cuda"), field,
                         "clamp", "nv12", mode="bicubic")
    with pytest.raises(RuntimeError):   # overlap: the source is the frames
        PF.edge_borders_(frames, frames, field, "clamp")
    assert PF.edge_borders_(frames[:0], source[:0], field[:0], "mirror").shape[0] == 0   # an empty clip
    assert PF.EDGES == ("pad", "clamp", "mirror") and PF.BORDERS == ("black", "keep", "mosaic")
    assert PF.lookup_format("bgr24").edge_entry == "pws_border_edge_u8" and PF.lookup_format("i444").edge_entry == "pws_border_edge_yuv_u8"
    assert PF.lookup_format("p010").edge_entry == "pws_border_edge_yuv_u16"
    assert chroma_ref.ALL.keys() <= set(PF.PACKED_FORMATS) and K.T == E.T
