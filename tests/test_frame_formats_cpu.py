"""CPU tests of the per-format record (functional.FrameFormat / FRAME_FORMATS): every C entry a record can name is declared in
hipabi.SIGNATURES, and FrameFormat.frame_shape holds the shape rules that yuv420_shape / yuv420_16_shape have always had -- the wrappers and
the record agree, message fragments included.  No GPU and no library load.

(2, 57, 52) is a packed 4:2:0 shape, so the four packed formats take it (H = 38); "bgr24" has no packed shape and takes the same frames as
(2, 38, 52, 3)."""
import pytest

torch = pytest.importorskip("torch")

from pwstablenet_amd import functional as PF  # noqa: E402
from pwstablenet_amd import hipabi  # noqa: E402

FORMATS = ("bgr24", "nv12", "i420", "p010", "i010")
PACKED = FORMATS[1:]
WRAPPERS = {torch.uint8: (PF.yuv420_shape, PF.yuv420_layout), torch.uint16: (PF.yuv420_16_shape, PF.yuv420_16_layout)}


def test_table():
    assert tuple(PF.FRAME_FORMATS) == FORMATS == PF.PIXEL_FORMATS + PF.PIXEL_FORMATS_16
    for name, fmt in PF.FRAME_FORMATS.items():
        assert fmt.name == name and fmt.packed == (name != "bgr24")
        assert fmt.dtype == (torch.uint16 if name in PF.PIXEL_FORMATS_16 else torch.uint8)
        with pytest.raises(AttributeError):   # immutable
            fmt.layout = 1
    for table in (PF.YUV420_LAYOUT, PF.YUV420_16_LAYOUT):
        for name, layout in table.items():
            assert PF.FRAME_FORMATS[name].layout == layout == PF.FRAME_FORMATS[name].extra(True)
    assert PF.FRAME_FORMATS["bgr24"].extra(True) == 1 and PF.FRAME_FORMATS["bgr24"].extra() == 0
    assert PF._FLOAT_FRAMES.dtype == torch.float32 and PF._FLOAT_FRAMES.name == "bgr24"


@pytest.mark.parametrize("name", FORMATS)
def test_entries_are_declared(name):
    fmt = PF.FRAME_FORMATS[name]
    entries = [fmt.warp_entry(mode) for mode in PF.INTERPOLATIONS] + [fmt.keep_entry, fmt.window_planes, fmt.plane_resize]
    assert len(set(entries)) == 5
    for entry in entries:
        assert entry in hipabi.SIGNATURES, entry
    for mode in PF.INTERPOLATIONS:
        assert PF._FLOAT_FRAMES.warp_entry(mode) in hipabi.SIGNATURES
    with pytest.raises(ValueError, match="mode must be one of"):
        fmt.warp_entry("nearest")


@pytest.mark.parametrize("name", PACKED)
def test_frame_shape_packed(name):
    fmt = PF.FRAME_FORMATS[name]
    shape_of, layout_of = WRAPPERS[fmt.dtype]
    other = torch.uint16 if fmt.dtype == torch.uint8 else torch.uint8
    assert layout_of(name) == fmt.layout
    ok = torch.zeros((2, 57, 52), dtype=fmt.dtype)
    assert fmt.frame_shape(ok) == shape_of(ok, name) == (2, 38, 52)
    assert fmt.frame_shape(torch.zeros((2, 57, 54), dtype=fmt.dtype), w_multiple=2) == (2, 38, 54)
    bad = [(torch.zeros((2, 56, 52), dtype=fmt.dtype), 4, "packed height 56 is not H * 3 // 2 of an even H"),
           (torch.zeros((2, 57, 51), dtype=fmt.dtype), 4, "width 51 must be even and a multiple of 4"),
           (torch.zeros((2, 57, 51), dtype=fmt.dtype), 1, "width 51 must be even and a multiple of 1"),
           (torch.zeros((2, 57, 54), dtype=fmt.dtype), 4, "width 54 must be even and a multiple of 4"),
           (torch.zeros((2, 57, 52, 3), dtype=fmt.dtype), 4, "%s frames must be %s (T, H * 3 // 2, W), got" % (name, str(fmt.dtype)[6:])),
           (torch.zeros((2, 57, 52), dtype=other), 4, "%s frames must be %s (T, H * 3 // 2, W), got %s" % (name, str(fmt.dtype)[6:], other))]
    for frames, multiple, fragment in bad:
        messages = []
        for call in (lambda: fmt.frame_shape(frames, multiple), lambda: shape_of(frames, name, multiple)):
            with pytest.raises(ValueError) as e:
                call()
            assert fragment in str(e.value)
            messages.append(str(e.value))
        assert messages[0] == messages[1]
    # the other depth's names are not this depth's
    for wrong in set(PACKED + ("bgr24", "p016")) - {n for n in PACKED if PF.FRAME_FORMATS[n].dtype == fmt.dtype}:
        with pytest.raises(ValueError, match="pixel_format must be one of"):
            shape_of(ok, wrong)
        with pytest.raises(ValueError, match="pixel_format must be one of"):
            layout_of(wrong)


def test_frame_shape_unpacked_and_depths_agree():
    bgr = PF.FRAME_FORMATS["bgr24"]
    assert bgr.frame_shape(torch.zeros((2, 38, 52, 3), dtype=torch.uint8)) == (2, 38, 52)
    assert PF._FLOAT_FRAMES.frame_shape(torch.zeros((2, 3, 38, 52))) == (2, 38, 52)
    for frames in (torch.zeros((2, 57, 52), dtype=torch.uint8), torch.zeros((2, 38, 52, 4, 1), dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"upsample_grid_sample_u8: frames must be uint8 \(N,H,W,3\), got"):
            bgr.frame_shape(frames)
    for shape in ((2, 57, 52), (1, 3, 4), (5, 1080 * 3 // 2, 1920)):
        assert PF.yuv420_shape(torch.zeros(shape, dtype=torch.uint8), "nv12") == PF.yuv420_16_shape(torch.zeros(shape, dtype=torch.uint16), "i010") \
            == (shape[0], shape[1] // 3 * 2, shape[2])


def test_frame_format_resolves_once():
    u8, u16 = torch.zeros((2, 57, 52), dtype=torch.uint8), torch.zeros((2, 57, 52), dtype=torch.uint16)
    for name in PACKED:
        good, wrong = (u8, u16) if PF.FRAME_FORMATS[name].dtype == torch.uint8 else (u16, u8)
        assert PF.frame_format(name, good, "run") is PF.FRAME_FORMATS[name]
        with pytest.raises(ValueError, match="%s frames must be" % name):   # before any tensor is required on the device
            PF.frame_format(name, wrong, "run")
    hwc = torch.zeros((2, 38, 52, 3), dtype=torch.uint8)
    assert PF.frame_format("bgr24", hwc, "run", float_frames=True) is PF.FRAME_FORMATS["bgr24"]
    assert PF.frame_format("bgr24", torch.zeros((2, 3, 38, 52)), "run", float_frames=True) is PF._FLOAT_FRAMES
    assert PF.frame_format("bgr24", torch.zeros((2, 3, 38, 52)), "run_video") is PF.FRAME_FORMATS["bgr24"]
    with pytest.raises(ValueError, match="run_video: uint16 frames need pixel_format"):
        PF.frame_format("bgr24", u16, "run_video")
    with pytest.raises(ValueError, match="pixel_format must be one of"):
        PF.frame_format("p016", u16, "run")
