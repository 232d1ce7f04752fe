"""Frames out without a GPU: the integer restatement of tests/frames_ref.py against torch's own ``(x * 255.0).astype(np.uint8)``, the
values DESIGN.md section 5 ("Frames out") works out by hand, the ranges of Y, U and V over all 2^24 colours, eight wrong readings of
the definition each told apart on a named case of tests/frames_cases.py, every refusal of the C ABI through ``artalk_op_frames_check``,
and the Y4M writer."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import frames_cases as fc
import frames_ref as fr
from artalk_amd import capi
from artalk_amd import frames

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ quantisation
def test_quantisation_is_the_references_cast_on_a_clamped_frame():
    t = fc.value_table()
    clamped = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(1))).astype(np.float32)
    want = (torch.from_numpy(clamped) * 255.0).numpy().astype(np.uint8)      # inference.py:83-86 on values inside [0, 1]
    assert np.array_equal(fr.quantise(t), want)
    assert fr.quantise(np.array([np.nan, -np.inf, np.inf, -0.0, 1.5], dtype=np.float32)).tolist() == [0, 0, 255, 0, 255]


def test_every_level_survives_and_its_lower_neighbour_does_not():
    lv = fc.levels()
    assert np.array_equal(fr.quantise(lv), np.arange(256))
    below = np.nextafter(lv[1:], np.float32(-np.inf))
    assert np.array_equal(fr.quantise(below), np.arange(255))
    assert np.array_equal(fr.quantise(np.nextafter(lv, np.float32(np.inf))), np.arange(256))


def test_truncation_is_not_rounding():
    x = np.random.default_rng(0).random(1 << 16, dtype=np.float32)
    share = float((fr.quantise(x) != fr.quantise(x, "round")).mean())
    print(f"truncation and round-to-nearest differ on {100 * share:.1f} % of uniform inputs")
    assert 0.45 < share < 0.55


# ------------------------------------------------------------------------------------------------ colours
@pytest.mark.parametrize("name", sorted(fc.HAND_COLOURS))
def test_hand_values(name):
    rgb, (Y, U, V) = fc.HAND_COLOURS[name]
    got = fr.yuv420p(fc.solid(rgb))[0]
    assert got.shape == (3, 2)
    assert got.reshape(-1).tolist() == [Y] * 4 + [U, V]
    assert fr.rgb24(fc.solid(rgb))[0, 0, 0].tolist() == [int(round(255 * c)) for c in rgb]


def test_ranges_over_all_colours():
    """Y in 16..235, U and V in 16..240 for every one of the 2^24 (R, G, B): the planes need no clamp."""
    G, B = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    lo, hi = np.full(3, 1 << 30), np.full(3, -1)
    for R in range(256):
        for i, plane in enumerate(fr.yuv_from_rgb8(np.int64(R), G, B)):
            lo[i], hi[i] = min(lo[i], plane.min()), max(hi[i], plane.max())
    assert lo.tolist() == [16, 16, 16] and hi.tolist() == [235, 240, 240]


# ------------------------------------------------------------------------------------------------ wrong readings
WRONG = {      # reading: the case of the table on which it must show
    "round": ("rgb24", (2, 7, 13), "random"),
    "noclamp": ("rgb24", (2, 7, 13), "table"),
    "fullrange": ("yuv420p", (1, 4, 10), "colours"),
    "topleft": ("yuv420p", (1, 16, 16), "blocks"),
    "mean_floor": ("yuv420p", (1, 16, 16), "blocks"),
    "bgr": ("rgb24", (3, 3, 5), "colours"),
    "uv_swapped": ("yuv420p", (1, 4, 10), "colours"),
    "nv12": ("yuv420p", (1, 4, 10), "colours"),
}


def test_the_table_names_every_reading():
    assert sorted(WRONG) == sorted(fr.READINGS)
    assert all(case in fc.CASES for case in WRONG.values())


@pytest.mark.parametrize("reading", fr.READINGS)
def test_wrong_readings_are_told_apart(reading):
    fmt, shape, fill = WRONG[reading]
    x = fc.make(shape, fill)
    right, wrong = fr.pack(x, fmt), fr.pack(x, fmt, reading)
    assert right.shape == wrong.shape
    n = int((right != wrong).sum())
    print(f"{reading}: {n} of {right.size} bytes differ on {fc.case_id((fmt, shape, fill))}")
    assert n > 0, f"the reading {reading!r} passes on {fc.case_id((fmt, shape, fill))}"


def test_the_bgr_reading_shows_in_yuv_too():
    x = fc.make((1, 4, 10), "colours")
    assert not np.array_equal(fr.yuv420p(x), fr.yuv420p(x, "bgr"))


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def _check(fmt, F, H, W, src=1, out=1):
    msg = C.create_string_buffer(256)
    rc = capi.lib().artalk_op_frames_check(fmt, F, H, W, src, out, msg, 256)
    return rc, msg.value.decode()


def test_refusals():
    RGB, YUV = capi.FRAMES_RGB24, capi.FRAMES_YUV420P
    assert (RGB, YUV) == (1, 2)
    assert _check(RGB, 3, 3, 5) == (capi.OK, "") and _check(YUV, 2, 2, 2) == (capi.OK, "")
    assert _check(RGB, 1, 16384, 16384)[0] == capi.OK and _check(RGB, 1, 1, 1)[0] == capi.OK
    assert _check(RGB, 0, 4, 4, 0, 0) == (capi.OK, "")      # F = 0: the pointers are not looked at
    for fmt in (0, 3, -1):
        rc, msg = _check(fmt, 1, 4, 4)
        assert rc == capi.EINVAL and "unknown frame format" in msg
    for H, W in ((0, 4), (4, 0), (-2, 4), (16385, 4), (4, 16385), (16386, 16386)):
        for fmt in (RGB, YUV):
            rc, msg = _check(fmt, 1, H, W)
            assert rc == capi.EINVAL and "1..16384" in msg, (fmt, H, W)
    for H, W in ((3, 4), (4, 3), (1, 1)):
        rc, msg = _check(YUV, 1, H, W)
        assert rc == capi.EINVAL and "even" in msg
        assert _check(RGB, 1, H, W)[0] == capi.OK
    rc, msg = _check(RGB, -1, 4, 4)
    assert rc == capi.EINVAL and "negative" in msg
    for src, out in ((0, 1), (1, 0), (0, 0)):
        rc, msg = _check(RGB, 1, 4, 4, src, out)
        assert rc == capi.EINVAL and "NULL" in msg
    rc, msg = _check(RGB, 2 ** 31 - 1, 16384, 16384)
    assert rc == capi.EINVAL and "too large" in msg


def test_the_entry_points_refuse_before_the_device_is_touched():
    L = capi.lib()
    fake = C.c_void_p(4096)      # never dereferenced: every call below is refused on the host, or launches nothing
    assert L.artalk_frames_pack(fake, 1, 4, 4, 7, fake, None) == capi.EINVAL and b"unknown frame format" in L.artalk_frames_last_error()
    assert L.artalk_frames_pack(fake, 1, 3, 4, capi.FRAMES_YUV420P, fake, None) == capi.EINVAL and b"even" in L.artalk_frames_last_error()
    assert L.artalk_frames_pack(None, 1, 4, 4, capi.FRAMES_RGB24, fake, None) == capi.EINVAL
    assert L.artalk_frames_pack(fake, 1, 4, 4, capi.FRAMES_RGB24, None, None) == capi.EINVAL
    assert L.artalk_frames_pack(fake, -1, 4, 4, capi.FRAMES_RGB24, fake, None) == capi.EINVAL
    assert L.artalk_frames_pack(None, 0, 4, 4, capi.FRAMES_RGB24, None, None) == capi.OK      # F = 0 launches nothing
    assert L.artalk_op_gaga_finish_pack(fake, 1, 16, None, 0, 0, 0, fake, None) == capi.EINVAL
    assert L.artalk_op_gaga_finish_pack(fake, 1, 15, None, 0, 0, capi.FRAMES_YUV420P, fake, None) == capi.EINVAL
    assert L.artalk_op_gaga_finish_pack(fake, 1, 16, fake, 17, 4, capi.FRAMES_RGB24, fake, None) == capi.EINVAL
    assert L.artalk_gaga_render_u8(None, fake, 106, 1, None, None, 1, capi.FRAMES_RGB24, fake, None, None) == capi.EINVAL


def test_frame_bytes():
    L = capi.lib()
    assert L.artalk_frames_bytes(capi.FRAMES_RGB24, 3, 5) == 45 and L.artalk_frames_bytes(capi.FRAMES_YUV420P, 2, 2) == 6
    assert L.artalk_frames_bytes(capi.FRAMES_RGB24, 512, 512) == 786432 and L.artalk_frames_bytes(capi.FRAMES_YUV420P, 512, 512) == 393216
    assert L.artalk_frames_bytes(capi.FRAMES_RGB24, 16384, 16384) == 3 * 2 ** 28
    for bad in ((0, 4, 4), (3, 4, 4), (capi.FRAMES_YUV420P, 3, 4), (capi.FRAMES_YUV420P, 4, 5), (capi.FRAMES_RGB24, 0, 4),
                (capi.FRAMES_RGB24, 4, 16385)):
        assert L.artalk_frames_bytes(*bad) < 0, bad
    assert frames.frame_bytes("rgb24", 3, 5) == 45 and frames.frame_bytes("yuv420p", 34, 66) == 3366
    assert frames.frame_shape("rgb24", 2, 3, 5) == (2, 3, 5, 3) and frames.frame_shape("yuv420p", 2, 4, 10) == (2, 6, 10)
    for bad in (("yuv420p", 3, 4), ("rgb24", 0, 1), ("nv12", 4, 4), (None, 4, 4)):
        with pytest.raises(ValueError):
            frames.frame_bytes(*bad)


NEW_SYMBOLS = ("artalk_frames_bytes", "artalk_frames_pack", "artalk_frames_last_error", "artalk_op_frames_check",
               "artalk_op_gaga_finish_pack", "artalk_gaga_render_u8")


def test_symbols_are_exported_and_declared():
    L = capi.lib()
    header = open(os.path.join(REPO, "include", "artalk_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in capi.SYMBOLS and name + "(" in header, name
    assert "#define ARTALK_FRAMES_RGB24 1" in header and "#define ARTALK_FRAMES_YUV420P 2" in header


def test_pack_frames_refuses_on_the_host():
    with pytest.raises(ValueError):
        frames.pack_frames(torch.zeros(1, 3, 4, 4), "nv12")
    with pytest.raises(ValueError):
        frames.pack_frames(torch.zeros(1, 4, 4, 4), "rgb24")
    with pytest.raises(ValueError):
        frames.pack_frames(torch.zeros(1, 3, 4, 4, dtype=torch.float64), "rgb24")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.pack_frames(torch.zeros(1, 3, 4, 4), "rgb24")


# ------------------------------------------------------------------------------------------------ Y4M
def test_y4m_round_trip(tmp_path):
    x = fc.make((3, 4, 10), "random")
    yuv = torch.from_numpy(fr.yuv420p(x))
    path = tmp_path / "clip.y4m"
    frames.write_y4m(path, yuv, size=(4, 10))
    raw = path.read_bytes()
    header = b"YUV4MPEG2 W10 H4 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert raw.startswith(header)
    assert len(raw) == len(header) + 3 * (len(b"FRAME\n") + 60)
    assert raw[len(header):len(header) + 6] == b"FRAME\n" and raw[len(header) + 6:len(header) + 66] == yuv[0].numpy().tobytes()
    back, fps, size = frames.read_y4m(path)
    assert fps == 25 and size == (4, 10) and back.dtype == torch.uint8 and torch.equal(back, yuv)
    frames.write_y4m(path, yuv[:0], fps=30)
    back, fps, size = frames.read_y4m(path)
    assert back.shape == (0, 6, 10) and fps == 30 and size == (4, 10)
    assert path.read_bytes() == header.replace(b"F25", b"F30")


def test_write_y4m_refuses_a_wrong_shape(tmp_path):
    path = tmp_path / "no.y4m"
    for bad in (torch.zeros(2, 4, 10, 3, dtype=torch.uint8),      # rgb24 frames
                torch.zeros(2, 6, 10),                             # not uint8
                torch.zeros(2, 7, 10, dtype=torch.uint8),          # 7 rows are H * 3 // 2 of no H
                torch.zeros(2, 6, 9, dtype=torch.uint8),           # an odd W
                torch.zeros(6, 10, dtype=torch.uint8)):            # a single frame without its leading dimension
        with pytest.raises(ValueError):
            frames.write_y4m(path, bad)
    with pytest.raises(ValueError):
        frames.write_y4m(path, torch.zeros(2, 6, 10, dtype=torch.uint8), size=(6, 10))      # the frames are 4 x 10
    with pytest.raises(ValueError):
        frames.write_y4m(path, torch.zeros(2, 6, 10, dtype=torch.uint8), fps=0)
    (tmp_path / "junk.y4m").write_bytes(b"RIFF....\n")
    with pytest.raises(ValueError):
        frames.read_y4m(tmp_path / "junk.y4m")


# ------------------------------------------------------------------------------------------------ the engine
def test_rendering_output_needs_a_renderer():
    from artalk_amd.engine import ARTAvatarInferEngine
    eng = ARTAvatarInferEngine(model=types.SimpleNamespace(cfg=None))
    eng.flame_model = object()      # the mesh branch would return vertices: there is nothing to pack
    assert getattr(eng, "mesh_renderer", None) is None
    for fmt in ("rgb24", "yuv420p"):
        with pytest.raises(ValueError, match="mesh_renderer"):
            eng.rendering(None, torch.zeros(2, 106), output=fmt)
    with pytest.raises(ValueError, match="unknown frame format"):
        eng.rendering(None, torch.zeros(2, 106), output="nv12")
    with pytest.raises(TypeError):
        eng.rendering(None, torch.zeros(2, 106), "mesh", None, "x.mp4", "rgb24")      # keyword only
