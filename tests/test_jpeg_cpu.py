"""JPEG out without a GPU: the numpy restatement of tests/jpeg_ref.py is a JPEG (Pillow decodes every case of tests/jpeg_cases.py with
warnings as errors and reports the tables and size the definition names), it is as good as Pillow's own encoder within a measured
allowance, the misreadings of the definition are told apart from it, and the host side of the feature - header, bound, refusals, the
Motion-JPEG file, the engine's option - does what include/artalk_hip.h and DESIGN.md section 5 ("JPEG out") say."""
import ctypes as C
import functools
import io
import os
import types
import warnings

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_ref
from artalk_amd import capi
from artalk_amd import frames

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# PSNR of the restatement's stream, decoded by Pillow, against Pillow's own encoder at the same quality and subsampling, over every frame of
# the table: the worst shortfall measured was 0.50 dB (8x8, 4:4:4, quality 100; elsewhere within +-0.15 dB except quality 100 in 4:4:4,
# 0.34 - 0.44 dB, where only the DCT's rounding is left).  The allowance is three times that; the DCT rounding and the chroma filter are
# the only differences.
WORST_MEASURED_DB = 0.50
ALLOWANCE_DB = 3 * WORST_MEASURED_DB


@functools.lru_cache(maxsize=None)
def _streams(case):
    name, ss, q = case
    return tuple(jpeg_ref.encode(x, q, ss) for x in jc.frames(name))


def _decode(data):
    Image = pytest.importorskip("PIL.Image")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
        return im, np.asarray(im.convert("RGB"))


def _pillow_encode(x, q, ss):
    Image = pytest.importorskip("PIL.Image")
    out = io.BytesIO()
    Image.fromarray(x).save(out, "JPEG", quality=q, subsampling=2 if ss == "420" else 0)
    return out.getvalue()


def _psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def _markers(data):
    """the scan's markers: counts of RSTn in order of appearance, and the number of FF DD segments in the header"""
    hdr, scan = data[:jpeg_ref.HEADER_BYTES], data[jpeg_ref.HEADER_BYTES:-2]
    rst = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    return rst, hdr.count(b"\xff\xdd")


# ------------------------------------------------------------------------------------------------ the restatement is a JPEG
@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_pillow_decodes_the_restatement(case):
    pytest.importorskip("PIL")
    name, ss, q = case
    QY, QC = jpeg_ref.quant_tables(q)
    for x, data in zip(jc.frames(name), _streams(case)):
        H, W, _ = x.shape
        im, got = _decode(data)
        assert im.size == (W, H) and im.mode == "RGB" and got.shape == x.shape
        assert im.format == "JPEG" and not getattr(im, "info", {}).get("progressive")
        tables = {k: [int(v) for v in t] for k, t in im.quantization.items()}      # Pillow undoes the zigzag order of the DQT segments
        assert tables == {0: [int(v) for v in QY], 1: [int(v) for v in QC]}
        _, mcuy, mcux = jpeg_ref.mcu_grid(H, W, ss)
        rst, dri = _markers(data)
        assert dri == 1 and rst == [0xD0 + r % 8 for r in range(mcuy - 1)]
        assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
        assert data.count(b"\xff\xd8") == 1 and data.count(b"\xff\xd9") == 1
        ref = _decode(_pillow_encode(x, q, ss))[1]
        err, ref_err = int(np.abs(got.astype(int) - x).max()), int(np.abs(ref.astype(int) - x).max())
        short = _psnr(ref, x) - _psnr(got, x)
        print(f"{jc.case_id(case)}: {len(data)} bytes, shortfall {short:+.3f} dB, max error {err} (Pillow's encoder: {ref_err})")
        if ref_err <= 1:      # flat and exactly reproduced pictures: no PSNR to speak of
            assert err <= ref_err if ref_err == 0 else err <= 1
        else:
            assert short <= ALLOWANCE_DB, f"{short:.3f} dB below Pillow's encoder"


def test_the_table_reaches_what_it_names():
    def stats(case):
        name, ss, q = case
        out = []
        for x in jc.frames(name):
            st = {}
            jpeg_ref.encode(x, q, ss, stats=st)
            out.append(st)
        return out
    assert stats(("blocks16x64", "444", 100))[0]["dc_category"] == 11
    st = stats(("checker16x32", "444", 100))[0]
    assert st["ac_category"] == 10 and st["no_eob"] > 0
    st = stats(("cosine16x24", "444", 90))[0]
    assert st["zrl"] == 18 and st["no_eob"] == 6      # three ZRL codes in each of the six luma blocks
    st = stats(("flat24x24", "420", 90))[0]
    assert st["ac_category"] == 0 and st["zrl"] == 0 and st["no_eob"] == 0
    st = stats(("noise32x48", "444", 100))[0]
    assert 30 <= st["stuffed"] <= 43
    assert len(_streams(("noise32x48", "444", 100))[0]) > jc.frames("noise32x48")[0].size      # larger than the raw frame
    assert stats(("rows136x16", "444", 90))[0]["restarts"] == 16 and stats(("rows272x16", "420", 90))[0]["restarts"] == 16
    assert stats(("17x23", "420", 90))[0]["restarts"] == 1
    sizes = [len(b) for b in _streams(("three48x64", "420", 90))]
    assert len(set(sizes)) == 3


# ------------------------------------------------------------------------------------------------ wrong readings
# reading -> (the case that tells it apart, how: Pillow refuses the stream / decodes a worse picture / only the bytes differ)
READINGS = {
    "no_stuffing": (("noise32x48", "444", 100), "refused"),
    "zero_padding": (("17x23", "420", 90), "bytes"),
    "dc_not_reset": (("17x23", "420", 90), "worse"),
    "rst_no_wrap": (("rows136x16", "444", 90), "refused"),
    "natural_dqt": (("24x40", "444", 50), "worse"),
    "rounding_quantiser": (("24x40", "444", 90), "bytes"),
    "limited_y": (("24x40", "444", 90), "worse"),
    "zero_edges": (("17x23", "444", 90), "worse"),
}


def test_every_reading_is_named():
    assert sorted(READINGS) == sorted(jpeg_ref.WRONG)


@pytest.mark.parametrize("reading", sorted(READINGS))
def test_wrong_readings_are_told_apart(reading):
    case, how = READINGS[reading]
    name, ss, q = case
    x = jc.frames(name)[0]
    right, wrong = _streams(case)[0], jpeg_ref.encode(x, q, ss, wrong=reading)
    assert wrong != right
    if how == "bytes":
        return
    pytest.importorskip("PIL")
    if how == "refused":
        with pytest.raises(Exception):
            _decode(wrong)
    else:
        assert _psnr(_decode(wrong)[1], x) < _psnr(_decode(right)[1], x) - 0.5


# ------------------------------------------------------------------------------------------------ header, bound, caps
def test_header_bytes():
    assert frames.JPEG_HEADER_BYTES == jpeg_ref.HEADER_BYTES == 629
    for H, W, q, ss in ((17, 23, 90, "420"), (1, 1, 50, "444"), (16384, 300, 100, "420"), (512, 512, 1, "444"), (300, 16384, 37, "444")):
        h = frames.jpeg_header(H, W, q, ss)
        assert len(h) == 629 and h == jpeg_ref.header(H, W, q, ss), (H, W, q, ss)
    h = frames.jpeg_header(17, 23, 90, "420")
    assert h[:20] == b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert h[20:25] == b"\xff\xdb\x00\x43\x00" and h[25:29] == bytes([3, 2, 2, 3])      # luma at quality 90, zigzag order
    sof = h.index(b"\xff\xc0")
    assert h[sof:sof + 19] == b"\xff\xc0\x00\x11\x08\x00\x11\x00\x17\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    assert h[-20:-14] == b"\xff\xdd\x00\x04\x00\x02" and h[-14:] == b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert all(_streams(c)[0][:629] == frames.jpeg_header(*jc.frames(c[0]).shape[1:3], c[2], c[1]) for c in jc.CASES)
    for bad in ((0, 4, 90, "420"), (4, 16385, 90, "420"), (4, 4, 0, "420"), (4, 4, 101, "444")):
        with pytest.raises(ValueError):
            frames.jpeg_header(*bad)
    with pytest.raises(ValueError, match="unknown subsampling"):
        frames.jpeg_header(4, 4, 90, "422")


def test_bound_and_default_cap():
    L = capi.lib()
    assert frames.jpeg_default_cap(512, 512) == 512 * 512 * 3 + 1024 and frames.jpeg_default_cap(1, 1) == 1027
    assert frames.jpeg_bound(16, 16, "420") == 629 + 2 * ((6 * 1658 + 7) // 8) + 2
    assert frames.jpeg_bound(8, 8, "444") == 629 + 2 * ((3 * 1658 + 7) // 8) + 2
    assert frames.jpeg_bound(16384, 16384, "444") == jpeg_ref.bound(16384, 16384, "444") > 2 ** 32
    for case in jc.CASES:
        name, ss, _ = case
        _, H, W, _ = jc.frames(name).shape
        assert frames.jpeg_bound(H, W, ss) == jpeg_ref.bound(H, W, ss)
        for data in _streams(case):
            assert len(data) <= frames.jpeg_bound(H, W, ss), case
            if name not in jc.NOISE:
                assert len(data) <= frames.jpeg_default_cap(H, W), case
    for bad in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        assert L.artalk_jpeg_default_cap(*bad) < 0 and L.artalk_jpeg_bound(*bad, capi.JPEG_420) < 0
        with pytest.raises(ValueError):
            frames.jpeg_default_cap(*bad)
    assert L.artalk_jpeg_bound(4, 4, 0) < 0 and L.artalk_jpeg_bound(4, 4, 3) < 0
    with pytest.raises(ValueError, match="unknown subsampling"):
        frames.jpeg_bound(4, 4, "422")


# ------------------------------------------------------------------------------------------------ refusals
def _check(F=1, H=8, W=8, quality=90, ss=capi.JPEG_420, cap=4096, rgb=1, out=1, sizes=1):
    msg = C.create_string_buffer(256)
    rc = capi.lib().artalk_op_jpeg_check(F, H, W, quality, ss, cap, rgb, out, sizes, msg, 256)
    return rc, msg.value.decode()


def test_refusals():
    assert (capi.JPEG_420, capi.JPEG_444) == (1, 2)
    assert _check() == (capi.OK, "") and _check(ss=capi.JPEG_444, H=1, W=1, quality=1) == (capi.OK, "")
    assert _check(H=16384, W=16384, quality=100, cap=631)[0] == capi.OK
    assert _check(F=0, rgb=0, out=0, sizes=0) == (capi.OK, "")      # F = 0: the pointers are not looked at
    for q in (0, 101, -5):
        rc, msg = _check(quality=q)
        assert rc == capi.EINVAL and "quality" in msg and "1..100" in msg
    for ss in (0, 3, -1):
        rc, msg = _check(ss=ss)
        assert rc == capi.EINVAL and "unknown subsampling" in msg
    for H, W in ((0, 4), (4, 0), (-2, 4), (16385, 4), (4, 16385)):
        rc, msg = _check(H=H, W=W)
        assert rc == capi.EINVAL and "1..16384" in msg, (H, W)
    rc, msg = _check(F=-1)
    assert rc == capi.EINVAL and "negative" in msg
    for ptrs in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        rc, msg = _check(rgb=ptrs[0], out=ptrs[1], sizes=ptrs[2])
        assert rc == capi.EINVAL and "NULL" in msg
    for cap in (630, 0, -1):
        rc, msg = _check(cap=cap)
        assert rc == capi.EINVAL and "cap" in msg and "631" in msg
    assert _check(cap=631)[0] == capi.OK


def test_the_entry_points_refuse_before_the_device_is_touched():
    L = capi.lib()
    fake = C.c_void_p(4096)      # never dereferenced: every call below is refused on the host, or launches nothing
    h = C.c_void_p()
    assert L.artalk_jpeg_create(0, None) == capi.EINVAL and L.artalk_jpeg_create(-1, C.byref(h)) == capi.EINVAL
    assert L.artalk_jpeg_create(0, C.byref(h)) == capi.OK and h.value      # the object takes nothing from the device before it encodes
    try:
        enc = lambda *a: L.artalk_jpeg_encode(h, *a)
        assert enc(fake, 1, 8, 8, 0, capi.JPEG_420, fake, 4096, fake, None) == capi.EINVAL and b"quality" in L.artalk_jpeg_last_error(h)
        assert enc(fake, 1, 8, 8, 90, 7, fake, 4096, fake, None) == capi.EINVAL and b"unknown subsampling" in L.artalk_jpeg_last_error(h)
        assert enc(fake, 1, 0, 8, 90, capi.JPEG_444, fake, 4096, fake, None) == capi.EINVAL and b"1..16384" in L.artalk_jpeg_last_error(h)
        assert enc(fake, 1, 8, 16385, 90, capi.JPEG_444, fake, 4096, fake, None) == capi.EINVAL
        assert enc(fake, -1, 8, 8, 90, capi.JPEG_420, fake, 4096, fake, None) == capi.EINVAL and b"negative" in L.artalk_jpeg_last_error(h)
        assert enc(None, 1, 8, 8, 90, capi.JPEG_420, fake, 4096, fake, None) == capi.EINVAL and b"NULL" in L.artalk_jpeg_last_error(h)
        assert enc(fake, 1, 8, 8, 90, capi.JPEG_420, None, 4096, fake, None) == capi.EINVAL
        assert enc(fake, 1, 8, 8, 90, capi.JPEG_420, fake, 4096, None, None) == capi.EINVAL
        assert enc(fake, 1, 8, 8, 90, capi.JPEG_420, fake, 630, fake, None) == capi.EINVAL and b"cap" in L.artalk_jpeg_last_error(h)
        assert enc(None, 0, 8, 8, 90, capi.JPEG_420, None, 4096, None, None) == capi.OK      # F = 0 launches nothing
        assert L.artalk_jpeg_encode(None, fake, 1, 8, 8, 90, capi.JPEG_420, fake, 4096, fake, None) == capi.EINVAL
        assert b"NULL" in L.artalk_jpeg_last_error(None)
        ms = (C.c_double * 2)(-1.0, -1.0)
        assert L.artalk_jpeg_set_timing(None, 1) == capi.EINVAL and L.artalk_jpeg_get_timing(None, ms, 2) == capi.EINVAL
        assert L.artalk_jpeg_set_timing(h, 1) == capi.OK and L.artalk_jpeg_get_timing(h, ms, 2) == 2 and list(ms) == [0.0, 0.0]
        assert enc(None, 0, 8, 8, 90, capi.JPEG_420, None, 4096, None, None) == capi.OK      # timed or not, F = 0 launches nothing
    finally:
        L.artalk_jpeg_destroy(h)
    L.artalk_jpeg_destroy(None)
    buf = (C.c_uint8 * 629)()
    assert L.artalk_jpeg_header(8, 8, 90, capi.JPEG_420, buf, 628) == capi.EINVAL and L.artalk_jpeg_header(8, 8, 90, capi.JPEG_420, None, 629) == capi.EINVAL
    assert L.artalk_jpeg_header(8, 8, 90, capi.JPEG_420, buf, 629) == 629


def test_encode_jpeg_refuses_on_the_host():
    rgb = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.encode_jpeg(rgb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.encode_jpeg(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.JpegEncoder(device="cpu")
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling="422"), dict(subsampling=None), dict(cap=630)):
        with pytest.raises(ValueError):
            frames.encode_jpeg(rgb, **kw)
    with pytest.raises(ValueError):
        frames.encode_jpeg(np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="not \\['colour'\\]"):
        frames.jpeg_options(dict(colour="gray"))
    assert frames.jpeg_options(None) == (90, "420", None) and frames.jpeg_options(dict(quality=75, subsampling="444", cap=9000)) == (75, "444", 9000)


def test_jpeg_is_not_a_frame_format():
    with pytest.raises(ValueError, match="unknown frame format"):
        frames.format_code("jpeg")
    with pytest.raises(ValueError, match="unknown frame format"):
        frames.frame_bytes("jpeg", 8, 8)
    assert sorted(frames.FORMATS) == ["rgb24", "yuv420p"]
    for code in (0, 3):      # the JPEG encoder is no third ARTALK_FRAMES_* code
        assert capi.lib().artalk_frames_bytes(code, 8, 8) < 0


NEW_SYMBOLS = ("artalk_jpeg_default_cap", "artalk_jpeg_bound", "artalk_jpeg_header", "artalk_jpeg_create", "artalk_jpeg_destroy",
               "artalk_jpeg_last_error", "artalk_jpeg_encode", "artalk_op_jpeg_check", "artalk_jpeg_set_timing", "artalk_jpeg_get_timing")


def test_symbols_are_exported_and_declared():
    L = capi.lib()
    header = open(os.path.join(REPO, "include", "artalk_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in capi.SYMBOLS and name + "(" in header, name
    assert "#define ARTALK_JPEG_420 1" in header and "#define ARTALK_JPEG_444 2" in header


def test_no_pillow_in_the_package():
    pkg = os.path.join(REPO, "artalk_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert "import PIL" not in src and "from PIL" not in src, f


# ------------------------------------------------------------------------------------------------ Motion-JPEG on the host
def _slots(streams, cap):
    data = np.full((len(streams), cap), 0xA5, np.uint8)
    for f, b in enumerate(streams):
        data[f, :len(b)] = np.frombuffer(b, np.uint8)
    return torch.from_numpy(data), torch.tensor([len(b) for b in streams], dtype=torch.int64)


def test_mjpeg_round_trip(tmp_path):
    streams = list(_streams(("three48x64", "444", 90))) + list(_streams(("noise32x48", "444", 100))) + list(_streams(("rows136x16", "444", 90)))
    data, sizes = _slots(streams, max(len(b) for b in streams) + 7)
    assert frames.split_jpeg(data, sizes) == streams
    assert frames.split_jpeg(data.numpy(), sizes.numpy()) == streams
    path = tmp_path / "clip.mjpeg"
    assert frames.write_mjpeg(path, data, sizes) == len(streams)
    assert path.read_bytes() == b"".join(streams)
    assert frames.read_mjpeg(path) == streams
    assert frames.write_mjpeg(path, data[:0], sizes[:0]) == 0 and path.read_bytes() == b"" and frames.read_mjpeg(path) == []
    assert frames.split_jpeg(data[:0], sizes[:0]) == []
    (tmp_path / "junk.mjpeg").write_bytes(b"RIFF....")
    with pytest.raises(ValueError, match="SOI"):
        frames.read_mjpeg(tmp_path / "junk.mjpeg")
    (tmp_path / "short.mjpeg").write_bytes(streams[0][:-2])
    with pytest.raises(ValueError, match="EOI"):
        frames.read_mjpeg(tmp_path / "short.mjpeg")


def test_read_mjpeg_is_not_fooled_by_marker_bytes_in_a_header(tmp_path):
    """a quantisation table may hold 255 next to 216 or 217: FF D8 / FF D9 inside DQT, where no stuffing protects them"""
    h = bytearray(jpeg_ref.header(8, 8, 90, "444"))
    h[25:27] = b"\xff\xd9"
    h[30:32] = b"\xff\xd8"
    fake = bytes(h) + _streams(("8x8", "444", 90))[0][629:]
    (tmp_path / "two.mjpeg").write_bytes(fake + fake)
    assert frames.read_mjpeg(tmp_path / "two.mjpeg") == [fake, fake]


def test_split_jpeg_raises_for_a_frame_that_did_not_fit():
    streams = list(_streams(("three48x64", "420", 90)))
    data, sizes = _slots(streams, 4000)
    sizes[1] = -5000
    with pytest.raises(ValueError, match="frame 1 .*4000 bytes.* needs 5000"):
        frames.split_jpeg(data, sizes)
    with pytest.raises(ValueError):
        frames.write_mjpeg(os.devnull, data, sizes)
    with pytest.raises(ValueError):
        frames.split_jpeg(data, sizes[:2])


# ------------------------------------------------------------------------------------------------ the engine and the head
def test_rendering_output_jpeg_needs_a_renderer():
    from artalk_amd.engine import ARTAvatarInferEngine
    eng = ARTAvatarInferEngine(model=types.SimpleNamespace(cfg=None))
    eng.flame_model = object()      # the mesh branch would return vertices: there is nothing to encode
    assert getattr(eng, "mesh_renderer", None) is None
    with pytest.raises(ValueError, match="mesh_renderer"):
        eng.rendering(None, torch.zeros(2, 106), output="jpeg")
    with pytest.raises(ValueError, match="quality"):
        eng.rendering(None, torch.zeros(2, 106), output="jpeg", jpeg=dict(quality=0))
    with pytest.raises(ValueError, match="jpeg= goes with"):
        eng.rendering(None, torch.zeros(2, 106), output="rgb24", jpeg=dict(quality=80))
    with pytest.raises(RuntimeError, match="GAGAvatar"):
        eng.stream_render([], torch.zeros(0, 4, 106), [], output="jpeg")
