"""The kernels of ``csrc/jpeg.hip`` alone: ``artalk_jpeg_encode`` on every case of tests/jpeg_cases.py, byte-equal to the numpy restatement
of tests/jpeg_ref.py, with ``data`` and ``sizes`` between poisoned guard bands; overflow (a negative size, nothing written outside the
slot, neighbours untouched); the guaranteed bound; a second run, a side stream, an unaligned source; the float front door; one encoder
object across sizes and subsamplings.  Needs only numpy on the GPU machine."""
import functools

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_ref
from artalk_amd import capi
from artalk_amd import frames

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = 0xA5


@functools.lru_cache(maxsize=None)
def _want(case):
    """-> the restatement's streams of the case's frames: computed once, shared"""
    name, ss, q = case
    return tuple(jpeg_ref.encode(x, q, ss) for x in jc.frames(name))


@functools.lru_cache(maxsize=None)
def _encoder(ss, q):
    return frames.JpegEncoder(quality=q, subsampling=ss)


def _encode(rgb_dev, ss, q, cap, stream=None, encoder=None):
    """one artalk_jpeg_encode call into guarded buffers -> (data (F, cap), sizes (F,)) as numpy, after the guard bands are checked"""
    F = int(rgb_dev.shape[0])
    buf = torch.full((F * cap + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
    szb = torch.full((F + 2,), -0x5A5A5A5A, dtype=torch.int64, device="cuda")
    data, sizes = buf[GUARD:GUARD + F * cap].view(F, cap), szb[1:1 + F]
    s = stream if stream is not None else torch.cuda.current_stream()
    torch.cuda.synchronize()      # the source and the poison are in place whichever stream the launch goes to
    with torch.cuda.stream(s):
        (encoder or _encoder(ss, q)).encode(rgb_dev, cap=cap, out=(data, sizes))
    s.synchronize()
    whole, sz = buf.cpu().numpy(), szb.cpu().numpy()
    assert (whole[:GUARD] == POISON).all() and (whole[GUARD + F * cap:] == POISON).all(), "the kernels wrote outside data"
    assert sz[0] == -0x5A5A5A5A and sz[-1] == -0x5A5A5A5A, "the kernels wrote outside sizes"
    return whole[GUARD:GUARD + F * cap].reshape(F, cap), sz[1:1 + F]


def _assert_streams(data, sizes, want, what=""):
    for f, w in enumerate(want):
        assert int(sizes[f]) == len(w), f"{what}frame {f}: size {int(sizes[f])}, the restatement's stream has {len(w)} bytes"
        got = data[f, :len(w)]
        bad = np.flatnonzero(got != np.frombuffer(w, np.uint8))
        assert bad.size == 0, f"{what}frame {f}: {bad.size} of {len(w)} bytes differ, the first at {bad[:4]}"


def _cap(case):
    name, ss, _ = case
    _, H, W, _ = jc.frames(name).shape
    return frames.jpeg_bound(H, W, ss) if name in jc.NOISE else frames.jpeg_default_cap(H, W)


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_encode_equals_the_restatement(case):
    name, ss, q = case
    rgb = torch.from_numpy(jc.frames(name).copy()).cuda()
    data, sizes = _encode(rgb, ss, q, _cap(case))
    _assert_streams(data, sizes, _want(case))
    again, sizes2 = _encode(rgb, ss, q, _cap(case))      # a second run: byte-identical below sizes
    assert (sizes2 == sizes).all()
    for f, n in enumerate(sizes):
        assert (again[f, :n] == data[f, :n]).all()


@pytest.mark.parametrize("ss", jc.BOTH)
def test_overflow_reports_the_bytes_needed_and_writes_nothing_outside_the_slot(ss):
    case = ("noise32x48", ss, 100)
    want = _want(case)
    cap = frames.JPEG_HEADER_BYTES + 64
    data, sizes = _encode(torch.from_numpy(jc.frames("noise32x48").copy()).cuda(), ss, 100, cap)
    assert len(want[0]) > cap and int(sizes[0]) == -len(want[0])


@pytest.mark.parametrize("ss", jc.BOTH)
def test_neighbours_of_an_overflowing_frame_keep_their_solo_bytes(ss):
    case = ("three48x64", ss, 90)
    want = _want(case)
    cap = max(len(want[0]), len(want[2])) + 5      # the noise frame in the middle needs more
    assert len(want[1]) > cap
    data, sizes = _encode(torch.from_numpy(jc.frames("three48x64").copy()).cuda(), ss, 90, cap)
    assert int(sizes[1]) == -len(want[1])
    for f in (0, 2):
        assert int(sizes[f]) == len(want[f])
        assert data[f, :len(want[f])].tobytes() == want[f]


@pytest.mark.parametrize("case", [c for c in jc.CASES if c[0] in ("noise32x48", "checker16x32", "1x1")], ids=jc.case_id)
def test_the_bound_never_overflows(case):
    name, ss, q = case
    x = jc.frames(name)
    cap = frames.jpeg_bound(x.shape[1], x.shape[2], ss)
    assert cap == jpeg_ref.bound(x.shape[1], x.shape[2], ss)
    data, sizes = _encode(torch.from_numpy(x.copy()).cuda(), ss, q, cap)
    assert (sizes > 0).all() and (sizes <= cap).all()
    _assert_streams(data, sizes, _want(case))


def _edge_picture(H, W, seed):
    """half smooth, half noise: long and short segments side by side"""
    x = jc._smooth(H, W, seed).copy()
    x[:, W // 2:] = jc._noise(H, W - W // 2, seed)
    return x[None]


# the kernels' own edges: a segment of more than 252 blocks (two pieces: the DC predictors and the bit offset carry over), a segment of
# more than 2048 bytes (two pieces of the stuffing copy), more than 256 MCU rows (the sum over a frame's segments takes two rounds)
@pytest.mark.parametrize("shape,ss", [((8, 1000), "444"), ((16, 700), "420"), ((8, 2030), "444"), ((2056, 8), "444"), ((4112, 16), "420")],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_kernel_edges(shape, ss):
    x = _edge_picture(*shape, seed=11)
    want = (jpeg_ref.encode(x[0], 100, ss),)
    cap = frames.jpeg_bound(shape[0], shape[1], ss)
    data, sizes = _encode(torch.from_numpy(x).cuda(), ss, 100, cap)
    _assert_streams(data, sizes, want)


def test_side_stream_and_unaligned_source():
    case = ("17x23", "420", 90)
    x = jc.frames("17x23")
    flat = torch.zeros(x.size + 16, dtype=torch.uint8, device="cuda")
    flat[1:1 + x.size] = torch.from_numpy(x.copy()).cuda().reshape(-1)
    view = flat[1:1 + x.size].view(x.shape)      # one byte off a 16-byte boundary
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    side = torch.cuda.Stream()
    data, sizes = _encode(view, "420", 90, _cap(case), stream=side)
    _assert_streams(data, sizes, _want(case), "side stream, unaligned: ")


def test_float_frames_go_through_pack_frames():
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(2, 3, 24, 40, generator=g) * 1.2 - 0.1).cuda()
    rgb = frames.pack_frames(x, "rgb24")
    a, an = frames.encode_jpeg(x, quality=90, subsampling="444")
    b, bn = frames.encode_jpeg(rgb, quality=90, subsampling="444")
    assert torch.equal(an, bn) and (an > 0).all()
    for f in range(2):
        assert torch.equal(a[f, :an[f]], b[f, :bn[f]])
    want = [jpeg_ref.encode(r, 90, "444") for r in rgb.cpu().numpy()]
    assert frames.split_jpeg(a, an) == want
    h, hn = frames.encode_jpeg(rgb, quality=90, subsampling="444", host=True)
    torch.cuda.current_stream().synchronize()
    assert h.is_pinned() and hn.is_pinned() and not h.is_cuda
    assert frames.split_jpeg(h, hn) == want


def test_one_encoder_across_sizes_and_subsamplings():
    """scratch grows (a small picture first, then one with more and longer segments) and the header cache holds one entry per size"""
    for ss in jc.BOTH:
        enc = frames.JpegEncoder(quality=90, subsampling=ss)
        for name in ("8x8", "three48x64", "8x8", "17x23"):
            case = (name, ss, 90)
            rgb = torch.from_numpy(jc.frames(name).copy()).cuda()
            data, sizes = _encode(rgb, ss, 90, _cap(case), encoder=enc)
            _assert_streams(data, sizes, _want(case), f"{name} {ss}: ")
        enc.close()


def test_zero_frames_launch_nothing():
    data, sizes = frames.encode_jpeg(torch.empty(0, 8, 8, 3, dtype=torch.uint8, device="cuda"))
    assert tuple(data.shape) == (0, frames.jpeg_default_cap(8, 8)) and tuple(sizes.shape) == (0,)
    assert frames.split_jpeg(data, sizes) == []
