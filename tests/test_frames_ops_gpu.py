"""The kernels of ``csrc/frames.hip`` alone: ``artalk_frames_pack`` on every case of tests/frames_cases.py, byte-equal to the integer
restatement of tests/frames_ref.py, with its output between poisoned guard bands; the same bytes from a second call and from a side
stream; a source that starts one float past a 16-byte boundary; and the fused finish-and-pack kernel (``artalk_op_gaga_finish_pack``)
against ``artalk_op_gaga_finish`` followed by ``artalk_frames_pack``."""
import functools

import numpy as np
import pytest
import torch

import frames_cases as fc
import frames_ref as fr
import gaga_cases as gc
import gaga_ref
from artalk_amd import capi
from artalk_amd import frames

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = 0xA5


@functools.lru_cache(maxsize=None)
def _case(case):
    """-> (source float32 (F, 3, H, W), expected bytes, flat): computed once, shared, read only"""
    fmt, shape, fill = case
    x = fc.make(shape, fill)
    want = fr.pack(x, fmt).reshape(-1)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def _pack(x_dev, fmt, stream=None):
    """one artalk_frames_pack launch into a guarded buffer -> the bytes, flat, after the guard bands are checked"""
    F, _, H, W = x_dev.shape
    n = F * frames.frame_bytes(fmt, H, W)
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream()
    torch.cuda.synchronize()      # the source and the poison are in place whichever stream the launch goes to
    rc = capi.lib().artalk_frames_pack(capi.ptr(x_dev), F, H, W, frames.FORMATS[fmt], capi.ptr(buf[GUARD:]), s.cuda_stream)
    assert rc == capi.OK, capi.lib().artalk_frames_last_error()
    s.synchronize()
    whole = buf.cpu().numpy()
    assert (whole[:GUARD] == POISON).all() and (whole[GUARD + n:] == POISON).all(), "the kernel wrote outside its output"
    return whole[GUARD:GUARD + n]


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_pack_equals_the_restatement(case):
    x, want = _case(case)
    got = _pack(torch.from_numpy(x.copy()).cuda(), case[0])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {want.size} bytes differ, the first at {bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}"


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_pack_is_the_same_on_every_call_and_stream(case):
    x, want = _case(case)
    dev = torch.from_numpy(x.copy()).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    first, second, third = _pack(dev, case[0]), _pack(dev, case[0]), _pack(dev, case[0], stream=side)
    assert np.array_equal(first, second) and np.array_equal(first, third) and np.array_equal(first, want)


@pytest.mark.parametrize("case", fc.OFFSET_CASES, ids=fc.case_id)
def test_a_view_off_a_16_byte_boundary(case):
    fmt, shape, _ = case
    x, want = _case(case)
    aligned = torch.from_numpy(x.copy()).cuda()
    flat = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(aligned.shape)
    view.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    got = frames.pack_frames(view, fmt)      # the view goes in as it is
    assert got.dtype == torch.uint8 and tuple(got.shape) == frames.frame_shape(fmt, *shape)
    assert np.array_equal(got.cpu().numpy().reshape(-1), _pack(aligned, fmt))
    assert np.array_equal(_pack(view, fmt), want)


def test_pack_frames_takes_a_non_contiguous_tensor_and_no_frames():
    x, want = _case(("rgb24", (2, 7, 13), "random"))
    nhwc = torch.from_numpy(x.copy()).cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not nhwc.is_contiguous()
    assert np.array_equal(frames.pack_frames(nhwc, "rgb24").cpu().numpy().reshape(-1), want)
    for fmt in ("rgb24", "yuv420p"):
        empty = frames.pack_frames(torch.empty(0, 3, 4, 6, device="cuda"), fmt)
        assert tuple(empty.shape) == frames.frame_shape(fmt, 0, 4, 6) and empty.dtype == torch.uint8
    with pytest.raises(ValueError, match="even"):
        frames.pack_frames(torch.zeros(1, 3, 3, 4, device="cuda"), "yuv420p")


@pytest.mark.parametrize("fmt", ("rgb24", "yuv420p"))
@pytest.mark.parametrize("mark", gc.FINISH_MARKS)
def test_fused_finish_and_pack_equals_finish_then_pack(mark, fmt):
    L = capi.lib()
    S, F = gc.FINISH_S, 2
    g = torch.Generator().manual_seed(9)
    img = torch.randn(F, 3, S, S, generator=g) * 0.8 + 0.5
    img.view(-1)[:9] = torch.tensor([-3.0e38, 3.0e38, -1e-30, 0.0, 1.0, 1.0 + 2.0 ** -23, 1e-30, 1.0 - 2.0 ** -24, float("nan")])
    img[1, :, -1, -1] = torch.tensor([-5.0, 7.0, 0.5])      # the last pixel, inside every watermark
    wm = gc.water_mark(*mark) if mark else None
    dwm = wm.cuda() if mark else None
    h, w = mark if mark else (0, 0)
    src = img.cuda()
    n = F * frames.frame_bytes(fmt, S, S)
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
    s = capi.current_stream_ptr()
    assert L.artalk_op_gaga_finish_pack(capi.ptr(src), F, S, capi.ptr(dwm), h, w, frames.FORMATS[fmt], capi.ptr(buf[GUARD:]), s) == capi.OK
    torch.cuda.synchronize()
    assert torch.equal(src.cpu().view(torch.int32), img.view(torch.int32)), "the fused kernel modified its source"
    whole = buf.cpu().numpy()
    assert (whole[:GUARD] == POISON).all() and (whole[GUARD + n:] == POISON).all(), "the kernel wrote outside its output"
    fused = whole[GUARD:GUARD + n]
    two = src.clone()
    assert L.artalk_op_gaga_finish(capi.ptr(two), F, S, capi.ptr(dwm), h, w, s) == capi.OK
    assert np.array_equal(fused, _pack(two, fmt)), "fused differs from finish followed by pack"
    # and both are what the torch statement of the finish, quantised on the CPU, gives
    finished = gaga_ref.finish_torch(torch.nan_to_num(img, nan=0.0), wm).numpy()
    assert np.array_equal(fused, fr.pack(finished, fmt).reshape(-1))
    if mark:
        assert not np.array_equal(fused, fr.pack(img.numpy(), fmt).reshape(-1)), "the watermark does not show"
