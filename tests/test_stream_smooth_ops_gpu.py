"""savgol_stream_kernel alone (artalk_op_savgol_stream): the Savitzky-Golay filter of artalk_savgol on live sessions, 4 frames late.

The bar is identical bits: a frame is the same operations in the same order whichever of the two kernels emits it (both go through one
device function), so the concatenated emitted frames must EQUAL artalk_savgol on the concatenated raw frames.  The same output is also
held against scipy's savgol_filter at the bar of test_e2e_gpu.py::test_savgol_device_matches_scipy, 2e-6.

Every launch serves 3 sessions in different phases: X, the stream under test, from its first frame; Y and Z, two companions that are
1 and 2 chunks into a longer stream (their carries are written by hand before the first launch, by the kernel afterwards).  Slot
pointers are permuted and non-contiguous, the raw stride is wider than a row, raw rows past n_frames are NaN, the output is pre-filled
with 0xAB, and every pool byte outside the three carries must stay what it was."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import get_gpu_model

pytestmark = pytest.mark.gpu

D = 106
CARRY_OFF = 768 + 181 * 768 + 100 * 32              # [style | prev_in | prev_fdec | carry]: the carry's place in a pool slot, in floats
CARRY = 9 * D                                       # 954 floats, padded to 956 (16 bytes)
SLOT = CARRY_OFF + 956
RAW_STRIDE = 100 * D + 22
OUT_STRIDE = 104 * D + 10
FILL = np.array([0xABABABAB], dtype=np.uint32).view(np.int32)[0].item()
COMPANION = [(100, False)] * 5 + [(57, True)]       # Y starts at its call 1, Z at its call 2

SCHEDULES = {
    "100_100_1L": [(100, False), (100, False), (1, True)],
    "100L": [(100, True)],
    "9L": [(9, True)],
    "100_8L": [(100, False), (8, True)],
    "100_100_flush": [(100, False), (100, False), (0, True)],
    "100_100_100_57L": [(100, False), (100, False), (100, False), (57, True)],
}

_shared = {}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def savgol_device(x):
    """artalk_savgol on a whole clip (T, 106): the reference of the bit comparison."""
    from artalk_amd.engine import ARTAvatarInferEngine
    eng = ARTAvatarInferEngine.__new__(ARTAvatarInferEngine)
    eng.ARTalk = get_gpu_model("tiny")
    return eng.smooth_motion_savgol(x.cuda()).cpu()


def companion_clips():
    """The raw frames of Y and Z and their whole-clip filter outputs, computed once and left unchanged."""
    if "companions" not in _shared:
        total = sum(nf for nf, _ in COMPANION)
        clips = [torch.randn(total, D, generator=torch.Generator().manual_seed(900 + i)) for i in range(2)]
        _shared["companions"] = [(c, savgol_device(c)) for c in clips]
    return _shared["companions"]


def span(seen, nf, last):
    first = max(0, seen - 4)
    return first, (seen + nf if last else seen + nf - 4) - first


@pytest.mark.parametrize("case", sorted(SCHEDULES))
def test_stream_equals_whole_clip_filter_bit_for_bit(case):
    from artalk_amd import capi
    L = capi.lib()
    sched = SCHEDULES[case]
    T = sum(nf for nf, _ in sched)
    x = torch.randn(T, D, generator=torch.Generator().manual_seed(sum(map(ord, case))))
    want = savgol_device(x)
    (y, want_y), (z, want_z) = companion_clips()
    # three streams: (raw clip, whole-clip reference, schedule, index of the first call made here, pool slot)
    streams = [dict(raw=x, want=want, calls=sched, at=0, slot=3), dict(raw=y, want=want_y, calls=COMPANION, at=1, slot=0),
               dict(raw=z, want=want_z, calls=COMPANION, at=2, slot=4)]
    rows = [2, 0, 1]                                 # row order of every launch: Z, X, Y
    g = torch.Generator().manual_seed(7)
    pool0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (5, SLOT), dtype=torch.int32, generator=g)      # X's carry starts as garbage: seen == 0 must not read it
    for st in streams:
        st["seen"] = sum(nf for nf, _ in st["calls"][:st["at"]])
        if st["seen"]:
            pool0[st["slot"], CARRY_OFF:CARRY_OFF + CARRY] = st["raw"][st["seen"] - 9:st["seen"]].reshape(-1).view(torch.int32)
        st["got"] = []
    pool = pool0.cuda()
    table = torch.tensor([pool.data_ptr() + streams[r]["slot"] * SLOT * 4 for r in rows], dtype=torch.int64, device="cuda")
    expect_pool = pool0.clone()
    for j in range(len(sched)):
        live = [streams[r] for r in rows]
        calls = [st["calls"][st["at"] + j] for st in live]
        raw = torch.full((3, RAW_STRIDE), float("nan"))
        for i, (st, (nf, _)) in enumerate(zip(live, calls)):
            raw[i, :nf * D] = st["raw"][st["seen"]:st["seen"] + nf].reshape(-1)
        raw_d = raw.cuda()
        out = torch.full((3, OUT_STRIDE), FILL, dtype=torch.int32, device="cuda")
        seen = (C.c_int32 * 3)(*[st["seen"] for st in live])
        nfs = (C.c_int32 * 3)(*[nf for nf, _ in calls])
        last = (C.c_uint8 * 3)(*[int(l) for _, l in calls])
        assert len({st["seen"] for st in live}) == 3, "the three sessions of a launch are in different phases"
        assert L.artalk_op_savgol_stream(_p(table), _p(raw_d), RAW_STRIDE, seen, nfs, last, _p(out), OUT_STRIDE, 3, None) == capi.OK
        res = out.cpu()
        for i, (st, (nf, lst)) in enumerate(zip(live, calls)):
            first, count = span(st["seen"], nf, lst)
            got = res[i, :count * D].view(torch.float32).reshape(count, D)
            ref = st["want"][first:first + count]
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), \
                f"{case} launch {j} row {i}: frames {first}..{first + count - 1} differ from artalk_savgol by {(got - ref).abs().max().item():.3e}"
            assert (res[i, count * D:] == FILL).all(), f"{case} launch {j} row {i}: output past frame {count} was written"
            st["got"].append(got)
            st["seen"] += nf
            keep = min(9, st["seen"])
            expect_pool[st["slot"], CARRY_OFF:CARRY_OFF + keep * D] = st["raw"][st["seen"] - keep:st["seen"]].reshape(-1).view(torch.int32)
        assert torch.equal(pool.cpu(), expect_pool), f"{case} launch {j}: a pool word outside the carries changed, or a carry is not the last 9 raw frames"
    mine = torch.cat(streams[0]["got"])
    assert mine.shape == (T, D) and torch.equal(mine.view(torch.int32), want.view(torch.int32))
    from scipy.signal import savgol_filter          # what the reference calls (inference.py:91-94)
    ref = savgol_filter(x.numpy(), window_length=5, polyorder=2, axis=0)
    ref[..., 100:103] = savgol_filter(x.numpy()[..., 100:103], window_length=9, polyorder=3, axis=0)
    err = float(np.abs(mine.numpy() - ref).max())
    print(f"{case}: {T} frames in {len(sched)} calls, bit-identical to artalk_savgol, max-abs difference from scipy {err:.3e}")
    assert err < 2e-6
