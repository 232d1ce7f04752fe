"""The live audio front door without a GPU (artalk_amd/live_audio.py, csrc/pcm.hip): the arithmetic that host and device share - which
groups are final, what a push emits, what it carries - by brute force; a float32 emulation of push, carry and end that pins the
definition (any packetisation gives the bits of the whole signal); every refusal, on a handle without a device; the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from artalk_amd import capi, live_audio
from audio_cases import RATES, RATIOS, ceil_out, make_signal, taps
from audio_ref import kernel_order_f32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = sorted({(o, nw, w) for o, nw, w, _ in RATES.values()} | {(1, 1, 0)})
PLAN_KEYS = ("n_out", "lead", "carry_n", "carry_from", "carry_out_n", "groups")


def c_plan(n_before, frames, end, orig, nw, width):
    out = (C.c_int64 * 6)()
    assert capi.lib().artalk_op_pcm_plan(n_before, frames, int(end), orig, nw, width, out) == capi.OK
    return dict(zip(PLAN_KEYS, out))


# ---------------------------------------------------------------------------------------------- the arithmetic
def test_rates_are_the_whole_clip_paths():
    from artalk_amd.audio import sinc_resample_kernel
    for sr, (orig, nw, width, ntaps) in RATES.items():
        assert live_audio.rate_geometry(sr) == (orig, nw, width)
        t, o, n, w = live_audio.rate_taps(sr)
        ref = sinc_resample_kernel(sr, 16000)[0]
        assert (o, n, w) == (orig, nw, width) and t.shape == (nw, ntaps) and torch.equal(t.view(torch.int32), ref.view(torch.int32))
    t, o, n, w = live_audio.rate_taps(16000)
    assert (o, n, w) == (1, 1, 0) and t.tolist() == [[1.0]]


@pytest.mark.parametrize("orig,nw,width", GEOMETRIES)
def test_emitted_count_is_the_number_of_groups_whose_last_read_has_arrived(orig, nw, width):
    ntaps = 2 * width + orig
    for n_in in range(0, 3 * (width + orig) + 1):
        # group j reads frames j orig - width .. j orig - width + ntaps - 1; it is final when the largest has arrived
        final = sum(1 for j in range(n_in + 1) if j * orig - width + ntaps - 1 < n_in)
        assert live_audio.final_groups(n_in, orig, width) == final
        assert live_audio.emitted(n_in, orig, nw, width) == nw * final == nw * max(0, (n_in - width) // orig)
        assert c_plan(0, n_in, False, orig, nw, width)["n_out"] == nw * final
        assert nw * final <= live_audio.total_outputs(n_in, orig, nw) == -((-n_in * nw) // orig)


@pytest.mark.parametrize("orig,nw,width", GEOMETRIES)
def test_any_split_emits_the_whole_signals_samples_and_carries_less_than_a_filter(orig, nw, width):
    g = np.random.default_rng(orig * 1000 + nw)
    ntaps = 2 * width + orig
    for trial in range(40):
        n = int(g.integers(0, 4 * ntaps + 7))
        sizes, left = [], n
        while left > 0:
            s = int(min(left, g.choice([0, 1, 2, 7, orig, max(0, ntaps - 2), ntaps, 2 * ntaps + 1])))
            sizes.append(s)
            left -= s
        n_in = written = 0
        carry = 0
        for s in sizes:
            q = live_audio.plan(n_in, s, False, orig, nw, width)
            assert q == c_plan(n_in, s, False, orig, nw, width)
            assert q["carry_n"] == carry <= ntaps - 1 and 0 <= q["lead"] <= width
            assert q["carry_from"] >= q["lead"] and q["carry_from"] + q["carry_out_n"] == q["lead"] + q["carry_n"] + s
            assert q["n_out"] == q["groups"] * nw
            # every group the push emits reads inside what has arrived
            assert q["groups"] == 0 or (q["groups"] - 1) * orig + ntaps <= q["lead"] + q["carry_n"] + s
            n_in += s
            written += q["n_out"]
            carry = q["carry_out_n"]
            assert written == live_audio.emitted(n_in, orig, nw, width) and carry <= ntaps - 1
        q = live_audio.plan(n_in, 0, True, orig, nw, width)
        assert q == c_plan(n_in, 0, True, orig, nw, width)
        assert q["carry_n"] == carry and q["n_out"] >= 0
        assert written + q["n_out"] == live_audio.total_outputs(n, orig, nw) == -((-n * nw) // orig)


# ---------------------------------------------------------------------------------------------- the definition, in float32
def emulate(x, tp, orig, nw, width, sizes):
    """push, carry and end with the kernel's order (audio_ref.kernel_order_f32) on each launch's span alone."""
    nch = x.shape[0]

    def launch(span, q):
        # zeros in front so that the launch's group g is kernel_order_f32's group g + m (they stand where that function pads anyway)
        m = -((q["lead"] - width) // orig)
        z = m * orig - width + q["lead"]
        assert m >= 0 and z >= 0 and (q["lead"] == 0 or z == 0)
        xp = np.concatenate([np.zeros((nch, z), np.float32), span], axis=1)
        return kernel_order_f32(xp, tp, orig, nw, width, m * nw + q["n_out"])[m * nw:]

    carry, n_in, outs = x[:, :0], 0, []
    for s in sizes:
        q = live_audio.plan(n_in, s, False, orig, nw, width)
        assert carry.shape[1] == q["carry_n"]
        span = np.concatenate([carry, x[:, n_in:n_in + s]], axis=1)
        outs.append(launch(span, q))
        lo = q["carry_from"] - q["lead"]
        carry = span[:, lo:lo + q["carry_out_n"]]
        assert lo + q["carry_out_n"] == span.shape[1]
        n_in += s
    assert n_in == x.shape[1]
    outs.append(launch(carry, live_audio.plan(n_in, 0, True, orig, nw, width)))
    return np.concatenate(outs)


def split(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


@pytest.mark.parametrize("ratio,nch,n,sizes", [
    ("ta48000", 1, 300, "1"), ("ta48000", 2, 1501, "7"), ("ta48000", 3, 1501, "97"), ("ta48000", 2, 1501, "mixed"),
    ("ta44100", 1, 2003, "97"), ("ta44100", 2, 2003, "441"), ("ta8000", 3, 701, "7"), ("ta8000", 1, 701, "mixed"),
    ("dense_1_1_0", 2, 501, "97")])
def test_float32_emulation_of_push_carry_and_end_gives_the_whole_signals_bits(ratio, nch, n, sizes):
    r = RATIOS[ratio]
    x = make_signal("noise", nch, n, 1234 + n + nch)
    tp = taps(ratio)
    ntaps = 2 * r.width + r.orig
    if sizes == "mixed":
        parts = [0, 1, ntaps - 2, 0, 2 * ntaps + 1, 13, 1, 1]
        sz = []
        while sum(sz) < n:
            sz.append(min(parts[len(sz) % len(parts)], n - sum(sz)))
    else:
        sz = split(n, int(sizes))
    want = kernel_order_f32(x, tp, r.orig, r.nw, r.width, ceil_out(n, r))
    got = emulate(x, tp, r.orig, r.nw, r.width, sz)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- refusals (a handle without a device)
class Dry:
    """artalk_pcm_* on a handle made with ARTALK_PCM_NO_DEVICE: every call checks and counts, nothing is allocated or launched."""

    def __init__(self, block=640, ring_blocks=2, max_streams=3):
        self.L = capi.lib()
        self.h = C.c_void_p()
        assert self.L.artalk_pcm_create(-1, block, ring_blocks, max_streams, C.byref(self.h)) == capi.OK
        self.buf = bytes(1 << 16)

    def close(self):
        self.L.artalk_pcm_destroy(self.h)

    def err(self):
        return self.L.artalk_pcm_last_error(self.h).decode()

    def rate(self, sr):
        t, orig, nw, width = live_audio.rate_taps(sr)
        return self.L.artalk_pcm_set_rate(self.h, sr, capi.ptr(t), orig, nw, width)

    def open(self, sr=48000, ch=1, fmt=capi.PCM_S16):
        sid = C.c_int64(-1)
        rc = self.L.artalk_pcm_open(self.h, sr, ch, fmt, C.byref(sid))
        return rc, sid.value

    def push(self, ids, frames):
        n = len(ids)
        addr = C.cast(C.c_char_p(self.buf), C.c_void_p).value
        return self.L.artalk_pcm_push(self.h, (C.c_int64 * n)(*ids), n, (C.c_void_p * n)(*[addr] * n), (C.c_int64 * n)(*frames), 0, None)

    def end(self, ids):
        return self.L.artalk_pcm_end(self.h, (C.c_int64 * len(ids))(*ids), len(ids), None)

    def take(self, ids):
        nv = (C.c_int64 * len(ids))(*[-1] * len(ids))
        rc = self.L.artalk_pcm_take(self.h, (C.c_int64 * len(ids))(*ids), len(ids), None, 640, nv, None)
        return rc, list(nv)

    def available(self, sid):
        n, e = C.c_int64(-1), C.c_int(-1)
        rc = self.L.artalk_pcm_available(self.h, sid, C.byref(n), C.byref(e))
        return rc, n.value, e.value


@pytest.fixture
def dry():
    d = Dry()
    yield d
    d.close()


def test_create_and_formats_are_refused_before_the_device_is_touched(dry):
    L, h = capi.lib(), C.c_void_p()
    for args in ((-1, 0, 2, 1), (-1, 640, 1, 1), (-1, 640, 2, 0), (-1, 640, 2, 4097), (-1, 1 << 29, 2, 1), (-2, 640, 2, 1),
                 (0, 640, 1, 1)):      # (the last one names a real device and is refused on its numbers alone)
        assert L.artalk_pcm_create(*args, C.byref(h)) == capi.EINVAL and not h.value
    assert L.artalk_pcm_create(-1, 640, 2, 1, None) == capi.EINVAL
    assert dry.open(48000)[0] == capi.EINVAL and "tap table" in dry.err()            # a rate that was never set
    assert dry.rate(48000) == capi.OK and dry.rate(48000) == capi.OK
    t = torch.ones(1, 41)
    assert L.artalk_pcm_set_rate(dry.h, 48000, capi.ptr(t), 3, 1, 18) == capi.EINVAL  # set before, with another geometry
    assert L.artalk_pcm_set_rate(dry.h, 9, capi.ptr(t), 1000, 1, 13) == capi.EINVAL and "1026 taps" in dry.err()
    assert L.artalk_pcm_set_rate(dry.h, 9, None, 3, 1, 19) == capi.EINVAL
    assert L.artalk_pcm_set_rate(dry.h, 9, capi.ptr(t), 0, 1, 19) == capi.EINVAL
    for ch, fmt in ((0, capi.PCM_S16), (9, capi.PCM_S16), (1, 0), (1, 3)):
        assert dry.open(48000, ch, fmt)[0] == capi.EINVAL
    for ch in (1, 8):
        assert dry.open(48000, ch, capi.PCM_F32)[0] == capi.OK
    # the Python side says the same before it loads anything
    for sr in (44101, 0, -5):
        with pytest.raises(ValueError):
            live_audio.rate_geometry(sr)
    for ch, dt in ((0, "s16"), (9, "f32"), (1, "s24"), (1, "s32")):
        with pytest.raises(ValueError):
            live_audio.check_format(ch, dt)
    for kw in (dict(ring_blocks=1), dict(block=0), dict(max_streams=0)):
        with pytest.raises(ValueError):
            live_audio.LiveAudio(**kw)
    with pytest.raises(RuntimeError):
        live_audio.LiveAudio(device="cpu")


def test_every_call_is_checked_whole_and_a_refusal_changes_nothing(dry):
    assert dry.rate(48000) == capi.OK and dry.rate(16000) == capi.OK
    (_, a), (_, b), (_, c) = dry.open(48000, 2), dry.open(16000), dry.open(48000)
    assert (a, b, c) == (1, 2, 3)
    assert dry.open(48000)[0] == capi.ECAPACITY                                       # max_streams = 3
    assert dry.push([a, b], [960, 100]) == capi.OK
    state = lambda: [dry.available(s) for s in (a, b, c)]
    assert state() == [(0, 313, 0), (0, 100, 0), (0, 0, 0)]
    before = state()
    assert dry.push([a, 99], [960, 10]) == capi.EINVAL and "99" in dry.err()          # an unknown id
    assert dry.push([a, b, a], [1, 1, 1]) == capi.EINVAL and "twice" in dry.err()     # an id listed twice
    assert dry.push([a, b], [1, -1]) == capi.EINVAL                                   # a negative count
    assert dry.push([], []) == capi.EINVAL
    assert dry.take([a]) == (capi.ESTATE, [-1]) and "neither" in dry.err()            # 313 < 640 and not ended
    assert dry.take([b, c])[0] == capi.ESTATE
    assert dry.available(77)[0] == capi.EINVAL
    assert state() == before
    # the ring holds 1280: 313 + 3 x 320 = 1273 fit, the next 320 do not - and the 16 kHz stream listed with it does not move either
    for _ in range(3):
        assert dry.push([a], [960]) == capi.OK
    assert dry.push([b, a], [5, 960]) == capi.ECAPACITY and "free space" in dry.err()
    assert state() == [(0, 1273, 0), (0, 100, 0), (0, 0, 0)]
    assert dry.take([a]) == (capi.OK, [640]) and dry.available(a) == (0, 633, 0)
    assert dry.push([b, a], [5, 960]) == capi.OK and dry.available(a) == (0, 953, 0) and dry.available(b) == (0, 105, 0)
    # end: the rest is written; no push and no second end after it; the whole call is refused, its other streams included
    assert dry.end([b]) == capi.OK and dry.available(b) == (0, 105, 1)
    assert dry.push([c, b], [30, 1]) == capi.ESTATE and "ended" in dry.err() and dry.available(c) == (0, 0, 0)
    assert dry.end([c, b]) == capi.ESTATE and dry.available(c) == (0, 0, 0)
    assert dry.take([b]) == (capi.OK, [105]) and dry.available(b) == (0, 0, 1)        # ended and >= 1 sample: a short last row
    assert dry.take([b])[0] == capi.ESTATE                                            # drained
    assert dry.end([c]) == capi.OK and dry.take([c])[0] == capi.ESTATE                # ended with nothing: never ready
    # a closed id is unknown from then on, and ids are not reused
    assert dry.L.artalk_pcm_close(dry.h, b) == capi.OK and dry.L.artalk_pcm_close(dry.h, b) == capi.EINVAL
    assert dry.push([b], [1]) == capi.EINVAL and dry.end([b]) == capi.EINVAL and dry.take([b])[0] == capi.EINVAL
    assert dry.open(16000) == (capi.OK, 4)
    for fn in (dry.L.artalk_pcm_close, ):
        assert fn(None, 1) == capi.EINVAL
    assert dry.L.artalk_pcm_last_error(None) is not None


def test_counts_follow_the_arithmetic_through_pushes_end_and_takes(dry):
    assert dry.rate(44100) == capi.OK
    _, a = dry.open(44100, 1, capi.PCM_F32)
    g = np.random.default_rng(3)
    n_in = taken = 0
    for _ in range(60):
        s = int(g.choice([0, 1, 441, 882, 2000]))
        if live_audio.emitted(n_in + s, 441, 160, 17) - taken > 1280:
            assert dry.push([a], [s]) == capi.ECAPACITY
        else:
            assert dry.push([a], [s]) == capi.OK
            n_in += s
        have = live_audio.emitted(n_in, 441, 160, 17) - taken
        assert dry.available(a) == (0, have, 0)
        if have >= 640:
            assert dry.take([a]) == (capi.OK, [640])
            taken += 640
    assert dry.end([a]) == capi.OK
    have = live_audio.total_outputs(n_in, 441, 160) - taken
    assert dry.available(a) == (0, have, 1)
    while have > 0:
        assert dry.take([a]) == (capi.OK, [min(have, 640)])
        have -= min(have, 640)
    assert dry.available(a) == (0, 0, 1)


def test_descriptors_are_checked_before_a_launch():
    L = capi.lib()
    assert L.artalk_op_pcm_desc_bytes(0) == C.sizeof(capi.PcmDesc) and L.artalk_op_pcm_desc_bytes(1) == C.sizeof(capi.PcmTakeDesc)
    table = (C.c_char * 4096)()
    fake = C.addressof(table)      # stands for device addresses: a refused call reads none of them

    def desc(**kw):
        d = dict(taps=fake, data=fake, carry_in=fake, carry_out=fake, ring=fake, orig=3, nw=1, width=19, nch=2, format=capi.PCM_S16,
                 frames=960, lead=0, carry_n=38, carry_from=960, carry_out_n=38, carry_stride=41, ring_cap=1000, ring_pos=999, n_out=320)
        d.update(kw)
        return (capi.PcmDesc * 1)(capi.PcmDesc(**d))

    bad = [dict(orig=0), dict(width=-1), dict(width=511), dict(nch=0), dict(nch=9), dict(format=0), dict(frames=-1), dict(taps=None),
           dict(data=None), dict(data=fake + 1), dict(lead=20), dict(lead=-1), dict(carry_n=41), dict(carry_n=-1), dict(carry_in=None),
           dict(carry_stride=37), dict(carry_out_n=41), dict(carry_out=None), dict(carry_from=961), dict(carry_from=-1), dict(ring_cap=0),
           dict(ring_pos=1000), dict(ring_pos=-1), dict(n_out=1001), dict(n_out=-1), dict(ring=None), dict(format=capi.PCM_F32, data=fake + 2)]
    for kw in bad:
        assert L.artalk_op_pcm_push(desc(**kw), 1, fake, 4096, None) == capi.EINVAL, kw
    assert L.artalk_op_pcm_push(desc(), 1, fake, 103, None) == capi.EINVAL
    assert L.artalk_op_pcm_push(desc(), 0, fake, 4096, None) == capi.EINVAL
    assert L.artalk_op_pcm_push(desc(), 1, None, 4096, None) == capi.EINVAL
    take = lambda **kw: (capi.PcmTakeDesc * 1)(capi.PcmTakeDesc(**dict(dict(ring=fake, ring_cap=1000, read_pos=0, n_valid=640), **kw)))
    for kw in (dict(ring=None), dict(ring_cap=0), dict(read_pos=1000), dict(read_pos=-1), dict(n_valid=641), dict(n_valid=-1)):
        assert L.artalk_op_pcm_take(take(**kw), 1, fake, 4096, fake, 640, 640, None) == capi.EINVAL, kw
    assert L.artalk_op_pcm_take(take(), 1, fake, 4096, fake, 639, 640, None) == capi.EINVAL
    assert L.artalk_op_pcm_take(take(), 1, fake, 4096, None, 640, 640, None) == capi.EINVAL
    assert L.artalk_op_pcm_plan(-1, 0, 0, 3, 1, 19, (C.c_int64 * 6)()) == capi.EINVAL
    assert L.artalk_op_pcm_plan(0, 0, 0, 3, 1, 19, None) == capi.EINVAL


# ---------------------------------------------------------------------------------------------- the symbols
PCM_SYMBOLS = ("artalk_pcm_create", "artalk_pcm_destroy", "artalk_pcm_last_error", "artalk_pcm_set_rate", "artalk_pcm_open", "artalk_pcm_close",
               "artalk_pcm_push", "artalk_pcm_end", "artalk_pcm_available", "artalk_pcm_take", "artalk_op_pcm_plan", "artalk_op_pcm_desc_bytes",
               "artalk_op_pcm_push", "artalk_op_pcm_take")


def test_symbols_are_exported_and_declared():
    L = capi.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "artalk_hip.h")).read(), flags=re.S)
    for name in PCM_SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert getattr(L, name).argtypes is not None
    assert "pcm.hip" in open(os.path.join(REPO, "artalk_amd", "csrc", "Makefile")).read()
    assert (capi.PCM_S16, capi.PCM_F32, capi.PCM_MAX_TAPS, capi.PCM_MAX_CHANNELS) == (1, 2, 1024, 8)
    for macro, value in (("ARTALK_PCM_S16", 1), ("ARTALK_PCM_F32", 2), ("ARTALK_PCM_MAX_TAPS", 1024), ("ARTALK_PCM_MAX_CHANNELS", 8),
                         ("ARTALK_PCM_NO_DEVICE", "(-1)")):
        assert re.search(rf"#define {macro} {re.escape(str(value))}\b", header) or f"#define {macro} {value}" in header
    from artalk_amd.engine import ARTAvatarInferEngine
    for name in ("stream_feed", "stream_audio_end", "stream_ready", "stream_drained"):
        assert callable(getattr(ARTAvatarInferEngine, name))
