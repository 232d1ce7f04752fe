"""``artalk_op_resample_mean`` (resample_mean_kernel of csrc/w2v_front.hip) on the device against its float64 statement
(tests/audio_ref.py) over the case table of tests/audio_cases.py: every case between guard bands of NaN with ``out`` pre-filled with
NaN, inputs bit-equal afterwards, a second launch bit-equal, the impulse cases to the bit and everything else within

    |got_i - r64_i| <= 4 * max(e32, 2^-23 * mag_i)

(e32: the float32 restatement's error on the case's yardstick of 1024 or more outputs; mag_i: what output i sums, in magnitude).
Then the Python wrapper at the eight rates, and ``load_audio_16k`` from a file against the reference-derived 16 kHz fixture.
tests/test_audio_cpu.py shows that a correct kernel keeps half of this allowance and that eleven wrong readings miss it."""
import math
import os
import wave

import numpy as np
import pytest
import torch

from artalk_amd import capi
from audio_cases import (GROUPS, GUARD, RATES, RATIOS, TABLE, allowance, case_allowance, case_refs, is_impulse, make_signal, signal, taps,
                         worst_ratio)
from audio_ref import resample_mean_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# one ratio per taps kind also runs on a stream of its own
OWN_STREAM = ("ta44100", "dense_5_7_3")


def _bits(t):
    return t.view(torch.int32)


def _device_copy(a, unaligned):
    """`a` on the device, contiguous; ``unaligned``: one float past a 16-byte boundary."""
    a = torch.from_numpy(np.array(a, dtype=np.float32, order="C"))      # (a copy: the table's arrays are read-only)
    if not unaligned:
        return a.cuda()
    buf = torch.empty(a.numel() + 1, dtype=torch.float32, device="cuda")
    d = buf[1:].view(a.shape)
    d.copy_(a)
    assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    return d


def launch_case(x, tp, orig, nw, width, n_out, unaligned=None, stream=None):
    """One launch between guard bands; checks finiteness, the guards, the inputs and a second launch.  Returns the float32 output."""
    L = capi.lib()
    nch, n = x.shape
    xd, td = _device_copy(x, unaligned == "x"), _device_copy(tp, unaligned == "taps")
    off = 1 if unaligned == "out" else 0
    buf = torch.full((GUARD + off + n_out + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    lo, hi = GUARD + off, GUARD + off + n_out
    assert buf.data_ptr() % 16 == 0 and (buf[lo:].data_ptr() % 16 == 4) == bool(off)
    poisoned, x0, t0 = _bits(buf).clone(), _bits(xd).clone(), _bits(td).clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if stream == "own" else torch.cuda.current_stream()
    runs = []
    for _ in range(2):
        with torch.cuda.stream(s):
            rc = L.artalk_op_resample_mean(capi.ptr(xd), nch, n, capi.ptr(td), orig, nw, width, capi.ptr(buf[lo:]), n_out, capi.current_stream_ptr())
        assert rc == capi.OK
        s.synchronize()
        torch.cuda.synchronize()
        after = _bits(buf)
        assert torch.equal(after[:lo], poisoned[:lo]) and torch.equal(after[hi:], poisoned[hi:]), "a guard band was written"
        assert torch.equal(_bits(xd), x0) and torch.equal(_bits(td), t0), "an input was written"
        runs.append(buf[lo:hi].clone())
        _bits(buf).copy_(poisoned)
    assert torch.isfinite(runs[0]).all(), f"{int((~torch.isfinite(runs[0])).sum())} outputs are unwritten or not finite"
    assert torch.equal(_bits(runs[0]), _bits(runs[1])), "a second launch gives other bits"
    return runs[0].cpu().numpy()


def _run_table_case(c, stream=None):
    r = RATIOS[c.ratio]
    got = launch_case(signal(c.name), taps(c.ratio), r.orig, r.nw, r.width, c.n_out, unaligned=c.unaligned, stream=stream)
    r64, _ = case_refs(c.name)
    assert got.shape == r64.shape and got.dtype == np.float32
    if is_impulse(c):      # every output is the float32 tap it lands on, or 0.0: no allowance
        want = r64.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), r64) and np.count_nonzero(want) > 0
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"{c.name}: {bad.size} outputs differ from the tap they land on, first at {bad[:4]}"
        return 0.0
    q = worst_ratio(got, r64, case_allowance(c.name))
    assert q <= 1.0, f"{c.name}: error / allowed {q:.3f}"
    return q


@pytest.mark.parametrize("group", GROUPS)
def test_resample_mean_case_table(group):
    cases = [c for c in TABLE.values() if c.group == group]
    assert cases
    worst = {}
    for c in cases:
        q = _run_table_case(c)
        if not is_impulse(c):
            key = c.name if group in ("grid", "unaligned") else c.ratio
            worst[key] = max(worst.get(key, 0.0), q)
    for key, q in worst.items():
        print(f"resample_mean {key}: largest error / allowed {q:.3f} over {len(cases)} cases of the group")


@pytest.mark.parametrize("ratio", OWN_STREAM)
def test_resample_mean_on_a_stream_of_its_own(ratio):
    cases = [c for c in TABLE.values() if c.group == ratio]
    assert any(is_impulse(c) for c in cases) and any(not is_impulse(c) for c in cases)
    for c in cases:
        _run_table_case(c, stream="own")


def test_n_times_nw_beyond_int32_is_taken_in_64_bits():
    """n * nw = 2^31 + 64 here: the ceiling that bounds n_out is computed in 64 bits, so the first outputs of a very long clip are served
    (and equal those of the clip's head, which is all they read)."""
    orig = nw = 64
    n, n_out = (1 << 25) + 1, 257
    head = 64 * 8
    g = np.random.default_rng(5)
    tp = g.uniform(-1.0, 1.0, size=(nw, orig)).astype(np.float32)
    x_head = (g.standard_normal((1, head), dtype=np.float32) * np.float32(0.3)).astype(np.float32)
    xd = torch.zeros(1, n, dtype=torch.float32, device="cuda")
    xd[:, :head] = torch.from_numpy(x_head).cuda()
    td = torch.from_numpy(tp).cuda()
    out = torch.full((n_out,), float("nan"), dtype=torch.float32, device="cuda")
    rc = capi.lib().artalk_op_resample_mean(capi.ptr(xd), 1, n, capi.ptr(td), orig, nw, 0, capi.ptr(out), n_out, capi.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == capi.OK
    r64, mag = resample_mean_ref(x_head, tp, orig, nw, 0, n_out)
    r32, _ = resample_mean_ref(x_head, tp, orig, nw, 0, n_out, dtype=np.float32)
    # (n_out < 1024, so the yardstick is a run of its own on 1024 outputs with these taps)
    x_y = (g.standard_normal((1, 64 * 16), dtype=np.float32) * np.float32(0.3)).astype(np.float32)
    y64, _ = resample_mean_ref(x_y, tp, orig, nw, 0, 1024)
    y32, _ = resample_mean_ref(x_y, tp, orig, nw, 0, 1024, dtype=np.float32)
    allowed = 4.0 * np.maximum(np.abs(y32 - y64).max(), 2.0 ** -23 * mag)
    q = worst_ratio(out.cpu().numpy(), r64, allowed)
    print(f"resample_mean n * nw = 2^31 + 64: largest error / allowed {q:.3f}")
    assert q <= 1.0


# ---------------------------------------------------------------------------------------------- the wrapper
@pytest.mark.parametrize("sr", sorted(RATES))
def test_wrapper_against_float64(sr):
    from artalk_amd.audio import resample_mean_16k
    name = f"ta{sr}"
    r = RATIOS[name]
    for nch in (1, 2, 3):
        n = r.orig * 7 + 1201 + nch
        x = make_signal("noise", nch, n, 100 * sr + nch)
        got = resample_mean_16k(torch.from_numpy(x), sr, "cuda")
        n_out = int(math.ceil(n * 16000 / sr))
        assert got.shape == (n_out,) and got.dtype == torch.float32 and got.is_cuda
        r64, mag = resample_mean_ref(x, taps(name), r.orig, r.nw, r.width, n_out)
        q = worst_ratio(got.cpu().numpy(), r64, allowance(name, nch, "noise", mag))
        print(f"resample_mean_16k {sr} Hz, {nch} channel(s), {n_out} outputs: largest error / allowed {q:.3f}")
        assert q <= 1.0


def test_wrapper_at_16k_is_the_channel_mean():
    from artalk_amd.audio import resample_mean_16k
    for nch in (1, 2, 3):
        x = torch.from_numpy(make_signal("noise", nch, 3001, 16000 + nch))
        got = resample_mean_16k(x, 16000, "cuda")
        assert got.shape == (3001,) and torch.equal(_bits(got), _bits(x.cuda().mean(0)))
        if nch <= 2:      # (halving is exact, so the host's mean has the same bits whatever its order)
            assert torch.equal(_bits(got.cpu()), _bits(x.mean(0)))


# ---------------------------------------------------------------------------------------------- from a file to the fixture
def test_load_audio_16k_matches_the_demo_fixture(tmp_path):
    """The three stretches of the reference's demo/eng1.wav (48 kHz stereo) through read_wav and the kernel: away from a cut inside the
    file every value, scaled to int16 units, lies within rounding (0.5) plus the kernel's allowance of the 16 kHz fixture that the
    CPU restatement produced from the whole file (tests/test_audio.py::test_demo_fixture_is_reproducible)."""
    from artalk_amd.audio import load_audio_16k, read_wav
    src = np.load(os.path.join(GOLDEN, "demo_eng1_48k_segments.npz"))
    fx = np.load(os.path.join(GOLDEN, "demo_16k_s16.npz"))["eng1"].astype(np.float64)
    n_file, margin = int(src["n_frames"]), 16
    r = RATIOS["ta48000"]
    for i, (start, pcm) in enumerate(zip(src["start"], src["pcm"])):
        start = int(start)
        path = str(tmp_path / f"eng1_{i}.wav")
        with wave.open(path, "wb") as w:
            w.setnchannels(pcm.shape[1]); w.setsampwidth(2); w.setframerate(int(src["sr"]))
            w.writeframes(pcm.astype("<i2").tobytes())
        a = load_audio_16k(path).cpu().numpy()
        wav, sr = read_wav(path)
        assert sr == 48000 and a.shape == (pcm.shape[0] // 3,) and a.dtype == np.float32
        r64, mag = resample_mean_ref(wav.numpy(), taps("ta48000"), r.orig, r.nw, r.width, a.shape[0])
        allowed = allowance("ta48000", wav.shape[0], "noise", mag)
        q = worst_ratio(a, r64, allowed)
        lo = 0 if start == 0 else margin
        hi = a.shape[0] if start + pcm.shape[0] == n_file else a.shape[0] - margin
        j0 = start // 3
        d = np.abs(32768.0 * a.astype(np.float64) - fx[j0:j0 + a.shape[0]])[lo:hi]
        print(f"load_audio_16k stretch at frame {start}: error / allowed against float64 {q:.3f}, largest distance to the fixture {d.max():.4f} of an int16 step")
        assert q <= 1.0
        assert (d <= 0.5 + 32768.0 * allowed[lo:hi]).all(), f"stretch at frame {start} leaves the 16 kHz fixture"
