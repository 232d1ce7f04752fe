"""The audio front-end, the part that needs no GPU: the allowance of tests/test_audio_ops_gpu.py holds for a correct kernel (its order of
summation emulated on the CPU) with room to spare and is missed by eleven wrong readings of the definition; the geometry of the tap tables;
``read_wav`` at every sample width; the refusals of ``artalk_op_resample_mean`` and of ``resample_mean_16k``."""
import ctypes as C
import struct
import wave

import numpy as np
import pytest
import torch

from artalk_amd import capi
from artalk_amd.audio import MAX_TAP_TABLE, read_wav, resample_mean_16k, sinc_resample_kernel, tap_table_geometry
from audio_cases import (DENSE, GROUPS, RATES, RATIOS, TABLE, case_allowance, case_refs, is_impulse, run_kernel_order, run_ref, taps, worst_ratio,
                         yardstick)
from audio_oracle import get_sinc_resample_kernel
from audio_ref import GRID_THREADS, VARIANTS

INT_MAX = 2 ** 31 - 1


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------- the allowance and a correct kernel
@pytest.mark.parametrize("group", GROUPS)
def test_allowance_holds_for_the_kernels_order(group):
    """A float32 kernel that sums in the HIP kernel's order stays at or below half of the allowance on every case, and the allowance is
    never zero; on the impulse cases it gives the bits of the float64 statement."""
    cases = [c for c in TABLE.values() if c.group == group]
    worst, name = 0.0, None
    for c in cases:
        r64, mag = case_refs(c.name)
        assert r64.shape == (c.n_out,) and np.isfinite(r64).all()
        k = run_kernel_order(c)
        assert k.dtype == np.float32
        if is_impulse(c):
            want = r64.astype(np.float32)
            assert _same_bits(k, want) and np.count_nonzero(want) > 0
            assert np.isin(want, np.append(taps(c.ratio).ravel(), np.float32(0.0))).all()      # the tap it lands on, or 0.0
            continue
        allowed = case_allowance(c.name)
        assert allowed.shape == (c.n_out,) and (allowed > 0).all(), f"{c.name}: an allowance of zero"
        q = worst_ratio(k, r64, allowed)
        assert q <= 0.5, f"{c.name}: the kernel's order measures {q:.3f} of the allowance"
        if q > worst:
            worst, name = q, c.name
    print(f"{group}: {len(cases)} cases, kernel order at most {worst:.3f} of the allowance ({name})")


def test_table_covers_what_it_should():
    cs = list(TABLE.values())
    assert {c.nch for c in cs} == {1, 2, 3, 6}
    assert {c.signal for c in cs} == {"noise", "zero_channel", "constant", "impulse", "impulse2"}
    assert {c.unaligned for c in cs} == {None, "x", "taps", "out"}
    for name, r in RATIOS.items():
        mine = [c for c in cs if c.group == name]
        ns = {c.n for c in mine}
        assert {1, r.orig * 256, r.orig * 256 + 1} <= ns and (r.width == 0 or {r.width, r.width + 1} <= ns)
        assert r.orig == 1 or any(c.n % r.orig and c.n_out == -((-c.n * r.nw) // r.orig) for c in mine)
        assert {c.signal for c in mine} >= {"impulse", "impulse2", "noise", "constant", "zero_channel"} and {c.nch for c in mine} == {1, 2, 3, 6}
        outs = {c.n_out for c in mine}
        assert outs & {255, 256, 257} and (r.nw > r.orig or {255, 256, 257} <= outs)      # (nw = 3 reaches 255 only, nw = 2 only 256)
        if r.kind == "dense":
            assert 1 in outs and any(c.n_out == -((-c.n * r.nw) // r.orig) - 1 for c in mine)
    grid = sorted(c.n_out for c in cs if c.group == "grid")
    assert grid == [GRID_THREADS - 1, GRID_THREADS, GRID_THREADS + 1, GRID_THREADS + 257, GRID_THREADS + 257, 2 * GRID_THREADS + 3]
    for (o, nw, w) in DENSE:
        t = taps(f"dense_{o}_{nw}_{w}")
        assert t.shape == (nw, 2 * w + o) and t.dtype == np.float32 and np.abs(t).min() >= np.float32(0.05) and np.abs(t).max() < 1.0


# ---------------------------------------------------------------------------------------------- wrong readings
# the cases a wrong reading is tried on: every case of the table that is cheap to state (outputs x taps x channels)
def _cost(c):
    r = RATIOS[c.ratio]
    return c.n_out * (2 * r.width + r.orig) * c.nch


SMALL = [c for c in TABLE.values() if c.group in RATIOS and _cost(c) <= 60_000]
# readings that an impulse case can show (the others need a second non-zero channel, a cut last group or 2^20 outputs)
ON_IMPULSES = ("pad_plus", "pad_minus", "phases_reversed", "taps_reversed", "drop_first_tap", "drop_last_tap", "no_right_guard",
               "no_division", "j_by_orig")


def _misses(variant, cases):
    """[(case, error / allowed or None, impulse bits differ or None)]"""
    rows = []
    for c in cases:
        r64, _ = case_refs(c.name)
        bad, _ = run_ref(c, variant=variant)
        if is_impulse(c):
            rows.append((c, None, not _same_bits(bad.astype(np.float32), r64.astype(np.float32))))
        else:
            rows.append((c, worst_ratio(bad, r64, case_allowance(c.name)), None))
    return rows


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "no_grid_stride"])
def test_wrong_reading_misses_the_allowance(variant):
    rows = _misses(variant, SMALL)
    shown = [c.name for c, q, _ in rows if q is not None and q >= 100.0]
    exact = [c.name for c, _, differs in rows if differs]
    print(f"{variant}: misses the allowance a hundredfold on {len(shown)} and bit-equality on {len(exact)} of {len(rows)} cases")
    assert shown, f"{variant} stays within 100 x the allowance on every case"
    if variant in ON_IMPULSES:
        assert exact, f"{variant} passes every impulse case"
    if variant == "phases_reversed":      # can only show where there is more than one phase
        assert all(not q and not d for c, q, d in rows if RATIOS[c.ratio].nw == 1)
        assert {RATIOS[TABLE[n].ratio].nw > 1 for n in shown + exact} == {True}
    if variant == "j_by_orig":
        assert all(not q and not d for c, q, d in rows if RATIOS[c.ratio].nw == RATIOS[c.ratio].orig)
    if variant == "n_out_floored":        # only a cut last group loses outputs
        assert all((q == np.inf) == bool((c.n * RATIOS[c.ratio].nw) % RATIOS[c.ratio].orig and c.n_out > c.n * RATIOS[c.ratio].nw // RATIOS[c.ratio].orig)
                   for c, q, _ in rows if q is not None)
    if variant == "no_division":
        assert all(not q and not d for c, q, d in rows if c.nch == 1)


def test_outer_taps_of_torchaudio_hide_a_dropped_tap():
    """Why the table has dense taps: at 48 kHz tap 0 and the last three taps are exact zeros, so a kernel that drops the first or the last
    tap computes the same bits; with dense taps it does not."""
    t = taps("ta48000")
    assert t.shape == (1, 41) and t[0, 0] == 0.0 and (t[0, -3:] == 0.0).all() and np.count_nonzero(t[0, 1:-3]) == 37
    t8 = taps("ta8000")
    assert (t8[:, 0] == 0.0).all() and (t8[:, -1] == 0.0).all()
    for variant in ("drop_first_tap", "drop_last_tap"):
        for c in (c for c in SMALL if c.ratio == "ta48000"):
            assert np.array_equal(run_ref(c, variant=variant)[0], case_refs(c.name)[0]), (variant, c.name)
        dense = [q for c, q, _ in _misses(variant, [c for c in SMALL if c.ratio == "dense_3_1_0"]) if q is not None]
        assert max(dense) >= 100.0
    # the last tap shows with dense taps only: on no torchaudio case of the small set does dropping it cost a hundredth of the allowance
    assert all(q < 0.01 for c, q, _ in _misses("drop_last_tap", [c for c in SMALL if RATIOS[c.ratio].kind == "torchaudio"]) if q is not None)


def test_missing_edge_guards_show_where_channels_meet():
    """Without the right-edge guard channel c reads on into channel c + 1: only the last outputs of a channel that has one behind it
    change, and at least one of them leaves the allowance.  Without the left-edge guard it is the first outputs."""
    for variant, at_end in (("no_right_guard", True), ("no_left_guard", False)):
        seen = 0
        for c in SMALL:
            r = RATIOS[c.ratio]
            if c.signal != "noise" or c.nch < 2 or r.width == 0 or c.n_out < 8 or c.name.endswith("/short"):
                continue
            r64, _ = case_refs(c.name)
            bad, _ = run_ref(c, variant=variant)
            j = np.arange(c.n_out) // r.nw
            edge = (j * r.orig - r.width + 2 * r.width + r.orig - 1 >= c.n) if at_end else (j * r.orig - r.width < 0)
            assert np.array_equal(bad[~edge], r64[~edge]) and edge.any(), c.name
            fails = np.abs(bad - r64) > case_allowance(c.name)
            assert fails[edge].any(), f"{variant} stays within the allowance on {c.name}"
            seen += 1
        assert seen >= 10
    # one channel has no neighbour to read: neither reading shows
    c = next(c for c in SMALL if c.nch == 1 and c.signal == "noise" and RATIOS[c.ratio].width > 0)
    assert np.array_equal(run_ref(c, variant="no_right_guard")[0], case_refs(c.name)[0])
    assert np.array_equal(run_ref(c, variant="no_left_guard")[0], case_refs(c.name)[0])


def test_a_kernel_without_the_grid_stride_loop_leaves_outputs_unwritten():
    """Outputs from index 4096 * 256 on come from a later trip of the loop.  A kernel without the loop leaves them as they were: the GPU
    test pre-fills ``out`` with NaN and demands finite outputs, which is what catches it (a zero-filled buffer would only be wrong by
    the size of the signal).  Here the reading is NaN from that index on and counts as infinitely wrong."""
    c = TABLE[f"dense_1_2_7/n{(GRID_THREADS + 2) // 2}/c1/noise/out{GRID_THREADS + 1}"]
    r64, _ = case_refs(c.name)
    bad, _ = run_ref(c, variant="no_grid_stride")
    assert np.array_equal(bad[:GRID_THREADS], r64[:GRID_THREADS]) and np.isnan(bad[GRID_THREADS:]).all() and bad[GRID_THREADS:].size == 1
    assert worst_ratio(bad, r64, case_allowance(c.name)) == np.inf
    below = TABLE[f"dense_1_2_7/n{GRID_THREADS // 2}/c1/noise/out{GRID_THREADS - 1}"]
    assert below.n_out == GRID_THREADS - 1      # (the largest size that one trip serves is in the table too)
    small = SMALL[0]
    assert np.array_equal(run_ref(small, variant="no_grid_stride")[0], case_refs(small.name)[0])


# ---------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("sr", sorted(RATES))
def test_tap_table_geometry(sr):
    t, width, orig, nw = sinc_resample_kernel(sr, 16000)
    assert (orig, nw, width, t.shape[1]) == RATES[sr] and t.shape == (nw, 2 * width + orig) and t.dtype == torch.float32
    assert tap_table_geometry(sr, 16000) == (orig, nw, t.shape[1]) and nw * t.shape[1] < 300_000 < MAX_TAP_TABLE
    import math
    k, w = get_sinc_resample_kernel(sr, 16000, math.gcd(sr, 16000))
    assert w == width and torch.equal(k.reshape(nw, -1).view(torch.int32), t.view(torch.int32))
    if orig >= nw:      # downsampling: every phase has unit gain at DC
        sums = t.double().sum(dim=1)
        assert float((sums - 1.0).abs().max()) < 2e-3, sums
    assert yardstick(f"ta{sr}", 2, "noise") > 0.0


# ---------------------------------------------------------------------------------------------- read_wav
def _pcm_values(sw, count, rng):
    bits = 8 * sw
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    v = rng.integers(lo, hi + 1, size=count, dtype=np.int64)
    v[:5] = (lo, hi, -1, 0, 1)
    return v


def _pcm_bytes(v, sw):
    if sw == 1:
        return (v + 128).astype(np.uint8).tobytes()      # 8-bit WAV is unsigned, offset by 128
    if sw == 2:
        return v.astype("<i2").tobytes()
    if sw == 4:
        return v.astype("<i4").tobytes()
    u = (v & 0xFFFFFF).astype(np.uint32)                  # 24 bits: three little-endian bytes of the two's complement
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()


@pytest.mark.parametrize("nch", (1, 2, 3))
@pytest.mark.parametrize("sw", (1, 2, 3, 4))
def test_read_wav_every_sample_width(tmp_path, sw, nch):
    rng = np.random.default_rng(10 * sw + nch)
    frames = 211
    v = _pcm_values(sw, frames * nch, rng)
    path = str(tmp_path / f"w{sw}_{nch}.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(nch); w.setsampwidth(sw); w.setframerate(22050)
        w.writeframes(_pcm_bytes(v, sw))
    wav, sr = read_wav(path)
    assert sr == 22050 and wav.shape == (nch, frames) and wav.dtype == torch.float32 and wav.is_contiguous()
    want = (v.astype(np.float64) / float(1 << (8 * sw - 1))).astype(np.float32).reshape(frames, nch).T      # frame-major in the file
    assert _same_bits(wav.numpy(), np.ascontiguousarray(want))
    assert float(wav.min()) == -1.0 and float(wav.max()) == float(np.float32(((1 << (8 * sw - 1)) - 1) / (1 << (8 * sw - 1))))


def test_read_wav_refuses_ieee_float(tmp_path):
    data = np.linspace(-1.0, 1.0, 16, dtype="<f4").tobytes()
    header = (b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 3, 1, 16000, 16000 * 4, 4, 32)
              + b"data" + struct.pack("<I", len(data)))
    assert len(header) == 44
    path = tmp_path / "float.wav"
    path.write_bytes(header + data)
    with pytest.raises((wave.Error, ValueError)):
        read_wav(str(path))


# ---------------------------------------------------------------------------------------------- refusals
def _op(null=(), nch=2, n=100, orig=3, nw=2, width=4, n_out=67):
    """artalk_op_resample_mean with host buffers standing in for device pointers: only for calls that return before the device is touched."""
    buf = np.zeros(4096, dtype=np.float32)
    p = {k: (None if k in null else buf.ctypes.data_as(C.c_void_p)) for k in ("x", "taps", "out")}
    return capi.lib().artalk_op_resample_mean(p["x"], nch, n, p["taps"], orig, nw, width, p["out"], n_out, None)


def test_op_refusals_without_gpu():
    for kw in (dict(null=("x",)), dict(null=("taps",)), dict(null=("out",)), dict(nch=0), dict(nch=-1), dict(n=0), dict(n=-5), dict(orig=0),
               dict(orig=-3), dict(nw=0), dict(nw=-2), dict(width=-1),
               dict(n_out=-1), dict(n_out=-INT_MAX),
               dict(n_out=68),                                               # ceil(100 * 2 / 3) = 67
               dict(n=10, orig=1, nw=1, n_out=11),
               dict(n=1 << 30, orig=1 << 30, nw=4, width=0, n_out=5),         # n * nw = 2^32 needs 64 bits; the ceiling is 4
               dict(n=INT_MAX, orig=1, nw=1, n_out=INT_MAX - (1 << 20) + 1),  # i += gridDim.x * 256 is an int
               dict(n=INT_MAX, orig=1, nw=2, n_out=INT_MAX)):
        assert _op(**kw) == capi.EINVAL, kw
    # nothing to do: a success that launches nothing
    assert _op(n_out=0) == capi.OK and _op(n=1, orig=1000, nw=1, width=0, n_out=0) == capi.OK


def test_wrapper_refuses_a_huge_tap_table():
    assert tap_table_geometry(16001, 16000) == (16001, 16000, 2 * 7 + 16001)
    with pytest.raises(ValueError, match="16001:16000"):
        resample_mean_16k(torch.zeros(1, 100), 16001, device="cpu")
    with pytest.raises(ValueError, match="limit"):
        resample_mean_16k(torch.zeros(2, 100), 15999)
