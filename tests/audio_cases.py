"""The case table of ``artalk_op_resample_mean`` (tests/test_audio_ops_gpu.py runs it on the device, tests/test_audio_cpu.py shows on
the CPU that a correct kernel keeps the allowance on it and that wrong readings do not).  TEST INFRASTRUCTURE ONLY.

A case is (orig, nw, width, taps kind, nch, n, n_out, signal); seeds are fixed (a CRC of the case's name).  Taps are either torchaudio's
(``sinc_resample_kernel(sr, 16000)``: the outermost taps are exact zeros there) or dense: U(-1, 1) with no magnitude below 0.05, so
that every tap index matters.
"""
import collections
import functools
import zlib

import numpy as np

from audio_ref import GRID_THREADS, kernel_order_f32, resample_mean_ref

# rate -> (orig, nw, width, taps per phase) of sinc_resample_kernel(rate, 16000); asserted in tests/test_audio_cpu.py
RATES = {48000: (3, 1, 19, 41), 44100: (441, 160, 17, 475), 22050: (441, 320, 9, 459), 8000: (1, 2, 7, 15), 32000: (2, 1, 13, 28),
         24000: (3, 2, 10, 23), 11025: (441, 640, 7, 455), 96000: (6, 1, 37, 80)}
# (orig, nw, width) with dense taps: a single tap, no pad, up- and down-sampling, a ratio that is not reduced, 256 taps, 64 phases
# (the last one is 8 kHz's geometry, which the grid-stride cases run: with dense taps, not torchaudio's zero-ended ones)
DENSE = ((1, 1, 0), (1, 1, 4), (3, 1, 0), (1, 3, 2), (5, 7, 3), (7, 5, 1), (2, 4, 6), (64, 1, 96), (1, 64, 1), (1, 2, 7))

Ratio = collections.namedtuple("Ratio", "name kind orig nw width sr")
RATIOS = collections.OrderedDict()
for _sr, (_o, _nw, _w, _) in RATES.items():
    RATIOS[f"ta{_sr}"] = Ratio(f"ta{_sr}", "torchaudio", _o, _nw, _w, _sr)
for _o, _nw, _w in DENSE:
    RATIOS[f"dense_{_o}_{_nw}_{_w}"] = Ratio(f"dense_{_o}_{_nw}_{_w}", "dense", _o, _nw, _w, None)

Case = collections.namedtuple("Case", "name group ratio nch n n_out signal unaligned")
CHANNELS = (1, 2, 3, 6)
SIGNALS = ("noise", "zero_channel", "constant")      # and "impulse", "impulse2" (bit-exact cases)
GUARD = 4096                                          # NaN words on either side of `out` on the device
FACTOR = 4.0                                          # the project's margin over the float32 yardstick
ULP = 2.0 ** -23


def ceil_out(n, r):
    return -((-n * r.nw) // r.orig)


# Cases drawn again, as the issue provides where a correct kernel comes within half of the allowance: with the seed of its name alone the
# kernel-order emulation measured 0.514 x the allowance on this one (the largest of 1 048 575 errors against a yardstick of 1024 values).
RESEEDED = {"dense_1_2_7/n524288/c1/noise/out1048575": 1}


def _seed(name):
    return zlib.crc32(f"{name}#{RESEEDED[name]}".encode() if name in RESEEDED else name.encode())


@functools.lru_cache(maxsize=None)
def taps(ratio_name):
    """float32 (nw, 2 * width + orig), read-only."""
    r = RATIOS[ratio_name]
    if r.kind == "torchaudio":
        from artalk_amd.audio import sinc_resample_kernel
        t, width, orig, nw = sinc_resample_kernel(r.sr, 16000)
        assert (orig, nw, width) == (r.orig, r.nw, r.width)
        t = t.numpy().copy()
    else:
        g = np.random.default_rng(_seed("taps/" + ratio_name))
        t = g.uniform(-1.0, 1.0, size=(r.nw, 2 * r.width + r.orig))
        t = np.where(np.abs(t) < 0.05, np.copysign(0.05, t), t).astype(np.float32)
    t.setflags(write=False)
    return t


def impulse_positions(n):
    return (0, n // 2, n - 1)


def make_signal(kind, nch, n, seed):
    """float32 (nch, n)."""
    g = np.random.default_rng(seed)
    if kind in ("noise", "zero_channel"):
        x = (g.standard_normal((nch, n), dtype=np.float32) * np.float32(0.3)).astype(np.float32)
        if kind == "zero_channel":
            assert nch >= 2
            x[seed % nch] = 0.0
        return x
    if kind == "constant":
        return np.ones((nch, n), dtype=np.float32)
    x = np.zeros((nch, n), dtype=np.float32)
    if kind == "impulse":            # one channel, 1.0 at both ends and once inside
        assert nch == 1
        x[0, list(impulse_positions(n))] = 1.0
    elif kind == "impulse2":         # two channels, 2.0 in channel 1 only: (0 + 2 tap) / 2 is exact as well
        assert nch == 2
        x[1, list(impulse_positions(n))] = 2.0
    else:
        raise KeyError(kind)
    return x


def _lengths(r):
    """n of the issue's list for one ratio, in order, without repeats: 1, width, width + 1, orig * 256 (+ 1), n_out = 255 / 256 / 257 where the
    ratio allows it, and an n that is no multiple of orig."""
    ns = [1]
    if r.width > 0:
        ns += [r.width, r.width + 1]
    ns += [r.orig * 256, r.orig * 256 + 1]
    for target in (255, 256, 257):
        n = ((target - 1) * r.orig) // r.nw + 1      # the smallest n with ceil(n * nw / orig) >= target
        if ceil_out(n, r) == target:
            ns.append(n)
    if r.orig > 1:
        ns.append(r.orig * 40 + (r.orig + 1) // 2)
    return list(dict.fromkeys(ns))


def _build_table():
    table = collections.OrderedDict()

    def add(group, r, nch, n, n_out, signal, unaligned=None, tag=""):
        if signal == "zero_channel" and nch < 2:
            signal = "noise"
        name = f"{r.name}/n{n}/c{nch}/{signal}{tag}"
        assert name not in table, name
        table[name] = Case(name, group, r.name, nch, n, n_out, signal, unaligned)

    for ri, r in enumerate(RATIOS.values()):
        ntaps = 2 * r.width + r.orig
        for li, n in enumerate(_lengths(r)):
            nch = CHANNELS[(ri + li) % 4]
            if ceil_out(n, r) * ntaps > 10_000_000:      # the three 441:x ratios at n = 441 * 256: keep the float64 statement quick
                nch = 1 + li % 2
            add(r.name, r, nch, n, ceil_out(n, r), SIGNALS[(2 * ri + li) % 3])
        n_mid = r.orig * 33 + r.orig // 2 + 3                # every channel count and every signal at one more length per ratio
        for ci, nch in enumerate(CHANNELS):
            for si, signal in enumerate(SIGNALS):
                if signal == "zero_channel" and nch < 2:
                    continue
                if (ci + si + ri) % 3 != 2 or nch == 6:      # (two of the three signals per channel count, all three at 6)
                    add(r.name, r, nch, n_mid + ci, ceil_out(n_mid + ci, r), signal, tag="/sweep")
        n_imp = 3 * ntaps + 2 * r.orig + 7                   # the three impulses are more than ntaps apart: no output sees two
        add(r.name, r, 1, n_imp, ceil_out(n_imp, r), "impulse")
        add(r.name, r, 2, n_imp + 1, ceil_out(n_imp + 1, r), "impulse2")
        if r.kind == "dense":                                 # n_out below the ceiling is legal: the first n_out outputs
            n = r.orig * 19 + 1
            add(r.name, r, 2, n, 1, "noise", tag="/first")
            add(r.name, r, 3, n, ceil_out(n, r) - 1, "noise", tag="/short")

    # the launcher caps the grid at 4096 blocks of 256 threads: the smallest sizes that reach the second and the third trip of the loop
    up, down = RATIOS["dense_1_2_7"], RATIOS["ta48000"]
    for n_out in (GRID_THREADS - 1, GRID_THREADS, GRID_THREADS + 1, GRID_THREADS + 257, 2 * GRID_THREADS + 3):
        add("grid", up, 1, (n_out + 1) // 2, n_out, "noise", tag=f"/out{n_out}")
    n = 3 * (GRID_THREADS + 257) - 1
    add("grid", down, 2, n, ceil_out(n, down), "noise", tag="/grid")
    assert ceil_out(n, down) == GRID_THREADS + 257

    # x, taps and out one float off a 16-byte boundary
    for r, nch, n, which in ((RATIOS["ta44100"], 2, 2003, "x"), (RATIOS["dense_5_7_3"], 3, 999, "taps"), (RATIOS["ta8000"], 1, 701, "out")):
        add("unaligned", r, nch, n, ceil_out(n, r), "noise", unaligned=which, tag="/off_" + which)
    return table


TABLE = _build_table()
GROUPS = list(dict.fromkeys(c.group for c in TABLE.values()))


def is_impulse(c):
    return c.signal in ("impulse", "impulse2")


@functools.lru_cache(maxsize=None)
def signal(name):
    c = TABLE[name]
    x = make_signal(c.signal, c.nch, c.n, _seed(name))
    x.setflags(write=False)
    return x


def run_ref(c, dtype=np.float64, variant=None):
    r = RATIOS[c.ratio]
    return resample_mean_ref(signal(c.name), taps(c.ratio), r.orig, r.nw, r.width, c.n_out, dtype=dtype, variant=variant)


def run_kernel_order(c):
    r = RATIOS[c.ratio]
    return kernel_order_f32(signal(c.name), taps(c.ratio), r.orig, r.nw, r.width, c.n_out)


@functools.lru_cache(maxsize=None)
def case_refs(name):
    """(float64 statement, mag) of a TABLE case, computed once per session and left unchanged."""
    out, mag = run_ref(TABLE[name])
    out.setflags(write=False)
    mag.setflags(write=False)
    return out, mag


@functools.lru_cache(maxsize=None)
def yardstick(ratio_name, nch, kind):
    """e32: the max-abs error of the float32 restatement against float64 with the same taps, channel count and signal kind, on the
    shortest n that gives at least 1024 outputs (at most 1024 + nw - 1 < 2048 of them)."""
    r = RATIOS[ratio_name]
    n = -((-1024 * r.orig) // r.nw)
    n_out = ceil_out(n, r)
    assert 1024 <= n_out < 2048
    x = make_signal(kind, nch, n, _seed(f"yardstick/{ratio_name}/{nch}/{kind}"))
    r64, _ = resample_mean_ref(x, taps(ratio_name), r.orig, r.nw, r.width, n_out)
    r32, _ = resample_mean_ref(x, taps(ratio_name), r.orig, r.nw, r.width, n_out, dtype=np.float32)
    assert r32.dtype == np.float32
    return float(np.abs(r32.astype(np.float64) - r64).max())


def allowance(ratio_name, nch, kind, mag):
    """4 * max(e32, one float32 unit of what is summed), per output."""
    return FACTOR * np.maximum(yardstick(ratio_name, nch, kind), ULP * mag)


def case_allowance(name):
    c = TABLE[name]
    return allowance(c.ratio, c.nch, c.signal, case_refs(name)[1])


def worst_ratio(got, r64, allowed):
    """max error / allowed; an unwritten (NaN) or non-finite output counts as infinitely wrong."""
    err = np.abs(np.asarray(got, dtype=np.float64) - r64)
    err = np.where(np.isfinite(err), err, np.inf)
    return float((err / allowed).max()) if err.size else 0.0
