"""``artalk_op_resample_mean`` stated in numpy: the polyphase FIR of the audio front-end and its channel mean.  TEST INFRASTRUCTURE ONLY.

    out[j * nw + p] = mean_c sum_k taps[p][k] * xpad_c[j * orig + k]

with xpad_c = channel c zero-padded by ``width`` on the left and as far as needed on the right.  ``x`` (nch, n) and ``taps``
(nw, 2 * width + orig) are arbitrary: nothing here knows about sinc filters.  Vectorised over the outputs, a loop over taps and channels.

``resample_mean_ref`` gives the statement in float64 (with ``mag``, the mean over channels of the summed magnitudes: what one float32
unit of the sum is measured against), the float32 yardstick (the same formulas in float32, numpy's order) and, through ``variant``,
wrong readings of the definition that the tests must tell apart.  ``kernel_order_f32`` emulates the order of the HIP kernel.
"""
import numpy as np

GRID_THREADS = 4096 * 256      # launch_resample_mean caps the grid here; outputs from this index on come from a later trip of the loop

# wrong readings of the definition (tests/test_audio_cpu.py shows that each misses the allowance on a case of the table)
VARIANTS = ("pad_plus", "pad_minus", "phases_reversed", "taps_reversed", "drop_first_tap", "drop_last_tap", "no_right_guard",
            "no_left_guard", "no_division", "j_by_orig", "n_out_floored", "no_grid_stride")


def _geometry(x, taps, orig, nw, width, n_out, variant):
    """Index vectors shared by every statement: per output the phase, the position of tap 0 in the padded channel, and per channel the
    padded signal with the offset of its sample 0."""
    x = np.ascontiguousarray(x)
    taps = np.ascontiguousarray(taps)
    nch, n = x.shape
    ntaps = 2 * width + orig
    assert taps.shape == (nw, ntaps) and n_out >= 0
    i = np.arange(n_out, dtype=np.int64)
    j = i // (orig if variant == "j_by_orig" else nw)
    p = i % nw if variant == "j_by_orig" else i - j * nw
    if variant == "phases_reversed":
        p = nw - 1 - p
    base = j * orig - width + {"pad_plus": 1, "pad_minus": -1}.get(variant, 0)
    left = width + 1                                                            # zeros in front (one more for pad_minus)
    right = int(base.max()) + ntaps + 1 if n_out else 1                         # zeros behind: the last output reads on to here
    chans = []
    for c in range(nch):
        pre, post = x[:0].ravel(), x[:0].ravel()
        if variant == "no_left_guard":
            pre = x[:c].ravel()                                                 # t < 0 reads the tail of the channel(s) before
        if variant == "no_right_guard":
            post = x[c + 1:].ravel()                                            # t >= n reads on into the channel(s) behind
        xp = np.concatenate([np.zeros(left, x.dtype), pre, x[c], post, np.zeros(right, x.dtype)])
        chans.append((xp, left + pre.shape[0]))
    unwritten = np.zeros(n_out, dtype=bool)
    if variant == "n_out_floored":
        unwritten = i >= (n * nw) // orig
    if variant == "no_grid_stride":
        unwritten = i >= GRID_THREADS
    k_of = (lambda k: ntaps - 1 - k) if variant == "taps_reversed" else (lambda k: k)
    ks = [k for k in range(ntaps) if not (variant == "drop_first_tap" and k == 0) and not (variant == "drop_last_tap" and k == ntaps - 1)]
    return nch, ntaps, p, base, chans, unwritten, k_of, ks, taps.reshape(-1)


def resample_mean_ref(x, taps, orig, nw, width, n_out, dtype=np.float64, variant=None):
    """(out, mag).  ``dtype=np.float64``: the statement.  ``dtype=np.float32``: the yardstick, every product and every sum rounded to
    float32, the taps in order, then numpy's mean over the channels.  ``mag`` is float64 in both.  An output that a wrong reading
    leaves unwritten is NaN (the tests pre-fill ``out`` with NaN)."""
    assert variant is None or variant in VARIANTS, variant
    nch, ntaps, p, base, chans, unwritten, k_of, ks, tflat = _geometry(x, taps, orig, nw, width, n_out, variant)
    t_d = tflat.astype(dtype)
    t_64 = tflat.astype(np.float64)
    sums = np.zeros((nch, n_out), dtype=dtype)
    mag = np.zeros(n_out, dtype=np.float64)
    row = p * ntaps
    for c, (xp, off) in enumerate(chans):
        xd, x64 = xp.astype(dtype), xp.astype(np.float64)
        s = sums[c]
        for k in ks:
            ti, xi = row + k_of(k), base + (off + k)
            prod = t_d[ti] * xd[xi]
            s += prod
            mag += np.abs(prod if dtype == np.float64 else t_64[ti] * x64[xi])
    out = sums.sum(axis=0, dtype=dtype) if variant == "no_division" else sums.mean(axis=0, dtype=dtype)
    out[unwritten] = np.nan
    return out, mag / nch


def kernel_order_f32(x, taps, orig, nw, width, n_out):
    """The HIP kernel's order on the CPU: per channel a sequential multiply-add over k, each step computed in float64 and rounded to
    float32 (the product of two float32 values is exact in float64); the channels are then summed and divided by nch in float32."""
    x = np.asarray(x, dtype=np.float32)
    taps = np.asarray(taps, dtype=np.float32)
    nch, ntaps, p, base, chans, _, _, ks, tflat = _geometry(x, taps, orig, nw, width, n_out, None)
    t_64 = tflat.astype(np.float64)
    row = p * ntaps
    acc = np.zeros(n_out, dtype=np.float32)
    for xp, off in chans:
        x64 = xp.astype(np.float64)
        s = np.zeros(n_out, dtype=np.float32)
        for k in ks:
            s = (t_64[row + k] * x64[base + (off + k)] + s.astype(np.float64)).astype(np.float32)
        acc = acc + s
    return acc / np.float32(nch)
