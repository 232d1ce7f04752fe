"""numpy restatement of the P8 split format of artalk_amd/csrc/common.h, for the tests (checked by test_p8_format_cpu.py).

A row of K fp32 values (K % 8 == 0) is stored in the same 4 K bytes: every 8 consecutive elements are 32 bytes
[8 x f16 hi][8 x f16 lo] with hi = f16(x * 2^e), lo = f16(x * 2^e - hi) (round to nearest even, fp32 arithmetic), e the site exponent."""
import numpy as np

F16_MAX = 65504.0
EXPS = range(-8, 5)          # what artalk_set_site_scales accepts


def pack(x, e):
    """float32 [..., K] -> int32 words [..., K] in the P8 layout."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.shape[-1] % 8 == 0
    with np.errstate(over="ignore", invalid="ignore"):
        xs = x * np.float32(2.0 ** e)
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
    g = x.shape[:-1] + (x.shape[-1] // 8, 1, 8)
    halves = np.concatenate([hi.reshape(g), lo.reshape(g)], axis=-2)       # [..., K/8, 2, 8]
    return np.ascontiguousarray(halves).view(np.int32).reshape(x.shape)


def halves(words):
    """int32 words [..., K] -> (hi, lo) float16 arrays [..., K]."""
    w = np.ascontiguousarray(words, dtype=np.int32)
    h = w.view(np.float16).reshape(w.shape[:-1] + (w.shape[-1] // 8, 2, 8))
    return h[..., 0, :].reshape(w.shape), h[..., 1, :].reshape(w.shape)


def unpack(words, e):
    """int32 words [..., K] -> float64 values (hi + lo) / 2^e."""
    hi, lo = halves(words)
    return (hi.astype(np.float64) + lo.astype(np.float64)) / 2.0 ** e


def bound(x, e):
    """Round-trip error bound per element: hi carries 11 significand bits and lo 11 more of the residual (|x| * 2^-21 with a bit to
    spare) while lo is a normal fp16; below that lo is quantised in steps of fp16's subnormal quantum 2^-24, half of which, in units
    of x, is 2^-25 / 2^e."""
    return np.maximum(np.abs(np.asarray(x, dtype=np.float64)) * 2.0 ** -21, 2.0 ** -25 / 2.0 ** e)


def max_value(e):
    """Largest magnitude a site with exponent e can hold: 65504 / 2^e (exact in fp32)."""
    return np.float32(F16_MAX / 2.0 ** e)


def maxbits(e):
    """p8_maxbits_of(e) of common.h: the bit pattern the range guard compares |x| with (status bit 3 when above)."""
    return 0x477FE000 - e * 0x00800000
