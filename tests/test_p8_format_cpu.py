"""The numpy restatement of the P8 split format (tests/p8_format.py) that the GPU tests use as their reference: layout, round-trip
accuracy at every site exponent and the guard threshold.  No GPU."""
import os
import re

import numpy as np
import pytest

import p8_format as p8

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _values(e, n=1 << 16):
    """Magnitudes over the whole range of a site with exponent e: log-uniform from 2^-30 / 2^e up to the largest value, signs mixed."""
    rng = np.random.default_rng(100 + e)
    top = float(p8.max_value(e))
    x = np.exp2(rng.uniform(np.log2(top) - 46.0, np.log2(top), n)) * rng.choice([-1.0, 1.0], n)
    x = np.minimum(np.abs(x), top) * np.sign(x)
    x[:8] = [top, -top, 0.0, top / 2, 1.0 / 2.0 ** e, 3.0 / 2.0 ** e, 2.0 ** -14 / 2.0 ** e, 2.0 ** -24 / 2.0 ** e]
    return x.astype(np.float32)


@pytest.mark.parametrize("e", list(p8.EXPS))
def test_round_trip_bound(e):
    x = _values(e)
    w = p8.pack(x, e)
    assert w.dtype == np.int32 and w.shape == x.shape
    hi, lo = p8.halves(w)
    assert np.isfinite(hi).all() and np.isfinite(lo).all(), "values up to 65504 / 2^e are stored finite"
    err = np.abs(p8.unpack(w, e) - x.astype(np.float64))
    lo_normal = np.abs(lo.astype(np.float64)) >= 2.0 ** -14
    rel = err[lo_normal] / np.abs(x[lo_normal].astype(np.float64))
    assert lo_normal.sum() > 1000 and (~lo_normal).sum() > 1000
    assert rel.max() <= 2.0 ** -21, rel.max()
    assert err[~lo_normal].max() <= 2.0 ** -25 / 2.0 ** e, (err[~lo_normal].max(), 2.0 ** -25 / 2.0 ** e)
    assert (err <= p8.bound(x, e)).all()


def test_layout_is_8_hi_then_8_lo():
    x = (np.arange(1, 33, dtype=np.float32) + np.float32(2.0 ** -12)).reshape(2, 16)
    w = p8.pack(x, 0)
    h = w.view(np.float16).reshape(2, 2, 2, 8)          # row, group of 8, half, element
    assert np.array_equal(h[:, :, 0, :].reshape(2, 16), np.arange(1, 33, dtype=np.float16).reshape(2, 16))
    assert (h[:, :, 1, :] == np.float16(2.0 ** -12)).all()
    assert np.array_equal(p8.unpack(w, 0), x.astype(np.float64))
    # exactly representable inputs: the same value at every exponent, lo = 0
    ints = (np.arange(-16, 16, dtype=np.float32) * 4).reshape(4, 8)
    for e in p8.EXPS:
        we = p8.pack(ints, e)
        assert np.array_equal(p8.unpack(we, e), ints.astype(np.float64)) and not p8.halves(we)[1].any()


@pytest.mark.parametrize("e", list(p8.EXPS))
def test_guard_threshold_is_the_largest_finite_value(e):
    top = p8.max_value(e)
    assert float(top) * 2.0 ** e == p8.F16_MAX
    assert int(np.float32(top).view(np.uint32)) == p8.maxbits(e)
    up = np.nextafter(top, np.float32(np.inf))
    assert int(up.view(np.uint32)) == p8.maxbits(e) + 1
    for bad in (np.float32(np.inf), np.float32(np.nan)):
        assert int(np.abs(bad).view(np.uint32)) > p8.maxbits(e), "inf and NaN patterns lie above every finite one"
    hi, lo = p8.halves(p8.pack(np.full(8, top, np.float32), e))
    assert (hi == np.float16(65504.0)).all() and not lo.any()
    # the first value the guard reports (|x| * 2^e just above 65504) still rounds to a finite hi: the guard is on the safe side
    assert np.isfinite(p8.halves(p8.pack(np.full(8, up, np.float32), e))[0]).all()


def test_constants_match_common_h():
    src = open(os.path.join(REPO, "artalk_amd", "csrc", "common.h")).read()
    m = re.search(r"p8_maxbits_of\(int e\)\s*\{\s*return \(unsigned int\)\((0x[0-9A-Fa-f]+) - e \* (0x[0-9A-Fa-f]+)\);", src)
    assert m, "p8_maxbits_of changed its form: restate it in tests/p8_format.py"
    assert all(int(m.group(1), 16) - e * int(m.group(2), 16) == p8.maxbits(e) for e in p8.EXPS)
    assert re.search(r"kStatusP8Range\s*=\s*8\b", src) and re.search(r"kActExp\s*=\s*4\b", open(os.path.join(REPO, "artalk_amd", "csrc", "kernels.h")).read())
