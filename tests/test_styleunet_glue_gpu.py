"""The StyleUNet's style path and layout kernels alone (artalk_op_su_* of include/artalk_hip.h: linear_kernel, normstyle_kernel,
demod_kernel, add_kernel and the two layout kernels of artalk_amd/csrc/styleunet.hip), through the launchers the network uses, on the
case table of tests/su_glue_cases.py.  Every output lies NaN-filled between poisoned guard bands: the bands must stay poisoned, every
payload value must be written and finite, the inputs must be unchanged, and a second launch must give the same bits (no atomics).
add and the layouts without the sigmoid are bit-equal to the torch float32 statement; linear, normstyle, demod and the sigmoid stay
within the project's allowance for a float32 kernel against the float64 statement of tests/su_glue_ref.py: max-abs error <= 4 x e32,
with a floor of one float32 ulp of the case's largest output.  Run with -s for error / e32 per case."""
import numpy as np
import pytest
import torch

import su_glue_cases as sc
from artalk_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 256
POISON = -7.25e9


def _guarded(n):
    """A device buffer of n floats, NaN inside, between two poisoned bands."""
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf


def _payload(buf, n, what):
    torch.cuda.synchronize()
    whole = buf.cpu()
    assert bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all()), f"{what} wrote outside its output"
    got = whole[GUARD:GUARD + n]
    assert bool(torch.isfinite(got).all()), f"{what} left an output value unwritten, or wrote one that is not finite"
    return got


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(case, host, call):
    """One launch of call(device inputs, output pointer) into a guarded buffer, and a second one into another: the payload of the first,
    after the checks every kernel of this file shares.  host: the float32 CPU tensors the kernel reads (None: an absent one)."""
    what = sc.case_id(case)
    n = sc.reference(case).want.numel()
    dev = [None if h is None else h.contiguous().cuda() for h in host]
    first, second = _guarded(n), _guarded(n)
    assert call(dev, capi.ptr(first[GUARD:])) == capi.OK
    got = _payload(first, n, what)
    for h, d in zip(host, dev):
        assert h is None or torch.equal(_bits(d.cpu()), _bits(h)), f"{what} changed an input"
    assert call(dev, capi.ptr(second[GUARD:])) == capi.OK
    assert torch.equal(_bits(_payload(second, n, what)), _bits(got)), f"{what}: a second launch gave other bits"
    return got


def _within(case, got):
    r = sc.reference(case)
    got = got.reshape(r.want.shape).double()
    err = float((got - r.want).abs().max())
    print(f"{sc.case_id(case)}: max-abs error {err:.3e}, e32 {r.e32:.3e}, allowed {r.allowed:.3e}, error / e32 {err / max(r.e32, 1e-300):.2f}")
    assert err <= r.allowed, f"{sc.case_id(case)}: error {err:.3e} > allowed {r.allowed:.3e} (e32 {r.e32:.3e})"
    return got


def _exact(case, got):
    want32 = sc.reference(case).want32
    assert torch.equal(_bits(got.reshape(want32.shape)), _bits(want32)), f"{sc.case_id(case)} differs from the float32 statement"


@pytest.mark.parametrize("case", sc.LINEAR, ids=sc.case_id)
def test_linear(case):
    x, W, bias = sc.linear_inputs(case)
    got = _launch(case, (x, W, bias), lambda d, out: capi.lib().artalk_op_su_linear(
        capi.ptr(d[0]), capi.ptr(d[1]), capi.ptr(d[2]), out, case.B, case.In, case.Out, case.lrelu, capi.current_stream_ptr()))
    got = _within(case, got)
    if case.kind == "zero":
        r = sc.reference(case)
        pre = x.double() @ W.double().t() + bias.double()      # integers: exact in every order
        zero, neg = pre == 0, pre < -r.allowed
        assert int(zero.sum()) >= 3 and int(neg.sum()) >= 2 * (case.Out - 2)
        assert bool((got[zero] == 0.0).all()), "an exact zero must stay zero"
        assert float((got[neg] - 0.2 * pre[neg]).abs().max()) <= r.allowed and bool((got[neg] < 0.0).all())


@pytest.mark.parametrize("case", sc.NORMSTYLE, ids=sc.case_id)
def test_normstyle(case):
    (x,) = sc.normstyle_inputs(case)
    got = _launch(case, (x,), lambda d, out: capi.lib().artalk_op_su_normstyle(capi.ptr(d[0]), out, case.B, case.n, capi.current_stream_ptr()))
    got = _within(case, got)
    if case.zero_row >= 0:
        assert bool((got[case.zero_row] == 0.0).all()), "an all-zero row must give exact zeros"
        assert float(got.abs().max()) > 1.0


@pytest.mark.parametrize("case", sc.DEMOD, ids=sc.case_id)
def test_demod(case):
    s, wsq = sc.demod_inputs(case)
    rows, off, ld = sc.demod_rows(case, s)
    assert bool(torch.isnan(rows).any())
    got = _launch(case, (rows, wsq), lambda d, out: capi.lib().artalk_op_su_demod(
        capi.ptr(d[0][off:]), ld, capi.ptr(d[1]), out, case.B, case.Cin, case.Cout, capi.current_stream_ptr()))
    _within(case, got)


@pytest.mark.parametrize("case", sc.ADD, ids=sc.case_id)
def test_add(case):
    a, b = sc.add_inputs(case)
    got = _launch(case, (a, b), lambda d, out: capi.lib().artalk_op_su_add(capi.ptr(d[0]), capi.ptr(d[1]), out, case.n, capi.current_stream_ptr()))
    _exact(case, got)


@pytest.mark.parametrize("case", sc.TO_NHWC, ids=sc.case_id)
def test_to_nhwc(case):
    (x,) = sc.to_nhwc_inputs(case)
    got = _launch(case, (x,), lambda d, out: capi.lib().artalk_op_su_to_nhwc(capi.ptr(d[0]), out, case.B, case.C, case.HW, capi.current_stream_ptr()))
    _exact(case, got)


@pytest.mark.parametrize("case", sc.TO_NCHW, ids=sc.case_id)
def test_to_nchw(case):
    (x,) = sc.to_nchw_inputs(case)
    got = _launch(case, (x,), lambda d, out: capi.lib().artalk_op_su_to_nchw(
        capi.ptr(d[0]), out, case.B, case.C, case.HW, case.sigmoid, capi.current_stream_ptr()))
    if not case.sigmoid:
        _exact(case, got)
        return
    r = sc.reference(case)
    got = _within(case, got)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0, "a sigmoid output outside [0, 1]"
    v = x.transpose(1, 2).double()
    hi, lo = v >= sc.SIGMOID_EXTREME, v <= -sc.SIGMOID_EXTREME
    floor = float(np.spacing(np.float32(r.largest)))      # the allowance's floor: one float32 ulp of the case's largest output
    if x.numel() >= len(sc.SIGMOID_SPECIALS):
        assert int(hi.sum()) >= 4 and int(lo.sum()) >= 4
        assert float((1.0 - got[hi]).abs().max()) <= floor and float(got[lo].abs().max()) <= floor
