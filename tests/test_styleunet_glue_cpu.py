"""The StyleUNet style path and layout entry points (artalk_op_su_*) and their case table (tests/su_glue_cases.py) without a GPU: the
entry points refuse NULL pointers, non-positive sizes and ld < Cin before they touch the device; the table holds the edges it names;
no allowance is silently zero; and the allowance of tests/test_styleunet_glue_gpu.py can see the faults these kernels could have: for
each deliberately wrong float64 reading of tests/su_glue_ref.py at least one case misses its allowance.  Run with -s for the size of
every miss."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import su_glue_cases as sc
from artalk_amd import capi
from su_glue_ref import Reading

P = C.c_void_p(1 << 26)      # an address that is never dereferenced: every call below is refused before the device is touched


def test_the_symbols_are_exported():
    L = capi.lib()
    for name in ("linear", "normstyle", "demod", "add", "to_nhwc", "to_nchw"):
        assert "artalk_op_su_" + name in capi.SYMBOLS and hasattr(L, "artalk_op_su_" + name)


def test_refusals():
    L = capi.lib()
    linear = lambda x=P, W=P, b=P, y=P, B=2, In=8, Out=3: L.artalk_op_su_linear(x, W, b, y, B, In, Out, 1, None)
    normstyle = lambda x=P, y=P, B=2, n=8: L.artalk_op_su_normstyle(x, y, B, n, None)
    demod = lambda s=P, ld=8, wsq=P, d=P, B=2, Cin=8, Cout=3: L.artalk_op_su_demod(s, ld, wsq, d, B, Cin, Cout, None)
    add = lambda a=P, b=P, out=P, n=8: L.artalk_op_su_add(a, b, out, n, None)
    to_nhwc = lambda x=P, out=P, B=2, Ch=3, HW=8: L.artalk_op_su_to_nhwc(x, out, B, Ch, HW, None)
    to_nchw = lambda x=P, out=P, B=2, Ch=3, HW=8, sg=1: L.artalk_op_su_to_nchw(x, out, B, Ch, HW, sg, None)
    refused = [
        (linear, [dict(x=None), dict(W=None), dict(y=None), dict(B=0), dict(In=0), dict(Out=0), dict(B=-1), dict(In=-8), dict(Out=-3)]),
        (normstyle, [dict(x=None), dict(y=None), dict(B=0), dict(n=0), dict(B=-2), dict(n=-8)]),
        (demod, [dict(s=None), dict(wsq=None), dict(d=None), dict(B=0), dict(Cin=0), dict(Cout=0), dict(B=-1), dict(Cin=-8), dict(Cout=-1),
                 dict(ld=7), dict(ld=0), dict(ld=-8)]),
        (add, [dict(a=None), dict(b=None), dict(out=None), dict(n=0), dict(n=-1)]),
        (to_nhwc, [dict(x=None), dict(out=None), dict(B=0), dict(Ch=0), dict(HW=0), dict(B=-1), dict(Ch=-3), dict(HW=-8)]),
        (to_nchw, [dict(x=None), dict(out=None), dict(B=0), dict(Ch=0), dict(HW=0), dict(B=-1), dict(Ch=-3), dict(HW=-8)]),
    ]
    n = 0
    for fn, kws in refused:
        for kw in kws:
            assert fn(**kw) == capi.EINVAL, kw
            n += 1
    assert n == 48
    # a size whose grid would not fit a launch is refused too, without overflow on the way
    assert add(n=1 << 62) == capi.EINVAL and to_nhwc(B=1 << 30, Ch=1 << 30, HW=1 << 40) == capi.EINVAL
    assert to_nchw(B=1 << 30, Ch=1 << 30, HW=1 << 40) == capi.EINVAL


def test_the_table_holds_the_edges_it_names():
    rand = [c for c in sc.LINEAR if c.kind == "rand"]
    assert {c.In for c in rand} == {1, 63, 64, 65, 512, 4096}
    # rows(): a nominal (B, Out) short of 16 outputs runs with B + 4 j rows, which keeps B * Out % 4
    assert [sc.rows(B, w) for B, w in ((1, 1), (3, 3), (1, 5), (2, 3), (1, 7), (2, 512), (3, 171), (1, 16), (3, 5))] == [17, 7, 5, 6, 5, 2, 3, 1, 7]
    assert {(c.B, c.Out) for c in rand} >= {(sc.rows(B, Out), Out) for B, Out in ((1, 1), (3, 3), (1, 5), (2, 512), (3, 171))}
    assert all(c.B * c.Out >= sc.MIN_OUTPUTS for c in rand) and all(c.B * c.Cout >= sc.MIN_OUTPUTS for c in sc.DEMOD)
    for In in sc.LINEAR_IN:
        assert {(c.B * c.Out % 4, c.bias, c.lrelu) for c in rand if c.In == In} == {(m, b, a) for m in range(4) for b in (True, False) for a in (0, 1)}
    plain = [c for c in sc.NORMSTYLE if c.zero_row < 0]
    assert {(c.n, c.B, c.scale) for c in plain} == {(n, sc.rows(B, n), s) for n in (1, 63, 64, 65, 512) for B in (1, 3) for s in (1.0, 1e-4)}
    assert {(c.Cin, c.Cout, c.B, c.scale) for c in sc.DEMOD} >= {(ci, co, sc.rows(B, co), s) for ci in (16, 32, 64, 65, 256, 512)
                                                                  for co in (1, 3, 32, 512) for B in (1, 3) for s in (1.0, 1e-4)}
    assert len(plain) == 20 and len(sc.DEMOD) == 98 and len(rand) == 168
    assert {c.B * c.Cout % 4 for c in sc.DEMOD} == {0, 1, 2, 3}
    assert sc.MOD_OFF % 4 != 0 and sc.LD_EXTRA > sc.MOD_OFF
    assert [c.n for c in sc.ADD] == [1, 255, 256, 257, 1025]
    shapes = {(1, 1, 1), (3, 3, 16), (1, 5, 63), (2, 32, 64), (1, 3, 4096)}
    assert {tuple(c) for c in sc.TO_NHWC} == shapes and {tuple(c) for c in sc.TO_NCHW} == {s + (g,) for s in shapes for g in (0, 1)}
    assert len({sc.case_id(c) for c in sc.ALL}) == len(sc.ALL)


def test_the_inputs_hold_what_the_cases_promise():
    x, W, bias = sc.linear_inputs(sc.ZERO_LINEAR)
    pre = x.double() @ W.double().t() + bias.double()
    assert bool((pre[:, 0] == 0).all()) and float(pre[0, 1]) == 0.0 and float((x[0] @ W[1]).abs()) > 0.0 and float(pre[:, 2:].max()) < -600.0
    assert torch.equal(pre, pre.round()) and float(x.abs().max() * W.abs().max()) * sc.ZERO_LINEAR.In < 2 ** 24
    (x,) = sc.normstyle_inputs(sc.ZERO_NORMSTYLE)
    assert float(x[1].abs().max()) == 0.0 and float(x[0].abs().min()) > 0.0 and float(x[2].abs().min()) > 0.0
    for c in sc.NORMSTYLE + sc.DEMOD:      # at scale 1e-4 the mean (the sum) of squares is of the order of the 1e-8
        if c.scale == 1e-4:
            a = sc.inputs(c)
            v = (a[0].double() ** 2).mean(dim=1) if isinstance(c, sc.NormStyle) else (a[0].double() ** 2) @ a[1].double().t()
            assert 1e-11 < float(v.min()) and float(v.max()) < 1e-6, sc.case_id(c)
    c = sc.Demod(65, 3, 3, 1.0)
    s, _ = sc.demod_inputs(c)
    buf, off, ld = sc.demod_rows(c, s)
    rows = buf.reshape(c.B, ld)
    assert ld > c.Cin and off % 4 != 0 and torch.equal(rows[:, off:off + c.Cin], s)
    assert bool(torch.isnan(rows[:, :off]).all()) and bool(torch.isnan(rows[:, off + c.Cin:]).all())
    for c in sc.TO_NCHW:
        if c.sigmoid:
            (x,) = sc.to_nchw_inputs(c)
            have = x.reshape(-1).tolist()
            for v in (float(np.float32(s)) for s in sc.SIGMOID_SPECIALS[:x.numel()]):
                assert any(h == v and math.copysign(1.0, h) == math.copysign(1.0, v) for h in have), (sc.case_id(c), v)
            assert x.numel() < len(sc.SIGMOID_SPECIALS) or int((x.abs() >= sc.SIGMOID_EXTREME).sum()) >= 8
    assert set(sc.SIGMOID_SPECIALS) == {0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e30, -1e30}


@pytest.mark.parametrize("case", [c for c in sc.ALL if not sc.is_exact(c)], ids=sc.case_id)
def test_no_allowance_is_silently_zero(case):
    r = sc.reference(case)
    floor = float(np.spacing(np.float32(r.largest)))
    assert bool(torch.isfinite(r.want).all()) and bool(torch.isfinite(r.want32).all())
    assert r.allowed > 0.0 and (r.e32 > 0.0 or r.allowed == floor) and r.allowed == max(4.0 * r.e32, floor)


@pytest.mark.parametrize("case", [c for c in sc.ALL if sc.is_exact(c)], ids=sc.case_id)
def test_exact_cases_are_exact_in_float32(case):
    r = sc.reference(case)
    assert r.allowed == 0.0 and r.want32.dtype == torch.float32
    if not isinstance(case, sc.Add):      # (a sum rounds; a layout only moves values)
        assert r.e32 == 0.0 and sorted(r.want32.reshape(-1).tolist()) == sorted(sc.inputs(case)[0].reshape(-1).tolist())


# ---- what the allowance can tell apart ----
def _misses(tag, cases, reading):
    """The cases whose right reference the wrong reading misses by more than the case's allowance (a NaN counts as a miss: the GPU
    test refuses a payload that is not finite)."""
    caught = []
    for c in cases:
        r = sc.reference(c)
        with torch.no_grad():
            wrong = sc.statement(c, sc.to64(sc.inputs(c)), reading)
        miss = float(torch.nan_to_num((wrong - r.want).abs(), nan=float("inf")).max())
        if miss > r.allowed:
            caught.append(c)
            print(f"{tag}: {sc.case_id(c)} misses by {miss:.3e} = {miss / r.allowed if r.allowed else float('inf'):.3g} x the allowance {r.allowed:.2e}")
    return caught


def test_wrong_reading_eps_outside_the_root():
    wrong = Reading(eps_outside_root=True)
    for cases in (sc.NORMSTYLE, sc.DEMOD):
        caught = _misses("eps outside the root", cases, wrong)
        assert {c for c in cases if c.scale == 1e-4} <= set(caught), "every small-scale case must see the place of the 1e-8"


def test_wrong_reading_eps_on_the_sum():
    caught = _misses("eps added to the sum, not the mean", sc.NORMSTYLE, Reading(eps_on_sum=True))
    assert {c for c in sc.NORMSTYLE if c.scale == 1e-4 and c.n > 1} <= set(caught)
    assert not [c for c in caught if c.n == 1], "with one element the sum is the mean"


def test_wrong_reading_style_not_squared():
    assert len(_misses("style not squared", sc.DEMOD, Reading(style_squared=False))) == len(sc.DEMOD)


def test_wrong_reading_wsq_indexed_ci_co():
    caught = _misses("wsq indexed [ci][co]", sc.DEMOD, Reading(wsq_transposed=True))
    assert {c for c in sc.DEMOD if c.Cout > 1} <= set(caught) and not [c for c in caught if c.Cout == 1]


def test_wrong_reading_w_transposed():
    caught = _misses("W transposed", sc.LINEAR, Reading(w_transposed=True))
    assert {c for c in sc.LINEAR if c.kind == "rand" and c.In > 1 and c.Out > 1} <= set(caught)


def test_wrong_reading_leaky_slope():
    caught = _misses("leaky slope 0.01", sc.LINEAR, Reading(slope=0.01))
    assert caught and all(c.lrelu for c in caught) and sc.ZERO_LINEAR in caught
    assert {(c.In, c.bias) for c in caught} >= {(In, b) for In in sc.LINEAR_IN for b in (True, False)}


def test_wrong_reading_leaky_before_the_bias():
    caught = _misses("leaky before the bias", sc.LINEAR, Reading(lrelu_before_bias=True))
    assert caught and all(c.lrelu and c.bias for c in caught) and {c.In for c in caught} == set(sc.LINEAR_IN)


def test_wrong_reading_last_input_element_dropped():
    """The tail of every lane-strided sum: at each length of the table at least one case sees one dropped element - one of 4096 too."""
    wrong = Reading(drop_last=True)
    caught = _misses("last input element dropped", sc.LINEAR, wrong)
    assert {c.In for c in caught} == set(sc.LINEAR_IN) and {(c.B, c.Out) for c in caught if c.In == 4096} >= {(2, 512), (3, 171)}
    caught = _misses("last input element dropped", sc.NORMSTYLE, wrong)
    assert {c.n for c in caught} == set(sc.NORMSTYLE_N) and {c.scale for c in caught} == set(sc.SCALES)
    caught = _misses("last input element dropped", sc.DEMOD, wrong)
    assert {c.Cin for c in caught} == set(sc.DEMOD_CIN) and {c.scale for c in caught} == set(sc.SCALES)


def test_wrong_reading_to_nhwc_with_c_and_hw_swapped():
    caught = _misses("to_nhwc with C and HW swapped", sc.TO_NHWC, Reading(nhwc_swapped=True))
    assert {tuple(c) for c in caught} == {(3, 3, 16), (1, 5, 63), (2, 32, 64), (1, 3, 4096)}      # (1, 1, 1) has nothing to swap
