"""Every case of tests/conv_edge_cases.py as one launch of artalk_op_conv2d_ex in precision 0, 1 and 2, against the float64 statement of
that mode (tests/styleunet_ref.py, tests/styleunet_prec_ref.py).  Allowance, the project's rule unchanged: max-abs error <= max(4 x e32,
one float32 ulp of the largest output), e32 being the float32-vs-float64 distance of the same statement on the CPU - never derived from
the kernel.  What this bar can see of each edge is tests/test_conv_edges_cpu.py.

Guard bands everywhere: the output starts as NaN between poisoned bands that must stay poisoned, and every operand - x with the padding
between its samples, w, in_scale, out_scale, noise and its weight, bias, SFT scale and shift, residual - is a view into a larger device
tensor whose surroundings are NaN, so an over-read that reaches a sum shows as a non-finite output.  A variant that moves an operand off
its 16-byte boundary or pads the sample stride must also give the bits of its aligned twin: the values staged into LDS are the same and
the rest is the same code.  Run with -s for the instantiation and the error / e32 ratio of every case; the ranges are in DESIGN.md."""
import pytest
import torch

import conv_edge_cases as ce
from artalk_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 256      # floats: a multiple of 16 bytes, so a band moves no alignment
POISON = -7.25e9
NAN = float("nan")


def _banded(flat, shift=0):
    """flat: CPU float32, one dimension -> its values on the device, `shift` floats past a 16-byte boundary, NaN on both sides."""
    n = flat.numel()
    big = torch.full((n + 2 * GUARD + shift,), NAN, dtype=torch.float32, device="cuda")
    view = big[GUARD + shift:GUARD + shift + n]      # (the view keeps `big` alive)
    view.copy_(flat)
    assert view.data_ptr() % 16 == 4 * shift
    return view


def _cl(t):
    """(B, C, H, W) float64 -> channels-last float32, flat, on the CPU"""
    return t.permute(0, 2, 3, 1).contiguous().float().reshape(-1)


def _launch(c, precision):
    """One launch; returns (output as (B, Cout, H, W) float32 on the CPU, the plan for the addresses that were passed)."""
    Cin, Cout, k, B, H, W = c.shape
    a = ce.case_inputs(c.shape, c.on, c.seed)
    lay = ce.layout(c)
    tight, stride = H * W * Cin, lay["x_bstride"]
    xs = torch.full((B, stride), NAN, dtype=torch.float32)      # the padding between samples is NaN as well
    xs[:, :tight] = _cl(a["x"]).reshape(B, tight)
    x = _banded(xs.reshape(-1), lay["x"])
    w = _banded(a["w"].permute(2, 3, 1, 0).contiguous().float().reshape(-1), lay["w"])
    flat = lambda key, shift=0: None if key not in a else _banded(a[key].float().reshape(-1), shift)
    ins, outs, noise, nw, bias = flat("in_scale", lay["in_scale"]), flat("out_scale"), flat("noise"), flat("noise_weight"), flat("bias")
    sc, sh, res = (None if key not in a else _banded(_cl(a[key])) for key in ("sft_scale", "sft_shift", "residual"))
    for t, off in ((x, lay["x"]), (w, lay["w"]), (ins, lay["in_scale"])):
        assert t is None or t.data_ptr() % 16 == 4 * off
    nstride = 0 if noise is None or a["noise"].shape[0] == 1 else H * W

    n = B * H * W * Cout
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float32, device="cuda")
    out = buf[GUARD:GUARD + n]
    out.fill_(NAN)
    plan = capi.conv2d_plan(x.data_ptr(), stride, w.data_ptr(), 0 if ins is None else ins.data_ptr(), B, H, W, Cin, Cout, k, precision)
    rc = capi.lib().artalk_op_conv2d_ex(capi.ptr(x), stride, capi.ptr(w), capi.ptr(out), B, H, W, Cin, Cout, k, capi.ptr(ins), capi.ptr(outs),
                                        a.get("gain", 1.0), capi.ptr(noise), nstride, capi.ptr(nw), capi.ptr(bias), 1 if "slope" in a else 0,
                                        capi.ptr(sc), capi.ptr(sh), capi.ptr(res), precision, capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()
    whole = buf.cpu()
    assert bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all()), "the kernel wrote outside its output"
    got = whole[GUARD:GUARD + n].reshape(B, H, W, Cout).permute(0, 3, 1, 2)
    bad = int((~torch.isfinite(got)).sum())
    assert bad == 0, f"{bad} output values are not finite: not written, or summed from outside an operand"
    return got, plan


_twins = {}      # (aligned case, precision) -> its output, computed once


def _twin_output(c, precision):
    key = (ce.twin(c), precision)
    if key not in _twins:
        _twins[key] = _launch(key[0], precision)[0]
    return _twins[key]


@pytest.mark.parametrize("mode", ce.MODES)
@pytest.mark.parametrize("case", ce.CASES, ids=ce.case_id)
def test_edge_case(case, mode):
    precision = ce.MODES.index(mode)
    want, allowed, e32 = ce.reference(case, mode)
    got, plan = _launch(case, precision)
    assert plan == ce.expected_plan(case, mode), "the launch did not run the instantiation the table names"
    err = float((got.double() - want).abs().max())
    print(f"{case.family} {mode} {ce.case_id(case)} {capi.conv_kernel_name(plan)} steps {plan['steps']}: max-abs error {err:.3e}, e32 {e32:.3e}, "
          f"error / e32 {err / max(e32, 1e-300):.2f}, allowed {allowed:.2e}")
    assert err <= allowed, f"{mode} {ce.case_id(case)}: error {err:.3e} > allowed {allowed:.3e} (e32 {e32:.3e})"
    if case.variant != "aligned":
        same = torch.equal(got, _twin_output(case, precision))
        assert same, f"{mode} {ce.case_id(case)} ({capi.conv_kernel_name(plan)}): not the bits of the aligned launch"
