"""Torch-CPU restatement of the StyleUNet precision modes from DESIGN.md section 5 ("Precision modes"), in whatever dtype the input has
(float64 for the oracle, float32 for the e32 yardstick), on top of tests/styleunet_ref.py.  The operands of a convolution are fp32 by
definition in every dtype: a = fl32(x * in_scale), hi(v) = bf16(v), lo(v) = bf16(v - hi(v)); the products, their sum and the epilogue
run in the dtype.  ``terms`` replaces a mode's list of (activation part, weight part) products so that deliberately wrong variants can be
built.  Also the case table and input generator that the op-level tests of the modes share.  Not a product path."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import styleunet_ref as ref

_conv2d = ref.conv2d      # the unpatched restatement (styleunet_forward_mode swaps the module's name for the length of a call)

TERMS = {
    "f32": (("full", "full"),),
    "bf16x3": (("lo", "hi"), ("hi", "lo"), ("hi", "hi")),      # the two small products first, as the kernel adds them
    "bf16": (("hi", "hi"),),
}
# wrong variants per mode: what a kernel that drops a product, skips a rounding or silently runs another mode would compute
WRONG = {
    "bf16x3": {"without lo(a) hi(w)": (("hi", "lo"), ("hi", "hi")), "without hi(a) lo(w)": (("lo", "hi"), ("hi", "hi")),
               "hi hi only": TERMS["bf16"], "exact fp32 product": TERMS["f32"]},
    "bf16": {"activations not rounded": (("full", "hi"),), "weights not rounded": (("hi", "full"),), "three products": TERMS["bf16x3"]},
}
FACTOR = 4.0

# (Cin, Cout, k, B, H, W): the seven cases of tests/test_styleunet_ops_gpu.py, Cin and Cout off every tile multiple, Cin below one MFMA K
CASES = [(16, 16, 3, 1, 40, 24), (32, 16, 1, 2, 33, 17), (64, 32, 3, 2, 16, 16), (512, 512, 3, 3, 4, 4), (32, 3, 1, 2, 32, 32),
         (16, 32, 3, 1, 1, 1), (17, 5, 3, 1, 7, 9), (40, 72, 3, 1, 12, 11), (8, 16, 3, 1, 9, 130)]
SWITCHES = ("in_scale", "out_scale", "gain", "noise", "noise_shared", "bias", "lrelu", "sft", "residual")


def case_id(c):
    return "x".join(map(str, c))


def inputs(case, on, seed=0, ring=False):
    """The generator of tests/test_styleunet_ops_gpu.py: float32-exact values held in float64, so both sides round the same operands."""
    Cin, Cout, k, B, H, W = case
    g = torch.Generator().manual_seed(1000 * seed + Cin + 7 * Cout + 13 * H)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()
    x = rnd(B, Cin, H, W)
    if ring:
        inner = torch.zeros(H, W, dtype=torch.bool)
        inner[1:-1, 1:-1] = True
        x[:, :, inner] = 0.0
    a = dict(x=x, w=rnd(Cout, Cin, k, k) / math.sqrt(Cin * k * k))
    a["w"] = a["w"].float().double()      # (the division left float64 values: the kernel reads fp32 weights)
    if "in_scale" in on:
        a["in_scale"] = (1.0 + 0.3 * rnd(B, Cin)).float().double()
    if "out_scale" in on:
        a["out_scale"] = (1.0 + 0.3 * rnd(B, Cout)).float().double()
    if "gain" in on:
        a["gain"] = float(np.float32(math.sqrt(2.0)))
    if "noise" in on or "noise_shared" in on:
        a["noise"] = rnd(1 if "noise_shared" in on else B, 1, H, W)
        a["noise_weight"] = (rnd(1) * 0.5).float().double()
    if "bias" in on:
        a["bias"] = (rnd(Cout) * 0.3).float().double()
    if "lrelu" in on:
        a["slope"] = 0.2
    if "sft" in on:
        a["sft_scale"], a["sft_shift"] = (1.0 + 0.3 * rnd(B, Cout, H, W)).float().double(), rnd(B, Cout, H, W)
    if "residual" in on:
        a["residual"] = rnd(B, Cout, H, W)
    return a


def _part(v, which):
    """v: float32.  hi = bf16(v) (round to nearest even), lo = bf16(v - hi) (the difference is exact in fp32)."""
    if which == "full":
        return v
    hi = v.to(torch.bfloat16).float()
    return hi if which == "hi" else (v - hi).to(torch.bfloat16).float()


def conv2d_mode(mode, x, w, in_scale=None, terms=None, **epilogue):
    """``styleunet_ref.conv2d`` with the convolution of mode ``mode`` ("f32", "bf16x3", "bf16") in the dtype of x; the epilogue is
    that function's own (applied through an identity 1 x 1 convolution, which changes no value)."""
    dt = x.dtype
    a = x.float()
    if in_scale is not None:
        a = a * in_scale.float()[:, :, None, None]      # one rounded fp32 multiply
    wf = w.float()
    core = None
    for pa, pw in (TERMS[mode] if terms is None else terms):
        t = F.conv2d(_part(a, pa).to(dt), _part(wf, pw).to(dt), padding=w.shape[-1] // 2)
        core = t if core is None else core + t
    eye = torch.eye(w.shape[0], dtype=dt)[:, :, None, None]
    return _conv2d(core, eye, **epilogue)


def styleunet_forward_mode(mode, sd, x, terms=None, **kw):
    """``styleunet_ref.styleunet_forward`` with every convolution in mode ``mode``; everything else is that function's."""
    ref.conv2d = lambda t, w, **k: conv2d_mode(mode, t, w, terms=terms, **k)
    try:
        return ref.styleunet_forward(sd, x, **kw)
    finally:
        ref.conv2d = _conv2d


def allowance(want64, want32):
    """(allowed, e32): the project's rule per mode - 4 x the float32-vs-float64 distance of the mode's own definition, with a floor of
    one float32 ulp of the largest output."""
    e32 = float((want32.double() - want64).abs().max())
    ulp = float(np.spacing(np.float32(want64.abs().max())))
    return max(FACTOR * e32, ulp), e32
