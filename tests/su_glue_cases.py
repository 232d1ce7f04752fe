"""Case table of the StyleUNet style path and layout kernels' tests (tests/test_styleunet_glue_cpu.py, test_styleunet_glue_gpu.py): the
smallest shapes that still reach each path of linear_kernel, normstyle_kernel, demod_kernel, add_kernel and the two layout kernels of
artalk_amd/csrc/styleunet.hip.

  lane-strided sums (for (i = lane; i < n; i += 64)): lengths 1, 63, 64, 65 - fewer inputs than a wave has lanes, one short, exact, one
      over - and the widths the network runs (512 and 4096 in linear, 512 in normstyle, 16 .. 512 in demod: the style convs of the
      head's 512 x 512 output go down to Cin = 32 and 16)
  one wave per output value, four waves per workgroup: B * Out (B * Cout) takes every residue mod 4, so a last workgroup has 3, 2, 1 and
      no idle waves; a case of fewer than 16 outputs runs with more rows, in fours (rows() below says why)
  the 1e-8 of normstyle and demod: inputs at scale 1e-4 make the sum of squares of the order of the 1e-8, so its place matters
  demod's rows: ld > Cin apart, starting MOD_OFF floats (not a multiple of 4) into the buffer, NaN everywhere outside the Cin windows
  one thread per value, 256 per workgroup: n = 1, 255, 256, 257, 1025; layouts with C and HW odd, equal to 1, and across workgroups

Inputs are rebuilt from seeds and not stored.  reference(case) is computed once per case and read only: the float64 statement
(tests/su_glue_ref.py), e32 - the same statement in float32 on the CPU against it, over the whole output of the case - and the
project's allowance for a float32 kernel made of the two (gsgen_cases.allowance: 4 x e32, with a floor of one float32 ulp of the case's
largest output).  add and the layouts without the sigmoid are exact: their allowance is 0 and the GPU test compares bits."""
import zlib
from collections import namedtuple

import numpy as np
import torch

import su_glue_ref as ref
from gsgen_cases import allowance

Linear = namedtuple("Linear", "In B Out bias lrelu kind")      # kind: "rand", or "zero" (exact integers, see linear_inputs)
NormStyle = namedtuple("NormStyle", "n B scale zero_row")      # zero_row: index of an all-zero row, or -1
Demod = namedtuple("Demod", "Cin Cout B scale")
Add = namedtuple("Add", "n")
ToNhwc = namedtuple("ToNhwc", "B C HW")
ToNchw = namedtuple("ToNchw", "B C HW sigmoid")

LINEAR_IN = (1, 63, 64, 65, 512, 4096)
LINEAR_B_OUT = ((1, 1), (3, 3), (1, 5), (2, 512), (3, 171), (2, 3), (1, 7))      # B * Out % 4 = 1, 1, 1, 0, 1 and, the last two, 2 and 3
NORMSTYLE_N = (1, 63, 64, 65, 512)
DEMOD_CIN = (16, 32, 64, 65, 256, 512)
DEMOD_COUT = (1, 3, 32, 512)
ADD_N = (1, 255, 256, 257, 1025)
LAYOUT_SHAPES = ((1, 1, 1), (3, 3, 16), (1, 5, 63), (2, 32, 64), (1, 3, 4096))
SCALES = (1.0, 1e-4)
MOD_OFF, LD_EXTRA = 5, 9      # demod: the row window starts 5 floats into its row, rows are Cin + 9 apart
SIGMOID_SPECIALS = (0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e30, -1e30)
SIGMOID_EXTREME = 20.0        # |v| >= 20: the logistic function is within 2.1e-9 of 0 or 1, far inside one ulp of 1

MIN_OUTPUTS = 16


def rows(B, per_row):
    """The rows a case of nominally B rows runs with: B, plus fours (B * per_row % 4, and with it the idle waves of the last workgroup,
    stays what it was) until the case has MIN_OUTPUTS output values.  e32 is a maximum over the case's outputs; taken over one or a few
    values it is whatever rounding those few happen to meet - down to a fraction of an ulp - and a correct kernel that sums in another
    order exceeds four times it by chance: one run on the MI355X measured 2.07 x and 1.17 x the allowance at (B, Out) = (1, 1),
    In = 65 (e32 3.9e-9 and 1.6e-9 from the one output value), 0.93 x at demod (B, Cout) = (1, 1) and 0.82 x at (B, Out) = (1, 7); with
    these rows the same kernels measured at most 0.58 x over the whole table.  The rule for a float32 kernel stays as it is; such a case
    gets more rows."""
    while B * per_row < MIN_OUTPUTS:
        B += 4
    return B


ZERO_LINEAR = Linear(65, 2, 7, True, 1, "zero")      # (integers: the only rounding is the one product with 0.2, the same in any order)
LINEAR = [Linear(In, rows(B, Out), Out, bias, lrelu, "rand") for In in LINEAR_IN for B, Out in LINEAR_B_OUT for bias in (True, False)
          for lrelu in (0, 1)]
LINEAR.append(ZERO_LINEAR)
ZERO_NORMSTYLE = NormStyle(65, 3, 1.0, 1)
NORMSTYLE = [NormStyle(n, rows(B, n), sc, -1) for n in NORMSTYLE_N for B in (1, 3) for sc in SCALES] + [ZERO_NORMSTYLE]
DEMOD = [Demod(Cin, Cout, rows(B, Cout), sc) for Cin in DEMOD_CIN for Cout in DEMOD_COUT for B in (1, 3) for sc in SCALES]      # B * Cout % 4: 1, 3, 0
DEMOD += [Demod(32, 3, rows(2, 3), 1.0), Demod(65, 3, rows(2, 3), 1e-4)]                                                      # ... and 2
ADD = [Add(n) for n in ADD_N]
TO_NHWC = [ToNhwc(*s) for s in LAYOUT_SHAPES]
TO_NCHW = [ToNchw(*s, sg) for s in LAYOUT_SHAPES for sg in (0, 1)]
ALL = LINEAR + NORMSTYLE + DEMOD + ADD + TO_NHWC + TO_NCHW


def case_id(c):
    return type(c).__name__.lower() + "-" + "-".join(f"{v:g}" if isinstance(v, float) else str(int(v) if isinstance(v, bool) else v) for v in c)


def is_exact(c):
    """The kernel only moves or adds float32 values: the torch float32 statement gives its bits."""
    return isinstance(c, (Add, ToNhwc)) or (isinstance(c, ToNchw) and not c.sigmoid)


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))


def _rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def linear_inputs(c):
    """x (B, In), W (Out, In), bias (Out) or None.  kind "zero": small integers, so that every pre-activation is an integer that float32
    sums without rounding in any order: column 0 is 0 + 0, column 1 of row 0 is a sum cancelled by its bias, the columns from 2 on are
    negative by hundreds."""
    g = _gen(c)
    if c.kind == "zero":
        x = torch.randint(-3, 4, (c.B, c.In), generator=g).float()
        W = torch.randint(-3, 4, (c.Out, c.In), generator=g).float()
        W[0] = 0.0
        bias = torch.full((c.Out,), -700.0)
        bias[0] = 0.0
        bias[1] = -float(x[0] @ W[1])
        return x, W, bias
    x = _rnd(g, c.B, c.In)
    W = _rnd(g, c.Out, c.In) / float(np.sqrt(c.In))
    bias = 0.5 * _rnd(g, c.Out) if c.bias else None
    return x, W, bias


def normstyle_inputs(c):
    x = c.scale * _rnd(_gen(c), c.B, c.n)
    if c.zero_row >= 0:
        x[c.zero_row] = 0.0
    return (x,)


def demod_inputs(c):
    """s (B, Cin) at the case's scale, and wsq (Cout, Cin) as finalize makes it: the sum over nine taps of squared weights."""
    g = _gen(c)
    s = c.scale * _rnd(g, c.B, c.Cin)
    w = _rnd(g, c.Cout, c.Cin, 9) / float(np.sqrt(9 * c.Cin))
    return s, (w * w).sum(dim=2)


def demod_rows(c, s):
    """The buffer the kernel is given, and the offset of its s pointer: rows ld apart, NaN outside the windows."""
    ld = c.Cin + LD_EXTRA
    buf = torch.full((c.B, ld), float("nan"), dtype=torch.float32)
    buf[:, MOD_OFF:MOD_OFF + c.Cin] = s
    return buf.reshape(-1), MOD_OFF, ld


def add_inputs(c):
    g = _gen(c)
    return _rnd(g, c.n), _rnd(g, c.n)


def to_nhwc_inputs(c):
    return (_rnd(_gen(c), c.B, c.C, c.HW),)


def to_nchw_inputs(c):
    """x (B, HW, C); with the sigmoid on, the special values are spread over it (as many as fit)."""
    x = 3.0 * _rnd(_gen(c), c.B, c.HW, c.C)
    if c.sigmoid:
        flat, n, k = x.reshape(-1), x.numel(), len(SIGMOID_SPECIALS)
        for j, v in enumerate(SIGMOID_SPECIALS[:n]):
            flat[j * n // k if n >= k else j] = v
    return (x,)


def inputs(c):
    return {Linear: linear_inputs, NormStyle: normstyle_inputs, Demod: demod_inputs, Add: add_inputs, ToNhwc: to_nhwc_inputs,
            ToNchw: to_nchw_inputs}[type(c)](c)


def statement(c, args, r=ref.RIGHT):
    """The statement of the case's kernel on args (the tensors of inputs(c), in the dtype to compute in)."""
    if isinstance(c, Linear):
        return ref.linear(args[0], args[1], args[2], c.lrelu, r)
    if isinstance(c, NormStyle):
        return ref.normstyle(args[0], r)
    if isinstance(c, Demod):
        return ref.demod(args[0], args[1], r)
    if isinstance(c, Add):
        return ref.add(*args)
    if isinstance(c, ToNhwc):
        return ref.to_nhwc(args[0], r)
    return ref.to_nchw(args[0], c.sigmoid)


def to64(args):
    return tuple(None if a is None else a.double() for a in args)


Reference = namedtuple("Reference", "want want32 e32 largest allowed")
_refs = {}      # by case_id: namedtuples of different kinds compare equal where their fields do


def reference(c):
    key = case_id(c)
    if key not in _refs:
        args = inputs(c)
        with torch.no_grad():
            want = statement(c, to64(args))
            want32 = statement(c, args)
        e32 = float((want32.double() - want).abs().max())
        largest = float(want.abs().max())
        _refs[key] = Reference(want, want32, e32, largest, 0.0 if is_exact(c) else allowance(e32, largest))
    return _refs[key]
