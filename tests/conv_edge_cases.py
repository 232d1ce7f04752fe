"""The edge cases of the implicit-GEMM convolution (conv_mfma_kernel<NT, VA, VB> of styleunet.hip, conv_bf16_kernel<NT, NP, VA> of
styleunet_bf16.hip) that tests/test_conv_edges_cpu.py and tests/test_conv_edges_gpu.py share: one table, the launcher's documented
choice restated in Python (``expected_plan``), the K walk of each kernel (``k_steps``, ``step_of``), where every operand sits relative to
a 16-byte boundary (``layout``) and the float64 reference with its allowance (``reference``).  Images are tiny: each shape is the
smallest at which its edge exists.  Every case runs in all three precisions.  Not a product path."""
import functools
import math
from collections import namedtuple

import styleunet_ref as ref
from styleunet_prec_ref import SWITCHES, allowance, conv2d_mode, inputs

MODES = ("f32", "bf16x3", "bf16")      # precision 0, 1, 2 of artalk_op_conv2d_ex
BM = 128                               # pixels of a workgroup tile, both kernels
BK = {"f32": 16, "bf16x3": 32, "bf16": 32}      # K depth of one step (CV_BK, CB_BK): asserted through the plan, never assumed
BLOCK = {"f32": 16, "bf16x3": 8, "bf16": 8}     # steps whose sums close into one block of the three-level sum

# family: which edge the case is there for.  shape: (Cin, Cout, k, B, H, W).  variant: where the operands sit -
#   aligned      every pointer 16-byte aligned, x_bstride = H W Cin
#   x+1          x one float past a 16-byte boundary       w+1   w likewise       in_scale+1   in_scale likewise
#   stride+N     x_bstride = H W Cin + N (the N floats between samples are never the kernel's to read)
# on: the switches of styleunet_prec_ref.inputs that are on.
Case = namedtuple("Case", "family shape variant on seed")
VARIANTS = ("aligned", "x+1", "w+1", "in_scale+1", "stride+8", "stride+5", "stride+1")
ALL_PER_SAMPLE = tuple(s for s in SWITCHES if s != "noise_shared")      # every switch, with per-sample noise


def _table():
    t = []
    for cin in (8, 9):
        for cout in (1, 31, 32, 33, 36, 63, 64, 65, 68, 96, 100):
            t.append(Case("cout", (cin, cout, 3, 1, 5, 7), "aligned", (), 10))
    for cout in (16, 40):
        for cin in (1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 40):
            t.append(Case("cin", (cin, cout, 3, 1, 5, 7), "aligned", (), 11))
        for cin in (8, 24, 33):
            t.append(Case("cin", (cin, cout, 1, 1, 5, 7), "aligned", (), 12))
    # fp32: 15 / 16 / 17 steps of 16 (k = 1, Cin 240 / 256 / 272); bf16: 7 / 8 / 9 steps of 32 (Cin 224 / 256 / 288);
    # k = 3, Cin 144: 9 x 9 = 81 = 16 x 5 + 1 steps in fp32 and 1312 / 32 = 41 = 8 x 5 + 1 in the bf16 modes
    for cin in (224, 240, 256, 272, 288):
        t.append(Case("sum", (cin, 8, 1, 1, 3, 3), "aligned", (), 13))
    t.append(Case("sum", (144, 8, 3, 1, 3, 3), "aligned", (), 13))
    for shape in ((8, 16, 3, 1, 1, 127), (8, 16, 3, 1, 1, 128), (8, 16, 3, 1, 1, 129), (8, 16, 3, 1, 129, 1)):
        t.append(Case("pixel", shape, "aligned", (), 14))
    t.append(Case("pixel", (16, 40, 3, 3, 7, 9), "aligned", ALL_PER_SAMPLE, 14))      # H W = 63: a tile holds parts of three samples
    for cout in (16, 40):
        for v in ("stride+8", "stride+5"):
            t.append(Case("stride", (8, cout, 3, 3, 5, 7), v, ("in_scale",), 15))
    for cout in (16, 40):      # NT = 1 and 2; the aligned twin first
        for v in ("aligned", "x+1", "w+1", "in_scale+1", "stride+1"):
            t.append(Case("align", (8, cout, 3, 3, 5, 7), v, ("in_scale",), 15))
    return t


CASES = _table()
# expected K steps of the sum family per mode (asserted against the plan): the counts on each side of a block boundary
SUM_STEPS = {"f32": {240: 15, 256: 16, 272: 17, 144: 81}, "bf16x3": {224: 7, 256: 8, 288: 9, 144: 41}, "bf16": {224: 7, 256: 8, 288: 9, 144: 41}}


def case_id(c):
    return f"{c.family}-{'x'.join(map(str, c.shape))}-{c.variant}"


def twin(c):
    """The aligned case with the same shape, switches and values."""
    return c._replace(variant="aligned")


def layout(c):
    """Offsets, in floats past a 16-byte boundary, of x, w and in_scale, and x_bstride."""
    Cin, _, _, _, H, W = c.shape
    tight = H * W * Cin
    lay = dict(x=0, w=0, in_scale=0, x_bstride=tight)
    if c.variant.startswith("stride+"):
        lay["x_bstride"] = tight + int(c.variant[len("stride+"):])
    elif c.variant != "aligned":
        lay[c.variant[:-2]] = 1
    return lay


def plan_args(c, precision, base=1 << 26):
    """The arguments of capi.conv2d_plan for the case with every buffer at ``base`` (16-byte aligned) plus its offset of ``layout``."""
    Cin, Cout, k, B, H, W = c.shape
    lay = layout(c)
    ins = base + 4 * lay["in_scale"] if "in_scale" in c.on else 0
    return (base + 4 * lay["x"], lay["x_bstride"], base + 4 * lay["w"], ins, B, H, W, Cin, Cout, k, precision)


def k_steps(mode, Cin, k):
    """(steps, Cinp, Kp) of the kernel's K loop: fp32 walks each tap in ceil(Cin / 16) chunks; the bf16 modes walk K = tap * Cinp + ci,
    zero-padded to Kp, in steps of 32."""
    if mode == "f32":
        return k * k * ((Cin + BK[mode] - 1) // BK[mode]), 0, 0
    Cinp = (Cin + 7) // 8 * 8
    Kp = (k * k * Cinp + 31) // 32 * 32
    return Kp // BK[mode], Cinp, Kp


def step_of(mode, Cin, k, tap, ci):
    """The step of the kernel's K loop in which input channel ci of tap ``tap`` is summed."""
    if mode == "f32":
        return tap * ((Cin + BK[mode] - 1) // BK[mode]) + ci // BK[mode]
    return (tap * k_steps(mode, Cin, k)[1] + ci) // BK[mode]


def expected_plan(c, mode):
    """What launch_conv / launch_conv_bf16 document: NT by Cout alone; VA needs Cin % 8 == 0, x and in_scale 16-byte aligned and
    x_bstride % 4 == 0; VB (fp32 only) needs Cout % 4 == 0 and w 16-byte aligned."""
    Cin, Cout, k, B, H, W = c.shape
    lay = layout(c)
    nt = 1 if Cout <= 32 else 2
    va = Cin % 8 == 0 and lay["x"] == 0 and lay["x_bstride"] % 4 == 0 and ("in_scale" not in c.on or (lay["in_scale"] == 0 and Cin % 4 == 0))
    steps, Cinp, Kp = k_steps(mode, Cin, k)
    return dict(NT=nt, VA=int(va), VB=int(Cout % 4 == 0 and lay["w"] == 0) if mode == "f32" else -1, NP={"f32": 0, "bf16x3": 3, "bf16": 1}[mode],
                grid_x=(B * H * W + BM - 1) // BM, grid_y=(Cout + 32 * nt - 1) // (32 * nt), steps=steps, Cinp=Cinp, Kp=Kp)


@functools.lru_cache(maxsize=None)
def case_inputs(shape, on, seed):
    """float32-exact values held in float64 (styleunet_prec_ref.inputs); shared, read only."""
    return inputs(shape, set(on), seed=seed)


def statement(mode, a):
    """The float64 (or, for float32 inputs, the float32) statement of one launch in mode ``mode``: the existing references, unchanged -
    tests/styleunet_ref.py for the exact fp32 kernel, tests/styleunet_prec_ref.py for the bf16 modes."""
    return ref.conv2d(**a) if mode == "f32" else conv2d_mode(mode, **a)


@functools.lru_cache(maxsize=None)
def _reference(shape, on, seed, mode):
    import torch
    a = case_inputs(shape, on, seed)
    with torch.no_grad():
        want = statement(mode, a)
        a32 = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}
        allowed, e32 = allowance(want, statement(mode, a32))
    return want, allowed, e32


def reference(c, mode):
    """(want float64, allowed, e32): the project's rule, max(4 x e32, one float32 ulp of the largest output), e32 being the
    float32-vs-float64 distance of the same statement on the CPU.  Independent of the variant: where the operands sit changes no value."""
    return _reference(c.shape, c.on, c.seed, mode)


assert len({case_id(c) for c in CASES}) == len(CASES) and all(c.variant in VARIANTS for c in CASES)
assert all(math.prod(c.shape[3:]) * max(c.shape[0], c.shape[1]) <= 1 << 16 for c in CASES), "keep the images tiny"
