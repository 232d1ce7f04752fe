"""Case table of the DINO depth tests (tests/test_dino_depth_cpu.py, tests/test_dino_depth_ops_gpu.py): the GEMM and attention forms of
dino.hip at the depths of the ViT-B checkpoint - K = 608, 768 and 3072, K = 9216 in eight slabs, 1370 keys in 12 heads - as single
kernel launches at small M and N.  Inputs are rebuilt from the fixed seeds 0, 1, 2 and not stored; every form is stated once in torch on the
CPU and evaluated in float64 (the oracle) and in float32 (the yardstick: what a float32 evaluation loses by itself).  The allowance is
dino_cases.allowance(e32, largest): nothing here is derived from a kernel."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import dino_cases

SEEDS = (0, 1, 2)
N = 128
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH = 0, 1, 2      # enum Act of csrc/kernels.h
# fp32 tile configurations of gemm_config (csrc/gemm_f32.hip): 3 = 32 x 128 (M <= 32), 2 = 64 x 64
GEMM_MS = {26: 3, 82: 2}
# name: (K, activation, gate and residual in place, distribution of A)
GEMM_FORMS = {
    "patch": (608, ACT_NONE, False, "randn"),          # the patch embedding: 588 zero-padded to 608, 19 K-steps of 32
    "qkv": (768, ACT_NONE, False, "randn"),            # q|k|v and the four projections: a LayerNorm's output in, bias
    "fc1": (768, ACT_GELU_ERF, False, "randn"),
    "proj": (768, ACT_NONE, True, "randn"),            # x += ls1 * (proj(o) + b)
    "fc2": (3072, ACT_NONE, True, "gelu"),             # x += ls2 * (fc2(h) + b), h = gelu(fc1(.))
}
SPLITK_K, SPLITK_S, SPLITK_MS = 9216, 8, (9, 25)       # the stride-2 conv of the head: 9 x 1024 in DN_SPLITK slabs; 3 x 3 and 5 x 5 pixels
ATTN_H, ATTN_HD, ATTN_SCALE = 12, 64, 0.125
ATTN_D = ATTN_H * ATTN_HD
ATTN_LS = (130, 257, 1370)                              # 3, 5 and 22 key blocks of 64, the last partial each time; 1370 = 37 x 37 + 1
BLOCK = 256                                            # depth of one block of the blocked sum order (conv_mfma_kernel's)
# wrong reading: the forms it is a reading of
VARIANTS = {
    "gelu_tanh": ("fc1",),
    "gate_before_bias": ("proj", "fc2"),
    "no_residual": ("proj", "fc2"),
    "scale_1": ("attention",),
    "drop_key": ("attention",),
}

_cases = {}
_bars = {}


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


class Case:
    """One form at one size and seed: its name, its sizes and its float32 inputs (CPU tensors, read only)."""

    def __init__(self, form, size, seed):
        self.form, self.size, self.seed = form, size, seed
        g = torch.Generator().manual_seed(seed)
        if form == "attention":
            self.T = size
            qkv = _randn(g, size, 3 * ATTN_D)
            qkv[:, :ATTN_D] *= 2.0      # q . k over 64 randn pairs has a deviation of 8: scores of 0.125 * 2 * 8 = 2
            self.qkv = qkv
            return
        self.M = size
        if form == "splitk":
            self.K, self.act, self.gated, dist = SPLITK_K, ACT_NONE, False, "randn"
        else:
            self.K, self.act, self.gated, dist = GEMM_FORMS[form]
        a = _randn(g, size, self.K)
        self.A = F.gelu(a) if dist == "gelu" else a
        self.W = _randn(g, N, self.K) * math.sqrt(2.0 / self.K)
        self.bias = 0.1 * _randn(g, N)
        # LayerScale is an [N] vector; artalk_op_gemm takes a full [M][N] gate, so the vector is laid out as M equal rows
        self.gate = (1.0 + 0.1 * _randn(g, N)).expand(size, N).contiguous() if self.gated else None
        self.R = _randn(g, size, N) if self.gated else None

    def __repr__(self):
        return f"{self.form} {self.size} seed {self.seed}"


def case(form, size, seed):
    key = (form, size, seed)
    if key not in _cases:
        _cases[key] = Case(form, size, seed)
    return _cases[key]


def gemm_cases():
    return [(f, M, s) for f in GEMM_FORMS for M in GEMM_MS for s in SEEDS]


def epilogue(c, acc, dtype, variant=None):
    """R + gate * act(acc + bias) in dtype: what every GEMM form does with its sums."""
    bias = c.bias.to(dtype)
    if variant == "gate_before_bias":
        y = acc * c.gate.to(dtype) + bias
    else:
        y = acc + bias
        if c.act == ACT_GELU_ERF:
            y = F.gelu(y, approximate="tanh" if variant == "gelu_tanh" else "none")
        if c.gated:
            y = y * c.gate.to(dtype)
    if c.gated and variant != "no_residual":
        y = y + c.R.to(dtype)
    return y


def attention(c, dtype, variant=None):
    """softmax(q k^T * 0.125) v, written out, per head: [T][768]"""
    T = c.T
    q, k, v = (c.qkv[:, i * ATTN_D:(i + 1) * ATTN_D].to(dtype).reshape(T, ATTN_H, ATTN_HD).transpose(0, 1) for i in range(3))
    if variant == "drop_key":      # the last key: the one a short partial block loses
        k, v = k[:, :-1], v[:, :-1]
    s = q @ k.transpose(-1, -2) * (1.0 if variant == "scale_1" else ATTN_SCALE)
    s = s - s.max(dim=-1, keepdim=True).values
    p = s.exp()
    p = p / p.sum(dim=-1, keepdim=True)
    return (p @ v).transpose(0, 1).reshape(T, ATTN_D)


def reference(c, dtype, variant=None):
    """The form in torch on the CPU in dtype: float64 is the oracle, float32 the yardstick."""
    with torch.no_grad():
        if c.form == "attention":
            return attention(c, dtype, variant)
        return epilogue(c, c.A.to(dtype) @ c.W.to(dtype).t(), dtype, variant)


def bar(c):
    """(oracle, e32, allowance) of a case, computed once and read only."""
    key = (c.form, c.size, c.seed)
    if key not in _bars:
        want = reference(c, torch.float64)
        e32 = float((reference(c, torch.float32).double() - want).abs().max())
        _bars[key] = (want, e32, dino_cases.allowance(e32, float(want.abs().max())))
    return _bars[key]


# ---- the two sum orders of gemm_f32_kernel, emulated with float32 running sums (numpy, no GPU)
def _k_order(K):
    """The order in which gemm_f32_kernel adds the products of one output: per 32-deep K step, lane half h holds k in [16 h, 16 h + 16)
    and one MFMA adds k and k + 16, so the chain runs 0, 16, 1, 17, ..., 15, 31."""
    step = np.stack([np.arange(16), np.arange(16) + 16], axis=1).reshape(-1)
    return (np.arange(0, K, 32)[:, None] + step[None, :]).reshape(-1)


def emulate_sums(c, block=0):
    """A W^T with one float32 running sum per output, each product added by a fused multiply-add (the product of two float32 is exact in
    float64, so rounding float64(acc) + a * w to float32 is that operation up to a double rounding).  block = 0: one chain over K;
    block > 0: every `block` of K the chain is added into a second float32 sum and restarts from zero."""
    A, W = c.A.numpy().astype(np.float64), c.W.numpy().astype(np.float64)
    acc = np.zeros((c.M, N), dtype=np.float32)
    total = np.zeros((c.M, N), dtype=np.float32)
    for i, k in enumerate(_k_order(c.K)):
        if block and i and i % block == 0:
            total = total + acc
            acc = np.zeros_like(acc)
        acc = (acc.astype(np.float64) + A[:, k, None] * W[None, :, k]).astype(np.float32)
    return torch.from_numpy(total + acc if block else acc)
