"""Plain statements of the StyleUNet's style path and layout kernels (artalk_op_su_* of include/artalk_hip.h), after the comments of
artalk_amd/csrc/styleunet.hip and the style path of tests/styleunet_ref.py, in whatever dtype the inputs have: float64 for the
reference, float32 for the e32 yardstick.  Sums are torch's own (matmul, sum): nothing here follows the kernels' lane-strided order.
``Reading`` holds one switch per way of getting a kernel subtly wrong, so that tests/test_styleunet_glue_cpu.py can show that the case
table tells each of them from the right reading.  Not a product path: only the tests import it."""
from dataclasses import dataclass

import torch

EPS = 1e-8


@dataclass(frozen=True)
class Reading:
    eps_outside_root: bool = False      # True: 1 / (sqrt(v) + eps) where rsqrt(v + eps) belongs (normstyle, demod)
    eps_on_sum: bool = False            # True: eps joins the sum of squares, before the division by n (normstyle)
    style_squared: bool = True          # False: sum of s wsq (demod)
    wsq_transposed: bool = False        # True: wsq's memory read as [Cin][Cout] (demod)
    w_transposed: bool = False          # True: W's memory read as [In][Out] (linear)
    slope: float = 0.2                  # LeakyReLU slope (linear)
    lrelu_before_bias: bool = False     # True: act(x W^T) + bias (linear)
    drop_last: bool = False             # True: the last input element never reaches the sum (linear, normstyle, demod)
    nhwc_swapped: bool = False          # True: to_nhwc with C and HW taken for each other


RIGHT = Reading()


def linear(x, W, bias, lrelu, r=RIGHT):
    """x (B, In), W (Out, In), bias (Out) or None -> (B, Out): x W^T + bias, then LeakyReLU 0.2 if lrelu."""
    In, Out = x.shape[1], W.shape[0]
    if r.w_transposed:
        W = W.reshape(In, Out).t()
    if r.drop_last:
        x, W = x[:, :-1], W[:, :-1]
    act = lambda t: torch.where(t >= 0, t, t * r.slope)
    y = x @ W.t()
    if lrelu and r.lrelu_before_bias:
        y = act(y)
    if bias is not None:
        y = y + bias
    if lrelu and not r.lrelu_before_bias:
        y = act(y)
    return y


def normstyle(x, r=RIGHT):
    """x (B, n) -> x rsqrt(mean(x^2) + 1e-8), row by row."""
    n = x.shape[1]
    sq = x[:, :-1] if r.drop_last else x
    ss = (sq * sq).sum(dim=1, keepdim=True)
    if r.eps_outside_root:
        return x / (torch.sqrt(ss / n) + EPS)
    if r.eps_on_sum:
        return x * torch.rsqrt((ss + EPS) / n)
    return x * torch.rsqrt(ss / n + EPS)


def demod(s, wsq, r=RIGHT):
    """s (B, Cin), wsq (Cout, Cin) -> (B, Cout): rsqrt(sum_ci s^2 wsq + 1e-8)."""
    Cout, Cin = wsq.shape
    if r.wsq_transposed:
        wsq = wsq.reshape(Cin, Cout).t()
    if r.drop_last:
        s, wsq = s[:, :-1], wsq[:, :-1]
    acc = (s * s if r.style_squared else s) @ wsq.t()
    if r.eps_outside_root:
        return 1.0 / (torch.sqrt(acc) + EPS)
    return torch.rsqrt(acc + EPS)


def add(a, b):
    return a + b


def to_nhwc(x, r=RIGHT):
    """x (B, C, HW) -> (B, HW, C)."""
    B, C, HW = x.shape
    if r.nhwc_swapped:      # the memory taken as [B][HW][C] and "transposed" to [B][C][HW], then read back as [B][HW][C]
        return x.reshape(B, HW, C).transpose(1, 2).contiguous().reshape(B, HW, C)
    return x.transpose(1, 2).contiguous()


def to_nchw(x, sigmoid):
    """x (B, HW, C) -> (B, C, HW), through the logistic function if sigmoid."""
    y = x.transpose(1, 2).contiguous()
    return torch.sigmoid(y) if sigmoid else y
