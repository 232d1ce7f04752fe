"""The bf16 GEMM kernels (precision mode 2, gemm_bf16.hip) through artalk_op_gemm_bf16, against float64 math of the bf16-ROUNDED
operands: bf16 products, fp32 sums.  Bar: the fp32 accumulation bound of test_ops_gpu.py, 2e-5 * sum|a*w| per element (times |gate|),
which holds the kernel to exactly "round each operand to bf16 once, multiply, add in fp32".  Every tile of the register-staged
gemm_bf16_kernel (force_cfg 0: 64x64, 1: 128x128, 2: 32x128 - the M <= 32 steps of the AR body) runs every form the model uses: conv
window (lda < K), grouped positional-conv window (amode 1), grid.z batching, split-K finished by the shared reduce pass, bias / 4
activations / gate / residual.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KERNELS = [0, 1, 2]      # force_cfg: tiles 64x64, 128x128, 32x128


def _lib():
    from artalk_amd import capi
    return capi, capi.lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _b(t):
    """what the kernel multiplies: the operand rounded to bf16 (nearest even), in float64"""
    return t.to(torch.bfloat16).double()


def _epilogue(acc, bias, act, gate, R):
    ref = acc + (bias.double() if bias is not None else 0.0)
    ref = ref.float()
    if act == 1:
        ref = F.gelu(ref)
    elif act == 2:
        ref = F.gelu(ref, approximate="tanh")
    elif act == 3:
        ref = F.leaky_relu(ref, 0.2)
    if gate is not None:
        ref = ref * gate
    if R is not None:
        ref = ref + R
    return ref.double()


def _check(out, ref, mag, gate):
    bound = 2e-5 * mag * (gate.double().abs() if gate is not None else 1.0) + 1e-6 * (1.0 + ref.abs())
    err = (out.cpu().double() - ref).abs()
    assert torch.isfinite(out).all()
    worst = (err / bound).max().item()
    assert worst <= 1.0, f"error {err.max().item():.3e} exceeds the fp32-accumulation bound ({worst:.2f}x)"
    return err.max().item()


@pytest.mark.parametrize("cfg", KERNELS)
@pytest.mark.parametrize("M,N,K,act,use_bias,use_gate,use_res", [
    (1000, 512, 1536, 0, True, False, False),
    (2000, 1024, 1024, 1, True, False, True),
    (333, 768, 3072, 2, True, True, True),        # ragged M, gelu(tanh), gate, residual
    (32, 2304, 768, 0, True, False, False),
    (5, 64, 768, 0, True, False, False),
    (200, 106, 512, 0, True, False, False),       # N = 106
    (6400, 512, 32, 3, True, False, False),       # K = 32, leaky relu
    (40000, 64, 1024, 0, False, False, False),
])
def test_gemm_bf16(cfg, M, N, K, act, use_bias, use_gate, use_res):
    capi, L = _lib()
    g = torch.Generator().manual_seed(M * 7 + N)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g) if use_bias else None
    gate = torch.randn(M, N, generator=g) if use_gate else None
    R = torch.randn(M, N, generator=g) if use_res else None
    ref = _epilogue(_b(A) @ _b(W).t(), bias, act, gate, R)
    mag = _b(A).abs() @ _b(W).abs().t()
    dA, dW = A.cuda(), W.cuda()
    db, dg, dR = (x.cuda() if x is not None else None for x in (bias, gate, R))
    out = torch.full((M, N), float("nan"), device="cuda")
    assert L.artalk_op_gemm_bf16(_p(dA), K, _p(dW), _p(db), _p(dg), _p(dR), _p(out), M, N, K, act, cfg, None) == 0
    torch.cuda.synchronize()
    _check(out, ref, mag, gate)


@pytest.mark.parametrize("cfg", KERNELS + [-1])
def test_gemm_bf16_residual_in_place(cfg):
    """R aliasing C (the encoder's out-projection / FFN-out): C = C + A W^T + b."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(3)
    M, N, K = 777, 768, 768
    A, W, bias, R = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / 30, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ref = _epilogue(_b(A) @ _b(W).t(), bias, 0, None, R)
    mag = _b(A).abs() @ _b(W).abs().t()
    out = R.cuda()
    assert L.artalk_op_gemm_bf16(_p(A.cuda()), K, _p(W.cuda()), _p(bias.cuda()), None, _p(out), _p(out), M, N, K, 0, cfg, None) == 0
    _check(out, ref, mag, None)


@pytest.mark.parametrize("cfg", KERNELS)
def test_gemm_bf16_conv_window(cfg):
    """Stride-2 convolution as a GEMM (conv1-6 of the wav2vec2 stack): row m reads the K = 3*512 floats at m * lda, lda = 2*512 < K."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(5)
    M, N, K, lda = 399, 512, 1536, 1024
    buf = torch.randn((M - 1) * lda + K, generator=g)
    A = torch.as_strided(buf, (M, K), (lda, 1))
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    ref = _epilogue(_b(A) @ _b(W).t(), bias, 0, None, None)
    mag = _b(A).abs() @ _b(W).abs().t()
    out = torch.full((M, N), float("nan"), device="cuda")
    assert L.artalk_op_gemm_bf16(_p(buf.cuda()), lda, _p(W.cuda()), _p(bias.cuda()), None, None, _p(out), M, N, K, 0, cfg, None) == 0
    _check(out, ref, mag, None)


@pytest.mark.parametrize("cfg", KERNELS)
def test_gemm_bf16_posconv_window(cfg):
    """amode 1 (grouped positional convolution): group z, row m = (clip c, frame t), k = (tap, ci):
    A_z[m, k] = X[c*T + t + tap - pad, 64 z + ci] inside the clip, else 0; batched over the groups (grid.z), gelu + residual."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(9)
    T, nclip, groups, taps = 40, 3, 4, 16
    M, N, K, lda = nclip * T, 64, taps * 64, groups * 64
    pad = taps // 2
    X = torch.randn(M, lda, generator=g)
    W = torch.randn(groups, N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(groups, N, generator=g)
    R = torch.randn(groups, M, N, generator=g)
    Xb = _b(X)
    refs, mags = [], []
    for z in range(groups):
        Az = torch.zeros(M, K, dtype=torch.float64)
        for c in range(nclip):
            for t in range(T):
                for tap in range(taps):
                    ts = t + tap - pad
                    if 0 <= ts < T:
                        Az[c * T + t, tap * 64:(tap + 1) * 64] = Xb[c * T + ts, z * 64:(z + 1) * 64]
        refs.append(_epilogue(Az @ _b(W[z]).t(), bias[z], 1, None, R[z]))
        mags.append(Az.abs() @ _b(W[z]).abs().t())
    out = torch.full((groups, M, N), float("nan"), device="cuda")
    fc = cfg | (groups << 16) | (1 << 24) | (T << 25)
    assert L.artalk_op_gemm_bf16(_p(X.cuda()), lda, _p(W.cuda()), _p(bias.cuda()), None, _p(R.cuda()), _p(out), M, N, K, 1, fc, None) == 0
    _check(out, torch.stack(refs), torch.stack(mags), None)


@pytest.mark.parametrize("cfg", KERNELS)
def test_gemm_bf16_batched(cfg):
    capi, L = _lib()
    g = torch.Generator().manual_seed(13)
    nb, M, N, K = 3, 300, 192, 256
    A = torch.randn(nb, M, K, generator=g)
    W = torch.randn(nb, N, K, generator=g) / 16
    bias = torch.randn(nb, N, generator=g)
    ref = torch.stack([_epilogue(_b(A[z]) @ _b(W[z]).t(), bias[z], 2, None, None) for z in range(nb)])
    mag = torch.stack([_b(A[z]).abs() @ _b(W[z]).abs().t() for z in range(nb)])
    out = torch.full((nb, M, N), float("nan"), device="cuda")
    assert L.artalk_op_gemm_bf16(_p(A.cuda()), K, _p(W.cuda()), _p(bias.cuda()), None, None, _p(out), M, N, K, 2, cfg | (nb << 16), None) == 0
    _check(out, ref, mag, None)


@pytest.mark.parametrize("cfg", KERNELS)
@pytest.mark.parametrize("S", [3, 8])
def test_gemm_bf16_split_k(cfg, S):
    """Split-K partial slabs (the AR body's small-M steps) finished by the existing splitk_reduce pass: bias, gate, residual there."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(17 + S)
    M, N, K = 80, 768, 3072
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    bias, gate, R = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    ref = _epilogue(_b(A) @ _b(W).t(), bias, 0, gate, R)
    mag = _b(A).abs() @ _b(W).abs().t()
    out = torch.full((M, N), float("nan"), device="cuda")
    assert L.artalk_op_gemm_bf16(_p(A.cuda()), K, _p(W.cuda()), _p(bias.cuda()), _p(gate.cuda()), _p(R.cuda()), _p(out), M, N, K, 0,
                                 cfg | (S << 8), None) == 0
    _check(out, ref, mag, gate)


def test_gemm_bf16_is_bf16_deterministic_and_keeps_nan():
    """On random data the result is NOT the fp32 GEMM's (the products really are bf16); two identical calls are bit-identical; a NaN
    in A reaches its row of C as NaN (the conversion keeps NaN) and nothing else."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(21)
    M, N, K = 1000, 512, 1024
    A, W = torch.randn(M, K, generator=g).cuda(), (torch.randn(N, K, generator=g) / 32).cuda()
    for cfg in KERNELS + [-1]:
        o1, o2, o32 = (torch.empty(M, N, device="cuda") for _ in range(3))
        assert L.artalk_op_gemm_bf16(_p(A), K, _p(W), None, None, None, _p(o1), M, N, K, 0, cfg, None) == 0
        assert L.artalk_op_gemm_bf16(_p(A), K, _p(W), None, None, None, _p(o2), M, N, K, 0, cfg, None) == 0
        assert L.artalk_op_gemm(_p(A), K, _p(W), None, None, None, _p(o32), M, N, K, 0, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(o1, o2)
        d = (o1 - o32).abs().max().item()
        assert d > 1e-3 * o32.abs().max().item(), f"cfg {cfg}: bf16 result equals the fp32 GEMM to {d:.2e}: not bf16 products"
        An = A.clone()
        An[3, 5] = float("nan")
        on = torch.zeros(M, N, device="cuda")
        assert L.artalk_op_gemm_bf16(_p(An), K, _p(W), None, None, None, _p(on), M, N, K, 0, cfg, None) == 0
        torch.cuda.synchronize()
        assert torch.isnan(on[3]).all(), f"cfg {cfg}: a NaN operand did not reach its output row"
        rest = torch.cat([on[:3], on[4:]])
        assert torch.isfinite(rest).all() and torch.equal(rest, torch.cat([o1[:3], o1[4:]]))
