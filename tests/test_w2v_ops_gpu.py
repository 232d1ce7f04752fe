"""The kernels of the wav2vec2 stage in the chunk-strided forms run_wav2vec launches them, one launch per assertion group, against float64
on the CPU.  What each form stands for in the stage:

  a, b  launch_audio_normalize / launch_conv0 with a table of clip offsets and a row stride of T + 1    artalk_op_w2v_front_rows
  c     conv1-6 as GEMMs whose A rows overlap (lda = 2 * 512 < K) over chunks of S rows, T valid        artalk_op_gemm_rows
  d     the LayerNorm + GELU that follows each of them, in place, padding rows stored as zeros            artalk_op_layernorm_rows
  e     the grouped positional convolution over chunks of Ts = T + 1 rows                                artalk_op_posconv_rows
  f     the encoder attention out of the interleaved q|k|v buffer, 199 rows in 200-row clip strides       artalk_op_attention_rows
  g     pooling + SiLU reading with the 200-row stride                                                    artalk_op_pool_silu_rows

Every result buffer is a Guarded: int32 words pre-filled with 0x7fc00000 (an fp32 NaN, two fp16 NaNs) with 64 KiB of the same fill before
and after it; every test asserts that what the launch must not write - the guards, rows beyond M, the padding rows of a chunk where the
kernel leaves them alone - still holds the fill.  Padding rows of the INPUTS hold NaN (inf for the LayerNorm, whose contract is to
overwrite them): no valid row may read them.

Bars.  Each is either the bar the suite already holds for the same kernel in dense form (cited where it is used), or a rounding bound
derived in the test's docstring from the kernel's arithmetic (a: normalisation, g: pooling + SiLU)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import p8_format as p8

pytestmark = pytest.mark.gpu

CANARY = 0x7fc00000        # fp32 NaN; as P8 words, NaN halves
NAN16 = 0x7e007e00         # two fp16 NaNs: a P8 input row no valid row may read
GUARD = 16384              # guard words (64 KiB) on either side of a result
IDENT = (2 ** 31 - 1, 0, 0)
U = 2.0 ** -24             # unit roundoff of fp32 (round to nearest)
EPS = 2.0 ** -23


def _lib():
    from artalk_amd import capi
    return capi, capi.lib()


def _p(t):
    return None if t is None else t.data_ptr()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Guarded:
    """`words` int32 words of device memory filled with CANARY, between two guards of the same fill."""

    def __init__(self, words):
        self.n = int(words)
        self.raw = torch.full((GUARD + self.n + GUARD,), CANARY, dtype=torch.int32, device="cuda")
        self.t = self.raw[GUARD:GUARD + self.n]

    def ptr(self):
        return self.t.data_ptr()

    def f32(self, *shape):
        return self.t.view(torch.float32).view(*shape)

    def i32(self, *shape):
        return self.t.view(*shape)

    def check(self, what=""):
        torch.cuda.synchronize()
        assert bool((self.raw[:GUARD] == CANARY).all()), f"{what}: wrote before the buffer"
        assert bool((self.raw[GUARD + self.n:] == CANARY).all()), f"{what}: wrote past the buffer"


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _st(s):
    torch.cuda.synchronize()
    return int(s.item())


def _pack(L, x_dev, e):
    out = torch.empty(x_dev.shape, dtype=torch.int32, device="cuda")
    assert L.artalk_op_pack_split_ex(_p(x_dev), _p(out), x_dev.numel(), 0, e, None, None) == 0
    torch.cuda.synchronize()
    return out


def _unpack(t, e):
    return torch.from_numpy(p8.unpack(t.cpu().numpy(), e))


def _assert_stored(got64, ref64, e, arith, what):
    """test_p8_exps_ops_gpu.py::_assert_stored: a P8 result unpacked with its exponent against float64, the format bound plus the
    arithmetic bar of the op (a number, or a bound per element)"""
    assert bool(torch.isfinite(got64).all()), f"{what}: element(s) not written / not finite"
    err = (got64 - ref64).abs()
    tol = torch.from_numpy(p8.bound(ref64.numpy(), e)) + arith
    bad = err > tol
    assert not bool(bad.any()), (what, e, int(bad.sum()), float(err.max()), float((err - tol).max()), float(ref64.abs().max()))


def _assert_within(got, ref64, bound64, what):
    got64 = got.double()
    assert bool(torch.isfinite(got64).all()), f"{what}: {int((~torch.isfinite(got64)).sum())} element(s) not written / not finite"
    err = (got64 - ref64).abs()
    bad = err > bound64
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err / bound64.clamp_min(1e-300)).max()))


def _bf(t):
    return t.to(torch.bfloat16).double()


# ================================================================================================ a / b. normalise, conv0 + LN + GELU
FR_N, FR_LEN = 2583, 7000                       # samples per chunk (T = 515), samples in the clip buffer
FR_OFF = (7, 1300, 0, FR_LEN - FR_N)            # overlapping, unordered, the last chunk ends on the buffer end
_FRONT = {}


def _front_weights():
    g = _gen(3)
    w = torch.randn(512, 1, 10, generator=g) / math.sqrt(10)
    b = torch.randn(512, generator=g) * 0.3
    lw = 1 + 0.1 * torch.randn(512, generator=g)
    lb = 0.1 * torch.randn(512, generator=g)
    return w, b, lw, lb


def _front_ref(audio, offs, n, wts):
    """float64: chunks gathered at their offsets -> (x - mean) / (unbiased std + 1e-6) -> conv1d(k = 10, stride 5) -> LN(512) -> GELU"""
    w, b, lw, lb = wts
    x = torch.stack([audio[o:o + n] for o in offs]).double()
    assert bool(torch.isfinite(x).all())
    mean, sd = x.mean(-1, keepdim=True), x.std(-1, keepdim=True)
    xn = (x - mean) / (sd + 1e-6)
    h = F.conv1d(xn[:, None], w.double(), b.double(), stride=5).transpose(1, 2)
    return x, mean, sd, xn, F.gelu(F.layer_norm(h, (512,), lw.double(), lb.double(), 1e-5))


def _front_case():
    """4 chunks of 2583 samples (not a multiple of 1024 or 5; T = 515, one more than one pass of conv0's 128 x 4 frame grid) out of one
    7000-sample buffer that holds NaN wherever no chunk reads.  Samples 0 .. 2582 are zero: chunk 2 is all zero (std = 0, division by
    1e-6), chunk 0 is zero but for its last 7 samples; samples 2583 .. 3882 carry a DC offset of 3, which chunk 1 takes on."""
    if not _FRONT:
        g = _gen(31)
        audio = torch.full((FR_LEN,), float("nan"))
        audio[:FR_N] = 0.0
        audio[FR_N:3883] = torch.randn(3883 - FR_N, generator=g) * 0.1 + 3.0
        audio[FR_LEN - FR_N:] = torch.randn(FR_N, generator=g) * 0.1
        read = torch.zeros(FR_LEN, dtype=torch.bool)
        for o in FR_OFF:
            read[o:o + FR_N] = True
        assert bool((torch.isnan(audio) == ~read).all()) and int((~read).sum()) == FR_LEN - FR_N - 3883
        wts = _front_weights()
        _FRONT["case"] = (audio, wts) + _front_ref(audio, FR_OFF, FR_N, wts)
    return _FRONT["case"]


def _run_front(L, audio, offs, n, wts, row_stride, p8_exp=None):
    """one launch of artalk_op_w2v_front_rows; returns xnorm [C][n] and Y as Guarded buffers with exactly sufficient sizes"""
    Cn, T = len(offs), (n - 10) // 5 + 1
    w, b, lw, lb = wts
    dev = [t.contiguous().cuda() for t in (audio, w.view(512, 10), b, lw, lb)]
    xn = Guarded(Cn * n)
    y_elems = ((Cn - 1) * row_stride + T) * 512
    Y = Guarded(y_elems)
    st = _status()
    off = (C.c_int64 * Cn)(*offs)
    rc = L.artalk_op_w2v_front_rows(_p(dev[0]), audio.numel(), off, Cn, n, _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]), xn.ptr(), Y.ptr(),
                                    row_stride, y_elems, 0 if p8_exp is None else 1, 4 if p8_exp is None else p8_exp, _p(st), None)
    assert rc == 0, rc
    assert _st(st) == 0
    xn.check("xnorm")
    Y.check("conv0")
    return xn, Y


def test_normalize_reads_chunks_at_their_offsets():
    """audio_normalize_kernel through the offset table.  The kernel computes mean and sum of squares in double, so its roundings are: the
    mean rounded once to fp32 (m = mean (1 + d0)); the std rounded once - of the deviations from m, not from the mean, which multiplies it
    by sqrt(1 + n (m - mean)^2 / sum (x - mean)^2) <= 1 + (EPS mean / std)^2 / 2; the fp32 sum std + 1e-6f (one rounding more than the
    issue lists: the constant is added in fp32); one subtraction x - m; one division.  With every rounding <= EPS = 2^-23 relative:
        |y - ref| <= |ref| (4 EPS + (EPS mean / std)^2 / 2) + EPS |mean| / (std + 1e-6),
    the last term being the error of m itself, which the subtraction does not scale down.  A chunk of zeros gives 0 / 1e-6 = 0 exactly."""
    capi, L = _lib()
    audio, wts, x, mean, sd, xn_ref, _ = _front_case()
    xn, _ = _run_front(L, audio, FR_OFF, FR_N, wts, 515)
    got = xn.f32(4, FR_N).cpu()
    ratio = torch.where(sd > 0, mean.abs() / sd.clamp_min(1e-300), torch.zeros_like(sd))
    bound = xn_ref.abs() * (4 * EPS + 0.5 * (EPS * ratio) ** 2) * (1 + 2.0 ** -10) + EPS * mean.abs() / (sd + 1e-6) * (1 + 2.0 ** -10)
    assert float(mean[1].abs()) > 1.0 and float(sd[2]) == 0.0 and float(bound[2].max()) == 0.0
    print(f"normalize: max err {float((got.double() - xn_ref).abs().max()):.3e}, max bound {float(bound.max()):.3e}")
    _assert_within(got, xn_ref, bound, "xnorm")
    assert bool((got[2] == 0).all())


@pytest.mark.parametrize("p8_exp", [None, 4, 0])
@pytest.mark.parametrize("extra", [0, 1, 5])
def test_conv0_row_stride(extra, p8_exp):
    """conv0 + LN + GELU with row_stride = T + extra: frame t < T of chunk c at row c * row_stride + t, rows t >= T keep the fill.
    fp32: the bar of test_ops_gpu.py::test_w2v_front, 5e-5 absolute on O(1) outputs; P8: the format bound plus that bar as
    test_p8_exps_ops_gpu.py::test_w2v_front_p8_output scales it, 5e-5 * max|ref| / 4."""
    capi, L = _lib()
    audio, wts, *_, ref = _front_case()
    T = 515
    rs = T + extra
    _, Y = _run_front(L, audio, FR_OFF, FR_N, wts, rs, p8_exp)
    rows = (torch.arange(4)[:, None] * rs + torch.arange(T)[None, :]).reshape(-1)
    written = torch.zeros(3 * rs + T, dtype=torch.bool)
    written[rows] = True
    words = Y.i32(3 * rs + T, 512).cpu()
    assert bool((words[~written] == CANARY).all()), "a row t >= T of a chunk was written"
    if p8_exp is None:
        got = words[written].view(torch.float32).view(4, T, 512)
        assert bool(torch.isfinite(got).all())
        err = float((got.double() - ref).abs().max())
        print(f"conv0 fp32 row_stride {rs}: max err {err:.3e}")
        assert err < 5e-5, err
    else:
        _assert_stored(_unpack(words[written], p8_exp).view(4, T, 512), ref, p8_exp, 5e-5 * float(ref.abs().max()) / 4.0, f"conv0 P8 stride {rs}")


@pytest.mark.parametrize("p8_exp", [None, 4])
def test_conv0_fewer_frames_than_waves(p8_exp):
    """n = 15: T = 2 frames per chunk, fewer than the 4 waves of one workgroup; 2 chunks at offsets 3 and 0 of 20 samples, row_stride 3"""
    capi, L = _lib()
    audio = torch.randn(20, generator=_gen(32)) * 0.1 + 0.05
    audio[18:] = float("nan")
    wts = _front_weights()
    offs, n, T, rs = (3, 0), 15, 2, 3
    x, mean, sd, xn_ref, ref = _front_ref(audio, offs, n, wts)
    xn, Y = _run_front(L, audio, offs, n, wts, rs, p8_exp)
    assert float((xn.f32(2, n).cpu().double() - xn_ref).abs().max()) < 1e-5      # (the bar of test_w2v_front; the bound is test a's business)
    words = Y.i32(rs + T, 512).cpu()
    assert bool((words[2] == CANARY).all())
    got = words[[0, 1, 3, 4]]
    if p8_exp is None:
        err = float((got.view(torch.float32).view(2, T, 512).double() - ref).abs().max())
        assert err < 5e-5, err
    else:
        _assert_stored(_unpack(got, p8_exp).view(2, T, 512), ref, p8_exp, 5e-5 * float(ref.abs().max()) / 4.0, "conv0 P8 T = 2")


# ================================================================================================ c. conv layers as window GEMMs
CD = 512
CONV_LAYERS = {6: dict(k=2, S_out=200, T_out=199, T_in=399, n=3), 4: dict(k=3, S_out=800, T_out=799, T_in=1599, n=5)}
_CONV = {}


class _ConvCase:
    """A conv layer of the stack as the model lays it out: input [n * S_in + 16][512], T_in valid rows per chunk, every other row NaN;
    output row r = c * S_out + t reads the K = k * 512 floats at r * 1024.  float64 results for fp32 and for bf16-rounded operands, on the
    valid output rows."""

    def __init__(self, L, layer):
        d = CONV_LAYERS[layer]
        self.k, self.S_out, self.T_out, self.T_in, self.n = d["k"], d["S_out"], d["T_out"], d["T_in"], d["n"]
        self.S_in, self.K, self.N, self.lda = 2 * self.S_out, self.k * CD, CD, 2 * CD
        self.M = self.n * self.S_out
        assert self.T_out == (self.T_in - self.k) // 2 + 1
        g = _gen(600 + layer)
        rows = self.n * self.S_in + 16
        X = torch.randn(rows, CD, generator=g)
        pad = torch.ones(rows, dtype=torch.bool)
        pad[:self.n * self.S_in].view(self.n, self.S_in)[:, :self.T_in] = False
        self.pad = pad
        self.W = torch.randn(self.N, self.K, generator=g) / math.sqrt(self.K)
        self.bias = torch.randn(self.N, generator=g)
        m = torch.arange(self.M)
        self.valid = (m % self.S_out) < self.T_out
        Xz = X.clone()
        Xz[pad] = 0.0
        win = torch.as_strided(Xz.reshape(-1), (self.M, self.K), (self.lda, 1))
        A = win[self.valid]
        # no valid row reads a padding row: its window ends at input row 2 t + k - 1 <= T_in - 1
        assert int((m[self.valid] % self.S_out).max()) * 2 + self.k - 1 <= self.T_in - 1
        self.ref = A.double() @ self.W.double().t() + self.bias.double()
        self.ref_bf = _bf(A) @ _bf(self.W).t() + self.bias.double()
        self.mag_bf = _bf(A).abs() @ _bf(self.W).abs().t()
        Xn = X.clone()
        Xn[pad] = float("nan")
        self.dX = Xn.cuda()
        self.dW, self.db = self.W.cuda(), self.bias.cuda()
        self.dXz = Xz.cuda()
        self.L = L
        self._p8 = {}
        self.a_elems = (self.M - 1) * self.lda + self.K
        assert self.a_elems <= rows * CD

    def a_window(self, mode, a_exp):
        """the padded buffer as the mode reads it: fp32 with NaN rows, or P8 at a_exp with fp16-NaN rows"""
        if mode != 1:
            return self.dX
        if ("w", a_exp) not in self._p8:
            Ap = _pack(self.L, self.dXz, a_exp)
            Ap[self.pad.cuda()] = NAN16
            self._p8[("w", a_exp)] = Ap
        return self._p8[("w", a_exp)]

    def a_dense(self, mode, a_exp):
        """the windows of all M rows gathered on the host side into dense rows (lda = K)"""
        key = ("d", mode == 1, a_exp if mode == 1 else 0)
        if key not in self._p8:
            src = self.a_window(mode, a_exp)
            self._p8[key] = torch.as_strided(src.reshape(-1), (self.M, self.K), (self.lda, 1)).contiguous()
        return self._p8[key]

    def check(self, mode, got, what):
        """the bars of the dense tests: test_ops_gpu.py::test_gemm (3e-5 of scale), ::test_gemm_p8_dma_pipeline_and_producers (2e-6
        relative), test_bf16_ops_gpu.py::_check (2e-5 sum|a w| + 1e-6 (1 + |ref|), bf16-rounded operands)"""
        assert bool(torch.isfinite(got).all()), f"{what}: a valid row is not finite (it read a padding row?)"
        if mode == 2:
            err = (got.double() - self.ref_bf).abs()
            bound = 2e-5 * self.mag_bf + 1e-6 * (1.0 + self.ref_bf.abs())
            assert float((err / bound).max()) <= 1.0, (what, float(err.max()))
            return float(err.max())
        err = float((got.double() - self.ref).abs().max())
        scale = float(self.ref.abs().max())
        if mode == 0:
            assert err < 3e-5 * max(1.0, scale), (what, err)
        else:
            assert err / scale < 2e-6, (what, err / scale)
        return err


def _conv_case(L, layer):
    if layer not in _CONV:
        _CONV[layer] = _ConvCase(L, layer)
    return _CONV[layer]


def _conv_launch(capi, L, p, mode, A_dev, lda, a_elems, cfg, S, a_exp, c_p8=0, c_exp=4):
    """one launch of artalk_op_gemm_rows into a Guarded [M][512]; returns the buffer and (used_cfg, used_splitk)"""
    out = Guarded(p.M * p.N)
    used = [C.c_int32(-7) for _ in range(3)]
    a = capi.GemmRowsArgs(mode=mode, M=p.M, N=p.N, K=p.K, A=_p(A_dev), lda=lda, a_elems=a_elems, a_exp=a_exp, W=_p(p.dW), ldw=p.K,
                          w_elems=p.N * p.K, bias=_p(p.db), bias_elems=p.N, C=out.ptr(), ldc=p.N, c_elems=p.M * p.N, cmap=IDENT,
                          c_p8=c_p8, c_exp=c_exp, force_cfg=cfg, splitk=S, used_cfg=C.pointer(used[0]), used_splitk=C.pointer(used[1]),
                          fused_ln=C.pointer(used[2]))
    rc = L.artalk_op_gemm_rows(C.byref(a), None)
    assert rc == 0, (rc, mode, cfg, S)
    out.check(f"mode {mode} cfg {cfg}: rows beyond M")
    return out, (used[0].value, used[1].value)


# (mode, force_cfg, splitk, a_exp)
CONV_LAUNCHES = {
    0: [(0, c, 1, 4) for c in (-1, 1, 2, 3, 4)],
    1: [(1, c, 1, e) for e in (4, 1) for c in (99, 7, 12, 8, 20, 28, 31)] + [(1, c, 3, e) for e in (4, 1) for c in (20, 28)],
    2: [(2, c, 1, 4) for c in (0, 1, 2)],
}
_RAN = {}        # (layer, forced mode-1 configuration) -> the configuration that ran


@pytest.mark.parametrize("layer", [6, 4])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_conv_layer_window_gemm_over_padded_chunks(layer, mode):
    """Layer 6 (k = 2, 3 chunks of 200 rows, 199 valid) and layer 4 (k = 3, 5 chunks of 800 rows, 799 valid): lda = 1024 < K.  Valid
    rows finite and within the dense-form bar of their kernel; in modes 0 and 1 bit-identical to the same configuration on the windows
    gathered into dense rows (lda = K) - only the addressing differs; nothing beyond row M written."""
    capi, L = _lib()
    p = _conv_case(L, layer)
    vmask = p.valid.cuda()
    for m, cfg, S, a_exp in CONV_LAUNCHES[mode]:
        out, (ucfg, uS) = _conv_launch(capi, L, p, m, p.a_window(m, a_exp), p.lda, p.a_elems, cfg, S, a_exp)
        got = out.f32(p.M, p.N)[vmask]
        what = f"layer {layer} mode {m} cfg {cfg} -> {ucfg} S {uS} a_exp {a_exp}"
        err = p.check(m, got.cpu(), what)
        print(f"{what}: max err {err:.3e}")
        assert uS == S, what
        if m == 1 and cfg != 99:
            _RAN[(layer, cfg)] = ucfg
        if m == 0 and cfg != -1:
            assert ucfg == cfg, what
        if m != 2:
            dense, (dcfg, dS) = _conv_launch(capi, L, p, m, p.a_dense(m, a_exp), p.K, p.M * p.K, ucfg if cfg in (-1, 99) else cfg, S, a_exp)
            assert (dcfg, dS) == (ucfg, uS), (what, dcfg, dS)
            assert torch.equal(dense.i32(p.M, p.N)[vmask], out.i32(p.M, p.N)[vmask]), what + ": window and dense launches differ"


def test_conv_layer_every_f16x3_configuration_ran():
    """A forced configuration a shape cannot take falls back (used_cfg says so): every one of 7, 12, 8, 20, 28, 31 must have run, as
    itself, on at least one of the two layers.  Run again here (dry run: the planner's answer without a launch)."""
    capi, L = _lib()
    assert L.artalk_op_rows_dry_run(1) == 0
    try:
        ran = {}
        for layer in (6, 4):
            d = CONV_LAYERS[layer]
            M, K = d["n"] * d["S_out"], d["k"] * CD
            P = 1 << 26
            for cfg in (7, 12, 8, 20, 28, 31):
                u = C.c_int32(-7)
                a = capi.GemmRowsArgs(mode=1, M=M, N=CD, K=K, A=P, lda=2 * CD, a_elems=(M - 1) * 2 * CD + K, W=2 * P, ldw=K, w_elems=CD * K,
                                      bias=3 * P, bias_elems=CD, C=4 * P, ldc=CD, c_elems=M * CD, force_cfg=cfg, used_cfg=C.pointer(u))
                assert L.artalk_op_gemm_rows(C.byref(a), None) == 0
                ran[(layer, cfg)] = u.value
                if (layer, cfg) in _RAN:
                    assert _RAN[(layer, cfg)] == u.value
    finally:
        assert L.artalk_op_rows_dry_run(0) == 0
    print("forced -> ran:", ran)
    for cfg in (7, 12, 8, 20, 28, 31):
        assert any(ran[(layer, cfg)] == cfg for layer in (6, 4)), f"configuration {cfg} ran on neither layer"


@pytest.mark.parametrize("layer,cfg", [(4, 99), (4, 12), (6, 20)])
def test_conv_layer_window_gemm_p8_result(layer, cfg):
    """the result written in P8 at c_exp = 2, as layers 1-5 hand it to their LayerNorm: the format bound plus the 2e-6 of the dense test
    (test_p8_exps_ops_gpu.py::test_gemm_consumer_and_producer_exponents)"""
    capi, L = _lib()
    p = _conv_case(L, layer)
    out, (ucfg, uS) = _conv_launch(capi, L, p, 1, p.a_window(1, 4), p.lda, p.a_elems, cfg, 1, 4, c_p8=1, c_exp=2)
    got = _unpack(out.i32(p.M, p.N)[p.valid.cuda()], 2)
    _assert_stored(got, p.ref, 2, 2e-6 * float(p.ref.abs().max()), f"layer {layer} c_p8 cfg {cfg} -> {ucfg}")


# ================================================================================================ d. LayerNorm + GELU in place
@pytest.mark.parametrize("p8_exp", [None, 4, 1])
@pytest.mark.parametrize("S,T", [(200, 199), (8, 5)])
def test_conv_layernorm_gelu_in_place_over_padded_chunks(S, T, p8_exp):
    """The conv_ln call of the stack: D = 512, Y == X, junk_period = S, junk_from = T, GELU, fp32 or P8 output over the same bytes.
    Padding rows hold inf on entry and exact zeros afterwards and do not raise the guard.  Bars: test_ops_gpu.py::test_layernorm (2e-5,
    the same distributions), test_p8_exps_ops_gpu.py::test_layernorm_p8_producer (format bound + 2e-5 max|ref| / 4)."""
    capi, L = _lib()
    n, D = 3, 512
    M = n * S
    g = _gen(700 + S)
    X = torch.randn(M, D, generator=g) * 2 + 0.3
    w, b = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ref = F.gelu(F.layer_norm(X.double(), (D,), w.double(), b.double(), 1e-5))
    junk = torch.arange(M) % S >= T
    X[junk] = float("inf")
    ref[junk] = 0.0
    buf = Guarded(M * D)
    buf.f32(M, D).copy_(X)
    dw, db = w.cuda(), b.cuda()
    st = _status()
    act = 1 | (0 if p8_exp is None else 0x100)
    mm = (C.c_int32 * 3)(*IDENT)
    rc = L.artalk_op_layernorm_rows(buf.ptr(), buf.ptr(), _p(dw), _p(db), None, None, M, D, 1e-5, act, 4 if p8_exp is None else p8_exp, S, T,
                                    _p(st), D, D, D, mm, M * D, M * D, 0, None)
    assert rc == 0, rc
    assert _st(st) == 0, "inf in the padding rows must not raise the guard"
    buf.check("layernorm in place")
    words = buf.i32(M, D).cpu()
    assert not bool(words[junk].any()), "padding rows are stored as zeros"
    if p8_exp is None:
        _assert_within(words.view(torch.float32), ref, torch.full_like(ref, 2e-5), f"LN + GELU in place S={S}")
    else:
        _assert_stored(_unpack(words, p8_exp), ref, p8_exp, 2e-5 * float(ref.abs().max()) / 4.0, f"LN + GELU in place P8 S={S}")


# ================================================================================================ e. positional convolution
_POSCONV = {}


def _posconv_case(groups, cg, taps, T, Ts, n=3):
    """X [n * Ts][groups * cg] with chunk 1 at 8 times the scale of chunks 0 and 2 and NaN in the padding rows; float64 grouped conv1d with
    padding taps / 2 PER CHUNK (hf Wav2Vec2PositionalConvEmbedding: the last output frame dropped), as a product with the zero-padded
    windows (k = tap * cg + ci); X + gelu(conv + bias) on frames t < T, for fp32 and for bf16-rounded operands."""
    key = (groups, cg, taps, T, Ts)
    if key in _POSCONV:
        return _POSCONV[key]
    g = _gen(800 + T)
    H, K, pad = groups * cg, cg * taps, taps // 2
    X = torch.randn(n, Ts, H, generator=g)
    X[1] *= 8.0
    W = torch.randn(H, K, generator=g) / math.sqrt(K)
    bias = torch.randn(H, generator=g)
    ref, ref_bf, mag_bf = (torch.zeros(n, T, H, dtype=torch.float64) for _ in range(3))
    for c in range(n):
        xp = F.pad(X[c, :T].double(), (0, 0, pad, pad))                # zeros on both sides of the chunk's own frames
        xb = F.pad(_bf(X[c, :T]), (0, 0, pad, pad))
        for z in range(groups):
            cols = slice(z * cg, (z + 1) * cg)
            A = xp[:, cols].unfold(0, taps, 1)[:T].permute(0, 2, 1).reshape(T, K)        # A[t, tap * cg + ci] = xp[t + tap, ci]
            Ab = xb[:, cols].unfold(0, taps, 1)[:T].permute(0, 2, 1).reshape(T, K)
            Wz = W[cols]
            ref[c, :, cols] = A @ Wz.double().t()
            ref_bf[c, :, cols] = Ab @ _bf(Wz).t()
            mag_bf[c, :, cols] = Ab.abs() @ _bf(Wz).abs().t()
    res = X[:, :T].double()
    ref = res + F.gelu(ref + bias.double())
    ref_bf = res + F.gelu(ref_bf + bias.double())
    # check of the window layout against torch's grouped conv1d on one chunk
    w_t = W.view(H, taps, cg).permute(0, 2, 1).contiguous().double()
    y = F.conv1d(X[0, :T].double().t()[None], w_t, bias.double(), padding=pad, groups=groups)[0, :, :T].t()
    assert float((res[0] + F.gelu(y) - ref[0]).abs().max()) < 1e-9
    Xn = X.clone()
    Xn[:, T:] = float("nan")
    _POSCONV[key] = dict(X=X, Xn=Xn, W=W, bias=bias, ref=ref, ref_bf=ref_bf, mag_bf=mag_bf)
    return _POSCONV[key]


def _posconv_run(L, mode, case, groups, cg, taps, T, Ts, cfg=-1, n=3):
    H = groups * cg
    dX, dW, db = case["Xn"].reshape(n * Ts, H).cuda(), case["W"].cuda(), case["bias"].cuda()
    out = Guarded(n * Ts * H)
    resid = case["X"].clone()
    resid[:, T:] = 0.0                                                # the padding rows of the residual: finite, whatever
    out.f32(n, Ts, H).copy_(resid)
    st = _status()
    x_elems = ((n - 1) * Ts + T) * H
    rc = L.artalk_op_posconv_rows(mode, _p(dX), x_elems, _p(dW), _p(db), out.ptr(), out.ptr(), n * Ts * H, n, T, Ts, groups, cg, taps, 1, 4, cfg,
                                  _p(st), None)
    assert rc == 0, rc
    assert _st(st) == 0
    out.check(f"posconv mode {mode}")
    return out.f32(n, Ts, H)[:, :T].cpu()


def _posconv_check(mode, got, case, what):
    """mode 0: test_ops_gpu.py::test_gemm; mode 1: test_p8_exps_ops_gpu.py::test_posconv_p8_exponent_and_guard (2e-6 of max|ref|);
    mode 2: test_bf16_ops_gpu.py::test_gemm_bf16_posconv_window (_check)"""
    assert bool(torch.isfinite(got).all()), f"{what}: a valid frame is not finite (a padding row was read?)"
    ref = case["ref_bf"] if mode == 2 else case["ref"]
    err = (got.double() - ref).abs()
    worst = err.reshape(err.shape[0], -1).max(dim=1).values
    print(f"{what}: max err per chunk {[f'{float(v):.2e}' for v in worst]}, max|ref| {float(ref.abs().max()):.2f}")
    if mode == 0:
        assert float(err.max()) < 3e-5 * max(1.0, float(ref.abs().max())), (what, float(err.max()))
    elif mode == 1:
        assert float(err.max()) / float(ref.abs().max()) < 2e-6, (what, float(err.max()))
    else:
        bound = 2e-5 * case["mag_bf"] + 1e-6 * (1.0 + ref.abs())
        assert float((err / bound).max()) <= 1.0, (what, float(err.max()))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("T,Ts", [(39, 40), (199, 200)])
def test_posconv_over_padded_chunks(T, Ts, mode):
    """16 groups of 64 channels, 128 taps, 3 chunks of Ts = T + 1 rows, GELU and the residual in place.  Leakage across a chunk boundary
    (chunk 1 is 8 times its neighbours) or a read of the NaN padding row shows at frames t < 64 and t >= T - 64."""
    capi, L = _lib()
    case = _posconv_case(16, 64, 128, T, Ts)
    got = _posconv_run(L, mode, case, 16, 64, 128, T, Ts)
    _posconv_check(mode, got, case, f"posconv T={T} mode {mode}")


@pytest.mark.parametrize("mode,cfg", [(0, c) for c in (-1, 1, 2, 3, 4)] + [(2, c) for c in (-1, 0, 1, 2)])
def test_posconv_small_groups_every_frame_touches_both_paddings(mode, cfg):
    """3 groups of 32 channels, 8 taps, (T, Ts) = (5, 8): every output frame reaches past both ends of its chunk; every tile"""
    capi, L = _lib()
    case = _posconv_case(3, 32, 8, 5, 8)
    got = _posconv_run(L, mode, case, 3, 32, 8, 5, 8, cfg)
    _posconv_check(mode, got, case, f"posconv small mode {mode} cfg {cfg}")


# ================================================================================================ f. encoder attention in its buffer
_ATTN = {}


def _attn_case(B):
    if B not in _ATTN:
        g = _gen(900 + B)
        H, HD, Lq = 16, 64, 199
        qkv = torch.randn(B, 200, 3 * H * HD, generator=g)
        q, k, v = (qkv[:, :Lq, i * 1024:(i + 1) * 1024].reshape(B, Lq, H, HD).transpose(1, 2).double() for i in range(3))
        ref = ((q @ k.transpose(-1, -2) * HD ** -0.5).softmax(-1) @ v).transpose(1, 2).reshape(B, Lq, H * HD)
        _ATTN[B] = (qkv, ref)
    return _ATTN[B]


# (B, l2norm flags, P8 rows and output)
@pytest.mark.parametrize("B,flags,use_p8", [(3, 0, False), (3, 2, False), (3, 6, True), (20, 6, True)])
def test_encoder_attention_in_the_interleaved_buffer(B, flags, use_p8):
    """Lq = Lk = 199 in 200-row clip strides: Q / K / V at columns 0 / 1024 / 2048 of one [B * 200][3072] buffer (ld = 3072), O
    [B * 200][1024].  Row 199 of every clip holds NaN in q|k|v and keeps the fill in O (engine.hip rests on that row never being
    written).  fp32 rows on the fp32 kernel and on the f16-split kernel; P8 rows at qkv_exp = 2 with P8 output at o_exp = 3; B = 20 is
    the batch at which the wide kernel takes over.  Bars: test_ops_gpu.py::test_attention (2e-5, outputs of magnitude ~1),
    test_p8_exps_ops_gpu.py::test_attention_p8_in_and_out (format bound + 2e-5 max|ref|)."""
    capi, L = _lib()
    H, HD, Lq, D = 16, 64, 199, 1024
    qkv, ref = _attn_case(B)
    qe, oe = (2, 3) if use_p8 else (4, 4)
    if use_p8:
        src = torch.cat([_pack(L, qkv[:, :, i * D:(i + 1) * D].reshape(B * 200, D).contiguous().cuda(), qe) for i in range(3)], dim=1)
        src.view(B, 200, 3 * D)[:, Lq:] = NAN16
    else:
        x = qkv.clone()
        x[:, Lq:] = float("nan")
        src = x.reshape(B * 200, 3 * D).cuda()
    src = src.contiguous()
    out = Guarded(B * 200 * D)
    st = _status()
    bs = 200 * 3 * D
    in_elems = (B - 1) * bs + (Lq - 1) * 3 * D + D
    o_elems = (B - 1) * 200 * D + (Lq - 1) * D + D
    base = src.data_ptr()
    rc = L.artalk_op_attention_rows(base, base + 4 * D, base + 8 * D, out.ptr(), B, H, HD, Lq, Lq, HD ** -0.5, flags, None, 0, qe, oe,
                                    1 if use_p8 else 0, _p(st), 3 * D, 3 * D, 3 * D, D, bs, bs, bs, 200 * D, in_elems, in_elems, in_elems,
                                    o_elems, None)
    assert rc == 0, rc
    assert _st(st) == 0
    out.check("attention")
    words = out.i32(B, 200, D).cpu()
    assert bool((words[:, Lq:] == CANARY).all()), "the padding row of a clip was written"
    got = words[:, :Lq]
    if use_p8:
        _assert_stored(_unpack(got, oe), ref, oe, 2e-5 * float(ref.abs().max()), f"attention P8 B={B}")
    else:
        _assert_within(got.view(torch.float32), ref, torch.full_like(ref, 2e-5), f"attention flags {flags}")


# ================================================================================================ g. pooling + SiLU
PN = (1, 5, 25, 50, 100)


def _pool_ref_and_bound(X):
    """X [C][T][D] float32 -> float64 SiLU(adaptive_avg_pool1d per level) [C][181][D] and the rounding bound of pool_silu_kernel:
    s = fp32 sum of the nb frames of a bin in frame order (the first add, to 0, is exact): |s^ - s| <= U sum_{k=2..nb} |S_k| (1 + 2^-10),
    S_k the partial sums, U = 2^-24; m = s / nb: one division, U |m|; silu(m) = m / (1 + expf(-m)): the error of m is carried over by
    |silu'(m)| = |sigmoid(m) (1 + m (1 - sigmoid(m)))| (+ 2^-10 for the curvature: |silu''| <= 1/2 over an error of m below 1e-5); the addition 1 + e and the division are U each relative to the result, and the 2 ulp = 4 U allowed to e = expf(-m) reach the
    denominator weighted by e / (1 + e) (nothing for large positive m, all of it for negative m)."""
    Cn, T, D = X.shape
    x = X.double()
    refs, bounds = [], []
    for pn in PN:
        pooled = F.adaptive_avg_pool1d(x.permute(0, 2, 1), pn).permute(0, 2, 1)
        for i in range(pn):
            t0, t1 = (i * T) // pn, -((-(i + 1) * T) // pn)
            part = x[:, t0:t1].cumsum(dim=1)
            m = part[:, -1] / (t1 - t0)
            assert float((m - pooled[:, i]).abs().max()) < 1e-12
            sum_err = U * part[:, 1:].abs().sum(dim=1) * (1 + 2.0 ** -10)
            refs.append(F.silu(m))
            slope = (torch.sigmoid(m) * (1 + m * torch.sigmoid(-m))).abs() + 2.0 ** -10
            bounds.append(slope * (sum_err / (t1 - t0) + U * m.abs()) + (2 * U + 4 * U * torch.sigmoid(-m)) * F.silu(m).abs())
    return torch.stack(refs, dim=1), torch.stack(bounds, dim=1)


@pytest.mark.parametrize("p8_exp", [None, 4])
@pytest.mark.parametrize("T,D", [(199, 1024), (199, 8), (100, 64), (101, 64), (7, 64)])
def test_pool_silu_reads_with_the_frame_stride(T, D, p8_exp):
    """x_tstride in {T, T + 1} with NaN padding rows, C in {1, 3}.  T = 100: the bins of the last level are exactly one frame; T = 7:
    overlapping bins that repeat frames.  Bound: _pool_ref_and_bound; at the shape of test_ops_gpu.py::test_pool_silu it must not be
    looser than the 2e-6 that test holds."""
    capi, L = _lib()
    X = torch.randn(3, T, D, generator=_gen(1000 + T + D))
    ref, bound = _pool_ref_and_bound(X)
    if (T, D) == (199, 1024):
        assert float(bound.max()) <= 2e-6, float(bound.max())
    for Cn in (1, 3):
        for ts in (T, T + 1):
            Xp = torch.full((Cn, ts, D), float("nan"))
            Xp[:, :T] = X[:Cn]
            dX = Xp.cuda()
            out = Guarded(Cn * 181 * D)
            st = _status()
            x_elems = ((Cn - 1) * ts + T) * D
            rc = L.artalk_op_pool_silu_rows(_p(dX), Cn, T, D, out.ptr(), 0 if p8_exp is None else 1, 4 if p8_exp is None else p8_exp, _p(st), ts,
                                            x_elems, Cn * 181 * D, None)
            assert rc == 0, rc
            assert _st(st) == 0
            out.check("pool_silu")
            what = f"pool T={T} D={D} C={Cn} stride {ts}"
            if p8_exp is None:
                got = out.f32(Cn, 181, D).cpu()
                print(f"{what}: max err {float((got.double() - ref[:Cn]).abs().max()):.3e}, max bound {float(bound.max()):.3e}")
                _assert_within(got, ref[:Cn], bound[:Cn], what)
            else:
                _assert_stored(_unpack(out.i32(Cn, 181, D).cpu(), p8_exp), ref[:Cn], p8_exp, bound[:Cn], what)
