"""Site exponent and range guard of every P8 producer / consumer kernel, through the artalk_op_*_ex entry points.

A producer with site exponent e stores hi = f16(x * 2^e), lo = f16(x * 2^e - hi) and raises status bit 3 when |x| * 2^e > 65504 (or x is
NaN); a consumer removes the 2^e of the buffer it reads.  Every launch parameter defaults to 4, so a kernel (or call site) that holds a
literal 16 is invisible until a calibration lowers its site.  Here every kernel runs at e in {-8, -3, 0, 3, 4}, with inputs near the top
of the range that exponent gives (500 * 2^(4 - e) * N(0, 1): what a calibrated site holds), against float64 on the CPU and the numpy
restatement of the format (tests/p8_format.py, itself checked in test_p8_format_cpu.py).  Bars: the format bound of p8_format.bound for a
stored value, plus the bars test_ops_gpu.py already uses for the arithmetic (2e-6 of the largest result for the split GEMMs, 2e-5
absolute for attention outputs of magnitude ~1 - relative to the largest value here - and LayerNorm).  Guard tests feed inf / NaN as data.

The split-K reduce fused with the AdaLN LayerNorm (launch_splitk_reduce_ln takes a GemmArgs and an LnArgs of the AR residual stream) is
covered by test_rows_ops_gpu.py through artalk_op_gemm_rows, at ln_p8_exp 4, 0 and -8."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import p8_format as p8

pytestmark = pytest.mark.gpu

EXPS = [-8, -3, 0, 3, 4]
OTHER = {-8: -3, -3: 0, 0: 3, 3: 4, 4: -8}        # the exponent of the other side of a launch: never the same as e
BIG = (7, 12, 8)                                    # large-grid LDS-DMA kernels (256x256 / 320x256 persistent, two-workgroup 128x128)
SMALL = (20, 23, 24, 28, 31)                        # small-grid, deep-ring, mid-grid, ping-pong
SPLITK = (20 | (4 << 8), 23 | (8 << 8), 24 | (2 << 8), 28 | (3 << 8), 31 | (4 << 8))
CANARY = 0x7fc00000


def _lib():
    from artalk_amd import capi
    return capi, capi.lib()


def _dev(t):
    return t.contiguous().cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _sigma(e):
    return 500.0 * 2.0 ** (4 - e)


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _st(s):
    torch.cuda.synchronize()
    return int(s.item())


def _i32(rows, cols, canary_rows=0):
    return torch.full((rows + canary_rows, cols), CANARY, dtype=torch.int32, device="cuda")


def _unpack(t, e):
    return torch.from_numpy(p8.unpack(t.cpu().numpy(), e))


def _hi_finite(t):
    return bool(np.isfinite(p8.halves(t.cpu().numpy())[0]).all())


def _pack(L, x_dev, e, status=None):
    out = torch.empty(x_dev.shape, dtype=torch.int32, device="cuda")
    assert L.artalk_op_pack_split_ex(_p(x_dev), _p(out), x_dev.numel(), 0, e, _p(status), None) == 0
    return out


def _pack_w(L, w_dev):
    out = torch.empty(w_dev.shape, dtype=torch.int32, device="cuda")
    assert L.artalk_op_pack_split(_p(w_dev), _p(out), w_dev.numel(), 1, None) == 0
    return out


def _assert_stored(got64, ref64, e, arith, what):
    """A P8 result unpacked with its exponent against float64: the format bound plus the arithmetic bar of the op."""
    err = (got64 - ref64).abs()
    tol = torch.from_numpy(p8.bound(ref64.numpy(), e)) + arith
    bad = err > tol
    assert not bool(bad.any()), (what, e, float(err.max()), float((err - tol).max()), float(ref64.abs().max()))


def _bad_values(e):
    top = p8.max_value(e)
    return [("nextafter", float(np.nextafter(top, np.float32(np.inf)))), ("inf", float("inf")), ("nan", float("nan"))]


def test_exponents_are_validated_before_the_device():
    capi, L = _lib()
    x = torch.zeros(64, 64, device="cuda")
    o = torch.zeros(64, 64, dtype=torch.int32, device="cuda")
    for e in (-9, 5):
        assert L.artalk_op_pack_split_ex(_p(x), _p(o), x.numel(), 0, e, None, None) == capi.EINVAL
        assert L.artalk_op_layernorm_ex(_p(x), _p(o), None, None, None, None, 64, 512, 1e-5, 0x100, e, 0, 0, None, None) == capi.EINVAL
        assert L.artalk_op_gemm_f16s_packed_ex(_p(o), 1, 64, _p(o), None, _p(x), 64, 64, 64, 0, 20, e, 4, None, None, None) == capi.EINVAL
        assert L.artalk_op_gemm_f16s_packed_ex(_p(o), 1, 64, _p(o), None, _p(x), 64, 64, 64, 0, 20, 4, e, None, None, None) == capi.EINVAL
        assert L.artalk_op_gemm_f16s_ex(_p(x), 64, _p(x), None, _p(x), 64, 64, 64, 0, 1, e, None, None) == capi.EINVAL
        assert L.artalk_op_attention_ex(_p(x), _p(x), _p(x), _p(x), 1, 1, 64, 64, 64, 1.0, 6, None, 0, e, 4, 1, None, None) == capi.EINVAL
        assert L.artalk_op_attention_ex(_p(x), _p(x), _p(x), _p(x), 1, 1, 64, 64, 64, 1.0, 6, None, 0, 4, e, 1, None, None) == capi.EINVAL
        assert L.artalk_op_pool_silu_ex(_p(x), 1, 64, 64, _p(x), 1, e, None, None) == capi.EINVAL
    # the 128-wide LayerNorm (style encoder: its GEMMs split fp32 rows while staging) has no P8 store: refused, not written as fp32
    assert L.artalk_op_layernorm_ex(_p(x), _p(o), None, None, None, None, 32, 128, 1e-5, 0x100, 4, 0, 0, None, None) == capi.EINVAL
    assert L.artalk_op_layernorm(_p(x), _p(o), None, None, None, None, 32, 128, 1e-5, 0x100, None) == capi.EINVAL


# ------------------------------------------------------------------------------------------------------------------ pack_split
@pytest.mark.parametrize("e", EXPS)
def test_pack_split_producer_and_guard(e):
    capi, L = _lib()
    g = torch.Generator().manual_seed(e + 20)
    M, K = 300, 256
    x = torch.randn(M, K, generator=g) * _sigma(e)
    x[0, :8] = torch.tensor([0.0, 1.0, -1.0, 2.0 ** -20, 3.0, -2.0 ** -24, 0.5, 7.0]) / 2.0 ** e        # small values: the lo half is subnormal
    top = float(p8.max_value(e))
    x[5, 17] = top
    x[7, 100] = -top
    assert float(x.abs().max()) == top
    out = _i32(M, K, 8)
    st = _status()
    assert L.artalk_op_pack_split_ex(_p(_dev(x)), _p(out), M * K, 0, e, _p(st), None) == 0
    assert _st(st) == 0 and _hi_finite(out[:M]) and bool((out[M:] == CANARY).all())
    _assert_stored(_unpack(out[:M], e), x.double(), e, 0.0, "pack_split")
    assert np.array_equal(out[:M].cpu().numpy(), p8.pack(x.numpy(), e)), "the device stores the words of the numpy restatement"
    for what, v in _bad_values(e):
        y = x.clone()
        y[200, 77] = v
        st = _status()
        assert L.artalk_op_pack_split_ex(_p(_dev(y)), _p(out), M * K, 0, e, _p(st), None) == 0
        assert _st(st) == 8, (what, e)
    # weights have their own fixed scale and no guard
    st = _status()
    assert L.artalk_op_pack_split_ex(_p(_dev(x)), _p(out), M * K, 1, e, _p(st), None) == 0 and _st(st) == 0


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("e", EXPS)
@pytest.mark.parametrize("D,mod", [(512, False), (768, True), (1024, False), (768, False), (1024, True), (512, True)])
def test_layernorm_p8_producer(D, mod, e):
    """out_p8 at the three widths that have it, plain affine and AdaLN-modulated, small (one row per wave) and large (several rows per
    wave) launches, with layout-padding rows: the gain is chosen so that the output is near the top of the range of e."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(D + e)
    for M, period, frm in ((333, 37, 30), (8192 + 40, 0, 0)):
        X = torch.randn(M, D, generator=g) * 2 + 0.3
        w = torch.randn(D, generator=g) * (_sigma(e) / 8 if not mod else 1.0)      # |LN(x)| reaches ~4, |w| ~4: the output ~2 sigma
        b = torch.randn(D, generator=g)
        sc = torch.randn(M, D, generator=g) * _sigma(e) / 32 if mod else None
        sh = torch.randn(M, D, generator=g) if mod else None
        ref = F.layer_norm(X.double(), (D,), w.double(), b.double(), 1e-5)
        if mod:
            ref = ref * (sc.double() + 1) + sh.double()
        junk = (torch.arange(M) % period >= frm) if period else torch.zeros(M, dtype=torch.bool)
        if period:
            X[junk] = float("inf")            # whatever an earlier launch left in the padding rows
            ref[junk] = 0.0
        out = _i32(M, D, 8)
        st = _status()
        dX, dw, db = _dev(X), _dev(w), _dev(b)
        dsc, dsh = (_dev(sc), _dev(sh)) if mod else (None, None)
        assert L.artalk_op_layernorm_ex(_p(dX), _p(out), _p(dw), _p(db), _p(dsc), _p(dsh), M, D, 1e-5, 0x100, e, period, frm, _p(st), None) == 0
        assert _st(st) == 0, "inf in layout-padding rows must not raise the guard"
        assert bool((out[M:] == CANARY).all()) and float(ref.abs().max()) < float(p8.max_value(e))
        assert not out[:M][junk.cuda()].any(), "padding rows are stored as zeros"
        _assert_stored(_unpack(out[:M], e), ref, e, 2e-5 * float(ref.abs().max()) / 4.0, f"layernorm D={D} mod={mod} M={M}")


@pytest.mark.parametrize("e", EXPS)
@pytest.mark.parametrize("D,mod", [(512, False), (768, True), (1024, False)])
def test_layernorm_guard_threshold(D, mod, e):
    """Exact constructions: with a zero gain y = 0 * LN(x) + b = b, with AdaLN scale -1 y = t * 0 + shift = shift, so the produced
    values are the chosen ones bit for bit."""
    capi, L = _lib()
    M = 40
    X = torch.randn(M, D, generator=torch.Generator().manual_seed(1))
    top = float(p8.max_value(e))

    def run(v, row_is_junk=False):
        tgt = torch.ones(M, D) / 2.0 ** e
        tgt[13, 129] = v
        out = _i32(M, D)
        st = _status()
        if mod:
            args = (None, None, _dev(torch.full((M, D), -1.0)), _dev(tgt))
        else:
            tgt[:] = tgt[13]
            args = (_dev(torch.zeros(D)), _dev(tgt[13].clone()), None, None)
        period, frm = (14, 13) if row_is_junk else (0, 0)      # rows 13, 27: padding
        assert L.artalk_op_layernorm_ex(_p(_dev(X)), _p(out), _p(args[0]), _p(args[1]), _p(args[2]), _p(args[3]), M, D, 1e-5, 0x100, e, period,
                                        frm, _p(st), None) == 0
        return _st(st), out

    s, out = run(top)
    assert s == 0 and _hi_finite(out)
    assert float(_unpack(out, e)[13, 129]) == top and float(_unpack(out, e)[12, 0]) == 1.0 / 2.0 ** e
    for what, v in _bad_values(e):
        assert run(v)[0] == 8, (what, e)
    if mod:      # the same value in a padding row: stored as zero, no guard
        s, out = run(float("inf"), row_is_junk=True)
        assert s == 0 and not out[13].any()


# ------------------------------------------------------------------------------------------------------------------ split GEMMs
def _gemm_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    R = torch.randn(M, N, generator=g)
    return A, W, bias, R, A.double() @ W.double().t()


@pytest.mark.parametrize("e", EXPS)
@pytest.mark.parametrize("group", ["big", "small"])
def test_gemm_consumer_and_producer_exponents(group, e):
    """Every production configuration with A packed at a_exp = e and the result requested at c_exp != a_exp: as fp32 (plain, residual in
    place, GELU), as P8 (the c_p8 epilogue; the split-K configurations write it from the reduce pass) and as fp32 plus the c2 second copy.
    A is drawn near the top of the range of max(a_exp, c_exp) so that the result fits the range of c_exp."""
    capi, L = _lib()
    M, N, K = (1000, 1024, 512) if group == "big" else (400, 1024, 1024)
    cfgs = BIG if group == "big" else SMALL + SPLITK
    ce = OTHER[e]
    A, W, bias, R, AW = _gemm_case(M, N, K, M + e)
    s = _sigma(max(e, ce))
    A, bias, R, AW = A * s, bias * s, R * s, AW * s
    Ap, Wp, db = _pack(L, _dev(A), e), _pack_w(L, _dev(W)), _dev(bias)
    lin = AW + bias.double()
    for cfg in cfgs:
        for act, ref in ((0, lin), (0x200, lin + R.double()), (1, F.gelu(lin))):
            scale = float(ref.abs().max())
            # fp32 result
            out = torch.full((M + 8, N), float("nan"), device="cuda")
            if act & 0x200:
                out[:M] = _dev(R)
            st = _status()
            assert L.artalk_op_gemm_f16s_packed_ex(_p(Ap), 1, K, _p(Wp), _p(db), _p(out), M, N, K, act, cfg, e, ce, None, _p(st), None) == 0
            assert _st(st) == 0
            err = float((out[:M].cpu().double() - ref).abs().max()) / scale
            assert err < 2e-6, (cfg, act, e, err)
            assert bool(torch.isnan(out[M:]).all())
            if act & 0x200:
                continue
            # the same as a P8 result at c_exp
            outp = _i32(M, N, 8)
            st = _status()
            assert L.artalk_op_gemm_f16s_packed_ex(_p(Ap), 1, K, _p(Wp), _p(db), _p(outp), M, N, K, act | 0x100, cfg, e, ce, None, _p(st), None) == 0
            assert _st(st) == 0 and bool((outp[M:] == CANARY).all())
            _assert_stored(_unpack(outp[:M], ce), ref, ce, 2e-6 * scale, f"c_p8 cfg={cfg} act={act}")
            # fp32 result plus its second copy in P8 (fused into the epilogue of 20 / 23 / 24, a split pass otherwise)
            if act == 0:
                c2 = _i32(M, N, 8)
                st = _status()
                assert L.artalk_op_gemm_f16s_packed_ex(_p(Ap), 1, K, _p(Wp), _p(db), _p(out), M, N, K, 0, cfg, e, ce, _p(c2), _p(st), None) == 0
                assert _st(st) == 0 and bool((c2[M:] == CANARY).all())
                got = out[:M].cpu()
                assert float((got.double() - ref).abs().max()) / scale < 2e-6
                assert np.array_equal(c2[:M].cpu().numpy(), p8.pack(got.numpy(), ce)), f"cfg {cfg}: c2 is the fp32 result packed at c_exp"


@pytest.mark.parametrize("e", EXPS)
def test_gemm_results_are_bit_identical_across_exponents(e):
    """Small integers times a power of two are exact in the hi half at every exponent (lo = 0): a kernel that removes the scale it was
    given computes bit for bit what it computes at 4 - no tolerance; a literal 16 left anywhere is a factor 2^(4-e)."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(3)
    for cfgs, (M, N, K) in ((BIG, (1000, 1024, 512)), (SMALL + SPLITK + (0, 1), (400, 1024, 1024))):
        A = torch.randint(-4, 5, (M, K), generator=g).float()
        W = torch.randint(-2, 3, (N, K), generator=g).float() / 2
        bias = torch.randint(-8, 9, (N,), generator=g).float()
        ref = (A.double() @ W.double().t() + bias.double()).float()
        assert float(ref.abs().max()) < 1024
        dA, Wp, db = _dev(A), _pack_w(L, _dev(W)), _dev(bias)
        Ae, A4 = _pack(L, dA, e), _pack(L, dA, 4)
        assert not p8.halves(Ae.cpu().numpy())[1].any()
        for cfg in cfgs:
            res = []
            for Ap, ae, ce in ((A4, 4, 4), (Ae, e, OTHER[e])):
                out = torch.full((M, N), float("nan"), device="cuda")
                outp = _i32(M, N)
                assert L.artalk_op_gemm_f16s_packed_ex(_p(Ap), 1, K, _p(Wp), _p(db), _p(out), M, N, K, 0, cfg, ae, ce, None, None, None) == 0
                assert L.artalk_op_gemm_f16s_packed_ex(_p(Ap), 1, K, _p(Wp), _p(db), _p(outp), M, N, K, 0x100, cfg, ae, ce, None, None, None) == 0
                torch.cuda.synchronize()
                res.append((out.cpu(), _unpack(outp, ce)))
            assert torch.equal(res[0][0], ref), cfg
            assert torch.equal(res[1][0], res[0][0]), (cfg, e)
            assert torch.equal(res[1][1], res[0][1]) and torch.equal(res[1][1], ref.double()), (cfg, e)
        # fp32 A rows split while staging (the register-staged kernels of the "(fp32 A)" sites)
        for cfg in (0, 1):
            out = torch.full((M, N), float("nan"), device="cuda")
            assert L.artalk_op_gemm_f16s_packed_ex(_p(dA), 0, K, _p(Wp), _p(db), _p(out), M, N, K, 0, cfg, e, 4, None, None, None) == 0
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), ref), (cfg, e)


@pytest.mark.parametrize("e", EXPS)
def test_gemm_guard_threshold(e):
    """A = 0 and a bias holding the value: C = 0 + bias exactly, so the c_p8 epilogue (every configuration, the split-K reduce included)
    and the c2 copy see exactly 65504 / 2^e, the next float, inf and NaN in one column.
    The large-grid kernels (7, 12, 8) carry no guard in their epilogue by design (launch_gemm_p8: it cost the dominant kernel registers);
    what they promise instead is that an out-of-range result is not laundered: inf, NaN and anything that rounds beyond 65504 is stored
    as inf / NaN in the hi half, where the guard of the kernel that consumes it (attention output, LayerNorm) reports it.  Their second
    copy (c2) is written by the guarded split pass."""
    capi, L = _lib()
    top = float(p8.max_value(e))
    for cfgs, (M, N, K) in ((BIG, (1000, 1024, 512)), (SMALL + SPLITK, (400, 1024, 1024))):
        Ap = torch.zeros(M, K, dtype=torch.int32, device="cuda")
        Wp = _pack_w(L, _dev(torch.randn(N, K, generator=torch.Generator().manual_seed(2)) / 32))
        for cfg in cfgs:
            for what, v in [("top", top)] + _bad_values(e) + [("twice", 2 * top)]:
                bias = torch.ones(N) / 2.0 ** e
                bias[517] = v
                db = _dev(bias)
                outp = _i32(M, N)
                st = _status()
                assert L.artalk_op_gemm_f16s_packed_ex(_p(Ap), 1, K, _p(Wp), _p(db), _p(outp), M, N, K, 0x100, cfg, OTHER[e], e, None, _p(st), None) == 0
                if cfg in BIG:
                    hi = p8.halves(outp.cpu().numpy())[0]
                    assert _st(st) in ((0,) if what == "top" else (0, 8)) and np.isfinite(np.delete(hi, 517, axis=1)).all(), (cfg, what, e)
                    assert np.isfinite(hi[:, 517]).all() == (what in ("top", "nextafter")), (cfg, what, e)      # (the next float still rounds to 65504)
                else:
                    assert _st(st) == (0 if what == "top" else 8), (cfg, what, e)
                if what == "top":
                    assert _hi_finite(outp) and bool((_unpack(outp, e)[:, 517] == top).all())
                out = torch.empty(M, N, device="cuda")
                c2 = _i32(M, N)
                st = _status()
                assert L.artalk_op_gemm_f16s_packed_ex(_p(Ap), 1, K, _p(Wp), _p(db), _p(out), M, N, K, 0, cfg, OTHER[e], e, _p(c2), _p(st), None) == 0
                assert _st(st) == (0 if what == "top" else 8), ("c2", cfg, what, e)


@pytest.mark.parametrize("e", EXPS)
@pytest.mark.parametrize("cfg", [0, 1])
def test_gemm_fp32_a_split_while_staging(cfg, e):
    """The "(fp32 A)" sites: the register-staged kernels split fp32 A rows with 2^a_exp while staging them, and guard them."""
    capi, L = _lib()
    M, N, K = 1000, 512, 512
    A, W, bias, R, AW = _gemm_case(M, N, K, 77 + e)
    A, AW = A * _sigma(e), AW * _sigma(e)
    top = float(p8.max_value(e))
    A[123, 45] = top
    ref = A.double() @ W.double().t() + bias.double()
    dW, db = _dev(W), _dev(bias)

    def run(Ax):
        out = torch.full((M, N), float("nan"), device="cuda")
        st = _status()
        assert L.artalk_op_gemm_f16s_ex(_p(_dev(Ax)), K, _p(dW), _p(db), _p(out), M, N, K, 0, cfg, e, _p(st), None) == 0
        return _st(st), out.cpu()

    s, out = run(A)
    assert s == 0
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    assert err < 2e-6, err
    for what, v in _bad_values(e):
        B = A.clone()
        B[123, 45] = v
        assert run(B)[0] == 8, (what, e)


# ------------------------------------------------------------------------------------------------------------------ attention
def _attn_ref(Q, K, V, H, scale, split):
    B, Lq, D = Q.shape
    Lk = K.shape[1]
    q, k, v = (t.view(B, -1, H, 64).transpose(1, 2).double() for t in (Q, K, V))
    s = q @ k.transpose(-1, -2) * scale
    if split:
        mask = torch.zeros(Lq, Lk, dtype=torch.double)
        mask[:split, split:] = -float("inf")
        s = s + mask
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, Lq, D)


# (B, H, Lq, Lk, split): the 64-query kernel, the wide kernels (one / two workgroups per head), the masked VAE decoder shape and the
# persistent ping-pong kernel (two or more heads per compute unit) - the shapes of test_ops_gpu.py
P8_ATTN = [(2, 8, 100, 100, 0), (3, 16, 199, 199, 0), (2, 8, 200, 200, 100), (20, 16, 199, 199, 0), (40, 16, 199, 199, 0)]


@pytest.mark.parametrize("e", EXPS)
@pytest.mark.parametrize("B,H,Lq,Lk,split", P8_ATTN)
def test_attention_p8_in_and_out(B, H, Lq, Lk, split, e):
    """Q, K, V rows in P8 at qkv_exp = e (near the top of its range; the softmax scale brings the scores back to O(1)), O written in P8 at
    o_exp != qkv_exp and as fp32, against float64."""
    capi, L = _lib()
    oe = OTHER[e]
    g = torch.Generator().manual_seed(Lq * 1000 + Lk + e)
    D = H * 64
    s = _sigma(max(e, oe))
    Q, K, V = (torch.randn(B, n, D, generator=g) * s for n in (Lq, Lk, Lk))
    scale = 0.125 / (s * s)
    ref = _attn_ref(Q, K, V, H, scale, split)
    pk = [_pack(L, _dev(t).view(-1, D), e) for t in (Q, K, V)]
    vmax = float(ref.abs().max())
    out = torch.full((B * Lq, D), float("nan"), device="cuda")
    assert L.artalk_op_attention_ex(_p(pk[0]), _p(pk[1]), _p(pk[2]), _p(out), B, H, 64, Lq, Lk, scale, 2 | 4, None, split, e, oe, 0, None, None) == 0
    torch.cuda.synchronize()
    err = float((out.cpu().double() - ref.view(-1, D)).abs().max())
    assert err < 2e-5 * vmax, (err, vmax)
    outp = _i32(B * Lq, D, 8)
    st = _status()
    assert L.artalk_op_attention_ex(_p(pk[0]), _p(pk[1]), _p(pk[2]), _p(outp), B, H, 64, Lq, Lk, scale, 2 | 4, None, split, e, oe, 1, _p(st), None) == 0
    assert _st(st) == 0 and bool((outp[B * Lq:] == CANARY).all())
    _assert_stored(_unpack(outp[:B * Lq], oe), ref.view(-1, D), oe, 2e-5 * vmax, "attention out_p8")
    assert np.array_equal(outp[:B * Lq].cpu().numpy(), p8.pack(out.cpu().numpy(), oe)), "out_p8 stores the fp32 result packed at o_exp"


def _same_keys(B, Lq, Lk, D, n_same, seed):
    """Q and K whose softmax is exactly uniform over the first n_same keys: every query is 4 k0 and the first n_same keys are 4 k0
    (equal scores, p = exp(0) = 1 each), the other keys are -4 k0, whose scores lie 2 * 0.125 * 16 |k0|^2 ~ 250 per head below: p = 0.
    With n_same a power of two, O = n_same * v / n_same = v exactly while the sums stay integers times a power of two."""
    k0 = torch.randn(B, 1, D, generator=torch.Generator().manual_seed(seed)) * 4
    K = k0.expand(B, Lk, D).clone()
    K[:, n_same:] *= -1
    return k0.expand(B, Lq, D).contiguous(), K


# the shapes of P8_ATTN with 64 equal keys, and the ping-pong shape (it needs more than 128 keys): 128 equal keys + 64 with p = 0
GUARD_ATTN = [(2, 8, 100, 64, 0, 64), (3, 16, 199, 64, 0, 64), (2, 8, 200, 64, 32, 64), (20, 16, 199, 64, 0, 64), (40, 16, 199, 192, 0, 128)]


@pytest.mark.parametrize("e", EXPS)
@pytest.mark.parametrize("B,H,Lq,Lk,split,n_same", GUARD_ATTN)
def test_attention_guard_threshold(B, H, Lq, Lk, split, n_same, e):
    """Equal keys (_same_keys; with the decoder mask the first 32 queries see 32 of them): O = v exactly, so the exact threshold reaches
    the store of every P8-input kernel, the ping-pong kernel included.  The values above it: the sum cannot carry a one-ulp excess, so the
    next value the P8 input can hold (65504 + 64 at the scale of o_exp, fed at qkv_exp = o_exp - 1), inf and NaN."""
    capi, L = _lib()
    D = H * 64
    top = float(p8.max_value(e))
    Q, K = _same_keys(B, Lq, Lk, D, n_same, e + 9)

    def run(v, qe):
        V = torch.full((B, Lk, D), 1.0 / 2.0 ** e)
        V[:, :n_same, 70] = v
        pk = [_pack(L, _dev(t).view(-1, D), qe) for t in (Q, K, V)]
        outp = _i32(B * Lq, D, 8)
        st = _status()
        assert L.artalk_op_attention_ex(_p(pk[0]), _p(pk[1]), _p(pk[2]), _p(outp), B, H, 64, Lq, Lk, 0.125, 2 | 4, None, split, qe, e, 1, _p(st), None) == 0
        s = _st(st)
        assert bool((outp[B * Lq:] == CANARY).all())
        return s, outp[:B * Lq]

    s, outp = run(top, e)
    assert s == 0 and _hi_finite(outp)
    got = _unpack(outp, e)
    assert bool((got[:, 70] == top).all()) and bool((got[:, 71] == 1.0 / 2.0 ** e).all())
    bad = [("inf", float("inf"), e), ("nan", float("nan"), e)]
    if e > -8:
        bad.append(("65504 + 64", top * (1 + 2.0 ** -10), e - 1))
    for what, v, qe in bad:
        assert run(v, qe)[0] == 8, (what, e)


# fp32 Q, K, V rows (B, H, Lq, Lk, l2norm, split): the AR decoder's attention - L2-normalised q and k with a per-head scale, O written in
# P8 - on attention_short_kernel (scale steps 0 - 3), attention_f16_wide_ar_kernel (the 100-token step) and, with the decoder mask,
# attention_f16_kernel without P8 inputs.  These kernels split the fp32 rows UNSCALED (|v| <= 65504 whatever o_exp is).
F32_ATTN = [(2, 12, 1, 182, 1, 0), (2, 12, 5, 187, 1, 0), (2, 12, 25, 212, 1, 0), (2, 12, 50, 262, 1, 0), (2, 12, 100, 362, 1, 0),
            (2, 8, 200, 200, 0, 100)]


def _f32_attn_ref(Q, K, V, H, qs, scale, split):
    B, Lq, D = Q.shape
    q, k = (t.view(B, -1, H, 64).transpose(1, 2).double() for t in (Q, K))
    if qs is not None:
        q = F.normalize(q, dim=-1) * qs.double().view(1, H, 1, 1)
        k = F.normalize(k, dim=-1)
    Qn, Kn = (t.transpose(1, 2).reshape(B, -1, D) for t in (q, k))
    return _attn_ref(Qn, Kn, V, H, scale, split)


@pytest.mark.parametrize("e", EXPS)
@pytest.mark.parametrize("B,H,Lq,Lk,l2norm,split", F32_ATTN)
def test_attention_f32_rows_p8_output(B, H, Lq, Lk, l2norm, split, e):
    """O at o_exp = e from fp32 rows, values near the top of what both o_exp and the unscaled fp16 split can hold, against float64; the
    P8 result is the fp32 result packed at o_exp."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(Lq * 1000 + Lk + e)
    D = H * 64
    Q, K = torch.randn(B, Lq, D, generator=g), torch.randn(B, Lk, D, generator=g)
    V = torch.randn(B, Lk, D, generator=g) * min(_sigma(e), 8000.0)
    qs = (torch.rand(H, generator=g) * 4 + 1) if l2norm else None
    scale = 1.0 if l2norm else 512 ** -0.5
    ref = _f32_attn_ref(Q, K, V, H, qs, scale, split).reshape(-1, D)
    vmax = float(ref.abs().max())
    assert vmax < float(p8.max_value(e))
    dQ, dK, dV = _dev(Q), _dev(K), _dev(V)
    dqs = _dev(qs) if l2norm else None
    out = torch.full((B * Lq, D), float("nan"), device="cuda")
    assert L.artalk_op_attention_ex(_p(dQ), _p(dK), _p(dV), _p(out), B, H, 64, Lq, Lk, scale, l2norm | 2, _p(dqs), split, OTHER[e], e, 0, None, None) == 0
    torch.cuda.synchronize()
    err = float((out.cpu().double() - ref).abs().max())
    assert err < 2e-5 * vmax, (err, vmax)
    outp = _i32(B * Lq, D, 8)
    st = _status()
    assert L.artalk_op_attention_ex(_p(dQ), _p(dK), _p(dV), _p(outp), B, H, 64, Lq, Lk, scale, l2norm | 2, _p(dqs), split, OTHER[e], e, 1, _p(st), None) == 0
    assert _st(st) == 0 and bool((outp[B * Lq:] == CANARY).all())
    _assert_stored(_unpack(outp[:B * Lq], e), ref, e, 2e-5 * vmax, "attention out_p8 from fp32 rows")
    assert np.array_equal(outp[:B * Lq].cpu().numpy(), p8.pack(out.cpu().numpy(), e)), "out_p8 stores the fp32 result packed at o_exp"


@pytest.mark.parametrize("e", EXPS)
@pytest.mark.parametrize("B,H,Lq,l2norm,split", [(2, 12, 1, 1, 0), (2, 12, 50, 1, 0), (2, 12, 100, 1, 0), (2, 8, 200, 0, 64)])
def test_attention_f32_rows_guard_threshold(B, H, Lq, l2norm, split, e):
    """128 equal keys (64 seen under the mask): O = v exactly.  The fp32 rows are split unscaled, so v itself is bounded by 65504: where
    the threshold 65504 / 2^e lies inside that (e >= 0) it is fed exactly (status 0, stored exactly) and exceeded by one part in 1024
    (bit 3); at e < 0 the largest value the kernel can carry, 65504, is inside the range (status 0).  inf and NaN: bit 3 at every e."""
    capi, L = _lib()
    D, Lk = H * 64, 128
    g = torch.Generator().manual_seed(e + 31)
    Q = torch.randn(B, Lq, D, generator=g)
    K = torch.randn(B, 1, D, generator=g).expand(B, Lk, D).contiguous()
    dqs = _dev(torch.rand(H, generator=g) * 4 + 1) if l2norm else None
    scale = 1.0 if l2norm else 512 ** -0.5
    top = float(p8.max_value(e))
    small = min(1.0 / 2.0 ** e, 1.0)

    def run(v):
        V = torch.full((B, Lk, D), small)
        V[:, :, 70] = v
        outp = _i32(B * Lq, D, 8)
        st = _status()
        assert L.artalk_op_attention_ex(_p(_dev(Q)), _p(_dev(K)), _p(_dev(V)), _p(outp), B, H, 64, Lq, Lk, scale, l2norm | 2, _p(dqs), split, 4, e, 1,
                                        _p(st), None) == 0
        s = _st(st)
        assert bool((outp[B * Lq:] == CANARY).all())
        return s, outp[:B * Lq]

    v = min(top, 65504.0)
    s, outp = run(v)
    assert s == 0 and _hi_finite(outp)
    got = _unpack(outp, e)
    assert bool((got[:, 70] == v).all()) and bool((got[:, 71] == small).all())
    bad = [("inf", float("inf")), ("nan", float("nan"))]
    if e >= 0:
        bad.append(("one part in 1024 above", top * (1 + 2.0 ** -10)))
    for what, v in bad:
        assert run(v)[0] == 8, (what, e)


# ------------------------------------------------------------------------------------------------------------------ positional conv
def _posconv_ref(X, w, bias, T, Ts, act):
    """X [C * Ts, 1024] (frames t < T of a chunk valid), w [1024, 64, 128] as torch's grouped Conv1d holds it -> [C * Ts, 1024] float64:
    X + act(conv(X)) at frames t < T (hf Wav2Vec2PositionalConvEmbedding: padding 64, the last output frame dropped)."""
    C = X.shape[0] // Ts
    x = X.double().view(C, Ts, 1024)[:, :T].transpose(1, 2)
    y = F.conv1d(x, w.double(), bias.double(), padding=64, groups=16)[:, :, :T]
    if act == 1:
        y = F.gelu(y)
    return (x + y).transpose(1, 2)


def _posconv_weight(L, w):
    return _pack_w(L, _dev(w.permute(0, 2, 1).reshape(1024, 128 * 64)))      # k = tap * 64 + input channel


@pytest.mark.parametrize("e", EXPS)
def test_posconv_p8_exponent_and_guard(e):
    """launch_posconv_p8 (the "w2v.posconv.input(fp32 A)" site): the fp32 window is split with 2^a_exp while it is staged into LDS and the
    result unscaled again.  Input near the top of the range of e against float64; small integers bit-identical to the result at 4;
    guard at exactly 65504 / 2^e, the next float, inf and NaN; inf in a padding frame (t >= T) is not read."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(60 + e)
    C_, T, Ts = 2, 199, 200
    w = torch.randn(1024, 64, 128, generator=g) / math.sqrt(64 * 128)
    bias = torch.randn(1024, generator=g) * _sigma(e)
    X = torch.randn(C_ * Ts, 1024, generator=g) * _sigma(e)
    top = float(p8.max_value(e))
    X[17, 333] = top
    X.view(C_, Ts, 1024)[:, T:] = float("inf")            # the padding frame of every chunk
    Wp, db = _posconv_weight(L, w), _dev(bias)
    ref = _posconv_ref(X, w, bias, T, Ts, 1)

    def run(Xd, Wp_, b_, act, ae):
        out = torch.full((C_ * Ts + 8, 1024), float("nan"), device="cuda")
        st = _status()
        assert L.artalk_op_posconv_p8_ex(_p(Xd), _p(Wp_), _p(b_), _p(Xd), _p(out), C_, T, Ts, act, ae, _p(st), None) == 0
        s = _st(st)
        assert bool(torch.isnan(out[C_ * Ts:]).all())
        return s, out[:C_ * Ts].cpu().view(C_, Ts, 1024)[:, :T]

    s, out = run(_dev(X), Wp, db, 1, e)
    assert s == 0
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    assert err < 2e-6, err
    for what, v in _bad_values(e):
        Y = X.clone()
        Y[C_ * Ts - 30, 700] = v
        assert run(_dev(Y), Wp, db, 1, e)[0] == 8, (what, e)
    # exactly representable inputs: bit for bit the result at exponent 4, and the exact sums
    Xi = torch.randint(-4, 5, (C_ * Ts, 1024), generator=g).float() * 2.0 ** min(0, 4 - e)
    wi = torch.randint(-2, 3, (1024, 64, 128), generator=g).float() / 2
    bi = torch.randint(-8, 9, (1024,), generator=g).float()
    Wi, dbi, dXi = _posconv_weight(L, wi), _dev(bi), _dev(Xi)
    want = _posconv_ref(Xi, wi, bi, T, Ts, 0)
    assert float(want.abs().max()) < 2 ** 20
    s4, o4 = run(dXi, Wi, dbi, 0, 4)
    se, oe = run(dXi, Wi, dbi, 0, e)
    assert s4 == 0 and se == 0 and torch.equal(oe, o4) and torch.equal(oe.double(), want)


# ------------------------------------------------------------------------------------------------------------------ conv0, pool + SiLU
@pytest.mark.parametrize("e", EXPS)
def test_w2v_front_p8_output(e):
    """conv0 + LayerNorm + GELU written in P8: the LayerNorm gain puts the output near the top of the range of e; then the guard at
    exactly 65504 / 2^e, the next float, inf and NaN."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(3)
    Cn, n = 2, 16000
    audio = torch.randn(Cn, n, generator=g) * 0.1
    w = torch.randn(512, 1, 10, generator=g) / math.sqrt(10)
    b = torch.randn(512, generator=g) * 0.3
    lw = (1 + 0.1 * torch.randn(512, generator=g)) * _sigma(e) / 2
    lb = 0.1 * torch.randn(512, generator=g)
    xn = (audio.double() - audio.double().mean(-1, keepdim=True)) / (audio.double().std(-1, keepdim=True) + 1e-6)
    h = F.conv1d(xn[:, None], w.double(), b.double(), stride=5).transpose(1, 2)
    ref = F.gelu(F.layer_norm(h, (512,), lw.double(), lb.double(), 1e-5))
    T = ref.shape[1]
    assert float(ref.abs().max()) < float(p8.max_value(e))
    da, dw, db, dlb = _dev(audio), _dev(w.view(512, 10)), _dev(b), _dev(lb)
    dxn = torch.empty(Cn, n, device="cuda")

    def run(gain):
        out = _i32(Cn * T, 512, 8)
        st = _status()
        assert L.artalk_op_w2v_front_ex(_p(da), Cn, n, _p(dw), _p(db), _p(_dev(gain)), _p(dlb), _p(dxn), _p(out), 1, e, _p(st), None) == 0
        return _st(st), out

    s, out = run(lw)
    assert s == 0 and bool((out[Cn * T:] == CANARY).all())
    _assert_stored(_unpack(out[:Cn * T], e), ref.reshape(-1, 512), e, 5e-5 * float(ref.abs().max()) / 4.0, "conv0")
    # guard threshold, exact construction: the kernel computes gelu(fma(normalised, gain, shift)), so a zero gain makes the value before
    # the GELU the shift itself, and GELU(x) = x * Phi(x) is x for x >= 4094 (Phi rounds to 1): channel 300 of every frame holds the value
    top = float(p8.max_value(e))
    for what, v in [("top", top)] + _bad_values(e):
        shift = torch.ones(512) / 2.0 ** e
        shift[300] = v
        out = _i32(Cn * T, 512, 8)
        st = _status()
        assert L.artalk_op_w2v_front_ex(_p(da), Cn, n, _p(dw), _p(db), _p(_dev(torch.zeros(512))), _p(_dev(shift)), _p(dxn), _p(out), 1, e, _p(st),
                                        None) == 0
        assert _st(st) == (0 if what == "top" else 8), (what, e)
        assert bool((out[Cn * T:] == CANARY).all())
        if what == "top":
            assert _hi_finite(out[:Cn * T]) and bool((_unpack(out[:Cn * T], e)[:, 300] == top).all())


@pytest.mark.parametrize("e", EXPS)
def test_pool_silu_p8_output_and_guard(e):
    """Area pooling + SiLU written in P8.  Guard: a constant column pools to itself exactly (sums of up to 199 equal 12-bit values
    are exact in fp32) and SiLU(x) = x / (1 + exp(-x)) is x itself once exp(-x) vanishes, so 65504 / 2^e arrives unchanged."""
    capi, L = _lib()
    g = torch.Generator().manual_seed(4)
    X = torch.randn(2, 199, 1024, generator=g) * _sigma(e)
    xt = X.double().permute(0, 2, 1)
    ref = F.silu(torch.cat([F.interpolate(xt, size=(p), mode="area").permute(0, 2, 1) for p in (1, 5, 25, 50, 100)], dim=1)).reshape(-1, 1024)
    out = _i32(2 * 181, 1024, 8)
    st = _status()
    assert L.artalk_op_pool_silu_ex(_p(_dev(X)), 2, 199, 1024, _p(out), 1, e, _p(st), None) == 0
    assert _st(st) == 0 and bool((out[2 * 181:] == CANARY).all())
    _assert_stored(_unpack(out[:2 * 181], e), ref, e, 2e-6 * float(ref.abs().max()), "pool_silu")
    top = float(p8.max_value(e))
    for what, v in [("top", top)] + _bad_values(e):      # (top >= 4094 at every exponent: exp(-top) == 0 in fp32)
        Y = torch.ones(2, 199, 1024)
        Y[1, :, 333] = v
        st = _status()
        assert L.artalk_op_pool_silu_ex(_p(_dev(Y)), 2, 199, 1024, _p(out), 1, e, _p(st), None) == 0
        assert _st(st) == (0 if what == "top" else 8), (what, e)
        if what == "top":
            assert bool((_unpack(out[181:362], e)[:, 333] == top).all())
