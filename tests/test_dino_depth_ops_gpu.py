"""The GEMM and attention forms of dino.hip at the depths of the ViT-B checkpoint (tests/dino_depth_cases.py), one kernel launch each
through the entry points the suite already launches at these sizes: artalk_op_gemm and artalk_op_gemm_blocked (the sum order of the DINO
launches) for the five GEMM forms on the fp32 tiles of M = 26 and M = 82, artalk_op_gemm_rows for K = 9216 in eight slabs finished by the fixed-order reduce, artalk_op_attention_rows for 12 heads over 130,
257 and 1370 keys read out of one fused q|k|v buffer.  No DINO object is built here.  The bar is the head's rule for a float32 kernel:
max-abs error <= 4 x e32, e32 being torch's float32 CPU evaluation against its float64 one, with a floor of one float32 ulp
(dino_cases.allowance).  Every output lies between poisoned guard bands that must stay poisoned and starts as NaN - or, where the form
adds into its residual in place, as that residual (tests/test_dino_depth_cpu.py shows that the bar catches a value left unwritten).
Run with -s for error / e32 of every case."""
import ctypes as C

import pytest
import torch

import dino_depth_cases as dc
from artalk_amd import capi
from test_dino_ops_gpu import GUARD, _guarded, _payload, _s

pytestmark = pytest.mark.gpu


def _dev(t, *shape):
    """A CPU tensor on the device, checked to be the dense float32 array of that shape the entry point will be told it is."""
    assert t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()
    d = t.cuda()
    assert d.data_ptr() % 16 == 0 and d.numel() == t.numel()
    return d


def _judge(c, got, what):
    want, e32, allow = dc.bar(c)
    err = float((got.double().reshape(want.shape) - want).abs().max())
    print(f"{what}: error {err:.2e}, e32 {e32:.2e}, error / e32 {err / e32:.2f}, allowance {allow:.2e}")
    assert err <= allow, (what, err / e32)


def _planned_cfg(M, K):
    """What plan_gemm makes of an unsplit fp32 launch of this shape (gemm_config, the function launch_gemm asks), without a device."""
    L = capi.lib()
    used = C.c_int32(-7)
    a = capi.GemmRowsArgs(mode=0, M=M, N=dc.N, K=K, A=1 << 26, lda=K, a_elems=M * K, W=2 << 26, ldw=K, w_elems=dc.N * K, C=3 << 26, ldc=dc.N,
                          c_elems=M * dc.N, used_cfg=C.pointer(used))
    assert L.artalk_op_rows_dry_run(1) == 0
    try:
        assert L.artalk_op_gemm_rows(C.byref(a), None) == capi.OK
    finally:
        assert L.artalk_op_rows_dry_run(0) == 0
    return used.value


@pytest.mark.parametrize("seed", dc.SEEDS)
@pytest.mark.parametrize("M", list(dc.GEMM_MS))
@pytest.mark.parametrize("form", list(dc.GEMM_FORMS))
def test_gemm_form(form, M, seed):
    """The kernel DnRun::gemm launches - artalk_op_gemm_blocked: GemmArgs::ksum_blocks on, K summed in blocks of 256 - is held to the bar.
    The same launch with one chain over K (artalk_op_gemm, what every other caller runs) is measured beside it and only printed: at
    K = 3072 it is outside this bar ("DINO features"), which is why the DINO launches sum in blocks.  That the two results
    differ in some bit shows that the entry point reached the other kernel."""
    c = dc.case(form, M, seed)
    K, N = c.K, dc.N
    assert K % 32 == 0 and _planned_cfg(M, K) == dc.GEMM_MS[M]
    A, W, bias = _dev(c.A, M, K), _dev(c.W, N, K), _dev(c.bias, N)
    gate = _dev(c.gate, M, N) if c.gated else None      # a full [M][N] matrix of pitch N
    L = capi.lib()
    got = {}
    for name, entry in (("one chain", L.artalk_op_gemm), ("blocks of 256", L.artalk_op_gemm_blocked)):
        buf = _guarded(M * N)
        out = buf[GUARD:GUARD + M * N]
        R = None
        if c.gated:
            out.copy_(_dev(c.R, M, N).reshape(-1))
            R = capi.ptr(out)      # the residual in place: R = C, pitch N
        assert out.numel() == M * N and out.data_ptr() % 16 == 0 and buf.numel() == M * N + 2 * GUARD
        assert entry(capi.ptr(A), K, capi.ptr(W), capi.ptr(bias), capi.ptr(gate), R, capi.ptr(out), M, N, K, c.act, _s()) == capi.OK
        got[name] = _payload(buf, M * N, entry.__name__)
    want, e32, allow = dc.bar(c)
    print(f"{form} K {K} M {M} seed {seed}, one chain over K: error / e32 {float((got['one chain'].double().reshape(M, N) - want).abs().max()) / e32:.2f}")
    assert not torch.equal(got["one chain"], got["blocks of 256"])
    _judge(c, got["blocks of 256"], f"{form} K {K} M {M} seed {seed}, blocks of 256")


@pytest.mark.parametrize("seed", dc.SEEDS)
@pytest.mark.parametrize("M", dc.SPLITK_MS)
def test_splitk_form(M, seed):
    """K = 9216 in 8 slabs of 36 K-steps, one chain per slab, the slabs added in slab order by splitk_reduce_kernel<8> with the bias:
    artalk_op_gemm_rows in its fp32 mode with identity row maps and dense pitches is that launch pair."""
    c = dc.case("splitk", M, seed)
    K, N, S = c.K, dc.N, dc.SPLITK_S
    assert K == dc.SPLITK_K and K % (32 * S) == 0
    A, W, bias = _dev(c.A, M, K), _dev(c.W, N, K), _dev(c.bias, N)
    buf = _guarded(M * N)
    out = buf[GUARD:GUARD + M * N]
    used = [C.c_int32(-7) for _ in range(3)]
    a = capi.GemmRowsArgs(mode=0, M=M, N=N, K=K, A=A.data_ptr(), lda=K, a_elems=A.numel(), W=W.data_ptr(), ldw=K, w_elems=W.numel(),
                          bias=bias.data_ptr(), bias_elems=bias.numel(), C=out.data_ptr(), ldc=N, c_elems=out.numel(), splitk=S,
                          used_cfg=C.pointer(used[0]), used_splitk=C.pointer(used[1]), fused_ln=C.pointer(used[2]))
    assert (A.numel(), W.numel(), bias.numel(), out.numel()) == (M * K, N * K, N, M * N)
    assert capi.lib().artalk_op_gemm_rows(C.byref(a), _s()) == capi.OK
    assert (used[0].value, used[1].value, used[2].value) == (3, S, 0)      # 32 x 128 tiles (M <= 32), 8 slabs, the plain reduce
    _judge(c, _payload(buf, M * N, "artalk_op_gemm_rows"), f"splitk K {K} / {S} M {M} seed {seed}")


@pytest.mark.parametrize("seed", dc.SEEDS)
@pytest.mark.parametrize("T", dc.ATTN_LS)
def test_attention_form(T, seed):
    """q, k and v at columns 0, 768 and 1536 of one [T][2304] buffer, as DnRun::run hands the q|k|v GEMM's rows to launch_attention."""
    c = dc.case("attention", T, seed)
    H, HD, D = dc.ATTN_H, dc.ATTN_HD, dc.ATTN_D
    ld = 3 * D
    assert capi.lib().artalk_op_attention_plan(1, H, HD, T, T, 0, 0, 0, 256) == capi.ATTN_F32_64, "Lq = Lk > 64 plans attention_kernel<64>"
    qkv = _dev(c.qkv, T, ld)
    n = (T - 1) * ld + D      # from the first element of q, k or v to the last one read
    assert 2 * D + n == qkv.numel()
    buf = _guarded(T * D)
    out = buf[GUARD:GUARD + T * D]
    assert out.numel() == T * D and out.data_ptr() % 16 == 0
    base = qkv.data_ptr()
    rc = capi.lib().artalk_op_attention_rows(base, base + 4 * D, base + 8 * D, capi.ptr(out), 1, H, HD, T, T, dc.ATTN_SCALE, 0, None, 0, 4, 4, 0, None,
                                             ld, ld, ld, D, T * ld, T * ld, T * ld, T * D, n, n, n, T * D, _s())
    assert rc == capi.OK
    _judge(c, _payload(buf, T * D, "artalk_op_attention_rows"), f"attention {H} x {HD}, {T} keys, seed {seed}")
