"""The DINO depth cases without a GPU (tests/dino_depth_cases.py): whether the bar of tests/test_dino_depth_ops_gpu.py can be met at all
by a float32 kernel (the two sum orders of gemm_f32_kernel, emulated), whether the bar tells each wrong reading of a form from the right
one, and that the entry points the GPU file calls refuse a NULL pointer and a K that is no multiple of 32 before they touch the device.
Run with -s for the figures."""
import ctypes as C

import pytest
import torch

import dino_depth_cases as dc
from artalk_amd import capi


@pytest.mark.parametrize("M", list(dc.GEMM_MS))
def test_blocked_sums_meet_the_bar_at_k_3072(M):
    """fc2, the one form at K = 3072: one float32 chain over the whole of K against 256-deep chains added up, each finished by the form's
    epilogue in float32 and held against the float64 oracle.  Only the blocked order is asserted: that it stays inside the allowance is
    what makes the bar attainable; the one-chain ratio is printed as the expectation for the kernel as it stands."""
    for seed in dc.SEEDS:
        c = dc.case("fc2", M, seed)
        want, e32, allow = dc.bar(c)
        ratio = {}
        for name, block in (("one chain", 0), ("blocked", dc.BLOCK)):
            got = dc.epilogue(c, dc.emulate_sums(c, block), torch.float32)
            ratio[name] = float((got.double() - want).abs().max()) / e32
        print(f"fc2 M {M} seed {seed}: e32 {e32:.2e}, allowance {allow / e32:.2f} x e32; one chain over K = 3072 {ratio['one chain']:.2f} x e32, "
              f"{dc.BLOCK}-deep blocks added up {ratio['blocked']:.2f} x e32")
        assert ratio["blocked"] * e32 <= allow


def _variant_cases(form):
    if form == "attention":
        return [dc.case("attention", T, 0) for T in dc.ATTN_LS]
    return [dc.case(form, M, 0) for M in dc.GEMM_MS]


@pytest.mark.parametrize("which,form", [(w, f) for w, forms in dc.VARIANTS.items() for f in forms])
def test_a_wrong_reading_leaves_the_allowance(which, form):
    for c in _variant_cases(form):
        want, e32, allow = dc.bar(c)
        off = float((dc.reference(c, torch.float64, which) - want).abs().max())
        print(f"{which}, {c}: off by {off:.2e} = {off / allow:.1e} x the allowance ({allow:.2e})")
        assert off > 2 * allow


def test_an_unwritten_output_of_an_in_place_form_leaves_the_allowance():
    """proj and fc2 write over their residual, so their output buffer cannot be pre-filled with NaN: a value the kernel leaves out is
    the residual itself.  Such a value misses the oracle by the whole gated term.  The kernel stores runs of 4 columns: in every case
    every such run holds a term far above the bar (and all but a few of the single elements are above it)."""
    for form, M, seed in dc.gemm_cases():
        c = dc.case(form, M, seed)
        if c.gated:
            want, e32, allow = dc.bar(c)
            term = (c.R.double() - want).abs()
            assert float(term.reshape(M, dc.N // 4, 4).max(dim=-1).values.min()) > 100 * allow, c
            assert int((term <= allow).sum()) <= 2, c


def test_the_yardstick_is_sound():
    """e32 of every case is a float32 rounding level for values of order 1 to 10, neither zero nor a sign of a wrong statement."""
    for f, M, s in dc.gemm_cases():
        want, e32, allow = dc.bar(dc.case(f, M, s))
        assert 1e-8 < e32 < 5e-6 and 0.5 < float(want.abs().max()) < 20, (f, M, s, e32)
    c = dc.case("attention", dc.ATTN_LS[0], 0)
    want, e32, allow = dc.bar(c)
    s = (c.qkv[:, :64].double() @ c.qkv[:, dc.ATTN_D:dc.ATTN_D + 64].double().t()) * dc.ATTN_SCALE
    assert 1.7 < float(s.std()) < 2.3 and 1e-9 < e32 < 5e-6


def test_entry_points_refuse_before_the_device():
    """artalk_op_gemm, artalk_op_gemm_rows, artalk_op_attention_rows and artalk_op_attention_plan as the GPU file calls them, with host
    pointers that are never dereferenced: the refusal comes first."""
    L = capi.lib()
    x = torch.zeros(64)
    p = capi.ptr(x)
    M, K = 26, 768
    for gemm in (L.artalk_op_gemm, L.artalk_op_gemm_blocked):
        assert gemm(None, K, p, p, p, p, p, M, dc.N, K, 0, None) == capi.EINVAL
        assert gemm(p, K, None, p, p, p, p, M, dc.N, K, 0, None) == capi.EINVAL
        assert gemm(p, K, p, p, p, p, None, M, dc.N, K, 0, None) == capi.EINVAL
        assert gemm(p, K + 8, p, p, p, p, p, M, dc.N, K + 8, 0, None) == capi.EINVAL      # 776 = 8 * 97
        assert gemm(p, 600, p, p, None, None, p, M, dc.N, 600, 0, None) == capi.EINVAL    # the patch embedding unpadded: 588 + 12

    def rows(**kw):
        a = dict(mode=0, M=9, N=dc.N, K=dc.SPLITK_K, A=x.data_ptr(), lda=dc.SPLITK_K, a_elems=9 * dc.SPLITK_K, W=x.data_ptr(), ldw=dc.SPLITK_K,
                 w_elems=dc.N * dc.SPLITK_K, bias=x.data_ptr(), bias_elems=dc.N, C=x.data_ptr(), ldc=dc.N, c_elems=9 * dc.N, splitk=dc.SPLITK_S)
        a.update(kw)
        return L.artalk_op_gemm_rows(C.byref(capi.GemmRowsArgs(**a)), None)
    assert L.artalk_op_gemm_rows(None, None) == capi.EINVAL
    for name in ("A", "W", "C"):
        assert rows(**{name: None}) == capi.EINVAL
    assert rows(K=dc.SPLITK_K + 16, lda=dc.SPLITK_K + 16, ldw=dc.SPLITK_K + 16) == capi.EINVAL
    assert rows(c_elems=9 * dc.N - 1) == capi.EINVAL and rows(a_elems=9 * dc.SPLITK_K - 1) == capi.EINVAL
    # the same arguments without a defect are accepted, and planned as the GPU file asserts: 32 x 128 tiles, 8 slabs
    assert L.artalk_op_rows_dry_run(1) == 0
    try:
        used = [C.c_int32(-7), C.c_int32(-7)]
        assert rows(used_cfg=C.pointer(used[0]), used_splitk=C.pointer(used[1])) == capi.OK
        assert (used[0].value, used[1].value) == (3, dc.SPLITK_S)
    finally:
        assert L.artalk_op_rows_dry_run(0) == 0

    T, ld = 130, 3 * dc.ATTN_D
    n = (T - 1) * ld + dc.ATTN_D

    def attn(Q=p, K=p, V=p, O=p):
        return L.artalk_op_attention_rows(Q, K, V, O, 1, dc.ATTN_H, dc.ATTN_HD, T, T, dc.ATTN_SCALE, 0, None, 0, 4, 4, 0, None, ld, ld, ld, dc.ATTN_D,
                                          T * ld, T * ld, T * ld, T * dc.ATTN_D, n, n, n, T * dc.ATTN_D, None)
    for k in ("Q", "K", "V", "O"):
        assert attn(**{k: None}) == capi.EINVAL
    assert L.artalk_op_attention_plan(1, dc.ATTN_H, 48, T, T, 0, 0, 0, 256) == capi.EINVAL
    assert L.artalk_op_attention_plan(1, dc.ATTN_H, dc.ATTN_HD, T, 0, 0, 0, 0, 256) == capi.EINVAL
    for T in dc.ATTN_LS:
        assert L.artalk_op_attention_plan(1, dc.ATTN_H, dc.ATTN_HD, T, T, 0, 0, 0, 256) == capi.ATTN_F32_64
