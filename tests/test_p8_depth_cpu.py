"""The case table of tests/test_p8_depth_gpu.py without a GPU: every launch of that file passes the argument checks of artalk_op_gemm_rows
as it stands (artalk_op_rows_dry_run: ARTALK_OK where the device would first be touched) and would run as itself - the forced
configuration and split come back in used_cfg / used_splitk, so no case can silently test another kernel.  Beside it the checks this
table relies on: the cus field of artalk_op_gemm_rows_args and the split factor artalk_op_gemm_f16s_packed_ex takes."""
import ctypes as C

import pytest

from artalk_amd import capi
from artalk_amd.capi import GemmRowsArgs
from test_p8_depth_gpu import ALL, CASES, DEPTHS, RING, SPLIT, geometry, rows_args, select

P = 1 << 26       # 64 MiB apart: no two of the dummy buffers below overlap; never dereferenced
PTR = dict(A=P, W=2 * P, bias=3 * P, C=4 * P, gate=5 * P, status=6 * P, Y=7 * P, mod=8 * P)
KINDS = sorted({c.kind for c in CASES})


@pytest.fixture
def dry():
    L = capi.lib()
    assert L.artalk_op_rows_dry_run(1) == 0
    yield L
    assert L.artalk_op_rows_dry_run(0) == 0


def test_the_table_covers_what_it_claims():
    assert KINDS == ["edge", "epi", "guard", "ident", "ln", "split", "sweep", "wrap", "wrap_small"]
    for cfg in ALL:
        assert {c.nk for c in select("sweep", cfg=cfg)} == set(DEPTHS)
        assert {c.nk for c in select("edge", cfg=cfg)} == {1, RING[cfg] + 1}
        assert {c.nk for c in select("epi", cfg=cfg, epi="res")} == {1, 4, 5, 9}
    for cfg in SPLIT:
        assert {(c.S, c.nk - c.S) for c in select("split", cfg=cfg) if c.nk != 17} == {(S, d) for S in (2, 3, 4, 5, 6, 8) for d in (0, 1)}
    assert {c.S for c in select("ln")} == {2, 3, 4, 6, 8} and all(c.N == 768 for c in select("ln"))
    assert {(c.cfg, c.cus) for c in select("wrap")} == {(cfg, cus) for cfg in (7, 12, 8) for cus in (8, 0)}
    assert len(set(CASES)) == len(CASES)


@pytest.mark.parametrize("cfg", ALL)
@pytest.mark.parametrize("kind", KINDS)
def test_every_case_is_accepted_and_runs_as_itself(dry, kind, cfg):
    cases = select(kind, cfg=cfg)
    if not cases:
        assert kind in ("split", "ln", "wrap", "wrap_small")      # kinds that exist for some configurations only
        return
    for c in cases:
        a, used = rows_args(capi, c, PTR)
        assert dry.artalk_op_gemm_rows(C.byref(a), None) == capi.OK, c
        assert (used[0].value, used[1].value) == (c.cfg, c.S), (c, used[0].value, used[1].value)
        assert used[2].value == c.ln, c
        # the sizes are exactly sufficient: one element less of A or C is refused
        for f in ("a_elems", "c_elems"):
            setattr(a, f, geometry(c)[f] - 1)
            assert dry.artalk_op_gemm_rows(C.byref(a), None) == capi.EINVAL, (c, f)
            setattr(a, f, geometry(c)[f])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_cus_is_a_mode_1_field(dry, mode):
    """a CU partition sizes the grid of the persistent f16x3 kernels: negative, or given to the fp32 / bf16 families, it is refused"""
    def call(**kw):
        a = GemmRowsArgs(mode=mode, M=64, N=64, K=64, A=P, lda=64, a_elems=64 * 64, W=2 * P, ldw=64, w_elems=64 * 64, C=3 * P, ldc=64,
                         c_elems=64 * 64, **kw)
        return dry.artalk_op_gemm_rows(C.byref(a), None)
    assert call() == capi.OK and call(cus=0) == capi.OK
    assert call(cus=-1) == capi.EINVAL and call(cus=-8) == capi.EINVAL
    for cus in (1, 8, 12, 256, 4096):      # (rounded to a multiple of 8 and clamped to [8, the device's count] by the launcher)
        assert call(cus=cus) == (capi.OK if mode == 1 else capi.EINVAL), (mode, cus)
    if mode == 1:
        for cfg in ALL:
            u = C.c_int32(-7)
            assert call(cus=8, force_cfg=cfg, used_cfg=C.pointer(u)) == capi.OK and u.value == (8 if cfg in (7, 12) else cfg)      # N = 64: no 256-column tile


def test_packed_gemm_refuses_a_split_that_leaves_a_slice_empty():
    """bits 8-15 of force_cfg above K / 32: a workgroup would own no K step.  Refused before anything is allocated or launched (the
    pointers are never dereferenced); artalk_op_gemm_rows refuses the same"""
    L = capi.lib()
    vp = C.c_void_p
    for cfg in SPLIT:
        for K, S in ((64, 3), (32, 2), (256, 9), (512, 255)):
            assert L.artalk_op_gemm_f16s_packed_ex(vp(P), 1, K, vp(2 * P), None, vp(3 * P), 64, 64, K, 0, cfg | (S << 8), 4, 4, None, None, None) == capi.EINVAL
            assert L.artalk_op_gemm_f16s_packed(vp(P), 1, K, vp(2 * P), None, vp(3 * P), 64, 64, K, 0, cfg | (S << 8), None) == capi.EINVAL
            if S <= 16:
                a = GemmRowsArgs(mode=1, M=64, N=64, K=K, A=P, lda=K, a_elems=64 * K, W=2 * P, ldw=K, w_elems=64 * K, C=3 * P, ldc=64, c_elems=64 * 64,
                                 force_cfg=cfg, splitk=S)
                assert L.artalk_op_gemm_rows(C.byref(a), None) == capi.EINVAL
