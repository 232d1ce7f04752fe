"""plan_attention, asked through artalk_op_attention_plan, and artalk_op_attention_rows_cus under artalk_op_rows_dry_run - no device.

Every case of tests/attn_cases.py plans as the kernel it names on a device of 256 compute units and is accepted by the rows entry point
with the buffers tests/test_attn_edges_gpu.py gives it; every threshold of the dispatch is asserted from both sides; the refusals of the
two entry points are listed."""
import pytest

import attn_cases as ac
from artalk_amd import capi

P = 1 << 26       # a 4096-byte aligned address that is never dereferenced


def _plan(Lq, Lk, flags, B=2, H=3, HD=64, split=0, cus=0, n_cu=ac.N_CU):
    return capi.lib().artalk_op_attention_plan(B, H, HD, Lq, Lk, flags, split, cus, n_cu)


@pytest.fixture
def dry():
    L = capi.lib()
    assert L.artalk_op_rows_dry_run(1) == 0
    yield L
    assert L.artalk_op_rows_dry_run(0) == 0


def _rows(L, c, used=None, **kw):
    import ctypes as C
    r = ac.layout(c)
    a = dict(Q=P, K=P, V=P, O=P, B=c.B, H=c.H, HD=c.HD, Lq=c.Lq, Lk=c.Lk, scale=ac.scale_of(c), flags=c.flags, qs=P if c.flags & 1 else None,
             split=c.split, qe=ac.QKV_EXP, oe=c.o_exp, out_p8=c.out_p8, st=P if c.out_p8 else None, cus=c.cus)
    a.update(kw)
    return L.artalk_op_attention_rows_cus(a["Q"], a["K"], a["V"], a["O"], a["B"], a["H"], a["HD"], a["Lq"], a["Lk"], a["scale"], a["flags"], a["qs"],
                                          a["split"], a["qe"], a["oe"], a["out_p8"], a["st"], r["ld"], r["ld"], r["ld"], r["ld"], r["qbs"], r["kbs"],
                                          r["kbs"], r["qbs"], r["qn"], r["kn"], r["kn"], r["qn"], a["cus"],
                                          None if used is None else C.byref(used), None)


def test_kernel_numbers_agree_with_the_binding():
    assert [capi.ATTN_KERNELS[i] for i in range(9)] == list(ac.KERNELS)
    assert (ac.F32_64, ac.F32_32, ac.SHORT, ac.F16, ac.F16_P8, ac.WIDE, ac.PP, ac.WIDE_AR, ac.WIDE_AR_P8) == (
        capi.ATTN_F32_64, capi.ATTN_F32_32, capi.ATTN_SHORT, capi.ATTN_F16, capi.ATTN_F16_P8, capi.ATTN_F16_WIDE, capi.ATTN_F16_PP,
        capi.ATTN_F16_WIDE_AR, capi.ATTN_F16_WIDE_AR_P8)
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "artalk_hip.h")).read()
    for name in ("F32_64", "F32_32", "SHORT", "F16", "F16_P8", "F16_WIDE", "F16_PP", "F16_WIDE_AR", "F16_WIDE_AR_P8"):
        assert int(re.search(r"#define ARTALK_ATTN_%s (\d+)" % name, hdr).group(1)) == getattr(capi, "ATTN_" + name)


def test_the_table_is_complete_and_unambiguous():
    ids = [ac.case_id(c) for c in ac.ALL]
    assert len(set(ids)) == len(ids)
    for k in range(9):
        assert any(c.kernel == k for c in ac.CASES), ac.KERNELS[k]
    assert {c.B * c.H for c in ac.CASES if c.kernel == ac.SHORT} >= {1, 6, 9, 12}
    assert {c.B * c.H for c in ac.CASES if c.kernel == ac.PP} == {16, 17, 23} and all(c.cus == 8 for c in ac.CASES if c.kernel == ac.PP)
    assert all(c.B * c.H == 256 for c in ac.CASES if c.kernel == ac.WIDE)
    assert {c.flags for c in ac.CASES if c.kernel == ac.SHORT} == {0, 1, 2, 3}
    assert 8 <= len(ac.PEAKED) <= 12 and {c.kernel for c in ac.PEAKED} == {ac.F32_64, ac.SHORT, ac.F16, ac.WIDE_AR, ac.F16_P8, ac.WIDE_AR_P8, ac.WIDE, ac.PP}


@pytest.mark.parametrize("c", ac.ALL, ids=ac.case_id)
def test_case_plans_as_the_kernel_it_names_and_is_accepted(dry, c):
    import ctypes as C
    assert _plan(c.Lq, c.Lk, c.flags, c.B, c.H, c.HD, c.split, c.cus) == c.kernel
    used = C.c_int32(-7)
    assert _rows(dry, c, used) == capi.OK
    assert used.value == c.kernel
    if c.cus == 0:      # the entry point without the partition argument takes the same call
        r = ac.layout(c)
        assert dry.artalk_op_attention_rows(P, P, P, P, c.B, c.H, c.HD, c.Lq, c.Lk, ac.scale_of(c), c.flags, P if c.flags & 1 else None, c.split,
                                            ac.QKV_EXP, c.o_exp, c.out_p8, P if c.out_p8 else None, r["ld"], r["ld"], r["ld"], r["ld"], r["qbs"],
                                            r["kbs"], r["kbs"], r["qbs"], r["qn"], r["kn"], r["kn"], r["qn"], None) == capi.OK


def test_query_count_boundaries():
    S, F16, WAR, F64, P8, WP8 = ac.SHORT, ac.F16, ac.WIDE_AR, ac.F32_64, ac.F16_P8, ac.WIDE_AR_P8
    # 32 / 33: the wide-AR kernel's own lower bound never decides, because up to 64 queries on 64 keys and more are the short kernel's
    assert (_plan(32, 65, 2), _plan(33, 65, 2)) == (S, S) and (_plan(32, 63, 2), _plan(33, 63, 2)) == (F16, F16)
    # 64 / 65
    assert (_plan(64, 65, 0), _plan(65, 65, 0)) == (S, F64)
    assert (_plan(64, 65, 2), _plan(65, 65, 2)) == (S, WAR) and (_plan(64, 65, 3), _plan(65, 65, 3)) == (S, WAR)
    assert (_plan(64, 64, 2), _plan(65, 64, 2)) == (S, F16)
    # 112 / 113
    assert (_plan(112, 193, 2), _plan(113, 193, 2)) == (WAR, F16) and (_plan(112, 193, 3), _plan(113, 193, 3)) == (WAR, F16)
    # 128 / 129 and 208 / 209 (P8 rows)
    assert (_plan(128, 200, 6), _plan(129, 200, 6)) == (P8, WP8) and (_plan(208, 200, 6), _plan(209, 200, 6)) == (WP8, P8)
    assert (_plan(128, 200, 6, B=32, H=8), _plan(129, 200, 6, B=32, H=8)) == (P8, ac.WIDE)
    assert (_plan(208, 200, 6, B=32, H=8), _plan(209, 200, 6, B=32, H=8)) == (ac.WIDE, P8)
    assert (_plan(128, 200, 6, B=2, H=8, cus=8), _plan(129, 200, 6, B=2, H=8, cus=8)) == (P8, ac.PP)
    assert (_plan(208, 200, 6, B=2, H=8, cus=8), _plan(209, 200, 6, B=2, H=8, cus=8)) == (ac.PP, P8)
    # neither bound is looked at without its flags
    assert _plan(129, 200, 0) == F64 and _plan(100, 200, 0) == F64 and _plan(100, 200, 0, HD=32) == ac.F32_32


def test_key_count_boundaries():
    S, F16, WAR, F64, P8, WP8, PP, W = ac.SHORT, ac.F16, ac.WIDE_AR, ac.F32_64, ac.F16_P8, ac.WIDE_AR_P8, ac.PP, ac.WIDE
    # 63 / 64: the short kernel
    assert (_plan(16, 63, 0), _plan(16, 64, 0)) == (F64, S) and (_plan(16, 63, 3), _plan(16, 64, 3)) == (F16, S)
    # 64 / 65: the fp32-row wide-AR kernel
    assert (_plan(100, 64, 2), _plan(100, 65, 2)) == (F16, WAR)
    # 128 / 129 and 224 / 225: the ping-pong kernel's two buffers
    kw = dict(B=2, H=8, cus=8)
    assert (_plan(199, 128, 6, **kw), _plan(199, 129, 6, **kw)) == (WP8, PP) and (_plan(199, 224, 6, **kw), _plan(199, 225, 6, **kw)) == (PP, WP8)
    kw = dict(B=32, H=16, cus=0)
    assert (_plan(199, 128, 6, **kw), _plan(199, 129, 6, **kw)) == (W, PP) and (_plan(199, 224, 6, **kw), _plan(199, 225, 6, **kw)) == (PP, W)
    # 256 / 257: the one-workgroup-per-head forms
    assert (_plan(199, 256, 6), _plan(199, 257, 6)) == (WP8, P8)
    assert (_plan(199, 256, 6, B=32, H=8), _plan(199, 257, 6, B=32, H=8)) == (W, P8)


def test_head_count_boundaries():
    # 255 / 256 heads: two 7-wave workgroups per head, or one of 13 waves
    assert (_plan(199, 100, 6, B=85, H=3), _plan(199, 100, 6, B=32, H=8)) == (ac.WIDE_AR_P8, ac.WIDE)
    assert (_plan(199, 100, 6, B=255, H=1), _plan(199, 100, 6, B=256, H=1)) == (ac.WIDE_AR_P8, ac.WIDE)
    # 2 cus - 1 / 2 cus heads: the persistent kernel wants two heads per unit of the partition ...
    for cus in (8, 24, 128):
        assert (_plan(199, 199, 6, B=2 * cus - 1, H=1, cus=cus), _plan(199, 199, 6, B=2 * cus, H=1, cus=cus)) == (
            ac.WIDE_AR_P8 if 2 * cus - 1 < 256 else ac.WIDE, ac.PP), cus
    # ... of the device where there is no partition or one larger than the device
    assert (_plan(199, 199, 6, B=511, H=1), _plan(199, 199, 6, B=512, H=1)) == (ac.WIDE, ac.PP)
    assert (_plan(199, 199, 6, B=511, H=1, cus=300), _plan(199, 199, 6, B=512, H=1, cus=300)) == (ac.WIDE, ac.PP)
    assert (_plan(199, 199, 6, B=15, H=1, n_cu=8), _plan(199, 199, 6, B=16, H=1, n_cu=8)) == (ac.WIDE_AR_P8, ac.PP)
    assert (_plan(199, 199, 6, B=15, H=1, cus=64, n_cu=8), _plan(199, 199, 6, B=16, H=1, cus=64, n_cu=8)) == (ac.WIDE_AR_P8, ac.PP)


def test_a_mask_excludes_the_short_pingpong_and_fp32_row_wide_ar_kernels():
    assert (_plan(16, 100, 0), _plan(16, 100, 0, split=8)) == (ac.SHORT, ac.F32_64)
    assert (_plan(16, 100, 2), _plan(16, 100, 2, split=8)) == (ac.SHORT, ac.F16)
    assert (_plan(100, 200, 2), _plan(100, 200, 2, split=50)) == (ac.WIDE_AR, ac.F16)
    assert (_plan(200, 200, 6, B=2, H=8, cus=8), _plan(200, 200, 6, B=2, H=8, cus=8, split=100)) == (ac.PP, ac.WIDE_AR_P8)
    assert (_plan(200, 200, 6, B=32, H=16), _plan(200, 200, 6, B=32, H=16, split=100)) == (ac.PP, ac.WIDE)
    # the P8 one-workgroup-per-head forms keep a masked launch (the VAE decoder)
    assert _plan(200, 200, 6, split=100) == ac.WIDE_AR_P8 and _plan(200, 200, 6, B=32, H=8, split=100) == ac.WIDE


def test_p8_rows_exclude_the_short_kernel():
    assert (_plan(16, 100, 2), _plan(16, 100, 6)) == (ac.SHORT, ac.F16_P8)
    assert (_plan(64, 64, 3), _plan(64, 64, 6)) == (ac.SHORT, ac.F16_P8)


def test_plan_refusals():
    ok = dict(Lq=100, Lk=200, flags=2)
    assert _plan(**ok) == ac.WIDE_AR
    for kw in (dict(HD=48), dict(HD=128), dict(B=0), dict(H=0), dict(Lq=0), dict(Lk=0), dict(Lq=-1), dict(split=-1), dict(flags=-1), dict(flags=8),
               dict(cus=-1), dict(n_cu=0), dict(n_cu=-256), dict(flags=4), dict(flags=5), dict(flags=7), dict(flags=2, HD=32),
               dict(flags=6, HD=32)):
        assert _plan(**{**ok, **kw}) == capi.EINVAL, kw
    assert _plan(50, 50, 0, HD=32) == ac.F32_32 and _plan(50, 50, 1, HD=32) == ac.F32_32


def test_rows_cus_refusals(dry):
    c = ac._c(ac.PP, 199, 199, 6, B=2, H=8, cus=8)
    assert _rows(dry, c) == capi.OK
    for kw in (dict(cus=-1), dict(Q=None), dict(K=None), dict(V=None), dict(O=None), dict(HD=48), dict(B=0), dict(H=0), dict(Lq=0), dict(Lk=0),
               dict(split=-1), dict(flags=7), dict(flags=4), dict(flags=8), dict(qe=5), dict(oe=-9), dict(Q=P + 16), dict(O=P + 4),
               dict(Lq=200), dict(Lk=200), dict(B=3), dict(H=9)):
        assert _rows(dry, c, **kw) == capi.EINVAL, kw
    l2 = ac._c(ac.SHORT, 16, 100, 1)
    assert _rows(dry, l2) == capi.OK and _rows(dry, l2, qs=None) == capi.EINVAL and _rows(dry, l2, cus=-8) == capi.EINVAL
    # a partition is taken by every kernel and changes the answer of the persistent one only
    import ctypes as C
    used = C.c_int32(-7)
    assert _rows(dry, l2, used, cus=8) == capi.OK and used.value == ac.SHORT
    assert _rows(dry, c, used, cus=0) == capi.OK and used.value == ac.WIDE_AR_P8
    assert _rows(dry, c, used, cus=9) == capi.OK and used.value == ac.WIDE_AR_P8
