"""artalk_op_gemm_rows / artalk_op_layernorm_rows / artalk_op_attention_rows: the argument checks, every one of which is made before the
device is touched (no allocation, no launch).  Each call below takes the arguments of a launch of the AR body - the proj form with the
LayerNorm that follows, q|k|v into the cache, the grouped history K/V, the AdaLN LayerNorm, attention out of the interleaved cache - with
sizes that are exactly the furthest element + 1, and adds ONE defect; host-side dummy pointers are never dereferenced because the call
must return first.  The calls without the defect are shown to be accepted with artalk_op_rows_dry_run, which makes an entry point return
ARTALK_OK at the point where it would first touch the device: every EINVAL below is therefore the defect's, and every size is pinned from
both sides (exactly sufficient: accepted; one element less: refused).  tests/test_rows_ops_gpu.py launches the same forms."""
import ctypes as C

import pytest

from artalk_amd import capi
from artalk_amd.capi import GemmRowsArgs

P = 1 << 26       # a 4096-byte aligned address that is never dereferenced
P2, P3 = 2 * P, 3 * P   # two more, far enough apart that no two buffers below overlap
E, NTOK = 768, 181
LDG = 6 * E + 64  # pitch of a (smaller) AdaLN table
B, PN, OFF = 3, 5, 1


def _row(m, rpb, bstride, off):
    return (m // rpb) * bstride + off + m % rpb


def _proj(mode=0, **kw):
    """proj form at the 5-token level: gate rows through gmap, residual in place, split in 3, the LayerNorm that follows"""
    M = B * PN
    last_g = _row(M - 1, PN, NTOK, OFF)
    a = dict(mode=mode, M=M, N=E, K=E, A=P, lda=E, a_elems=M * E, W=P, ldw=E, w_elems=E * E, bias=P, bias_elems=E,
             C=P, ldc=E, c_elems=M * E, R=P, ldr=E, r_elems=M * E,
             gate=P, ldg=LDG, gmap=(PN, NTOK, OFF), gate_elems=last_g * LDG + E, splitk=3,
             ln_Y=P2, ln_ldy=E, ln_y_elems=M * E, ln_scale=P + 4 * 2 * E, ln_shift=P + 4 * 4 * E, ln_ldm=LDG, ln_mmap=(PN, NTOK, OFF),
             ln_mod_elems=last_g * LDG + 2 * E + E)
    a.update(kw)
    return GemmRowsArgs(**a)


def _qkv(mode=0, **kw):
    """q|k|v written into cache rows 181 + off .. of every clip"""
    M = B * PN
    last = _row(M - 1, PN, 2 * NTOK, NTOK + OFF)
    a = dict(mode=mode, M=M, N=3 * E, K=E, A=P, lda=E, a_elems=M * E, W=P, ldw=E, w_elems=3 * E * E, bias=P, bias_elems=3 * E,
             C=P, ldc=3 * E, cmap=(PN, 2 * NTOK, NTOK + OFF), c_elems=last * 3 * E + 3 * E)
    a.update(kw)
    return GemmRowsArgs(**a)


def _hist(**kw):
    """history K/V of 3 blocks in one launch of the persistent 128x128 kernel: column groups"""
    M, G = B * NTOK, 3
    cache_l = B * 2 * NTOK * 3 * E
    last = _row(M - 1, NTOK, 2 * NTOK, 0)
    a = dict(mode=1, M=M, N=G * 2 * E, K=E, A=P, lda=E, a_elems=M * E, W=P, ldw=E, bias=P, C=P, ldc=3 * E, cmap=(NTOK, 2 * NTOK, 0),
             force_cfg=8, ngrp=2 * E, grpW=3 * E * E, grpB=3 * E, grpC=cache_l,
             w_elems=(G - 1) * 3 * E * E + (2 * E - 1) * E + E, bias_elems=(G - 1) * 3 * E + 2 * E,
             c_elems=(G - 1) * cache_l + last * 3 * E + 2 * E)
    a.update(kw)
    return GemmRowsArgs(**a)


def _gemm(a):
    return capi.lib().artalk_op_gemm_rows(C.byref(a), None)


def _mm(t):
    return (C.c_int32 * 3)(*t)


def _ln(**kw):
    M = B * PN
    last = _row(M - 1, PN, NTOK, OFF)
    a = dict(X=P, Y=P2, w=None, b=None, scale=P + 4 * 2 * E, shift=P + 4 * 4 * E, M=M, D=E, eps=1e-6, act=0, p8_exp=4, junk_period=0,
             junk_from=0, status=None, ldx=E + 64, ldy=E, ldm=LDG, mmap=(PN, NTOK, OFF), x_elems=(M - 1) * (E + 64) + E, y_elems=M * E,
             mod_elems=last * LDG + 2 * E + E)
    a.update(kw)
    return capi.lib().artalk_op_layernorm_rows(a["X"], a["Y"], a["w"], a["b"], a["scale"], a["shift"], a["M"], a["D"], a["eps"], a["act"],
                                               a["p8_exp"], a["junk_period"], a["junk_from"], a["status"], a["ldx"], a["ldy"], a["ldm"],
                                               None if a["mmap"] is None else _mm(a["mmap"]), a["x_elems"], a["y_elems"], a["mod_elems"], None)


def _attn(**kw):
    """AR attention of the 5-token level out of the interleaved cache [B][362][2304]: Q at row 181 + off, K at column 768, V at 1536"""
    ld, bs, Lk = 3 * E, 2 * NTOK * 3 * E, NTOK + OFF + PN
    a = dict(Q=P, K=P, V=P, O=P, B=B, H=12, HD=64, Lq=PN, Lk=Lk, scale=1.0, l2norm=1, qscale=P, split=0, qkv_exp=4, o_exp=4, out_p8=0,
             status=None, ldq=ld, ldk=ld, ldv=ld, ldo=E, q_bstride=bs, k_bstride=bs, v_bstride=bs, o_bstride=PN * E,
             q_elems=(B - 1) * bs + (PN - 1) * ld + E, k_elems=(B - 1) * bs + (Lk - 1) * ld + E, v_elems=(B - 1) * bs + (Lk - 1) * ld + E,
             o_elems=B * PN * E)
    a.update(kw)
    order = ["Q", "K", "V", "O", "B", "H", "HD", "Lq", "Lk", "scale", "l2norm", "qscale", "split", "qkv_exp", "o_exp", "out_p8", "status",
             "ldq", "ldk", "ldv", "ldo", "q_bstride", "k_bstride", "v_bstride", "o_bstride", "q_elems", "k_elems", "v_elems", "o_elems"]
    return capi.lib().artalk_op_attention_rows(*[a[k] for k in order], None)


@pytest.fixture
def dry():
    """artalk_op_rows_dry_run on: a call that passes every check returns ARTALK_OK without touching the device"""
    L = capi.lib()
    assert L.artalk_op_rows_dry_run(1) == 0
    yield L
    assert L.artalk_op_rows_dry_run(0) == 0


def test_rows_ops_are_exported():
    L = capi.lib()
    for name in ("artalk_op_gemm_rows", "artalk_op_layernorm_rows", "artalk_op_attention_rows", "artalk_op_gemm_rows_layout",
                 "artalk_op_rows_dry_run"):
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert capi.lib().artalk_op_gemm_rows(None, None) == capi.EINVAL


def test_gemm_rows_struct_mirror_matches_the_c_layout():
    """sizeof and the offset of every field, in declaration order, as the library's compiler laid the struct out"""
    out = (C.c_int64 * 64)()
    n = capi.lib().artalk_op_gemm_rows_layout(out, 64)
    fields = [f[0] for f in GemmRowsArgs._fields_]
    assert n == 1 + len(fields) == 50 and fields[-1] == "cus"
    assert out[0] == C.sizeof(GemmRowsArgs)
    assert [out[1 + i] for i in range(len(fields))] == [getattr(GemmRowsArgs, f).offset for f in fields]
    assert capi.lib().artalk_op_gemm_rows_layout(out, 49) == capi.EINVAL and capi.lib().artalk_op_gemm_rows_layout(None, 64) == capi.EINVAL


def _used():
    u = [C.c_int32(-7) for _ in range(3)]
    return u, dict(used_cfg=C.pointer(u[0]), used_splitk=C.pointer(u[1]), fused_ln=C.pointer(u[2]))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_baselines_with_exactly_sufficient_sizes_are_accepted(dry, mode):
    """the calls every one-defect case below starts from pass validation as they stand, and report the path they would take"""
    u, kw = _used()
    assert _gemm(_proj(mode, **kw)) == capi.OK
    assert (u[1].value, u[2].value) == (3, 1), "proj form split in 3: the fused reduce"
    assert u[0].value == {0: 3, 1: 20, 2: 2}[mode]           # M = 15: 32x128 tiles (f32, bf16), the 64x64 LDS-DMA kernel
    u, kw = _used()
    assert _gemm(_proj(mode, splitk=5, **kw)) == capi.OK and (u[1].value, u[2].value) == (5, 0)      # no fused kernel for 5 slabs
    u, kw = _used()
    assert _gemm(_proj(mode, ln_ldy=E + 4, ln_y_elems=14 * (E + 4) + E, **kw)) == capi.OK and u[2].value == 0      # ldy % 8 != 0: unfused
    u, kw = _used()
    assert _gemm(_qkv(mode, **kw)) == capi.OK and (u[1].value, u[2].value) == (1, 0)
    if mode == 1:
        u, kw = _used()
        assert _gemm(_qkv(mode, splitk=0, **kw)) == capi.OK and (u[0].value, u[1].value) == (24, 4)      # the planner's own: 36 tiles
        u, kw = _used()
        assert _gemm(_hist(**kw)) == capi.OK and (u[0].value, u[1].value, u[2].value) == (8, 1, 0)
        assert _gemm(_qkv(mode, c_p8=1)) == capi.OK
    M = B * PN
    last = _row(M - 1, PN, NTOK, OFF)
    mapped = dict(cmap=(PN, NTOK, OFF), c_elems=last * E + E, r_elems=last * E + E)
    u, kw = _used()
    assert _gemm(_proj(mode, **mapped, **kw)) == capi.OK and u[2].value == 1      # x behind a row map: only with the fused reduce
    # a residual that is not C: anywhere that does not overlap it
    assert _gemm(_proj(mode, R=P3)) == capi.OK


def test_layernorm_and_attention_baselines_are_accepted(dry):
    assert _ln() == capi.OK and _ln(act=0x100) == capi.OK
    assert _ln(Y=P, ldx=E, x_elems=B * PN * E) == capi.OK                # in place, row on row
    assert _ln(D=128, ldx=130, ldy=128, w=P3, b=P3, scale=None, shift=None, x_elems=14 * 130 + 128, y_elems=15 * 128) == capi.OK
    assert _attn() == capi.OK and _attn(l2norm=3, out_p8=1) == capi.OK


def test_overlapping_buffers_are_refused(dry):
    """in place means row on row: R == C with ldr == ldc, Y == X with ldy == ldx; anything else would race between rows"""
    big = 1 << 30
    for mode in (0, 1, 2):
        assert _gemm(_proj(mode, R=P + 4 * E)) == capi.EINVAL                              # R one row into C
        assert _gemm(_proj(mode, ldr=2 * E, r_elems=big)) == capi.EINVAL                   # R == C with another pitch
        assert _gemm(_proj(mode, ln_Y=P)) == capi.EINVAL and _gemm(_proj(mode, ln_Y=P + 4 * 14 * E)) == capi.EINVAL
        assert _gemm(_proj(mode, R=P + 4 * 15 * E)) == capi.OK                             # right behind C
    assert _ln(Y=P) == capi.EINVAL                                                         # Y == X, ldx != ldy
    assert _ln(Y=P + 16, ldx=E, x_elems=big) == capi.EINVAL
    assert _ln(scale=P + 4 * 2 * E + 2) == capi.EINVAL                                     # scale and shift not whole elements apart


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_rows_null_pointers_and_shape(mode):
    for f in ("A", "W", "C"):
        assert _gemm(_proj(mode, **{f: None})) == capi.EINVAL, f
    for f in ("ln_scale", "ln_shift"):      # the LayerNorm that follows is the AdaLN-modulated one
        assert _gemm(_proj(mode, **{f: None})) == capi.EINVAL, f
    for K in (0, 16, 752, 800 - 16):
        assert _gemm(_proj(mode, K=K, lda=1024, ldw=1024, a_elems=1 << 30, w_elems=1 << 30)) == capi.EINVAL, K
    for f, v in (("M", 0), ("M", -1), ("N", 0), ("act", 4), ("act", -1), ("splitk", -1), ("splitk", 17),
                 ("force_cfg", 5 if mode == 0 else 3 if mode == 2 else 21), ("force_cfg", -2)):
        assert _gemm(_proj(mode, **{f: v})) == capi.EINVAL, (f, v)
    assert _gemm(_proj(3)) == capi.EINVAL and _gemm(_proj(-1)) == capi.EINVAL
    assert _gemm(_proj(mode, K=256, lda=256, ldw=256, splitk=16)) == capi.EINVAL      # 32 * 16 > K: a slab without a K step


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_rows_exponents_and_maps(mode):
    for f in ("a_exp", "c_exp", "ln_p8_exp"):
        for e in (-9, 5, 16, -100):
            assert _gemm(_proj(mode, **{f: e})) == capi.EINVAL, (f, e)
    for f in ("cmap", "gmap", "ln_mmap"):
        for bad in ((0, NTOK, OFF), (-1, NTOK, OFF), (PN, -1, OFF), (PN, NTOK, -1)):
            assert _gemm(_proj(mode, **{f: bad})) == capi.EINVAL, (f, bad)
    assert _gemm(_qkv(mode, cmap=(0, 2 * NTOK, NTOK))) == capi.EINVAL
    assert _gemm(_qkv(mode, cmap=(PN, PN - 1, NTOK))) == capi.EINVAL      # the rows of two clips would collide


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_rows_alignment(mode):
    """A and W rows are fetched as 16-byte vectors in every mode; the f16x3 kernels also need the 16-byte epilogue"""
    for f in ("A", "W"):
        assert _gemm(_proj(mode, **{f: P + 4})) == capi.EINVAL, f
    assert _gemm(_proj(mode, lda=E + 2, a_elems=1 << 30)) == capi.EINVAL
    assert _gemm(_proj(mode, ldw=E + 2, w_elems=1 << 30)) == capi.EINVAL
    if mode != 0:
        assert _gemm(_proj(mode, ldw=E + 4, w_elems=1 << 30)) == capi.EINVAL      # packed / bf16 weight rows: 8 elements
    if mode == 1:
        assert _gemm(_proj(mode, lda=E + 4, a_elems=1 << 30)) == capi.EINVAL      # P8 rows are 32-byte groups
        for f in ("C", "bias", "gate", "R"):
            assert _gemm(_proj(mode, **{f: P + 4})) == capi.EINVAL, f
        for f in ("ldc", "ldg", "ldr"):
            assert _gemm(_proj(mode, **{f: LDG + 2, "c_elems": 1 << 30, "r_elems": 1 << 30, "gate_elems": 1 << 30})) == capi.EINVAL, f
        assert _gemm(_qkv(mode, c_p8=1, ldc=3 * E + 4, c_elems=1 << 30)) == capi.EINVAL
    else:
        assert _gemm(_qkv(mode, c_p8=1)) == capi.EINVAL                            # only the f16x3 kernels write P8
    for f in ("ln_Y", "ln_scale", "ln_shift"):
        assert _gemm(_proj(mode, **{f: getattr(_proj(mode), f) + 4})) == capi.EINVAL, f
    assert _gemm(_proj(mode, ln_ldm=LDG + 2, ln_mod_elems=1 << 30)) == capi.EINVAL
    assert _gemm(_proj(mode, ln_out_p8=1, ln_ldy=E + 4, ln_y_elems=1 << 30)) == capi.EINVAL


SIZES = ["a_elems", "w_elems", "bias_elems", "c_elems", "r_elems", "gate_elems", "ln_y_elems", "ln_mod_elems"]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("field", SIZES)
def test_gemm_rows_proj_form_one_element_short(mode, field):
    """every buffer of the proj form on its own: the furthest element of the last mapped row lies one past the stated size"""
    a = _proj(mode)
    setattr(a, field, getattr(a, field) - 1)
    assert _gemm(a) == capi.EINVAL
    # a pitch or a map that reaches further than the size stated for the dense form
    assert _gemm(_proj(mode, ldg=LDG + 4)) == capi.EINVAL and _gemm(_proj(mode, gmap=(PN, NTOK, OFF + 1))) == capi.EINVAL
    assert _gemm(_proj(mode, ln_ldm=LDG + 4)) == capi.EINVAL and _gemm(_proj(mode, ln_mmap=(PN, NTOK + 1, OFF))) == capi.EINVAL
    assert _gemm(_proj(mode, ln_ldy=E + 8)) == capi.EINVAL and _gemm(_proj(mode, lda=E + 8)) == capi.EINVAL


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_rows_cache_form_one_element_short(mode):
    a = _qkv(mode)
    a.c_elems -= 1
    assert _gemm(a) == capi.EINVAL
    assert _gemm(_qkv(mode, cmap=(PN, 2 * NTOK, NTOK + OFF + 1))) == capi.EINVAL
    assert _gemm(_qkv(mode, cmap=(PN, 2 * NTOK + 1, NTOK + OFF))) == capi.EINVAL
    assert _gemm(_qkv(mode, M=B * PN + 1, a_elems=1 << 30)) == capi.EINVAL       # a fourth clip's first row
    assert _gemm(_qkv(mode, ldc=3 * E - 4)) == capi.EINVAL                        # a pitch shorter than a row


@pytest.mark.parametrize("field", ["w_elems", "bias_elems", "c_elems", "a_elems"])
def test_gemm_rows_group_form_one_element_short(field):
    a = _hist()
    setattr(a, field, getattr(a, field) - 1)
    assert _gemm(a) == capi.EINVAL
    for f in ("grpW", "grpB", "grpC"):      # a group stride that carries the last group past the size
        assert _gemm(_hist(**{f: getattr(_hist(), f) + 8})) == capi.EINVAL, f


def test_gemm_rows_column_groups_are_refused_where_no_kernel_takes_them():
    big = 1 << 40
    sizes = dict(w_elems=big, bias_elems=big, c_elems=big)
    for mode in (0, 2):
        assert _gemm(_hist(mode=mode, force_cfg=-1, **sizes)) == capi.EINVAL
    for cfg in (7, 12, 20, 23, 24, 28, 31):
        assert _gemm(_hist(force_cfg=cfg, **sizes)) == capi.EINVAL, cfg
    for cfg in (-1, 99):                     # 5 x 36 tiles: below what gemm_p8_eligible wants for the persistent kernels
        assert _gemm(_hist(force_cfg=cfg, **sizes)) == capi.EINVAL, cfg
    assert _gemm(_hist(ngrp=2 * E + 64, **sizes)) == capi.EINVAL and _gemm(_hist(ngrp=E + 64, N=4 * (E + 64), **sizes)) == capi.EINVAL
    assert _gemm(_hist(ngrp=-128, **sizes)) == capi.EINVAL
    assert _gemm(_hist(grpW=3 * E * E + 4, **sizes)) == capi.EINVAL and _gemm(_hist(grpB=3 * E + 2, **sizes)) == capi.EINVAL
    assert _gemm(_hist(splitk=2, **sizes)) == capi.EINVAL
    assert _gemm(_hist(gate=P, ldg=4 * E, gate_elems=big, **sizes)) == capi.EINVAL
    assert _gemm(_hist(R=P, ldr=3 * E, r_elems=big, **sizes)) == capi.EINVAL


@pytest.mark.parametrize("mode", [0, 2])
def test_gemm_rows_layernorm_needs_dense_x_unless_fused(mode):
    """launch_layernorm reads x as dense rows: with a row map on C only the fused reduce (S in 2, 3, 4, 6, 8) can follow"""
    M = B * PN
    last = _row(M - 1, PN, NTOK, OFF)
    mapped = dict(cmap=(PN, NTOK, OFF), c_elems=last * E + E, r_elems=last * E + E)
    for S in (1, 5, 7):
        assert _gemm(_proj(mode, splitk=S, **mapped)) == capi.EINVAL, S
    assert _gemm(_proj(mode, N=E + 64, w_elems=1 << 30, bias_elems=1 << 30, ldc=E + 64, ldr=E + 64, c_elems=1 << 30, r_elems=1 << 30,
                       gate_elems=1 << 30)) == capi.EINVAL      # the LayerNorm is the 768-wide one


def test_layernorm_rows_checks():
    for f in ("X", "Y", "mmap"):
        assert _ln(**{f: None}) == capi.EINVAL, f
    assert _ln(scale=None) == capi.EINVAL and _ln(shift=None) == capi.EINVAL and _ln(w=P) == capi.EINVAL
    for f, v in (("M", 0), ("D", 256), ("D", 0), ("p8_exp", -9), ("p8_exp", 5), ("junk_period", -1), ("ldx", E - 4), ("ldy", E - 4),
                 ("ldm", E - 4), ("X", P + 4), ("Y", P + 8), ("scale", P + 4), ("shift", P + 4), ("ldx", E + 2), ("ldy", E + 2), ("ldm", LDG + 2)):
        assert _ln(**{f: v, "x_elems": 1 << 30, "y_elems": 1 << 30, "mod_elems": 1 << 30}) == capi.EINVAL, (f, v)
    assert _ln(act=0x100, ldy=E + 4, y_elems=1 << 30) == capi.EINVAL               # P8 rows are 32-byte groups
    assert _ln(act=0x100, D=128, ldx=128, ldy=128, ldm=128, mod_elems=1 << 30) == capi.EINVAL
    for bad in ((0, NTOK, OFF), (-5, NTOK, OFF), (PN, -1, OFF), (PN, NTOK, -1)):
        assert _ln(mmap=bad) == capi.EINVAL, bad
    for f in ("x_elems", "y_elems", "mod_elems"):
        M = B * PN
        full = {"x_elems": (M - 1) * (E + 64) + E, "y_elems": M * E, "mod_elems": _row(M - 1, PN, NTOK, OFF) * LDG + 3 * E}[f]
        assert _ln(**{f: full - 1}) == capi.EINVAL, f
    assert _ln(mmap=(PN, NTOK, OFF + 1)) == capi.EINVAL and _ln(ldm=LDG + 4) == capi.EINVAL and _ln(ldx=E + 68) == capi.EINVAL
    assert _ln(M=B * PN + 1, x_elems=1 << 30, y_elems=1 << 30) == capi.EINVAL       # a fourth clip's modulation row


def test_attention_rows_checks():
    for f in ("Q", "K", "V", "O", "qscale"):
        assert _attn(**{f: None}) == capi.EINVAL, f
    for f, v in (("HD", 48), ("B", 0), ("H", 0), ("Lq", 0), ("Lk", 0), ("qkv_exp", -9), ("qkv_exp", 5), ("o_exp", -9), ("o_exp", 5),
                 ("split", -1), ("Q", P + 4), ("K", P + 8), ("V", P + 4), ("O", P + 4), ("ldq", 3 * E + 2), ("ldk", 3 * E + 2),
                 ("ldv", 3 * E + 2), ("ldo", E + 2), ("q_bstride", 2 * NTOK * 3 * E + 2), ("k_bstride", 2 * NTOK * 3 * E + 2),
                 ("v_bstride", 2 * NTOK * 3 * E + 2), ("o_bstride", PN * E + 2), ("ldq", E - 4), ("ldo", E - 4), ("k_bstride", -8),
                 ("o_bstride", PN * E - 4)):
        big = dict(q_elems=1 << 40, k_elems=1 << 40, v_elems=1 << 40, o_elems=1 << 40)
        assert _attn(**{f: v}, **big) == capi.EINVAL, (f, v)
    big = dict(q_elems=1 << 40, k_elems=1 << 40, v_elems=1 << 40, o_elems=1 << 40)
    assert _attn(out_p8=1, l2norm=3, ldo=E + 4, o_bstride=PN * (E + 4), **big) == capi.EINVAL      # P8 rows are 32-byte groups
    assert _attn(l2norm=6, qscale=None, ldk=3 * E + 4, **big) == capi.EINVAL
    assert _attn(HD=32, H=24, l2norm=3, **big) == capi.EINVAL                                       # the f16 kernels are 64-wide heads
    for f in ("q_elems", "k_elems", "v_elems", "o_elems"):
        ld, bs, Lk = 3 * E, 2 * NTOK * 3 * E, NTOK + OFF + PN
        full = {"q_elems": (B - 1) * bs + (PN - 1) * ld + E, "k_elems": (B - 1) * bs + (Lk - 1) * ld + E,
                "v_elems": (B - 1) * bs + (Lk - 1) * ld + E, "o_elems": B * PN * E}[f]
        assert _attn(**{f: full - 1}) == capi.EINVAL, f
    assert _attn(Lk=NTOK + OFF + PN + 1) == capi.EINVAL and _attn(B=B + 1) == capi.EINVAL
    assert _attn(k_bstride=2 * NTOK * 3 * E + 8) == capi.EINVAL and _attn(ldv=3 * E + 8) == capi.EINVAL
