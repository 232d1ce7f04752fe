"""The GEMM, LayerNorm and attention launchers in the forms run_chunk_body uses them - row maps, pitches wider than a row, column groups,
batch strides, split-K finished by the plain or the LayerNorm-fused reduce - one launch each through artalk_op_gemm_rows /
artalk_op_layernorm_rows / artalk_op_attention_rows.

Every case asserts (1) the float64 CPU reference, addressed with the restatement of the row map below (_row), at the bar the dense test of
the same kernel uses (cited at _BARS), and (2) that the mapped rows hold bit for bit what a dense launch of the same shape, mode,
configuration and split gives, while every other byte of the output buffer still holds the 0xAB fill: the device buffer is compared, as
int32 words, with a copy of the filled buffer into which the dense result was scattered on the host side of the map.

Sizes passed to the entry points are exactly the furthest element + 1 (tests/test_rows_ops_cpu.py passes one element less)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import p8_format as p8

pytestmark = pytest.mark.gpu

E, NTOK = 768, 181
PN = (1, 5, 25, 50, 100)
OFF = (0, 1, 6, 31, 81)
LDG = 6 * E + 64          # pitch of the AdaLN table here (the model's is (12 * 6 + 2) * 768): a swapped pitch cannot go unnoticed
FILL = -1414812757        # 0xABABABAB
IDENT = (2 ** 31 - 1, 0, 0)

# _BARS: where each bar comes from
#   mode 0  test_ops_gpu.py::test_gemm: |err| < 3e-5 * max(1, max|ref|)
#   mode 1  test_ops_gpu.py::test_gemm_p8_dma_pipeline_and_producers: |err| / max|ref| < 2e-6
#   mode 2  test_bf16_ops_gpu.py::_check: |err| <= 2e-5 * sum|a w| * |gate| + 1e-6 * (1 + |ref|), operands rounded to bf16 in the reference
#   LayerNorm fp32  test_ops_gpu.py::test_layernorm: |err| < 2e-5 (the same input and modulation distributions)
#   LayerNorm P8    test_p8_exps_ops_gpu.py::test_layernorm_p8_producer: p8_format.bound(ref, e) + 2e-5 * max|ref| / 4
#   attention fp32  test_ops_gpu.py::test_attention: |err| < 2e-5 (outputs of magnitude ~1)
#   attention P8    test_p8_exps_ops_gpu.py::test_attention_f32_rows_p8_output: p8_format.bound(ref, e) + 2e-5 * max|ref|


def _lib():
    from artalk_amd import capi
    return capi, capi.lib()


def _p(t):
    return None if t is None else t.data_ptr()


def _row(m, rpb, bstride, off):
    """the row map, restated: row(m) = (m // rpb) * bstride + off + m % rpb"""
    return (m // rpb) * bstride + off + m % rpb


def _rows(M, rmap):
    return torch.tensor([m if rmap[0] == IDENT[0] else _row(m, *rmap) for m in range(M)], dtype=torch.long)


def _filled(n):
    return torch.full((n,), FILL, dtype=torch.int32, device="cuda")


def _f32(t):
    return t.view(torch.float32)


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _pack(L, x_dev, e):
    out = torch.empty(x_dev.shape, dtype=torch.int32, device="cuda")
    assert L.artalk_op_pack_split_ex(_p(x_dev), _p(out), x_dev.numel(), 0, e, None, None) == 0
    return out


def _pack_w(L, w_dev):
    out = torch.empty(w_dev.shape, dtype=torch.int32, device="cuda")
    assert L.artalk_op_pack_split(_p(w_dev), _p(out), w_dev.numel(), 1, None) == 0
    return out


def _bf(t):
    return t.to(torch.bfloat16).double()


class _Gemm:
    """One GEMM problem: fp32 operands on the CPU, their device copies (A also in P8 at a_exp), the float64 result of the matrix product
    for fp32 operands and for bf16-rounded ones (computed once, shared by every launch of the problem)."""

    def __init__(self, L, M, N, K, seed, a_exp=4, ldw=None):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.a_exp = M, N, K, a_exp
        self.A = torch.randn(M, K, generator=g)
        self.W = torch.randn(N, K, generator=g) / math.sqrt(K)
        self.bias = torch.randn(N, generator=g)
        self.dA, self.dW, self.db = self.A.cuda(), self.W.cuda(), self.bias.cuda()
        self.dAp = _pack(L, self.dA, a_exp)
        self.acc = self.A.double() @ self.W.double().t()
        self.acc_bf = _bf(self.A) @ _bf(self.W).t()
        self.mag_bf = _bf(self.A).abs() @ _bf(self.W).abs().t()
        self._wp = None
        self.L = L

    def wp(self):
        if self._wp is None:
            self._wp = _pack_w(self.L, self.dW)
        return self._wp

    def ref(self, mode, gate=None, R=None):
        """float64: R + gate * (A W^T + bias), with the operands the mode multiplies"""
        r = (self.acc_bf if mode == 2 else self.acc) + self.bias.double()
        if gate is not None:
            r = r * gate.double()
        if R is not None:
            r = r + R.double()
        return r

    def check(self, mode, got, ref, gate=None, what=""):
        err = (got.double() - ref).abs()
        assert torch.isfinite(got).all(), what
        if mode == 0:
            assert float(err.max()) < 3e-5 * max(1.0, float(ref.abs().max())), (what, float(err.max()))
        elif mode == 1:
            assert float(err.max()) / float(ref.abs().max()) < 2e-6, (what, float(err.max()))
        else:
            bound = 2e-5 * self.mag_bf * (gate.double().abs() if gate is not None else 1.0) + 1e-6 * (1.0 + ref.abs())
            assert float((err / bound).max()) <= 1.0, (what, float(err.max()))


def _args(capi, p, mode, C_dev, c_elems, ldc, cmap, cfg=-1, splitk=1, **kw):
    used = [C.c_int32(-7) for _ in range(3)]
    a = capi.GemmRowsArgs(mode=mode, M=p.M, N=p.N, K=p.K, A=_p(p.dAp if mode == 1 else p.dA), lda=p.K, a_elems=p.M * p.K, a_exp=p.a_exp,
                          W=_p(p.dW), ldw=p.K, w_elems=p.N * p.K, bias=_p(p.db), bias_elems=p.N, C=C_dev, ldc=ldc, c_elems=c_elems,
                          cmap=cmap, force_cfg=cfg, splitk=splitk, used_cfg=C.pointer(used[0]), used_splitk=C.pointer(used[1]),
                          fused_ln=C.pointer(used[2]), **kw)
    return a, used


def _call(L, a):
    rc = L.artalk_op_gemm_rows(C.byref(a), None)
    assert rc == 0, rc
    torch.cuda.synchronize()


def _dense_gemm(capi, L, p, mode, cfg, S, gate=None, R=None):
    """the same shape, mode, configuration and split with dense rows, through the entry point that existed before where it can say it
    (mode 0: artalk_op_gemm / artalk_op_gemm_ex, mode 1: artalk_op_gemm_f16s_packed_ex, mode 2: artalk_op_gemm_bf16), otherwise through
    artalk_op_gemm_rows with identity maps and dense pitches.  cfg, S: what the mapped launch reported (used_cfg, used_splitk)."""
    M, N, K = p.M, p.N, p.K
    out = R.clone().cuda() if R is not None else torch.full((M, N), float("nan"), device="cuda")
    dg = gate.contiguous().cuda() if gate is not None else None
    if mode == 0 and S == 1 and gate is None and R is None:
        assert L.artalk_op_gemm_ex(_p(p.dA), K, _p(p.dW), _p(p.db), _p(out), M, N, K, 0, cfg, None) == 0
    elif mode == 0 and S == 1 and cfg == L_heuristic_f32(M, N):
        assert L.artalk_op_gemm(_p(p.dA), K, _p(p.dW), _p(p.db), _p(dg), _p(out) if R is not None else None, _p(out), M, N, K, 0, None) == 0
    elif mode == 2:
        assert L.artalk_op_gemm_bf16(_p(p.dA), K, _p(p.dW), _p(p.db), _p(dg), _p(out) if R is not None else None, _p(out), M, N, K, 0,
                                     cfg | (S << 8), None) == 0
    elif mode == 1 and gate is None:
        assert L.artalk_op_gemm_f16s_packed_ex(_p(p.dAp), 1, K, _p(p.wp()), _p(p.db), _p(out), M, N, K, 0x200 if R is not None else 0,
                                               cfg | (S << 8), p.a_exp, 4, None, None, None) == 0
    else:
        a, used = _args(capi, p, mode, _p(out), M * N, N, IDENT, cfg, S, **(dict(gate=_p(dg), ldg=N, gate_elems=M * N) if gate is not None else {}),
                        **(dict(R=_p(out), ldr=N, r_elems=M * N) if R is not None else {}))
        _call(L, a)
        assert (used[0].value, used[1].value) == (cfg, S)
    torch.cuda.synchronize()
    return out


def L_heuristic_f32(M, N):
    """gemm_config of gemm_f32.hip for a plain window: what artalk_op_gemm launches"""
    return 4 if ((M + 127) // 128) * ((N + 127) // 128) >= 1024 else (2 if M > 32 else 3)


def _expect(buf0, rows, ld, col0, dense):
    """the filled buffer with the dense result scattered to the mapped rows (int32 words)"""
    exp = buf0.clone()
    n = dense.shape[1]
    idx = (rows.cuda()[:, None] * ld + col0 + torch.arange(n, device="cuda")[None, :]).reshape(-1)
    exp[idx] = dense.contiguous().view(torch.int32).reshape(-1)
    return exp


# ------------------------------------------------------------------------------------------------------------ a. q|k|v into the cache
QKV_LAUNCHES = ([(0, c, 1) for c in (1, 2, 3, 4)] + [(0, -1, 3)] +
                [(1, -1, 0)] + [(1, c, 3) for c in (20, 24, 28, 31)] +
                [(2, c, 1) for c in (0, 1, 2)] + [(2, -1, 3)])


@pytest.mark.parametrize("level", [0, 1, 3])
def test_qkv_gemm_writes_cache_rows(level):
    """q|k|v of the level's tokens straight into rows 181 + off .. of every clip of a [B][362][2304] cache (run_chunk_body: ldc = 3 * 768,
    cmap = (pn, 2 * 181, 181 + off)), B = 3: every fp32 tile, every small-grid f16x3 configuration with a split and the planner's own
    plan, every bf16 tile, split in 3."""
    capi, L = _lib()
    B, pn, off = 3, PN[level], OFF[level]
    M, N, K = B * pn, 3 * E, E
    p = _Gemm(L, M, N, K, 100 + level)
    cmap = (pn, 2 * NTOK, NTOK + off)
    rows = _rows(M, cmap)
    c_elems = int(rows[-1]) * N + N
    assert c_elems == ((B - 1) * 2 * NTOK + NTOK + off + pn) * N
    buf0 = _filled(B * 2 * NTOK * N)
    for mode, cfg, S in QKV_LAUNCHES:
        buf = buf0.clone()
        a, used = _args(capi, p, mode, _p(buf), c_elems, N, cmap, cfg, S)
        _call(L, a)
        ucfg, uS = used[0].value, used[1].value
        if cfg != -1:
            assert ucfg == cfg, (mode, cfg, ucfg)
        assert uS == S if S else uS >= 1, (mode, cfg, S, uS)
        if mode == 1 and S == 0:
            assert uS > 1, "the planner splits q|k|v of the small scale steps (72 tiles at most)"
        what = f"level {level} mode {mode} cfg {ucfg} S {uS}"
        p.check(mode, _f32(buf).view(-1, N)[rows.cuda()].cpu(), p.ref(mode), None, what)
        dense = _dense_gemm(capi, L, p, mode, ucfg, uS)
        assert torch.equal(buf, _expect(buf0, rows, N, 0, dense)), what + ": mapped rows differ from the dense launch, or a byte outside them changed"


# ------------------------------------------------------------------------------------------------------------ b. history K/V
@pytest.mark.parametrize("mode", [0, 2])
def test_history_kv_one_layer(mode):
    """K/V of the 181 history tokens of one block: columns 768 .. 2303 of cache rows 0 .. 180 of every clip; the Q columns of those rows
    and rows 181 .. 361 keep the fill."""
    capi, L = _lib()
    B = 3
    M, N, K, ld = B * NTOK, 2 * E, E, 3 * E
    p = _Gemm(L, M, N, K, 200 + mode)
    cmap = (NTOK, 2 * NTOK, 0)
    rows = _rows(M, cmap)
    buf0 = _filled(B * 2 * NTOK * ld)
    buf = buf0.clone()
    cbase = buf.data_ptr() + 4 * E
    a, used = _args(capi, p, mode, cbase, int(rows[-1]) * ld + N, ld, cmap)
    _call(L, a)
    got = _f32(buf).view(-1, ld)[rows.cuda()][:, E:].cpu()
    p.check(mode, got, p.ref(mode), None, f"history mode {mode}")
    dense = _dense_gemm(capi, L, p, mode, used[0].value, 1)
    assert torch.equal(buf, _expect(buf0, rows, ld, E, dense))
    v = buf.view(B, 2 * NTOK, ld)
    assert bool((v[:, :NTOK, :E] == FILL).all()) and bool((v[:, NTOK:] == FILL).all())


@pytest.mark.parametrize("B,G,cfg", [(2, 12, -1), (3, 3, 8)])
def test_history_kv_column_groups(B, G, cfg):
    """The f16x3 form: all blocks in one launch of the persistent 128x128 kernel, column group j = block j's weight rows (W + j grpW), bias
    (bias + j grpB) and cache slab (C + j grpC).  12 groups at B = 2 are 3 x 144 tiles, the smallest grid gemm_p8_eligible accepts: the
    planner must take it (used_cfg 8); 3 groups at B = 3 are forced.  Each group against float64 and bit for bit against a dense launch
    of that group alone on the same kernel."""
    capi, L = _lib()
    M, K, ld, ng = B * NTOK, E, 3 * E, 2 * E
    grpW, grpB, grpC = (ng + 8) * K, ng + 16, B * 2 * NTOK * ld       # strides with gaps: a dropped stride lands in the wrong place
    g = torch.Generator().manual_seed(300 + G)
    A = torch.randn(M, K, generator=g)
    Wall = torch.randn(G, ng + 8, K, generator=g) / math.sqrt(K)
    ball = torch.randn(G, ng + 16, generator=g)
    dA, dW, db = A.cuda(), Wall.cuda(), ball.cuda()
    dAp = _pack(L, dA, 4)
    cmap = (NTOK, 2 * NTOK, 0)
    rows = _rows(M, cmap)
    buf0 = _filled(G * grpC)
    buf = buf0.clone()
    used = [C.c_int32(-7) for _ in range(3)]
    a = capi.GemmRowsArgs(mode=1, M=M, N=G * ng, K=K, A=_p(dAp), lda=K, a_elems=M * K, W=_p(dW), ldw=K, w_elems=(G - 1) * grpW + (ng - 1) * K + K,
                          bias=_p(db), bias_elems=(G - 1) * grpB + ng, C=buf.data_ptr() + 4 * E, ldc=ld,
                          c_elems=(G - 1) * grpC + int(rows[-1]) * ld + ng, cmap=cmap, force_cfg=cfg, ngrp=ng, grpW=grpW, grpB=grpB, grpC=grpC,
                          used_cfg=C.pointer(used[0]), used_splitk=C.pointer(used[1]), fused_ln=C.pointer(used[2]))
    _call(L, a)
    assert (used[0].value, used[1].value, used[2].value) == (8, 1, 0)
    exp = buf0.clone()
    for j in range(G):
        W, bias = Wall[j, :ng], ball[j, :ng]
        ref = A.double() @ W.double().t() + bias.double()
        got = _f32(buf)[j * grpC:(j + 1) * grpC].view(-1, ld)[rows.cuda()][:, E:].cpu()
        err = float((got.double() - ref).abs().max()) / float(ref.abs().max())
        assert err < 2e-6, (j, err)
        dense = torch.full((M, ng), float("nan"), device="cuda")
        Wp = _pack_w(L, dW[j, :ng].contiguous())
        assert L.artalk_op_gemm_f16s_packed_ex(_p(dAp), 1, K, _p(Wp), _p(db[j, :ng].contiguous()), _p(dense), M, ng, K, 0, 8, 4, 4, None, None, None) == 0
        torch.cuda.synchronize()
        exp[j * grpC:(j + 1) * grpC] = _expect(buf0[:grpC], rows, ld, E, dense)
    assert torch.equal(buf, exp), "a group differs from its dense launch, or the Q columns / rows 181 .. 361 lost the fill"


# ------------------------------------------------------------------------------------------------------------ c / d. proj and FFN-out
def _ada(B, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * NTOK, LDG, generator=g) * scale


def _resid_case(L, form, B, pn, seed):
    K, a_exp = (E, 4) if form == "proj" else (4 * E, 0)
    p = _Gemm(L, B * pn, E, K, seed, a_exp)
    g = torch.Generator().manual_seed(seed + 1)
    return p, torch.randn(B * pn, E, generator=g)


@pytest.mark.parametrize("form", ["proj", "ffn_out"])
@pytest.mark.parametrize("level", [0, 1, 2, 4])
def test_gated_residual_gemm_reads_the_adaln_table(form, level):
    """x += gate[gmap(m)] * (A W^T + b) in place (proj: K = 768; FFN-out: K = 3072, P8 A at a_exp = 0 in f16x3 mode): gate rows out of
    an AdaLN table of pitch 6 * 768 + 64 through gmap = (pn, 181, off), at column 768 of the table; split and unsplit, three modes."""
    capi, L = _lib()
    B, pn, off = 3, PN[level], OFF[level]
    M = B * pn
    p, R = _resid_case(L, form, B, pn, 400 + level)
    table = _ada(B, 17)
    dT = table.cuda()
    gmap = (pn, NTOK, off)
    grows = _rows(M, gmap)
    gate = table[grows][:, E:2 * E]
    gate_elems = int(grows[-1]) * LDG + E
    for mode in (0, 1, 2):
        ref = p.ref(mode, gate, R)
        for S in ((1, 0) if mode == 1 else (1, 3)):
            x = R.clone().cuda()
            a, used = _args(capi, p, mode, _p(x), M * E, E, IDENT, -1, S, gate=dT.data_ptr() + 4 * E, ldg=LDG, gmap=gmap, gate_elems=gate_elems,
                            R=_p(x), ldr=E, r_elems=M * E)
            _call(L, a)
            uS = used[1].value
            assert (uS > 1) == (S != 1), (mode, S, uS)
            what = f"{form} level {level} mode {mode} cfg {used[0].value} S {uS}"
            p.check(mode, x.cpu(), ref, gate, what)
            dense = _dense_gemm(capi, L, p, mode, used[0].value, uS, gate, R)
            assert torch.equal(x, dense), what
    # the gate at an odd column of the table: rows that are not 16-byte aligned take the one-column-at-a-time path of the GEMM epilogue
    # (S = 1) and of splitk_reduce_kernel (S = 3).  Float64 bar only: the dense launch with an aligned gate runs the 16-byte path, whose
    # multiply-add the compiler may contract differently.
    gate1 = table[grows][:, E + 1:2 * E + 1]
    for mode in (0, 2):
        ref = p.ref(mode, gate1, R)
        for S in (1, 3):
            x = R.clone().cuda()
            a, used = _args(capi, p, mode, _p(x), M * E, E, IDENT, -1, S, gate=dT.data_ptr() + 4 * (E + 1), ldg=LDG, gmap=gmap,
                            gate_elems=gate_elems, R=_p(x), ldr=E, r_elems=M * E)
            _call(L, a)
            assert used[1].value == S
            p.check(mode, x.cpu(), ref, gate1, f"{form} level {level} mode {mode} S {S}, unaligned gate")


# ------------------------------------------------------------------------------------------------------------ e. fused reduce + LayerNorm
def _ln_ref(x64, sc, sh, eps=1e-6):
    return F.layer_norm(x64, (x64.shape[-1],), None, None, eps) * (sc.double() + 1) + sh.double()


def _check_ln(y_dev, ref, out_p8, e, st, what):
    if out_p8:
        assert int(st.item()) == 0, what
        assert float(ref.abs().max()) < float(p8.max_value(e))
        got = torch.from_numpy(p8.unpack(y_dev.cpu().numpy(), e))
        tol = torch.from_numpy(p8.bound(ref.numpy(), e)) + 2e-5 * float(ref.abs().max()) / 4.0
        assert not bool(((got - ref).abs() > tol).any()), (what, float((got - ref).abs().max()))
    else:
        err = float((_f32(y_dev).cpu().double() - ref).abs().max())
        assert err < 2e-5, (what, err)


@pytest.mark.parametrize("form", ["proj", "ffn_out"])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_splitk_reduce_fused_with_adaln_layernorm(form, level):
    """launch_splitk_reduce_ln (S in 2, 3, 4, 6, 8; M = 3, 15, 75: no multiple of its 4 rows per workgroup): x = R + gate * (sum of slabs +
    bias) in place and y = LN(x) * (1 + scale[mmap(m)]) + shift[mmap(m)] dense, fp32 and P8 at exponents 4, 0, -8 (modulation scaled so that
    y nears the top of the exponent's range; the status word must stay 0).  fused_ln must report 1; S = 5 has no fused kernel, must
    report 0 and meet the same references through the plain reduce and launch_layernorm.
    x is bit-identical to the unfused S-way launch.  y is held to the float64 bar only, not to bit identity with
    artalk_op_layernorm_rows over that x: the two kernels state the same operations in the same order (the lane's elements
    (i * 64 + lane) * 4 + e in i, e order, the same butterfly), but the compiler contracts them differently - the fused kernel keeps the
    row as x + r values it has just computed and sums them with packed adds, layernorm_kernel<768> loads them and contracts the
    deviations and the modulation into other fused multiply-adds - and on an MI355X y differs in the last bits (1 to 8 ulp on most
    elements, 69 ulp seen on an element near zero, at M = 3, S = 2, fp32 y) while both meet the bar."""
    capi, L = _lib()
    B, pn, off = 3, PN[level], OFF[level]
    M = B * pn
    p, R = _resid_case(L, form, B, pn, 500 + level)
    mmap = (pn, NTOK, off)
    mrows = _rows(M, mmap)
    mod_elems = int(mrows[-1]) * LDG + 2 * E + E
    gate_t = _ada(B, 23)
    dG = gate_t.cuda()
    gate = gate_t[mrows][:, E:2 * E]
    gate_elems = int(mrows[-1]) * LDG + E
    outs = [(0, 4), (1, 4), (1, 0), (1, -8)]
    tables = {}
    for out_p8, e in outs:
        t = _ada(B, 29 + e)
        if out_p8:
            t[:, 2 * E:3 * E] *= 500.0 * 2.0 ** (4 - e) / 32        # test_p8_exps_ops_gpu.py: _sigma(e) / 32
        tables[(out_p8, e)] = (t, t.cuda())
    for mode in (0, 1, 2):
        ref_x = p.ref(mode, gate, R)
        for S in (2, 3, 4, 5, 6, 8):
            if S * 32 > p.K:
                continue
            xu = R.clone().cuda()          # the unfused S-way result
            a, used = _args(capi, p, mode, _p(xu), M * E, E, IDENT, 20 if mode == 1 else -1, S, gate=dG.data_ptr() + 4 * E, ldg=LDG, gmap=mmap,
                            gate_elems=gate_elems, R=_p(xu), ldr=E, r_elems=M * E)
            _call(L, a)
            assert used[1].value == S and used[2].value == 0
            p.check(mode, xu.cpu(), ref_x, gate, f"unfused {form} mode {mode} S {S}")
            for out_p8, e in outs:
                t, dT = tables[(out_p8, e)]
                x = R.clone().cuda()
                y = _filled((M + 2) * E)
                st = _status()
                a, used = _args(capi, p, mode, _p(x), M * E, E, IDENT, 20 if mode == 1 else -1, S, gate=dG.data_ptr() + 4 * E, ldg=LDG,
                                gmap=mmap, gate_elems=gate_elems, R=_p(x), ldr=E, r_elems=M * E, ln_Y=_p(y), ln_ldy=E, ln_y_elems=M * E,
                                ln_scale=dT.data_ptr() + 4 * 2 * E, ln_shift=dT.data_ptr() + 4 * 4 * E, ln_ldm=LDG, ln_mod_elems=mod_elems,
                                ln_mmap=mmap, ln_eps=1e-6, ln_out_p8=out_p8, ln_p8_exp=e, status_dev=_p(st))
                _call(L, a)
                what = f"{form} level {level} mode {mode} S {S} p8 {out_p8} e {e}"
                assert used[1].value == S and used[2].value == (0 if S == 5 else 1), what
                assert torch.equal(x, xu), what + ": x differs from the unfused split"
                assert bool((y[M * E:] == FILL).all()), what
                sc, sh = t[mrows][:, 2 * E:3 * E], t[mrows][:, 4 * E:5 * E]
                _check_ln(y[:M * E].view(M, E), _ln_ref(x.cpu().double(), sc, sh), out_p8, e, st, what)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fused_reduce_addresses_x_by_cmap_and_y_by_row(mode):
    """x (and its residual) through a non-identity cmap - rows 181 + off .. of a [B][362][768] buffer - while y stays dense: the x store
    takes crow, the y store row.  Every other row of the x buffer keeps its bytes."""
    capi, L = _lib()
    B, level = 3, 1
    pn, off = PN[level], OFF[level]
    M = B * pn
    p, R = _resid_case(L, "proj", B, pn, 600 + mode)
    cmap, mmap = (pn, 2 * NTOK, NTOK + off), (pn, NTOK, off)
    crows, mrows = _rows(M, cmap), _rows(M, mmap)
    t = _ada(B, 31)
    dT = t.cuda()
    gate = t[mrows][:, E:2 * E]
    x0 = torch.randn(B * 2 * NTOK, E, generator=torch.Generator().manual_seed(9))
    x0[crows] = R
    ref_x = p.ref(mode, gate, R)
    for S in (3, 8):
        x = x0.clone().cuda()
        y = _filled(M * E)
        c_elems = int(crows[-1]) * E + E
        a, used = _args(capi, p, mode, _p(x), c_elems, E, cmap, 20 if mode == 1 else -1, S, gate=dT.data_ptr() + 4 * E, ldg=LDG, gmap=mmap,
                        gate_elems=int(mrows[-1]) * LDG + E, R=_p(x), ldr=E, r_elems=c_elems, ln_Y=_p(y), ln_ldy=E, ln_y_elems=M * E,
                        ln_scale=dT.data_ptr() + 4 * 2 * E, ln_shift=dT.data_ptr() + 4 * 4 * E, ln_ldm=LDG,
                        ln_mod_elems=int(mrows[-1]) * LDG + 3 * E, ln_mmap=mmap, ln_eps=1e-6)
        _call(L, a)
        assert used[2].value == 1
        got = x.cpu()
        p.check(mode, got[crows], ref_x, gate, f"cmap x mode {mode} S {S}")
        keep = torch.ones(B * 2 * NTOK, dtype=torch.bool)
        keep[crows] = False
        assert torch.equal(got[keep].view(torch.int32), x0[keep].view(torch.int32))
        dense = _dense_gemm(capi, L, p, mode, used[0].value, S, gate, R)
        assert torch.equal(got[crows].view(torch.int32), dense.cpu().view(torch.int32))
        ref_y = _ln_ref(got[crows].double(), t[mrows][:, 2 * E:3 * E], t[mrows][:, 4 * E:5 * E])
        _check_ln(y.view(M, E), ref_y, 0, 4, None, f"cmap y mode {mode} S {S}")


# ------------------------------------------------------------------------------------------------------------ f. layernorm_rows
def _ln_rows(L, X, Y, w, b, sc, sh, M, D, eps, act, e, st, ldx, ldy, ldm, mmap, xe, ye, me):
    rc = L.artalk_op_layernorm_rows(X, Y, w, b, sc, sh, M, D, eps, act, e, 0, 0, st, ldx, ldy, ldm, (C.c_int32 * 3)(*mmap), xe, ye, me, None)
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("level", [0, 1, 3])
def test_layernorm_reads_modulation_rows_through_mmap(level):
    """The AR body's AdaLN LayerNorm: scale / shift rows out of the table through mmap = (pn, 181, off) and ldm = 6 * 768 + 64, X with a
    pitch of 768 + 64, Y dense; fp32 and P8 (exponents 4, 0, -8).  Bit-identical to artalk_op_layernorm_ex on gathered dense rows."""
    capi, L = _lib()
    B, pn, off = 3, PN[level], OFF[level]
    M, ldx = B * pn, E + 64
    g = torch.Generator().manual_seed(700 + level)
    X = torch.randn(M, ldx, generator=g) * 2 + 0.3
    mmap = (pn, NTOK, off)
    mrows = _rows(M, mmap)
    dX = X.cuda()
    dXd = X[:, :E].contiguous().cuda()
    for out_p8, e in ((0, 4), (1, 4), (1, 0), (1, -8)):
        t = _ada(B, 37 + e)
        if out_p8:
            t[:, 2 * E:3 * E] *= 500.0 * 2.0 ** (4 - e) / 32
        dT = t.cuda()
        sc, sh = t[mrows][:, 2 * E:3 * E].contiguous(), t[mrows][:, 4 * E:5 * E].contiguous()
        y = _filled((M + 2) * E)
        st = _status()
        _ln_rows(L, _p(dX), _p(y), None, None, dT.data_ptr() + 8 * E, dT.data_ptr() + 16 * E, M, E, 1e-6, 0x100 if out_p8 else 0, e, _p(st), ldx, E, LDG,
                 mmap, (M - 1) * ldx + E, M * E, int(mrows[-1]) * LDG + 3 * E)
        what = f"level {level} p8 {out_p8} e {e}"
        assert bool((y[M * E:] == FILL).all()), what
        _check_ln(y[:M * E].view(M, E), _ln_ref(X[:, :E].double(), sc, sh), out_p8, e, st, what)
        yd = _filled(M * E)
        assert L.artalk_op_layernorm_ex(_p(dXd), _p(yd), None, None, _p(sc.cuda()), _p(sh.cuda()), M, E, 1e-6, 0x100 if out_p8 else 0, e, 0, 0, None,
                                        None) == 0
        torch.cuda.synchronize()
        assert torch.equal(y[:M * E], yd), what


@pytest.mark.parametrize("D", [128, 512, 1024])
def test_layernorm_with_row_pitches(D):
    """The affine LayerNorms of the style / VAE / wav2vec2 widths with ldx, ldy > D and an identity map: the gaps of Y keep the fill."""
    capi, L = _lib()
    M, ldx, ldy = 203, D + 24, D + 40
    g = torch.Generator().manual_seed(D)
    X = torch.randn(M, ldx, generator=g) * 2 + 0.3
    w, b = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ref = F.layer_norm(X[:, :D].double(), (D,), w.double(), b.double(), 1e-5)
    dX, dw, db = X.cuda(), w.cuda(), b.cuda()
    y = _filled(M * ldy)
    _ln_rows(L, _p(dX), _p(y), _p(dw), _p(db), None, None, M, D, 1e-5, 0, 4, None, ldx, ldy, D, IDENT, (M - 1) * ldx + D, (M - 1) * ldy + D, 0)
    yv = y.view(M, ldy)
    assert bool((yv[:, D:] == FILL).all())
    got = _f32(yv[:, :D].contiguous())
    assert float((got.cpu().double() - ref).abs().max()) < 2e-5
    yd = torch.empty(M, D, device="cuda")
    assert L.artalk_op_layernorm_ex(_p(X[:, :D].contiguous().cuda()), _p(yd), _p(dw), _p(db), None, None, M, D, 1e-5, 0, 4, 0, 0, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), yd.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ g. attention_rows
def _attn_ref(Q, K, V, H, HD, scale, split, qs):
    B, Lq, Lk = Q.shape[0], Q.shape[1], K.shape[1]
    q, k, v = (t.reshape(B, -1, H, HD).transpose(1, 2).double() for t in (Q, K, V))
    if qs is not None:
        q = F.normalize(q, dim=-1) * qs.double().view(1, H, 1, 1)
        k = F.normalize(k, dim=-1)
    s = q @ k.transpose(-1, -2) * scale
    if split:
        mask = torch.zeros(Lq, Lk, dtype=torch.double)
        mask[:split, split:] = -float("inf")
        s = s + mask
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, Lq, H * HD)


def _attn_rows(L, Q, K, V, O, B, H, HD, Lq, Lk, scale, l2, qs, split, qe, oe, out_p8, st, ld, lo, bs, obs, qn, kn, vn, on):
    rc = L.artalk_op_attention_rows(Q, K, V, O, B, H, HD, Lq, Lk, scale, l2, qs, split, qe, oe, out_p8, st, ld, ld, ld, lo, bs, bs, bs, obs,
                                    qn, kn, vn, on, None)
    assert rc == 0, rc
    torch.cuda.synchronize()


def _check_attn(o_dev, ref, out_p8, e, st, what):
    ref = ref.reshape(o_dev.shape[0], -1)
    vmax = float(ref.abs().max())
    if out_p8:
        assert int(st.item()) == 0, what
        got = torch.from_numpy(p8.unpack(o_dev.cpu().numpy(), e))
        tol = torch.from_numpy(p8.bound(ref.numpy(), e)) + 2e-5 * vmax
        assert not bool(((got - ref).abs() > tol).any()), (what, float((got - ref).abs().max()))
    else:
        err = float((_f32(o_dev).cpu().double() - ref).abs().max())
        assert err < 2e-5, (what, err)


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
def test_ar_attention_reads_the_interleaved_cache(level):
    """Q, K and V out of one [B][362][2304] cache as run_chunk_body reads them: Q at row 181 + off, K at column 768, V at column 1536,
    Lk = 181 + off + pn keys, batch stride 2 * 181 * 2304; O compact with o_bstride = pn * 768.  fp32 and f16-split kernels, O as fp32
    and (f16x3 mode) in P8.  Bit-identical to artalk_op_attention_ex on gathered contiguous rows."""
    capi, L = _lib()
    B, H, HD, pn, off = 2, 12, 64, PN[level], OFF[level]
    ld, bs, Lk = 3 * E, 2 * NTOK * 3 * E, NTOK + OFF[level] + PN[level]
    g = torch.Generator().manual_seed(800 + level)
    cache = torch.randn(B, 2 * NTOK, ld, generator=g)
    qs = torch.rand(H, generator=g) * 4 + 1
    Q, K, V = cache[:, NTOK + off:NTOK + off + pn, :E], cache[:, :Lk, E:2 * E], cache[:, :Lk, 2 * E:]
    ref = _attn_ref(Q, K, V, H, HD, 1.0, 0, qs)
    dC, dqs = cache.cuda(), qs.cuda()
    dQ, dK, dV = (t.contiguous().cuda() for t in (Q, K, V))
    base = dC.data_ptr()
    qp, kp, vp = base + 4 * (NTOK + off) * ld, base + 4 * E, base + 8 * E
    total = B * 2 * NTOK * ld
    qn, kn, vn = (B - 1) * bs + (pn - 1) * ld + E, (B - 1) * bs + (Lk - 1) * ld + E, (B - 1) * bs + (Lk - 1) * ld + E
    assert qn <= total - (NTOK + off) * ld and kn <= total - E and vn <= total - 2 * E
    for l2, out_p8, oe in ((1, 0, 4), (3, 0, 4), (3, 1, 4), (3, 1, 0)):
        o = _filled((B * pn + 1) * E)
        st = _status()
        _attn_rows(L, qp, kp, vp, _p(o), B, H, HD, pn, Lk, 1.0, l2, _p(dqs), 0, 4, oe, out_p8, _p(st), ld, E, bs, pn * E, qn, kn, vn, B * pn * E)
        what = f"level {level} l2norm {l2} out_p8 {out_p8} o_exp {oe}"
        assert bool((o[B * pn * E:] == FILL).all()), what
        _check_attn(o[:B * pn * E].view(B * pn, E), ref, out_p8, oe, st, what)
        od = _filled(B * pn * E)
        assert L.artalk_op_attention_ex(_p(dQ), _p(dK), _p(dV), _p(od), B, H, HD, pn, Lk, 1.0, l2, _p(dqs), 0, 4, oe, out_p8, None, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(o[:B * pn * E], od), what


@pytest.mark.parametrize("name,H,HD,Lq,split,p8rows", [("vae_dec", 8, 64, 200, 100, 0), ("vae_dec", 8, 64, 200, 100, 1), ("vae_enc", 8, 64, 100, 0, 0),
                                                       ("vae_enc", 8, 64, 100, 0, 1), ("style", 4, 32, 50, 0, 0)])
def test_attention_reads_packed_qkv_rows(name, H, HD, Lq, split, p8rows):
    """The VAE and style stacks: q|k|v rows [B][L][3 * H * HD] as their q|k|v GEMM writes them (fp32, or P8 for the f16x3 VAE), Q / K / V
    at columns 0 / D / 2 D with ld = 3 D and a batch stride of L * 3 D; O [B][L][D] with a wider pitch."""
    capi, L = _lib()
    B, D = 2, H * HD
    ld, bs, lo = 3 * D, Lq * 3 * D, D + 64
    scale = 512 ** -0.5 if H == 8 else HD ** -0.5
    g = torch.Generator().manual_seed(900 + Lq + p8rows)
    qkv = torch.randn(B, Lq, ld, generator=g)
    Q, K, V = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    ref = _attn_ref(Q, K, V, H, HD, scale, split, None)
    dqkv = qkv.cuda()
    src = _pack(L, dqkv.view(-1, ld), 3) if p8rows else dqkv
    dense = [t.contiguous().cuda() for t in (Q, K, V)]
    if p8rows:
        dense = [_pack(L, t.view(-1, D), 3) for t in dense]
    n = (B - 1) * bs + (Lq - 1) * ld + D
    obs = Lq * lo
    for l2 in ((6,) if p8rows else ((0, 2) if HD == 64 else (0,))):
        o = _filled(B * obs)
        _attn_rows(L, src.data_ptr(), src.data_ptr() + 4 * D, src.data_ptr() + 8 * D, _p(o), B, H, HD, Lq, Lq, scale, l2, None, split, 3, 4, 0, None,
                   ld, lo, bs, obs, n, n, n, (B - 1) * obs + (Lq - 1) * lo + D)
        ov = o.view(B * Lq, lo)
        what = f"{name} l2norm {l2}"
        assert bool((ov[:, D:] == FILL).all()), what
        got = ov[:, :D].contiguous()
        _check_attn(got, ref, 0, 4, None, what)
        od = _filled(B * Lq * D)
        assert L.artalk_op_attention_ex(_p(dense[0]), _p(dense[1]), _p(dense[2]), _p(od), B, H, HD, Lq, Lq, scale, l2, None, split, 3, 4, 0, None,
                                        None) == 0
        torch.cuda.synchronize()
        assert torch.equal(got.reshape(-1), od), what
