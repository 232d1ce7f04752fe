"""The eight LDS-DMA GEMM configurations of f16x3 mode (gemm_f16s.hip: 7 / 12 gemm_p8_big_kernel, 8 gemm_p8_2wgp_kernel, 20 / 23 / 24
gemm_p8_sm_kernel with rings of 4 / 8 / 5 stages, 28 gemm_p8_mid_kernel, 31 gemm_p8_pp_kernel) at the depths where their hand-scheduled
pipelines branch: nk = K / 32 below, at and one above every ring depth (2, 3, 4, 5, 8), both sides of the two-workgroup kernel's nk >= 5
deferral, nk == 1 of the big kernel, split-K slices of one and two steps, and the persistent kernels' walk over several tiles per
workgroup on a grid of 8 compute units (GemmArgs::cus through artalk_op_gemm_rows_args::cus).

Every launch goes through artalk_op_gemm_rows, mode 1, with a forced configuration, and asserts used_cfg == force_cfg.  A is packed with
artalk_op_pack_split_ex and sits at pitch K + 8 in a buffer whose gap words and rows beyond M are NaN halves; C has pitch N + 8 inside a
0xAB-filled buffer of which every word outside the M x N result must keep the fill; a_elems / c_elems are exactly sufficient.  The
reference is float64 A W^T + bias (then the epilogue) from the fp32 inputs, at the bar of the dense P8 tests (test_ops_gpu.py::
test_gemm_p8_dma_pipeline_and_producers, K = 512 .. 1024): max |err| / max |ref| < 2e-6; a P8 result at the format bound + 2e-6 * max |ref|
(test_p8_exps_ops_gpu.py::_assert_stored).  The error of an fp32 accumulation shrinks with K, so the bars hold here unchanged.

CASES is the table of every launch below; tests/test_p8_depth_cpu.py runs all of it through artalk_op_rows_dry_run."""
import collections
import functools
import math

import ctypes as C
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import p8_format as p8
from test_p8_exps_ops_gpu import _assert_stored
from test_rows_ops_gpu import FILL, _ada, _call, _check_ln, _f32, _filled, _lib, _ln_ref, _pack, _rows, _status

pytestmark = pytest.mark.gpu

SMALL, SPLIT, ALL = (20, 23, 24), (20, 23, 24, 28, 31), (7, 12, 8, 20, 23, 24, 28, 31)
RING = {7: 2, 12: 2, 8: 2, 20: 4, 23: 8, 24: 5, 28: 4, 31: 3}                      # stages of the LDS ring
TILE = {7: (256, 256), 12: (320, 256), 8: (128, 128), 20: (64, 64), 23: (64, 64), 24: (64, 64), 28: (128, 128), 31: (256, 128)}
DEPTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 17)
# one shape per family, a ragged last tile in M and (where the kernel takes it: 7 / 12 need whole 256-column tiles) in N
SWEEP = {20: [(65, 72)], 23: [(65, 72)], 24: [(65, 72)], 28: [(129, 136)], 31: [(257, 136)], 8: [(129, 132)],
         7: [(257, 256), (321, 256)], 12: [(257, 256), (321, 256)]}
EPI_SHAPE = {20: (65, 72), 23: (65, 72), 24: (65, 72), 28: (129, 136), 31: (257, 136), 8: (129, 136), 7: (257, 256), 12: (321, 256)}
EPI_DEPTHS = (1, 4, 5, 9)
SPLITS = (2, 3, 4, 5, 6, 8)
WRAP_M = {7: 13 * 256 - 100, 12: 13 * 320 - 100, 8: 13 * 128 - 100}      # N = 512 on 8 CUs: 26 / 26 / 52 tiles on 8 / 8 / 16 workgroups, 3.25 each
WRAP_DEPTHS = (1, 2, 4, 5, 9)
IDENT_GROUPS = [((7, 12, 8), [(257, 256), (321, 256)]), ((20, 23, 24, 28, 31, 8), [(129, 136)])]
GMAP = (7, 11, 2)           # gate rows out of a table: row(m) = (m // 7) * 11 + 2 + m % 7
LN_MMAP = (13, 20, 3)       # modulation rows of the fused reduce + LayerNorm
E, LDG = 768, 6 * 768 + 64
NANS = 0x7E007E00           # two fp16 NaNs

# kind: which test launches it; epi: bias | gelu_p8 | res | gate_res | guard (P8 result, one bias column inf); ln: the fused reduce + LayerNorm
Case = collections.namedtuple("Case", "kind cfg M N nk S epi c_exp cus ln")


def _case(kind, cfg, M, N, nk, S=1, epi="bias", c_exp=4, cus=0, ln=0):
    return Case(kind, cfg, M, N, nk, S, epi, c_exp, cus, ln)


def _edge_shapes(cfg):
    tm, tn = TILE[cfg]
    Ms = ([1] if cfg in SMALL else []) + [33, tm - 1, tm, tm + 1, 2 * tm + 1]
    Ns = [256, 512] if cfg in (7, 12) else [tn, tn + 8, 2 * tn + 4]
    return [(M, N) for M in Ms for N in Ns]


def _table():
    t = []
    for cfg in ALL:
        t += [_case("sweep", cfg, M, N, nk) for nk in DEPTHS for M, N in SWEEP[cfg]]
        t += [_case("edge", cfg, M, N, nk) for nk in (1, RING[cfg] + 1) for M, N in _edge_shapes(cfg)]
        M, N = EPI_SHAPE[cfg]
        for nk in EPI_DEPTHS:
            t += [_case("epi", cfg, M, N, nk), _case("epi", cfg, M, N, nk, epi="gelu_p8", c_exp=4), _case("epi", cfg, M, N, nk, epi="gelu_p8", c_exp=0),
                  _case("epi", cfg, M, N, nk, epi="res")]
            if cfg in SPLIT:
                t.append(_case("epi", cfg, M, N, nk, epi="gate_res"))
        t += [_case("guard", cfg, M, N, nk, epi="guard") for nk in (1, 5)]
    for cfg in SPLIT:
        M, N = SWEEP[cfg][0]
        t += [_case("split", cfg, M, N, nk, S, epi="res") for S in SPLITS for nk in (S, S + 1, 17)]
    for S, cfg in zip((2, 3, 4, 6, 8), SPLIT):
        t.append(_case("ln", cfg, 65, E, S + 1, S, epi="res", ln=1))
    for cfg in (7, 12, 8):
        t += [_case("wrap", cfg, WRAP_M[cfg], 512, nk, epi=epi, cus=cus) for nk in WRAP_DEPTHS for epi in ("bias", "res") for cus in (8, 0)]
    t += [_case("wrap_small", 20, 129, 136, 5, cus=cus) for cus in (8, 0)]
    for cfgs, shapes in IDENT_GROUPS:
        t += [_case("ident", cfg, M, N, nk) for nk in DEPTHS for M, N in shapes for cfg in cfgs]
    return t


CASES = _table()


def select(kind, **kw):
    return [c for c in CASES if c.kind == kind and all(getattr(c, k) == v for k, v in kw.items())]


def geometry(c):
    """pitches and exactly sufficient sizes (4-byte elements) of the buffers of a case"""
    K = 32 * c.nk
    g = dict(K=K, lda=K + 8, ldc=c.N + 8, ldg=c.N + 12, ldy=E + 8)
    g["a_elems"] = (c.M - 1) * g["lda"] + K
    g["c_elems"] = (c.M - 1) * g["ldc"] + c.N
    g["gate_rows"] = int(_rows(c.M, GMAP).max()) + 1
    g["gate_elems"] = (g["gate_rows"] - 1) * g["ldg"] + c.N
    g["y_elems"] = (c.M - 1) * g["ldy"] + E
    g["mod_rows"] = int(_rows(c.M, LN_MMAP).max()) + 1
    g["mod_elems"] = (g["mod_rows"] - 1) * LDG + 2 * E + E      # counted from ln_scale (column 2 E); ln_shift is at column 4 E
    return g


def rows_args(capi, c, ptr):
    """the artalk_op_gemm_rows_args of a case; ptr: addresses of A, W, bias, C (and gate, status, Y, mod where the case has them)"""
    g = geometry(c)
    used = [C.c_int32(-7) for _ in range(3)]
    kw = dict(mode=1, M=c.M, N=c.N, K=g["K"], A=ptr["A"], lda=g["lda"], a_elems=g["a_elems"], a_exp=4, W=ptr["W"], ldw=g["K"], w_elems=c.N * g["K"],
              bias=ptr["bias"], bias_elems=c.N, C=ptr["C"], ldc=g["ldc"], c_elems=g["c_elems"], force_cfg=c.cfg, splitk=c.S, cus=c.cus,
              used_cfg=C.pointer(used[0]), used_splitk=C.pointer(used[1]), fused_ln=C.pointer(used[2]))
    if c.epi in ("res", "gate_res"):
        kw.update(R=ptr["C"], ldr=g["ldc"], r_elems=g["c_elems"])      # in place
    if c.epi == "gate_res":
        kw.update(gate=ptr["gate"], ldg=g["ldg"], gmap=GMAP, gate_elems=g["gate_elems"])
    if c.epi in ("gelu_p8", "guard"):
        kw.update(act=1 if c.epi == "gelu_p8" else 0, c_p8=1, c_exp=c.c_exp, status_dev=ptr["status"])
    if c.ln:
        kw.update(ln_Y=ptr["Y"], ln_ldy=g["ldy"], ln_y_elems=g["y_elems"], ln_scale=ptr["mod"] + 4 * 2 * E, ln_shift=ptr["mod"] + 4 * 4 * E, ln_ldm=LDG,
                  ln_mod_elems=g["mod_elems"], ln_mmap=LN_MMAP, ln_eps=1e-6)
    return capi.GemmRowsArgs(**kw), used


# ------------------------------------------------------------------------------------------------------------------ the GPU side
class _Problem:
    """fp32 operands of an M x N x K product, their device copies (A in P8 at pitch K + 8 among NaN halves) and the float64 product"""

    def __init__(self, M, N, nk):
        _, L = _lib()
        K = 32 * nk
        g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + nk)
        self.A = torch.randn(M, K, generator=g)
        self.W = torch.randn(N, K, generator=g) / math.sqrt(K)
        self.bias = torch.randn(N, generator=g)
        self.R = torch.randn(M, N, generator=g)
        self.gate = torch.randn(int(_rows(M, GMAP).max()) + 1, N + 12, generator=g)
        self.dA = torch.full((M + 3, K + 8), NANS, dtype=torch.int32, device="cuda")
        self.dA[:M, :K] = _pack(L, self.A.cuda(), 4)
        self.dW, self.db, self.dR, self.dgate = self.W.cuda(), self.bias.cuda(), self.R.cuda(), self.gate.cuda()
        self.lin = self.A.double() @ self.W.double().t() + self.bias.double()
        self.refs = {}

    def ref(self, epi):
        if epi not in self.refs:
            lin = self.lin
            self.refs[epi] = {"bias": lambda: lin, "guard": lambda: lin, "gelu_p8": lambda: F.gelu(lin), "res": lambda: lin + self.R.double(),
                              "gate_res": lambda: self.R.double() + self.gate[_rows(lin.shape[0], GMAP)][:, :lin.shape[1]].double() * lin}[epi]()
        return self.refs[epi]


@functools.lru_cache(maxsize=6)
def _problem(M, N, nk):
    return _Problem(M, N, nk)


def _launch(c, bias_dev=None, extra=None):
    """one launch of a case: returns (the M x N result words, the whole guard buffer, the status word).  Asserts the configuration and
    split that ran and that every word of the buffer outside the result kept the 0xAB fill."""
    capi, L = _lib()
    p, g = _problem(c.M, c.N, c.nk), geometry(c)
    ldc, off = g["ldc"], 2 * g["ldc"]
    buf = _filled(off + (c.M + 2) * ldc)
    cv = buf[off:off + c.M * ldc].view(c.M, ldc)
    if c.epi in ("res", "gate_res"):
        cv[:, :c.N] = p.dR.view(torch.int32)
    st = _status()
    ptr = dict(A=p.dA.data_ptr(), W=p.dW.data_ptr(), bias=(p.db if bias_dev is None else bias_dev).data_ptr(), C=buf.data_ptr() + 4 * off,
               gate=p.dgate.data_ptr(), status=st.data_ptr())
    ptr.update(extra or {})
    a, used = rows_args(capi, c, ptr)
    _call(L, a)
    assert (used[0].value, used[1].value) == (c.cfg, c.S), (c, used[0].value, used[1].value)
    words = cv[:, :c.N].clone()
    cv[:, :c.N] = FILL
    assert bool((buf == FILL).all()), (c, "a word outside the M x N result lost the 0xAB fill")
    cv[:, :c.N] = words
    return words, buf, (int(st.item()), used[2].value)


def _check(c, words, status, skip_col=None):
    """the float64 bar of the case's epilogue"""
    ref = _problem(c.M, c.N, c.nk).ref(c.epi)
    scale = float(ref.abs().max())
    if c.epi in ("gelu_p8", "guard"):
        got = torch.from_numpy(p8.unpack(words.cpu().numpy(), c.c_exp))
        if skip_col is not None:
            keep = [j for j in range(c.N) if j != skip_col]
            got, ref = got[:, keep], ref[:, keep]
        else:
            assert status == 0, (c, status)
        assert scale < float(p8.max_value(c.c_exp))
        _assert_stored(got, ref, c.c_exp, 2e-6 * scale, str(c))
    else:
        got = _f32(words.contiguous()).cpu()
        assert torch.isfinite(got).all(), c
        err = float((got.double() - ref).abs().max()) / scale
        assert err < 2e-6, (c, err)


def _run(c):
    words, buf, (status, _) = _launch(c)
    _check(c, words, status)
    return words, buf


@pytest.mark.parametrize("nk", DEPTHS)
@pytest.mark.parametrize("cfg", ALL)
def test_every_configuration_at_every_depth(cfg, nk):
    """K = 32 nk for nk below, at and above every ring depth, bias only, at the family's shape with ragged last tiles"""
    for c in select("sweep", cfg=cfg, nk=nk):
        _run(c)


@pytest.mark.parametrize("nk", DEPTHS)
def test_unsplit_results_are_bit_identical_across_kernels(nk):
    """every split kernel accumulates an output element in the same order (k ascending; hi hi, lo hi, hi lo per 16-deep block:
    test_ops_gpu.py::test_gemm_p8_auto_dispatch asserts it at K = 1024): 7 = 12 = 8 at the big kernel's shapes, 20 = 23 = 24 = 28 = 31 = 8
    at a shape all of them take"""
    for cfgs, shapes in IDENT_GROUPS:
        for M, N in shapes:
            res = {cfg: _f32(_run(select("ident", cfg=cfg, M=M, N=N, nk=nk)[0])[0]) for cfg in cfgs}
            for cfg in cfgs[1:]:
                assert torch.equal(res[cfg], res[cfgs[0]]), (cfg, cfgs[0], M, N, nk)


@pytest.mark.parametrize("cfg", ALL)
@pytest.mark.parametrize("deep", [0, 1])
def test_tile_edges(cfg, deep):
    """M in {1 (64x64 tiles), 33, tile - 1, tile, tile + 1, 2 tile + 1} x N in {tile, tile + 8, 2 tile + 4} (7 / 12: 256, 512) at nk = 1 and
    at nk = ring depth + 1"""
    cases = select("edge", cfg=cfg, nk=RING[cfg] + 1 if deep else 1)
    assert len(cases) == len(_edge_shapes(cfg))
    for c in cases:
        _run(c)


@pytest.mark.parametrize("nk", EPI_DEPTHS)
@pytest.mark.parametrize("cfg", ALL)
def test_epilogues_at_short_depths(cfg, nk):
    """bias; bias + GELU stored in P8 at c_exp 4 and 0 (status word 0); the residual in place; gate rows through a gmap + residual
    (20 / 23 / 24 / 28 / 31).  nk = 4 / 5: the two sides of the two-workgroup kernel's deferred store"""
    cases = select("epi", cfg=cfg, nk=nk)
    assert len(cases) == (5 if cfg in SPLIT else 4)
    for c in cases:
        _run(c)


@pytest.mark.parametrize("cfg", ALL)
def test_p8_result_out_of_range(cfg):
    """one bias column inf with the result in P8: the small-grid, mid-grid and ping-pong kernels raise bit 3 of the status word; the
    large-grid kernels carry no guard by design (launch_gemm_p8) and store the column with a non-finite hi half instead.  Every other
    column meets the reference."""
    for c in select("guard", cfg=cfg):
        p = _problem(c.M, c.N, c.nk)
        col = c.N - 3
        bias = p.bias.clone()
        bias[col] = float("inf")
        words, _, (status, _) = _launch(c, bias_dev=bias.cuda())
        hi = p8.halves(words.cpu().numpy())[0]
        assert not np.isfinite(hi[:, col]).any(), c
        assert status == 8 if cfg in SPLIT else status in (0, 8), (c, status)
        _check(c, words, status, skip_col=col)


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("cfg", SPLIT)
def test_split_k_slices_shorter_than_the_ring(cfg, S):
    """nk_all = S (every slice one step), S + 1 (one slice of two) and 17 (uneven slices around the ring depth), finished by the plain
    reduce with bias and the residual in place"""
    cases = select("split", cfg=cfg, S=S)
    assert [c.nk for c in cases] == [S, S + 1, 17]
    for c in cases:
        _run(c)


@pytest.mark.parametrize("S", [2, 3, 4, 6, 8])
def test_split_k_fused_reduce_layernorm(S):
    """N = 768, nk_all = S + 1, finished by launch_splitk_reduce_ln: x = R + sum of slabs + bias in place at the GEMM bar, y = LN(x) (1 +
    scale) + shift at the float64 bar of test_rows_ops_gpu.py::test_splitk_reduce_fused_with_adaln_layernorm (|err| < 2e-5, the same
    modulation distribution)"""
    (c,) = select("ln", S=S)
    g = geometry(c)
    table = _ada(1, 41 + S)[:g["mod_rows"]].contiguous()
    dT = table.cuda()
    y = _filled((c.M + 2) * g["ldy"])
    words, _, (_, fused) = _launch(c, extra=dict(Y=y.data_ptr(), mod=dT.data_ptr()))
    assert fused == 1, c
    _check(c, words, 0)
    yv = y.view(c.M + 2, g["ldy"])
    assert bool((yv[c.M:] == FILL).all()) and bool((yv[:, E:] == FILL).all()), c
    rows = _rows(c.M, LN_MMAP)
    ref = _ln_ref(_f32(words.contiguous()).cpu().double(), table[rows][:, 2 * E:3 * E], table[rows][:, 4 * E:5 * E])
    _check_ln(yv[:c.M, :E].contiguous(), ref, 0, 4, None, str(c))


@pytest.mark.parametrize("nk", WRAP_DEPTHS)
@pytest.mark.parametrize("cfg", [7, 12, 8])
def test_persistent_kernels_walk_several_tiles_per_workgroup(cfg, nk):
    """cus = 8: 8 (7 / 12) or 16 (8) persistent workgroups over 26 / 26 / 52 tiles - three or four each, a ragged last round and a ragged
    last row tile - with bias and with the residual in place; the same launch on the whole device (cus = 0).  Both meet the float64
    bar and hold the same bits: which workgroup computes a tile changes nothing about the tile"""
    for epi in ("bias", "res"):
        part, whole = select("wrap", cfg=cfg, nk=nk, epi=epi)
        assert (part.cus, whole.cus) == (8, 0)
        _, b8 = _run(part)
        _, b0 = _run(whole)
        assert torch.equal(b8, b0), (cfg, nk, epi)


def test_small_grid_kernel_ignores_the_partition():
    part, whole = select("wrap_small")
    assert torch.equal(_run(part)[1], _run(whole)[1])
