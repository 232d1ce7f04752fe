"""The case table of tests/test_gemm_edges_gpu.py without a GPU (tests/gemm_edge_cases.py): the conditions the table rests on (the integer
bound of the exact cases, K % 32, the depth limit of unsplit rounded cases), that the kernels' own sum order - emulated with float32
running sums - stays within HALF the allowance of every rounded case, that every launch is accepted by artalk_op_gemm_rows under
artalk_op_rows_dry_run and planned as the tile and split it names, and that the references tell wrong kernels from right ones.
Run with -s for the figures."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_edge_cases as ec
from artalk_amd import capi

P = 1 << 26      # a 16-byte aligned address that is never dereferenced


def test_table_conditions():
    assert len(ec.BY_ID) == len(ec.CASES)
    assert ec.K_DEEPEST * 9 * 3 + 64 * 3 + 64 < 2 ** 24      # |sum| <= K * 9, times |gate| <= 3, plus |bias| * 3 and |R|
    for c in ec.CASES:
        assert c.K % 32 == 0 and c.K <= ec.K_DEEPEST and c.M >= 1 and c.N >= 1, c
        if c.kind == "exact":
            assert c.act == ec.ACT_NONE, c
            d = ec.data(c)
            for t, lim in ((d.A, 3), (d.W, 3), (d.gate, 3), (d.bias, 64), (d.R, 64)):
                assert float(t.abs().max()) <= lim and bool((t == t.round()).all()) and torch.equal(t.to(torch.bfloat16).float(), t), c
        else:
            assert c.K <= 288 or c.S > 1 or c.block, c      # one chain over a deeper K is less accurate than the yardstick
            assert c.act == ec.ACT_NONE or not (c.gate or c.res), c
        assert c.entry == "bf16" or c.S == 1 or 32 * c.S <= c.K, c
    # every instantiation has an exact and a rounded case
    for mode, tile in ec.MODE_TILES:
        for kind in ("exact", "rounded"):
            assert ec.select(kind=kind, mode=mode, tile=tile, S=1, entry="rows", layout="aligned")          # epilogue_tile32, 16-byte
            assert ec.select(kind=kind, mode=mode, tile=tile, S=1, entry="rows", layout="unaligned")        # epilogue_tile32, 4-byte
            for S in (2, 3, 8, 5):                                                                          # splitk_reduce_kernel<2 | 3 | 8 | 0>
                assert [c for c in ec.select("split", kind, mode=mode, tile=tile, S=S) if c.N % 4 == 0]     # 16-byte partial and reduce
                assert [c for c in ec.select("split", kind, mode=mode, tile=tile, S=S) if c.N % 4 != 0]     # 4-byte partial and reduce
    for M, tile in ec.BLOCKED_MS.items():
        for kind in ("exact", "rounded"):
            assert ec.select("blocked", kind, M=M, tile=tile)


def test_tile_order_cases_wrap():
    """each 'order' case has more row tiles than one group of tile_order and a short last group; every tile has one whose tile count is
    no multiple of 8"""
    odd = set()
    for c in ec.select("order"):
        tm, tn = -(-c.M // c.BM), -(-c.N // c.BN)
        gm = ec.GM[c.BM]
        assert tm > gm and tm % gm != 0, (c, tm, tn)
        if (tm * tn) % 8 != 0:
            odd.add((c.mode, c.tile))
    assert odd == set(ec.MODE_TILES)


def test_k_range_covers_k_once():
    """the restatement of k_range: slabs are consecutive, cover every K step once, and the table holds one step per slab, uneven slabs
    and (bf16) empty ones"""
    seen = set()
    for c in ec.CASES:
        if c.S > 1:
            r = [ec.k_range(c.K // c.BK, y, c.S) for y in range(c.S)]
            assert r[0][0] == 0 and all(r[y][0] + r[y][1] == r[y + 1][0] for y in range(c.S - 1)) and sum(r[-1]) == c.K // c.BK, c
            n = [x[1] for x in r]
            seen |= {"empty"} if min(n) == 0 else set()
            seen |= {"one"} if max(n) == 1 and min(n) == 1 else set()
            seen |= {"uneven"} if max(n) != min(n) and min(n) > 0 else set()
            assert c.family == "empty" or min(n) >= 1, c
    assert seen == {"empty", "one", "uneven"}


def _rows_args(c, used):
    """artalk_op_gemm_rows_args of a case with addresses that are never dereferenced, at the alignment of the GPU file"""
    return c.rows_args(P, 2 * P, 3 * P + 4 * c.off, 4 * P + 4 * c.off, 5 * P + 4 * c.off, used)


def test_every_case_plans_as_it_is_named():
    L = capi.lib()
    assert L.artalk_op_rows_dry_run(1) == 0
    try:
        for c in ec.CASES:
            used = [C.c_int32(-7), C.c_int32(-7)]
            if c.entry == "rows":
                assert L.artalk_op_gemm_rows(C.byref(_rows_args(c, used)), None) == capi.OK, c
                assert (used[0].value, used[1].value) == (c.tile, c.S), c
                a = _rows_args(c, used)
                a.c_elems -= 1
                assert L.artalk_op_gemm_rows(C.byref(a), None) == capi.EINVAL, c      # the sizes are exactly sufficient
            elif c.entry == "blocked":      # the dense entry points ask gemm_config without a forced tile
                a = _rows_args(c, used)
                a.force_cfg = -1
                assert L.artalk_op_gemm_rows(C.byref(a), None) == capi.OK and (used[0].value, used[1].value) == (c.tile, 1), c
            elif c.family == "empty":       # artalk_op_gemm_rows refuses more slabs than K steps, in both modes: only artalk_op_gemm_bf16 takes them
                for mode, tile in ((2, c.tile), (0, 2)):
                    a = _rows_args(c, used)
                    a.mode, a.force_cfg = mode, tile
                    assert L.artalk_op_gemm_rows(C.byref(a), None) == capi.EINVAL, c
            else:                           # one batch of the grid.z case
                assert L.artalk_op_gemm_rows(C.byref(_rows_args(c, used)), None) == capi.OK and used[0].value == c.tile, c
    finally:
        assert L.artalk_op_rows_dry_run(0) == 0


@pytest.mark.parametrize("family", ["rounded", "split", "blocked"])
def test_the_kernel_order_keeps_half_the_allowance(family):
    worst = {}
    for c in ec.select(family, "rounded"):
        want, e32, allow = ec.bar(c)
        assert 1e-8 < e32 < 1e-5 and 0.5 < float(want.abs().max()) < 20, (c, e32)
        used = float((ec.emulate(c).double() - want).abs().max()) / allow
        key = (c.mode, c.tile, c.K, c.S)
        worst[key] = max(worst.get(key, 0.0), used)
        assert used <= 0.5, (c, used)
    for (mode, tile, K, S), u in sorted(worst.items()):
        print(f"{family} mode {mode} tile {tile} K {K} S {S}: the emulated order uses {u:.2f} of the allowance")


def test_restart_every_256_changes_no_bit_up_to_k_256():
    """one block: the blocked order adds the only chain to a zero sum; from K = 288 on the orders differ in some bit on rounded data"""
    for c in ec.select("blocked", "rounded"):
        same = np.array_equal(ec.add_slabs(ec.slab_sums(c, ec.BLOCK)).view(np.int32), ec.add_slabs(ec.slab_sums(c, 0)).view(np.int32))
        assert same == (c.K <= ec.BLOCK), c


# ---- the references tell wrong kernels apart: each wrong kernel below fails equality (exact) or leaves the allowance tenfold (rounded)
def _misses(c, got):
    want, e32, allow = ec.bar(c)
    if c.kind == "exact":
        return not torch.equal(got.double(), want.double())
    err = (got.double() - want).abs().max()
    return not bool(err <= 10 * allow)      # (a NaN left in the payload misses too)


def _three(kind, **kw):
    cs = ec.select(kind=kind, nb=1, **kw)
    assert len(cs) >= 3, (kind, kw)
    return cs[:: max(1, len(cs) // 3)][:3]


def _finish(c, acc):
    dtype = torch.float64 if c.kind == "exact" else torch.float32
    return ec.finish(c, acc.to(dtype), dtype)


KINDS = ("exact", "rounded")


@pytest.mark.parametrize("kind", KINDS)
def test_a_dropped_last_k_step_misses(kind):
    for c in _three(kind, S=1, entry="rows"):
        assert not _misses(c, ec.reference(c, torch.float64))
        assert _misses(c, _finish(c, ec.product(c, torch.float64, 0, c.K - c.BK) if c.K > c.BK else torch.zeros(1, c.M, c.N))), c


@pytest.mark.parametrize("kind", KINDS)
def test_a_tile_row_taken_from_the_row_above_misses(kind):
    for c in [x for x in ec.select(kind=kind, entry="rows") if x.M > x.BM and x.N >= x.BN][::20][:3]:
        acc = ec.product(c, torch.float64)
        acc[:, c.BM - 1] = acc[:, c.BM - 2]      # the last row of the first tile
        assert _misses(c, _finish(c, acc)), c


@pytest.mark.parametrize("kind", KINDS)
def test_an_unwritten_last_group_of_a_row_misses(kind):
    for c in _three(kind, S=1, entry="rows", layout="aligned"):
        got = ec.reference(c, torch.float64).float()
        first = (c.N - 1) // 4 * 4
        got[:, c.M // 2, first:] = ec.initial(c)[:, c.M // 2, first:]
        assert _misses(c, got), c


@pytest.mark.parametrize("kind", KINDS)
def test_gate_before_bias_misses(kind):
    for c in _three(kind, gate=True, bias=True):
        dtype = torch.float64
        assert _misses(c, ec.finish(c, ec.product(c, dtype), dtype, gate_first=True)), c


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("twice", [True, False])
def test_a_slab_added_twice_or_skipped_misses(kind, twice):
    for c in _three(kind, family="split"):
        for y in (0, c.S - 1):
            kt0, nk = ec.k_range(c.K // c.BK, y, c.S)
            slab = ec.product(c, torch.float64, kt0 * c.BK, (kt0 + nk) * c.BK)
            acc = ec.product(c, torch.float64)
            assert _misses(c, _finish(c, acc + slab if twice else acc - slab)), (c, y)


@pytest.mark.parametrize("kind", KINDS)
def test_truncation_to_bf16_misses(kind):
    """(the exact cases' operands are bf16 values: rounding cannot show on them, which is why the rounding table exists)"""
    for c in _three(kind, mode=2, S=1, entry="rows"):
        got = ec.finish(c, ec.product(c, torch.float64, trunc=True), torch.float64)
        assert _misses(c, got) == (kind == "rounded"), c
    want, ok = ec.rounding_expected("A")
    A, W = ec.rounding_operands("A")
    trunc = (A.view(torch.int32) & -65536).view(torch.float32)
    differs = (trunc != want) & ok & ~torch.isnan(want)
    assert int(differs.sum()) > 100 and bool(differs[:, 1::2].any()) and bool(differs[:, ::2].any())


@pytest.mark.parametrize("kind", KINDS)
def test_a_row_wrap_one_row_off_misses(kind):
    """splitk_reduce_kernel's 4-byte branch walks the M x N elements in groups of four; where N % 4 != 0 a group straddles two rows and
    its tail belongs to the next row (the `cc >= g.N` wrap).  Without the wrap the tail is finished with the gate and residual of the
    row above and lands there, and its own place stays unwritten."""
    for c in [x for x in ec.select("split", kind) if x.N % 4 != 0][::5][:3]:
        assert c.gate and c.res
        acc = ec.product(c, torch.float64)
        dtype = acc.dtype
        d = ec.data(c)
        got = ec.reference(c, torch.float64).float()
        init = ec.initial(c)
        n = 0
        for idx in range(0, c.M * c.N, 4):
            row = idx // c.N
            for e in range(4):
                r2, cc = divmod(idx + e, c.N)
                if r2 != row and r2 < c.M:
                    got[0, row, cc] = ((acc[0, r2, cc] + d.bias[0, cc].to(dtype)) * d.gate[row, cc].to(dtype) + d.R[0, row, cc].to(dtype)).float()
                    got[0, r2, cc] = init[0, r2, cc]
                    n += 1
        assert n > c.M // 2 and _misses(c, got), c


def test_rounding_table_holds_what_it_names():
    T = ec.rounding_table()
    bits = T.view(torch.int32)
    r = T.to(torch.bfloat16).float().view(torch.int32)
    for v, want in ((0x3F808000, 0x3F800000), (0x3F818000, 0x3F820000), (0x3F807FFF, 0x3F800000), (0x3F808001, 0x3F810000),
                    (0x3F817FFF, 0x3F810000), (0x3F818001, 0x3F820000), (0x7F7F0000, 0x7F7F0000), (0x7F7F7FFF, 0x7F7F0000)):
        for neg in (0, 1 << 31):      # as int32, the negative counterpart of bit pattern v is v - 2^31
            at = bits == v - neg
            assert int(at.sum()) >= 4 and bool((r[at] == want - neg).all()), hex(v)
            assert len({int(j) % 4 for j in at.nonzero()[:, 1]}) == 4, hex(v)      # every position of a 16-byte group
    assert int((bits == 0).sum()) >= 4 and int((bits == -(1 << 31)).sum()) >= 4
    assert float(T[ec.ROW_INF, ec.COL_INF]) == 3.3961775292304601e38 and torch.isinf(T.to(torch.bfloat16).float()[ec.ROW_INF, ec.COL_INF])
    assert int(torch.isinf(T.to(torch.bfloat16).float()).sum()) == 1 and int(torch.isnan(T).sum()) == 1 and bool(torch.isnan(T[ec.ROW_NAN, ec.COL_NAN]))
    sub = (T != 0) & (T.abs() < 2.0 ** -126)
    assert int(sub.sum()) == len(ec.SUBNORMALS) and bool(sub[ec.ROW_SUBNORMAL].any()) and int(sub.sum()) == int(sub[ec.ROW_SUBNORMAL].sum())
    for site in ("A", "W"):
        want, ok = ec.rounding_expected(site)
        assert int((~ok).sum()) == (ec.ROUND_N if site == "A" else ec.ROUND_M) - 1 + len(ec.SUBNORMALS)      # the 0 x inf products, the subnormals
