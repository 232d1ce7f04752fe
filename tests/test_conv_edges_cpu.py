"""The conv edge table (tests/conv_edge_cases.py) without a GPU: through artalk_op_conv2d_plan - plan_conv, the function both launchers
switch on - the table reaches all sixteen instantiations of the two conv kernels, every case plans as the table says, every alignment
variant lowers exactly the VA or VB the launcher documents, and the sum family sits on both sides of a block boundary of the
three-level sum; the plan refuses what artalk_op_conv2d_ex refuses; and the allowance of tests/test_conv_edges_gpu.py can see the edges:
per family, a float64 "wrong reading" of the reference - what a kernel with an off-by-one at that edge would compute - misses the case's
allowance by more than 2 x.  Run with -s for the instantiation of every case and the size of every miss."""
import ctypes as C

import pytest
import torch

import conv_edge_cases as ce
from artalk_amd import capi

P = 1 << 26      # a 16-byte aligned address that is never dereferenced


def _plan(c, mode):
    return capi.conv2d_plan(*ce.plan_args(c, ce.MODES.index(mode), base=P))


def test_the_symbol_is_exported():
    assert "artalk_op_conv2d_plan" in capi.SYMBOLS and hasattr(capi.lib(), "artalk_op_conv2d_plan")


@pytest.mark.parametrize("mode", ce.MODES)
@pytest.mark.parametrize("case", ce.CASES, ids=ce.case_id)
def test_every_case_plans_as_the_table_says(case, mode):
    got = _plan(case, mode)
    print(f"{ce.case_id(case)} {mode}: {capi.conv_kernel_name(got)}, grid {got['grid_x']} x {got['grid_y']}, {got['steps']} steps")
    assert got == ce.expected_plan(case, mode)


def test_the_table_reaches_all_sixteen_instantiations():
    reached = {}
    for c in ce.CASES:
        for mode in ce.MODES:
            reached.setdefault(capi.conv_kernel_name(_plan(c, mode)), []).append(ce.case_id(c))
    tf = ("true", "false")
    want = {f"conv_mfma_kernel<{nt},{va},{vb}>" for nt in (1, 2) for va in tf for vb in tf}
    want |= {f"conv_bf16_kernel<{nt},{np},{va}>" for nt in (1, 2) for np in (3, 1) for va in tf}
    for name in sorted(reached):
        print(f"{name}: {len(reached[name])} cases, first {reached[name][0]}")
    assert set(reached) == want and len(want) == 16
    # ... and each one by a case of a Cout, Cin or alignment family, not only by luck of a sum or pixel case
    by_family = {capi.conv_kernel_name(_plan(c, m)) for c in ce.CASES for m in ce.MODES if c.family in ("cout", "cin", "align")}
    assert by_family == want


def test_the_families_hold_the_edges_they_name():
    shapes = lambda fam: [c.shape for c in ce.CASES if c.family == fam]
    assert {s[1] for s in shapes("cout")} == {1, 31, 32, 33, 36, 63, 64, 65, 68, 96, 100} and {s[0] for s in shapes("cout")} == {8, 9}
    assert {s[0] for s in shapes("cin") if s[2] == 3} == {1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 40}
    assert {s[0] for s in shapes("cin") if s[2] == 1} == {8, 24, 33} and {s[1] for s in shapes("cin")} == {16, 40}
    assert {s[3] * s[4] * s[5] for s in shapes("pixel")} >= {127, 128, 129} and (8, 16, 3, 1, 129, 1) in shapes("pixel")
    straddle = [c for c in ce.CASES if c.family == "pixel" and c.shape[3] == 3]
    assert len(straddle) == 1 and ce.BM % (straddle[0].shape[4] * straddle[0].shape[5]) != 0 and 2 * straddle[0].shape[4] * straddle[0].shape[5] < ce.BM
    assert {"in_scale", "out_scale", "noise"} <= set(straddle[0].on) and "noise_shared" not in straddle[0].on
    assert {c.variant for c in ce.CASES if c.family == "stride"} == {"stride+8", "stride+5"} and all(s[3] == 3 for s in shapes("stride"))
    for nt_cout in (16, 40):
        assert {c.variant for c in ce.CASES if c.family == "align" and c.shape[1] == nt_cout} == {"aligned", "x+1", "w+1", "in_scale+1", "stride+1"}
    for c in ce.CASES:
        if c.variant != "aligned":
            assert ce.twin(c) in ce.CASES or c.family == "stride"      # (a stride case's twin is run by the GPU file on the fly)


@pytest.mark.parametrize("mode", ce.MODES)
def test_sum_family_sits_on_both_sides_of_a_block_boundary(mode):
    """15 / 16 / 17 steps in fp32 and 7 / 8 / 9 in the bf16 modes, and one k = 3 count of BLOCK n + 1, as the plan counts them: a change
    of CV_BK or CB_BK that moved the edge fails here."""
    blk = ce.BLOCK[mode]
    seen = set()
    for c in ce.CASES:
        if c.family == "sum" and c.shape[0] in ce.SUM_STEPS[mode]:
            steps = _plan(c, mode)["steps"]
            assert steps == ce.SUM_STEPS[mode][c.shape[0]], (c.shape, steps)
            seen.add((c.shape[2], steps))
    assert {s for k, s in seen if k == 1} == {blk - 1, blk, blk + 1}
    assert any(k == 3 and s > blk and s % blk == 1 for k, s in seen)


@pytest.mark.parametrize("mode", ce.MODES)
def test_alignment_variants_lower_exactly_what_the_launcher_documents(mode):
    n = 0
    for c in ce.CASES:
        if c.variant == "aligned" or c.family not in ("align", "stride"):
            continue
        base, got = _plan(ce.twin(c), mode), _plan(c, mode)
        assert base["VA"] == 1 and base["VB"] == (1 if mode == "f32" else -1), "the twin must take the vector loads"
        want = dict(base)
        if c.variant == "w+1":
            want["VB"] = 0 if mode == "f32" else -1      # the bf16 modes read the packed copy: nothing changes
        elif c.variant != "stride+8":                    # (a stride that stays a multiple of 4 floats keeps the vector loads)
            want["VA"] = 0
        assert got == want, (ce.case_id(c), mode)
        n += 1
    assert n == 12


def test_plan_output_length_and_its_own_refusals():
    L = capi.lib()
    args = ce.plan_args(ce.CASES[0], 0, base=P)
    full = (C.c_int32 * 9)()
    assert L.artalk_op_conv2d_plan(*args, full, 9) == 9
    assert L.artalk_op_conv2d_plan(*args, None, 0) == 9
    short = (C.c_int32 * 9)(*([-77] * 9))
    assert L.artalk_op_conv2d_plan(*args, short, 3) == 9
    assert list(short) == list(full)[:3] + [-77] * 6
    big = (C.c_int32 * 12)(*([-77] * 12))
    assert L.artalk_op_conv2d_plan(*args, big, 12) == 9 and list(big) == list(full) + [-77] * 3
    assert L.artalk_op_conv2d_plan(*args, None, 9) == capi.EINVAL and L.artalk_op_conv2d_plan(*args, full, -1) == capi.EINVAL


def test_plan_refuses_what_conv2d_ex_refuses():
    """The same arguments to both entry points: every refusal of artalk_op_conv2d_ex that lies in the plan's arguments, and beside each
    the nearest accepted value (the plan alone: the op would touch the device)."""
    L = capi.lib()
    p = C.c_void_p(P)
    out9 = (C.c_int32 * 9)()

    def both(prec=0, x=P, xb=0, w=P, B=1, H=4, W=4, Cin=16, Cout=16, k=3):
        ex = L.artalk_op_conv2d_ex(C.c_void_p(x) if x else None, xb, C.c_void_p(w) if w else None, p, B, H, W, Cin, Cout, k, None, None, 1.0,
                                   None, 0, None, None, 0, None, None, None, prec, None)
        return ex, L.artalk_op_conv2d_plan(x, xb, w, 0, B, H, W, Cin, Cout, k, prec, out9, 9)

    refused = [dict(x=0), dict(w=0), dict(B=0), dict(H=0), dict(W=0), dict(Cin=0), dict(Cout=0), dict(B=-1), dict(Cin=-8), dict(k=0), dict(k=2),
               dict(k=5), dict(xb=4 * 4 * 16 - 1), dict(xb=-1), dict(B=1 << 10, H=1 << 10, W=(1 << 10) + 1), dict(H=1 << 16, W=1 << 15)]
    for prec in (0, 1, 2):
        for kw in refused:
            assert both(prec, **kw) == (capi.EINVAL, capi.EINVAL), (prec, kw)
    for prec in (-1, 3, 100):
        assert both(prec) == (capi.EINVAL, capi.EINVAL)
    plan = lambda prec=0, x=P, xb=0, w=P, B=1, H=4, W=4, Cin=16, Cout=16, k=3: L.artalk_op_conv2d_plan(x, xb, w, 0, B, H, W, Cin, Cout, k, prec, out9, 9)
    for prec in (0, 1, 2):
        for kw in (dict(), dict(k=1), dict(xb=4 * 4 * 16), dict(xb=4 * 4 * 16 + 1), dict(B=1 << 10, H=1 << 10, W=1 << 10),
                   dict(x=P + 4), dict(w=P + 4), dict(Cin=1, Cout=1)):
            assert plan(prec, **kw) == 9, (prec, kw)


# ---- what the allowance can tell apart ----
def _miss(tag, case, mode, wrong):
    want, allowed, e32 = ce.reference(case, mode)
    miss = float((wrong - want).abs().max())
    print(f"{mode} {ce.case_id(case)} {tag}: misses by {miss:.3e} = {miss / allowed:.1f} x the allowance {allowed:.2e} (e32 {e32:.2e})")
    assert miss > 2.0 * allowed, f"{mode} {ce.case_id(case)} {tag}: {miss:.3e} is within 2 x the allowance {allowed:.3e}"


def _family(name):
    return [c for c in ce.CASES if c.family == name]


@pytest.mark.parametrize("mode", ce.MODES)
@pytest.mark.parametrize("case", _family("cin"), ids=ce.case_id)
def test_wrong_reading_last_cin_chunk_dropped(case, mode):
    """The channels of the last 8-group (one thread's load in either kernel, the packed weight's padding unit) never reach the sum; and
    the smallest form of it, the last channel alone."""
    a = ce.case_inputs(case.shape, case.on, case.seed)
    Cin = case.shape[0]
    for tag, lo in (("last 8-group of Cin dropped", (Cin - 1) // 8 * 8), ("last channel dropped", Cin - 1)):
        x = a["x"].clone()
        x[:, lo:] = 0.0
        with torch.no_grad():
            _miss(tag, case, mode, ce.statement(mode, {**a, "x": x}))


@pytest.mark.parametrize("mode", ce.MODES)
@pytest.mark.parametrize("case", _family("cout"), ids=ce.case_id)
def test_wrong_reading_last_column_of_a_cout_tile_dropped(case, mode):
    """The last live column, and the last column of each full 32-wide accumulator, sums nothing."""
    a = ce.case_inputs(case.shape, case.on, case.seed)
    Cout = case.shape[1]
    for co in sorted({Cout - 1} | {t for t in (31, 63, 95) if t < Cout}):
        w = a["w"].clone()
        w[co] = 0.0
        with torch.no_grad():
            _miss(f"output channel {co} dropped", case, mode, ce.statement(mode, {**a, "w": w}))


@pytest.mark.parametrize("mode", ce.MODES)
@pytest.mark.parametrize("case", _family("sum"), ids=ce.case_id)
def test_wrong_reading_last_sum_block_dropped(case, mode):
    """Every K step after the last closed block - the partial `mid` that is added after the loop - is lost (for a count of exactly one
    block or less: everything)."""
    a = ce.case_inputs(case.shape, case.on, case.seed)
    Cin, _, k = case.shape[:3]
    steps = ce.k_steps(mode, Cin, k)[0]
    first_lost = (steps - 1) // ce.BLOCK[mode] * ce.BLOCK[mode]
    w = a["w"].clone()
    lost = 0
    for tap in range(k * k):
        for ci in range(Cin):
            if ce.step_of(mode, Cin, k, tap, ci) >= first_lost:
                w[:, ci, tap // k, tap % k] = 0.0
                lost += 1
    assert 0 < lost <= ce.BLOCK[mode] * ce.BK[mode]
    with torch.no_grad():
        _miss(f"steps {first_lost} .. {steps - 1} of {steps} dropped ({lost} of {k * k * Cin} products)", case, mode, ce.statement(mode, {**a, "w": w}))


@pytest.mark.parametrize("mode", ce.MODES)
def test_wrong_reading_sample_index_from_the_tiles_first_pixel(mode):
    """Every per-sample operand (input scale, output scale, noise) of a pixel taken from the sample of its tile's first pixel."""
    (case,) = [c for c in _family("pixel") if c.shape[3] > 1]
    a = ce.case_inputs(case.shape, case.on, case.seed)
    _, _, _, B, H, W = case.shape
    with torch.no_grad():
        per_sample = []
        for b in range(B):
            ab = dict(a)
            for key in ("in_scale", "out_scale", "noise"):
                ab[key] = a[key][b:b + 1].expand(B, *a[key].shape[1:]).contiguous()
            per_sample.append(ce.statement(mode, ab))
    m = torch.arange(B * H * W)
    first = (m // ce.BM * ce.BM) // (H * W)
    assert int((first != m // (H * W)).sum()) > 0
    stacked = torch.stack(per_sample).permute(0, 1, 3, 4, 2).reshape(B, B * H * W, -1)      # [operand sample][pixel][Cout]
    wrong = stacked[first, m].reshape(B, H, W, -1).permute(0, 3, 1, 2)
    _miss("sample index of the tile's first pixel", case, mode, wrong)


@pytest.mark.parametrize("mode", ce.MODES)
@pytest.mark.parametrize("case", _family("stride"), ids=ce.case_id)
def test_wrong_reading_stride_padding_read_as_data(case, mode):
    """x_bstride taken as H W Cin: the floats between two samples are read as the next sample's first values."""
    a = ce.case_inputs(case.shape, case.on, case.seed)
    Cin, _, _, B, H, W = case.shape
    stride, tight = ce.layout(case)["x_bstride"], H * W * Cin
    g = torch.Generator().manual_seed(99)
    buf = torch.randn(B, stride, generator=g, dtype=torch.float32).double()
    buf[:, :tight] = a["x"].permute(0, 2, 3, 1).reshape(B, tight)
    x = buf.reshape(-1)[:B * tight].reshape(B, H, W, Cin).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(x[0], a["x"][0]) and not torch.equal(x[1], a["x"][1])
    with torch.no_grad():
        _miss("padding between samples read as data", case, mode, ce.statement(mode, {**a, "x": x}))
