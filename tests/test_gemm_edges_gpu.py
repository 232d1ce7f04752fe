"""gemm_f32_kernel and gemm_bf16_kernel at tile, K-step and split-K edges (tests/gemm_edge_cases.py), one launch per case through
artalk_op_gemm_rows (forced tile and split, `used_cfg` and `used_splitk` asserted), artalk_op_gemm / artalk_op_gemm_blocked (the blocked
sum) and artalk_op_gemm_bf16 (empty slabs, grid.z batches).

Every case: the output lies in a buffer filled with the 0xABABABAB pattern, 256 words longer either side than the launch may touch;
where the form adds into C, the payload starts as the residual.  After the launch every word outside the M x N payload - pitch columns,
the word in front of an offset C, both bands - still holds the fill (the whole buffer is compared as int32 with an image built on the
host), every payload word is written (no fill, no NaN), the payload equals the int64 reference (exact cases) or lies within
dino_cases.allowance of the float64 one (rounded cases), and a second launch gives the same bits.  Run with -s for error / e32 and
error / allowance of every rounded case and, for the fp32 kernel, the number of elements that differ in any bit from the CPU emulation
of its sum order (reported, not asserted: that the MFMA rounds like one fmaf per product is the design's reading, not pinned here)."""
import ctypes as C

import pytest
import torch

import gemm_edge_cases as ec
from artalk_amd import capi

pytestmark = pytest.mark.gpu

_payloads = {}      # case id -> payload, for the bit comparisons between two cases
_worst = {}         # (family, mode, tile) -> largest error / allowance
_emu = {}           # (family, tile) -> [elements that differ from the emulation, elements]


def _s():
    return capi.current_stream_ptr()


def _image(c):
    """(int32 image of the output buffer before the launch, indices [nb][M][N] of the payload words)"""
    span = (c.nb - 1) * c.M * c.N + (c.M - 1) * c.ldc + c.N
    assert c.nb == 1 or c.ldc == c.N
    img = torch.full((ec.GUARD + c.off + span + ec.GUARD,), ec.FILL, dtype=torch.int32)
    idx = (ec.GUARD + c.off + torch.arange(c.nb)[:, None, None] * (c.M * c.N) + torch.arange(c.M)[None, :, None] * c.ldc
           + torch.arange(c.N)[None, None, :])
    if c.res:
        img[idx] = ec.data(c).R.view(torch.int32)
    return img, idx


def _offset(t, off, n, pitch=None, rows=1):
    """a device buffer that holds the rows of t at `pitch`, `off` floats past its (16-byte aligned) start, among NaN"""
    pitch = pitch or n
    host = torch.full((off + (rows - 1) * pitch + n,), float("nan"))
    host[off:].as_strided((rows, n), (pitch, 1)).copy_(t.reshape(rows, n))
    dev = host.cuda()
    assert dev.data_ptr() % 16 == 0
    return dev


def _launch(c, dev, img):
    """one launch into a fresh copy of the image; returns the buffer as it is afterwards (CPU, int32)"""
    L = capi.lib()
    buf = img.cuda()
    assert buf.data_ptr() % 16 == 0
    Cp = buf.data_ptr() + 4 * (ec.GUARD + c.off)
    bias = dev["bias"].data_ptr() + 4 * c.off if c.bias else None
    gate = dev["gate"].data_ptr() + 4 * c.off if c.gate else None
    A, W = dev["A"].data_ptr(), dev["W"].data_ptr()
    if c.entry == "rows":
        used = [C.c_int32(-7), C.c_int32(-7)]
        assert L.artalk_op_gemm_rows(C.byref(c.rows_args(A, W, Cp, bias, gate, used)), _s()) == capi.OK, c
        assert (used[0].value, used[1].value) == (c.tile, c.S), c      # the launch reached the kernel it names
    elif c.entry in ("dense", "blocked"):
        assert c.layout == "aligned" and c.S == 1 and c.nb == 1
        entry = L.artalk_op_gemm_blocked if c.entry == "blocked" else L.artalk_op_gemm
        assert entry(A, c.K, W, bias, gate, Cp if c.res else None, Cp, c.M, c.N, c.K, c.act, _s()) == capi.OK, c
    else:
        assert c.layout == "aligned"
        cfg = c.tile | ((c.S << 8) if c.S > 1 else 0) | ((c.nb << 16) if c.nb > 1 else 0)
        assert L.artalk_op_gemm_bf16(A, c.K, W, bias, gate, Cp if c.res else None, Cp, c.M, c.N, c.K, c.act, cfg, _s()) == capi.OK, c
    torch.cuda.synchronize()
    return buf.cpu()


def _run(c):
    """the payload [nb][M][N] (float32, CPU) of a case, launched twice and checked for everything but its values"""
    d = ec.data(c)
    dev = {"A": d.A.cuda(), "W": d.W.cuda()}
    assert dev["A"].is_contiguous() and dev["W"].is_contiguous() and dev["A"].data_ptr() % 16 == 0 and dev["W"].data_ptr() % 16 == 0
    if c.bias:
        dev["bias"] = _offset(d.bias, c.off, c.nb * c.N)
    if c.gate:
        dev["gate"] = _offset(d.gate, c.off, c.N, c.ldg, c.M)
    img, idx = _image(c)
    got = _launch(c, dev, img)
    again = _launch(c, dev, img)
    expect = img.clone()
    expect[idx] = got[idx]
    assert torch.equal(got, expect), f"{c}: a word outside the payload changed"
    pay = got[idx]
    assert not bool((pay == ec.FILL).any()), f"{c}: a payload word still holds the fill"
    assert torch.equal(got, again), f"{c}: a second launch gives other bits"
    pay = pay.view(torch.float32)
    assert not bool(torch.isnan(pay).any()), f"{c}: NaN in the payload"
    if c.family == "rounded":
        _payloads[c.id] = pay
    return pay


def _payload(c):
    return _payloads[c.id] if c.id in _payloads else _run(c)


def _judge(c, pay):
    want, e32, allow = ec.bar(c)
    if c.kind == "exact":
        assert torch.equal(pay.double(), want.double()), (c, int((pay.double() != want.double()).sum()))
        return
    err = float((pay.double() - want).abs().max())
    line = f"{c}: error {err:.2e}, error / e32 {err / e32:.2f}, error / allowance {err / allow:.2f}"
    key = (c.family, c.mode, c.tile)
    _worst[key] = max(_worst.get(key, 0.0), err / allow)
    if c.mode == 0:
        diff = int((pay.view(torch.int32) != ec.emulate(c).view(torch.int32)).sum())
        line += f"; {diff} of {pay.numel()} elements differ from the emulated order"
        if c.act == ec.ACT_NONE:      # (an activation is evaluated by the kernel's own polynomial: no bit match to expect)
            e = _emu.setdefault((c.family, c.tile), [0, 0])
            e[0] += diff
            e[1] += pay.numel()
    print(line)
    assert err <= allow, (c, err / allow)


def _ids(cs):
    return [pytest.param(c, id=c.id) for c in cs]


@pytest.mark.parametrize("c", _ids(ec.select("edge")))
def test_tile_edges(c):
    _judge(c, _run(c))


@pytest.mark.parametrize("c", _ids(ec.select("order")))
def test_tile_order(c):
    _judge(c, _run(c))


@pytest.mark.parametrize("c", _ids(ec.select("ksteps")))
def test_k_steps(c):
    _judge(c, _run(c))


@pytest.mark.parametrize("c", _ids(ec.select("split")))
def test_split_k(c):
    _judge(c, _run(c))


@pytest.mark.parametrize("c", _ids(ec.select("empty") + ec.select("batch")))
def test_bf16_empty_slabs_and_batches(c):
    _judge(c, _run(c))


@pytest.mark.parametrize("c", _ids(ec.select("rounded")))
def test_rounded(c):
    pay = _payload(c)
    _judge(c, pay)
    if c.layout == "unaligned":      # the 16-byte epilogue of the same case: same sums, same epilogue arithmetic
        assert c.act == ec.ACT_NONE
        twin = ec.BY_ID[c.id[:-len("-una")]]
        assert (twin.M, twin.N, twin.K, twin.gate, twin.res, twin.seed, twin.layout) == (c.M, c.N, c.K, c.gate, c.res, c.seed, "aligned")
        assert torch.equal(pay.view(torch.int32), _payload(twin).view(torch.int32)), c


@pytest.mark.parametrize("c", _ids(ec.select("blocked")))
def test_blocked_sum(c):
    """artalk_op_gemm_blocked against the oracle, and against artalk_op_gemm (one chain): bit-equal up to K = 256 - one block, and adding
    zero changes no bit - and different in some bit from K = 288 on where the data rounds, which shows that the other instantiation ran"""
    pay = _run(c)
    _judge(c, pay)
    chain = _run(ec.Case(c.family, c.mode, c.tile, c.M, c.N, c.K, c.kind, bias=c.bias, gate=c.gate, res=c.res, entry="dense"))
    same = torch.equal(pay.view(torch.int32), chain.view(torch.int32))
    if c.K <= ec.BLOCK:
        assert same, c
    elif c.kind == "rounded":
        assert not same, c


@pytest.mark.parametrize("tile", list(ec.BF16_TILES))
@pytest.mark.parametrize("site", ["A", "W"])
def test_bf16_rounding(site, tile):
    """fp32 -> bf16 to nearest even at ties, at the largest finite value and at overflow, NaN kept: the product with the identity is the
    rounded operand itself.  site A: the cast in gemm_bf16_kernel's lstore; site W: pack_bf16_kernel."""
    M, N, K = ec.ROUND_M, ec.ROUND_N, ec.ROUND_K
    A, W = ec.rounding_operands(site)
    want, ok = ec.rounding_expected(site)
    dA, dW = A.cuda(), W.cuda()
    img = torch.full((2 * ec.GUARD + M * N,), ec.FILL, dtype=torch.int32)
    buf = img.cuda()
    used = [C.c_int32(-7), C.c_int32(-7)]
    a = capi.GemmRowsArgs(mode=2, M=M, N=N, K=K, A=dA.data_ptr(), lda=K, a_elems=M * K, W=dW.data_ptr(), ldw=K, w_elems=N * K,
                          C=buf.data_ptr() + 4 * ec.GUARD, ldc=N, c_elems=M * N, force_cfg=tile, used_cfg=C.pointer(used[0]),
                          used_splitk=C.pointer(used[1]))
    assert capi.lib().artalk_op_gemm_rows(C.byref(a), _s()) == capi.OK and (used[0].value, used[1].value) == (tile, 1)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool((got[:ec.GUARD] == ec.FILL).all()) and bool((got[ec.GUARD + M * N:] == ec.FILL).all())
    got = got[ec.GUARD:ec.GUARD + M * N].reshape(M, N)
    assert not bool((got == ec.FILL).any())
    gf = got.view(torch.float32)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(gf) & ok, nan & ok), "NaN in the operand's row (column) and nowhere else"
    if site == "A":
        assert bool(nan[ec.ROW_NAN].all()) and float(gf[ec.ROW_INF, ec.COL_INF]) == float("inf")
    else:
        assert bool(nan[:, ec.ROW_NAN].all()) and float(gf[ec.COL_INF, ec.ROW_INF]) == float("inf")
    sel = ok & ~nan
    zero = want == 0
    assert torch.equal(got[sel & ~zero], want.view(torch.int32)[sel & ~zero]), int((got != want.view(torch.int32))[sel & ~zero].sum())
    assert bool((gf[sel & zero] == 0).all())
    src = (A if site == "A" else W.t())[:N]
    sub = (src != 0) & (src.abs() < 2.0 ** -126)
    for r, col in sub.nonzero().tolist():
        print(f"site {site} tile {tile}: float32 subnormal {int(src[r, col].view(torch.int32)) & 0xFFFFFFFF:#010x} -> "
              f"{int(got[r, col]) & 0xFFFFFFFF:#010x} (round to nearest even: {int(want[r, col].view(torch.int32)) & 0xFFFFFFFF:#010x})")


def test_report():
    """with -s: the largest error / allowance per family and tile, and the bit matches with the emulated order (activation none)"""
    for (family, mode, tile), r in sorted(_worst.items()):
        print(f"{family} mode {mode} tile {tile}: largest error / allowance {r:.2f}")
    for (family, tile), (diff, n) in sorted(_emu.items()):
        print(f"{family} fp32 tile {tile}: {diff} of {n} elements differ in some bit from the emulated order")
