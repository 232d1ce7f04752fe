"""The small kernels between the GEMMs of the AR / VAE / style stages (csrc/ar_glue.hip), one launch each through artalk_op_*,
against float64 CPU math or the oracle's restatement of the reference, and the status bits 0, 1, 2 they raise - alone and through the model.

Every output lives between two guards (Guarded): guard bytes and output are pre-filled with 0xFF - an fp32 NaN - for float buffers and with
0xAB for integer ones, so an element the kernel does not write fails the comparison and a write outside the output is seen.

Bars.  Exact where the operation involves no rounding (bits, copies, zero padding, maxima, a single fp32 add); 1e-6 absolute for the
features built from bits (sums of at most five terms of magnitude 1/sqrt(32): the bar test_bsq_history_matches_oracle uses for the same
quantities); otherwise a rounding bound derived per op beside its test, k * 2^-23 * the largest intermediate of that element, k = the
number of fp32 roundings of the expression."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import p8_format as p8

pytestmark = pytest.mark.gpu

PN = (1, 5, 25, 50, 100)
OFF = (0, 1, 6, 31, 81, 181)
CD, E768, MD, EK = 32, 768, 106, 128
HQ = 1.0 / math.sqrt(32.0)
EPS = 2.0 ** -23
GUARD = 65536         # guard bytes on either side: a multiple of 16 (the guarded tensor stays 16-byte aligned), and more than a workgroup of
#                       any kernel here can write past its rows (vq_embed: 16 tokens x 768 floats = 48 KiB), so a missing tail check is seen here


def _lib():
    from artalk_amd import capi
    return capi, capi.lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_KEEP = []


def _dev(t):
    """Device copy of a host tensor, kept alive until the test ends: the launches are asynchronous, and a temporary handed over as
    `_p(_dev(x))` would return to the caching allocator - and to the next upload - before the kernel has read it."""
    d = t.contiguous().cuda()
    _KEEP.append(d)
    return d


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Guarded:
    """A device tensor of `shape` with GUARD bytes before and after it; see the module docstring."""

    def __init__(self, shape, dtype=torch.float32):
        self.fill = 0xFF if dtype.is_floating_point else 0xAB
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.n = n
        self.raw = torch.full((GUARD + (n + 15) // 16 * 16 + GUARD,), self.fill, dtype=torch.uint8, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(shape)

    def set(self, value):
        self.t.copy_(value)
        return self

    def check(self, what=""):
        torch.cuda.synchronize()
        raw = self.raw.cpu()
        assert bool((raw[:GUARD] == self.fill).all()), f"{what}: wrote before the buffer"
        assert bool((raw[GUARD + self.n:] == self.fill).all()), f"{what}: wrote past the buffer"

    def cpu(self):
        self.check()
        return self.t.cpu()


def _untouched(t_cpu):
    """True where a (float or integer) element still holds its pre-fill."""
    fill = 0xFF if t_cpu.dtype.is_floating_point else 0xAB
    b = t_cpu.contiguous().view(torch.uint8).view(t_cpu.shape + (t_cpu.element_size(),)) if t_cpu.element_size() > 1 \
        else t_cpu.contiguous().view(torch.uint8).unsqueeze(-1)
    return (b == fill).all(dim=-1)


def _status(v=0):
    return torch.full((1,), v, dtype=torch.int32, device="cuda")


def _st(s):
    torch.cuda.synchronize()
    return int(s.item())


def _assert_within(got, ref64, bound64, what):
    """|got - ref| <= bound per element; a NaN (an element that was never written) fails."""
    got64 = got.double()
    assert bool(torch.isfinite(got64).all()), f"{what}: {int((~torch.isfinite(got64)).sum())} element(s) not written / not finite"
    err = (got64 - ref64).abs()
    bad = err > bound64
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err / bound64.clamp_min(1e-300)).max()))


def _up(h, T=100):
    """[B, pn, 32] -> [B, 100, 32]: linear upsampling as the reference does it (bitwise_vae.py:284, F.interpolate mode='linear')."""
    if h.shape[1] == T:
        return h
    return F.interpolate(h.permute(0, 2, 1).contiguous(), size=(T), mode="linear").permute(0, 2, 1).contiguous()


def _area(f, pn):
    return F.interpolate(f.permute(0, 2, 1).contiguous(), size=(pn), mode="area").permute(0, 2, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- ar_bits_next
def _tie_logits(B, pn, seed):
    """Random logits [B * pn, 64] with, in the first token of the first clip and the last token of the last one, pairs that tie:
    l0 == l1, (+0.0, -0.0), (-0.0, +0.0), and an equal negative pair.  torch.argmax takes the first index of a tie: bit 0."""
    lg = torch.randn(B * pn, 64, generator=_gen(seed))
    ties = []
    for row, c0 in ((0, 0), (B * pn - 1, 28)):
        for k, (a, b) in enumerate(((0.37, 0.37), (0.0, -0.0), (-0.0, 0.0), (-2.5, -2.5))):
            lg[row, 2 * (c0 + k)], lg[row, 2 * (c0 + k) + 1] = a, b
            ties.append((row, c0 + k))
    return lg, ties


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
def test_ar_bits_next_single_level(level):
    capi, L = _lib()
    B, pn, off = 3, PN[level], OFF[level]
    lg, ties = _tie_logits(B, pn, 10 + level)
    want = lg.view(B, pn, CD, 2).argmax(dim=-1).to(torch.uint8)
    for row, c in ties:
        assert int(want[row // pn, row % pn, c]) == 0
    bits = Guarded((B, 181, CD), torch.uint8)
    fhat = Guarded((B, 100, CD))
    nxt = Guarded((B, PN[level + 1] if level < 4 else 100, CD))
    if level < 4:
        fhat.t.zero_()
    st = _status()
    assert L.artalk_op_ar_bits_next(_p(_dev(lg)), _p(bits.t), _p(fhat.t), _p(nxt.t), B, level, _p(st), None) == 0
    assert _st(st) == 0
    got = bits.cpu()
    assert torch.equal(got[:, off:off + pn], want), "bits differ from the pairwise argmax (ties -> 0)"
    rest = torch.ones(181, dtype=torch.bool)
    rest[off:off + pn] = False
    assert bool(_untouched(got[:, rest]).all()), "rows of other levels were written"
    f, n = fhat.cpu(), nxt.cpu()
    if level == 4:
        assert bool(_untouched(f).all()) and bool(_untouched(n).all()), "the last level must leave fhat / nextfeat alone"
    else:
        f_ref = _up((want.float() * 2 - 1) * HQ)
        assert (f - f_ref).abs().max().item() < 1e-6
        assert (n - _area(f_ref, PN[level + 1])).abs().max().item() < 1e-6


def test_ar_bits_next_chained_levels_and_dec_input():
    """Levels 0..4 from fhat = 0: the next level's input features and the f_hat recurrence against the oracle (bitwise_vae.py:291-305),
    then the decoder input built from them (bitwise_vae.py:105-110,264-288)."""
    from conftest import get_oracle, get_state_dict
    capi, L = _lib()
    o = get_oracle("tiny")
    B = 4
    bits = Guarded((B, 181, CD), torch.uint8)
    bits.t.zero_()
    fhat = Guarded((B, 100, CD))
    x0 = Guarded((B, E768))
    g = _gen(20)
    assert L.artalk_op_ar_begin(_p(_dev(torch.randn(B, E768, generator=g))), _p(_dev(torch.randn(E768, generator=g))), _p(x0.t), _p(fhat.t),
                                B, None) == 0
    assert float(fhat.cpu().abs().max()) == 0.0
    f_ref = torch.zeros(B, 100, CD)
    for p in range(5):
        lg = torch.randn(B * PN[p], 64, generator=g)
        nxt = Guarded((B, PN[p + 1] if p < 4 else 1, CD))
        assert L.artalk_op_ar_bits_next(_p(_dev(lg)), _p(bits.t), _p(fhat.t), _p(nxt.t), B, p, None, None) == 0     # (NULL status word)
        b = bits.cpu()
        assert torch.equal(b[:, OFF[p]:OFF[p + 1]], lg.view(B, PN[p], CD, 2).argmax(-1).to(torch.uint8))
        if p < 4:
            want = o.vqidx_to_ar_vqfeat(p, b[:, :OFF[p + 1]])[:, -PN[p + 1]:]
            assert (nxt.cpu() - want).abs().max().item() < 1e-6, p
            f_ref = f_ref + _up(o.bits_to_h(b[:, OFF[p]:OFF[p + 1]]))
            assert (fhat.cpu() - f_ref).abs().max().item() < 1e-6, p
        else:
            assert bool(_untouched(nxt.cpu()).all())
            assert (fhat.cpu() - f_ref).abs().max().item() < 1e-6
    b = bits.cpu()
    cfg, sd = get_state_dict("tiny")
    dpos = sd["basic_vae.dec_pos_embed"].reshape(200, CD).float()
    prev = 0.3 * torch.randn(B, 100, CD, generator=g)
    X = Guarded((B, 200, CD))
    assert L.artalk_op_dec_input(_p(_dev(prev)), _p(fhat.t), _p(bits.t), _p(_dev(dpos)), _p(X.t), B, None) == 0
    x = X.cpu()
    assert torch.equal(x[:, :100], prev + dpos[:100]), "first half: one fp32 add of prev_fdec and dec_pos"
    want = o.vqidx_to_feat(b, False).double() + dpos[100:].double()
    assert bool(torch.isfinite(x).all()) and (x[:, 100:].double() - want).abs().max().item() < 1e-6
    assert torch.equal(bits.cpu(), b)
    x0.check()


# ---------------------------------------------------------------------------------------------------------------- status words
@pytest.mark.parametrize("col", [0, 1], ids=["l0", "l1"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "pinf", "ninf"])
@pytest.mark.parametrize("where", ["first", "last"])
def test_ar_bits_next_status_bit0(bad, col, where):
    """A non-finite logit becomes a valid-looking bit: bit 0, and only bit 0, says so.  In the first and in the last token of the last clip."""
    capi, L = _lib()
    B, level = 3, 2
    pn = PN[level]
    lg = torch.randn(B * pn, 64, generator=_gen(30))
    row = (B - 1) * pn + (0 if where == "first" else pn - 1)
    lg[row, 2 * (5 if where == "first" else 31) + col] = bad
    bits, fhat, nxt = Guarded((B, 181, CD), torch.uint8), Guarded((B, 100, CD)), Guarded((B, PN[level + 1], CD))
    fhat.t.zero_()
    st = _status()
    assert L.artalk_op_ar_bits_next(_p(_dev(lg)), _p(bits.t), _p(fhat.t), _p(nxt.t), B, level, _p(st), None) == 0
    assert _st(st) == 1
    for b in (bits, fhat, nxt):
        b.check()
    # the same data without a status word: accepted, same bits
    bits2 = Guarded((B, 181, CD), torch.uint8)
    fhat.t.zero_()
    assert L.artalk_op_ar_bits_next(_p(_dev(lg)), _p(bits2.t), _p(fhat.t), _p(nxt.t), B, level, None, None) == 0
    assert torch.equal(bits2.cpu(), bits.cpu())


def test_ar_bits_next_status_stays_clear_and_keeps_other_bits():
    capi, L = _lib()
    B, level = 3, 4
    lg = torch.randn(B * 100, 64, generator=_gen(31))
    bits = Guarded((B, 181, CD), torch.uint8)
    for before in (0, 8):
        st = _status(before)
        assert L.artalk_op_ar_bits_next(_p(_dev(lg)), _p(bits.t), None, None, B, level, _p(st), None) == 0
        assert _st(st) == before
    bits.check()


def _bsq(L, enc, st):
    B = enc.shape[0]
    bits, fdec, ms = Guarded((B, 181, CD), torch.uint8), Guarded((B, 100, CD)), Guarded((B, 180, CD))
    assert L.artalk_op_bsq_history_ex(_p(_dev(enc)), _p(bits.t), _p(fdec.t), _p(ms.t), B, _p(st), None) == 0
    return bits.cpu(), fdec.cpu(), ms.cpu()


@pytest.mark.parametrize("bad", [None, float("nan"), float("inf"), float("-inf")], ids=["finite", "nan", "pinf", "ninf"])
def test_bsq_history_ex_status_bit1(bad):
    capi, L = _lib()
    B = 3
    enc = torch.randn(B, 100, CD, generator=_gen(32))
    for pos in ((B - 1, 99, 31), (0, 0, 0)):
        e = enc.clone()
        if bad is not None:
            e[pos] = bad
        st = _status()
        bits, fdec, ms = _bsq(L, e, st)
        assert _st(st) == (0 if bad is None else 2)
        assert bool((bits <= 1).all())
    if bad is None:      # the entry point without a status word is the same kernel
        b2, f2, m2 = Guarded((B, 181, CD), torch.uint8), Guarded((B, 100, CD)), Guarded((B, 180, CD))
        assert L.artalk_op_bsq_history(_p(_dev(enc)), _p(b2.t), _p(f2.t), _p(m2.t), B, None) == 0
        assert torch.equal(b2.cpu(), bits) and torch.equal(f2.cpu(), fdec) and torch.equal(m2.cpu(), ms)


def _dec_finish_inputs(B, seed):
    g = _gen(seed)
    dec = torch.randn(B, 200, MD, generator=g)
    mean = torch.randn(MD, generator=g)
    std = 0.5 + 1.5 * torch.rand(MD, generator=g)          # [0.5, 2]: a well-conditioned division
    epos = 0.1 * torch.randn(100, MD, generator=g)
    return dec, mean, std, epos


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "pinf", "ninf"])
def test_dec_finish_status_bit2(bad):
    capi, L = _lib()
    B = 3
    dec, mean, std, epos = _dec_finish_inputs(B, 33)
    stride = 100 * MD
    for pos in ((B - 1, 199, MD - 1), (0, 100, 0)):
        d = dec.clone()
        d[pos] = bad
        out, Eb = Guarded((B * stride,)), Guarded((B, 100, EK))
        st = _status()
        assert L.artalk_op_dec_finish(_p(_dev(d)), _p(_dev(mean)), _p(_dev(std)), _p(_dev(epos)), _p(out.t), stride, 0, _p(Eb.t), B, _p(st),
                                      None) == 0
        assert _st(st) == 4
        out.check(), Eb.check()


def test_dec_finish_does_not_read_the_first_half():
    """Rows t < 100 of the decoder output belong to the previous chunk: a NaN there raises nothing and reaches nothing."""
    capi, L = _lib()
    B = 3
    dec, mean, std, epos = _dec_finish_inputs(B, 34)
    dec[:, :100] = float("nan")
    stride = 100 * MD
    out, Eb = Guarded((B * stride,)), Guarded((B, 100, EK))
    st = _status()
    assert L.artalk_op_dec_finish(_p(_dev(dec)), _p(_dev(mean)), _p(_dev(std)), _p(_dev(epos)), _p(out.t), stride, 0, _p(Eb.t), B, _p(st),
                                  None) == 0
    assert _st(st) == 0
    assert bool(torch.isfinite(out.cpu()).all()) and bool(torch.isfinite(Eb.cpu()).all())
    # and without a status word
    assert L.artalk_op_dec_finish(_p(_dev(dec)), _p(_dev(mean)), _p(_dev(std)), _p(_dev(epos)), _p(out.t), stride, 0, _p(Eb.t), B, None, None) == 0
    out.check()


# ---------------------------------------------------------------------------------------------------------------- vq_embed
def _vq_embed_case(n, with_style):
    """Bound.  The kernel computes ((fma chain over the 32 code dims) + be) + pos in fp32.  With u = 2^-24: a chain of 32 fmas is off by at
    most gamma_32 * sum_c |We[e,c] * feat[c]|, gamma_k = k u / (1 - k u); each of the two adds rounds once more, relative to a partial
    sum that sum_c |We * feat| + |be| + |pos| bounds.  Together (32 + 2) u of that sum to first order; 36 u covers the higher-order terms
    ((1 + u)^34 - 1 < 34.0001 u) and the rounding of the float64 reference with a wide margin, and nothing else."""
    capi, L = _lib()
    B = 3
    g = _gen(40 + n + (1000 if with_style else 0))
    feat = torch.randn(B, n, CD, generator=g)
    We = torch.randn(E768, CD, generator=g) / math.sqrt(CD)
    be = torch.randn(E768, generator=g)
    pos = torch.randn(n, E768, generator=g)
    style = torch.randn(B, E768, generator=g) if with_style else None
    pos0 = torch.randn(E768, generator=g) if with_style else None
    xoff = 1 if with_style else 0
    xrows = n + xoff
    X = Guarded((B, xrows, E768))
    assert L.artalk_op_vq_embed(_p(_dev(feat)), n, _p(_dev(We)), _p(_dev(be)), _p(_dev(pos)), _p(X.t), xrows, xoff,
                                _p(_dev(style)) if with_style else None, _p(_dev(pos0)) if with_style else None, B, None) == 0
    x = X.cpu()
    ref = feat.double() @ We.double().T + be.double() + pos.double()
    mag = feat.double().abs() @ We.double().abs().T + be.double().abs() + pos.double().abs()
    _assert_within(x[:, xoff:], ref, 36 * 2.0 ** -24 * mag, f"vq_embed n={n} xoff={xoff}")
    if with_style:
        assert torch.equal(x[:, 0], style + pos0), "style row: one fp32 add"


@pytest.mark.parametrize("n", [1, 5, 25, 50, 100, 180])
def test_vq_embed_scale_step_form(n):
    """xoff = 0, no style row: row 0 of every clip's block is token 0 (tails of 1, 5, 9, 2, 4, 4 tokens in the last workgroup)."""
    _vq_embed_case(n, False)


@pytest.mark.parametrize("n", [5, 180])
def test_vq_embed_history_form(n):
    _vq_embed_case(n, True)


# ---------------------------------------------------------------------------------------------------------------- dec_finish
@pytest.mark.parametrize("chunk", [0, 2])
def test_dec_finish(chunk):
    """out = dec * std + mean: two roundings (one if contracted to an fma), of intermediates bounded by A = |dec * std| + |mean|: 2 * 2^-23 * A.
    E = (m - mean) / std + epos: m carries the error above, the subtraction, the division and the last add round once each, and every
    intermediate is bounded by I = max(2 A, 2 A / std, |epos|, |E|): 4 * 2^-23 * I."""
    capi, L = _lib()
    B, n_chunks = 3, 3
    dec, mean, std, epos = _dec_finish_inputs(B, 50 + chunk)
    stride = n_chunks * 100 * MD + 40          # > 3 * 100 * 106: a wrong stride or chunk offset lands in a guard or in another chunk's rows
    out, Eb = Guarded((B, stride)), Guarded((B, 100, EK))
    st = _status()
    assert L.artalk_op_dec_finish(_p(_dev(dec)), _p(_dev(mean)), _p(_dev(std)), _p(_dev(epos)), _p(out.t), stride, chunk, _p(Eb.t), B,
                                  _p(st), None) == 0
    assert _st(st) == 0
    o, e = out.cpu(), Eb.cpu()
    d64, m64, s64 = dec[:, 100:].double(), mean.double(), std.double()
    ref = d64 * s64 + m64
    A = (d64 * s64).abs() + m64.abs()
    lo, hi = chunk * 100 * MD, (chunk + 1) * 100 * MD
    _assert_within(o[:, lo:hi].reshape(B, 100, MD), ref, 2 * EPS * A, "dec_finish out")
    rest = torch.ones(stride, dtype=torch.bool)
    rest[lo:hi] = False
    assert bool(_untouched(o[:, rest]).all()), "rows of another chunk (or the gap between clips) were written"
    e_ref = (ref - m64) / s64 + epos.double()
    I = torch.maximum(torch.maximum(2 * A, 2 * A / s64), torch.maximum(epos.double().abs(), e_ref.abs()))
    _assert_within(e[:, :, :MD], e_ref, 4 * EPS * I, "dec_finish E")
    assert bool((e[:, :, MD:].view(torch.int32) == 0).all()), "padding columns 106..127 must be +0.0"


# ---------------------------------------------------------------------------------------------------------------- the one-line ops
def test_enc_input_zero():
    """E = (0 - mean) / std + epos: the subtraction from zero is exact, the division and the add round once each:
    2 * 2^-23 * I, I = max(|mean / std|, |epos|, |E|)."""
    capi, L = _lib()
    B = 3
    _, mean, std, epos = _dec_finish_inputs(1, 60)
    Eb = Guarded((B, 100, EK))
    assert L.artalk_op_enc_input_zero(_p(_dev(mean)), _p(_dev(std)), _p(_dev(epos)), _p(Eb.t), B, None) == 0
    e = Eb.cpu()
    q = (0.0 - mean.double()) / std.double()
    ref = (q + epos.double()).expand(B, 100, MD)
    I = torch.maximum(torch.maximum(q.abs().expand(100, MD), epos.double().abs()), ref[0].abs()).expand(B, 100, MD)
    _assert_within(e[:, :, :MD], ref, 2 * EPS * I, "enc_input_zero")
    assert bool((e[:, :, MD:].view(torch.int32) == 0).all())


def test_style_input():
    """X = (motion - mean) / std: two roundings, of I = max(|motion - mean|, |X|): 2 * 2^-23 * I."""
    capi, L = _lib()
    B = 3
    g = _gen(61)
    motion = torch.randn(B * 50, MD, generator=g)
    mean = torch.randn(MD, generator=g)
    std = 0.5 + 1.5 * torch.rand(MD, generator=g)
    X = Guarded((B * 50, EK))
    assert L.artalk_op_style_input(_p(_dev(motion)), _p(_dev(mean)), _p(_dev(std)), _p(X.t), B, None) == 0
    x = X.cpu()
    d = motion.double() - mean.double()
    ref = d / std.double()
    _assert_within(x[:, :MD], ref, 2 * EPS * torch.maximum(d.abs(), ref.abs()), "style_input")
    assert bool((x[:, MD:].view(torch.int32) == 0).all())


def test_add_row():
    """X[m, :] += v: one rounding of I = max(|x|, |v|, |x + v|): 2^-23 * I.  M * D = 896 is no multiple of the 256-lane block."""
    capi, L = _lib()
    M, D = 7, 128
    g = _gen(62)
    x0, v = torch.randn(M, D, generator=g), torch.randn(D, generator=g)
    X = Guarded((M, D)).set(_dev(x0))
    assert L.artalk_op_add_row(_p(X.t), _p(_dev(v)), M, D, None) == 0
    ref = x0.double() + v.double()
    I = torch.maximum(torch.maximum(x0.double().abs(), v.double().abs().expand(M, D)), ref.abs())
    _assert_within(X.cpu(), ref, EPS * I, "add_row")


def test_ar_begin():
    """x0 = style_cond + lvlpos[0]: one rounding, 2^-23 * max(|style|, |lvlpos|, |x0|); all of fhat zeroed."""
    capi, L = _lib()
    B = 3
    g = _gen(63)
    style, lvlpos = torch.randn(B, E768, generator=g), torch.randn(181, E768, generator=g)
    x0, fhat = Guarded((B, E768)), Guarded((B, 100, CD))
    assert L.artalk_op_ar_begin(_p(_dev(style)), _p(_dev(lvlpos)), _p(x0.t), _p(fhat.t), B, None) == 0
    ref = style.double() + lvlpos[0].double()
    I = torch.maximum(torch.maximum(style.double().abs(), lvlpos[0].double().abs().expand(B, E768)), ref.abs())
    _assert_within(x0.cpu(), ref, EPS * I, "ar_begin")
    assert bool((fhat.cpu().view(torch.int32) == 0).all()), "fhat must be +0.0 everywhere"


# ---------------------------------------------------------------------------------------------------------------- style_finish
def test_style_finish():
    """Rows with has_style == 1: 1.1 * (Ws . mean_t(feat) + bs) - 0.1 * null in fp32.  With u = 2^-24: the 50-term sum and its division leave
    the mean off by at most 50 u * mean_t |feat|; the 128-term fma chain adds gamma_128 of sum_c |Ws * mean|, and carries the error of
    the mean through |Ws|; the bias add, the two products and the subtraction are three more roundings of partial results, and the fp32
    constants 1.1f and 0.1f are each off by at most u relative.  All of it relative to S = 1.1 * (sum_c |Ws[e,c]| * mean_t |feat[t,c]| +
    |bs|) + 0.1 * |null|: (50 + 128 + 3 + 2) u S to first order, 186 u S with the higher-order terms."""
    capi, L = _lib()
    B, stride = 4, 800
    g = _gen(70)
    feat = torch.randn(B * 50, 128, generator=g)
    Ws = torch.randn(E768, 128, generator=g) / math.sqrt(128)
    bs, null = torch.randn(E768, generator=g), torch.randn(E768, generator=g)
    cached = torch.randn(B, stride, generator=g)
    has = torch.tensor([1, 0, 2, 1], dtype=torch.uint8)
    sc = Guarded((B, E768))
    args = (_p(_dev(feat)), _p(_dev(Ws)), _p(_dev(bs)), _p(_dev(null)))
    assert L.artalk_op_style_finish(*args, _p(_dev(has)), _p(sc.t), B, _p(_dev(cached)), stride, None) == 0
    s = sc.cpu()
    assert torch.equal(s[1], null), "has_style == 0: the null condition, copied"
    assert torch.equal(s[2], cached[2, :E768]), "has_style == 2: row 2 of the cached conditions, copied"
    f64 = feat.double().view(B, 50, 128)
    ref = 1.1 * (f64.mean(dim=1) @ Ws.double().T + bs.double()) - 0.1 * null.double()
    S = 1.1 * (f64.abs().mean(dim=1) @ Ws.double().abs().T + bs.double().abs()) + 0.1 * null.double().abs()
    for b in (0, 3):
        _assert_within(s[b], ref[b], 186 * 2.0 ** -24 * S[b], f"style_finish row {b}")
    sc2 = Guarded((B, E768))
    assert L.artalk_op_style_finish(*args, None, _p(sc2.t), B, None, 0, None) == 0
    assert torch.equal(sc2.cpu(), null.expand(B, E768)), "no has_style table: the null condition everywhere"


# ---------------------------------------------------------------------------------------------------------------- copies
@pytest.mark.parametrize("nbytes", [16, 16 * 255, 16 * 257, 16 * 2049 * 3])
def test_broadcast16(nbytes):
    """The last size is more than 8 blocks of 256 lanes: the grid-stride loop runs."""
    capi, L = _lib()
    B = 3
    src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=_gen(80))
    dst = Guarded((B, nbytes), torch.uint8)
    assert L.artalk_op_broadcast16(_p(_dev(src)), _p(dst.t), nbytes, B, None) == 0
    assert torch.equal(dst.cpu(), src.expand(B, nbytes))


def _slot_table(pool, order):
    unit = pool.t.shape[1] * 4
    return torch.tensor([pool.t.data_ptr() + s * unit for s in order], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("s16,p16,f16", [(192, 34752, 800), (3, 5, 2)], ids=["model", "tiny"])
def test_session_gather_scatter(s16, p16, f16):
    """Pool slots [style | prev_in | prev_fdec] <-> rows of the three workspace buffers, byte for byte (32-bit words, 4 per unit)."""
    capi, L = _lib()
    n, n_slots, order = 3, 5, [3, 0, 4]
    words = 4 * (s16 + p16 + f16)
    a, b = 4 * s16, 4 * (s16 + p16)
    g = _gen(81)
    content = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_slots, words), dtype=torch.int32, generator=g)
    pool = Guarded((n_slots, words), torch.int32).set(_dev(content))
    table = _slot_table(pool, order)
    style, prev_in, fdec = Guarded((n, 4 * s16), torch.int32), Guarded((n, 4 * p16), torch.int32), Guarded((n, 4 * f16), torch.int32)
    assert L.artalk_op_session_gather(_p(table), _p(style.t), _p(prev_in.t), _p(fdec.t), s16, p16, f16, n, None) == 0
    st, pi, fd = style.cpu(), prev_in.cpu(), fdec.cpu()
    for i, s in enumerate(order):
        assert torch.equal(st[i], content[s, :a]) and torch.equal(pi[i], content[s, a:b]) and torch.equal(fd[i], content[s, b:]), (i, s)
    assert torch.equal(pool.cpu(), content), "gather must not write the pool"
    # the way back into an empty pool: the exact inverse with the style field ...
    back = Guarded((n_slots, words), torch.int32)
    t2 = _slot_table(back, order)
    assert L.artalk_op_session_scatter(_p(t2), _p(style.t), _p(prev_in.t), _p(fdec.t), s16, p16, f16, n, 1, None) == 0
    got = back.cpu()
    for s in range(n_slots):
        if s in order:
            assert torch.equal(got[s], content[s]), s
        else:
            assert bool(_untouched(got[s]).all()), f"slot {s} was not named"
    # ... and without it the first s16 units of every slot keep what they held
    back2 = Guarded((n_slots, words), torch.int32)
    t3 = _slot_table(back2, order)
    assert L.artalk_op_session_scatter(_p(t3), _p(style.t), _p(prev_in.t), _p(fdec.t), s16, p16, f16, n, 0, None) == 0
    got = back2.cpu()
    for s in range(n_slots):
        if s in order:
            assert bool(_untouched(got[s, :a]).all()), f"slot {s}: the style field was written without with_style"
            assert torch.equal(got[s, a:], content[s, a:]), s
        else:
            assert bool(_untouched(got[s]).all()), f"slot {s} was not named"
    for t in (style, prev_in, fdec):
        t.check()


# ---------------------------------------------------------------------------------------------------------------- absmax
INF_BITS = 0x7F800000


def _f32_bits(v):
    return int(np.float32(v).view(np.uint32))


def _absmax(L, buf_dev, rows, cols, ld, is_p8=0, e=4, period=0, frm=0, before=0):
    slot = Guarded((1,), torch.int32)
    slot.t.fill_(before)
    assert L.artalk_op_absmax(_p(buf_dev), rows, cols, ld, is_p8, e, period, frm, _p(slot.t), None) == 0
    return int(slot.cpu().item()) & 0xFFFFFFFF


def test_absmax_fp32_row_pitch():
    """A maximum involves no rounding: the slot must hold the bit pattern of max |x| over the 64 columns; the pitch gap is not read."""
    capi, L = _lib()
    x = torch.randn(37, 72, generator=_gen(90))
    x[:, 64:] = 1e6
    x[36, 63] = -7.25          # the maximum is negative and sits in the last valid element
    assert _absmax(L, _dev(x), 37, 64, 72) == _f32_bits(7.25)
    assert _absmax(L, _dev(x), 37, 64, 72, before=_f32_bits(9.5)) == _f32_bits(9.5), "a larger slot value must be kept (atomicMax across calls)"
    assert _absmax(L, _dev(x), 37, 64, 72, before=_f32_bits(1.5)) == _f32_bits(7.25)
    assert _absmax(L, _dev(x), 0, 64, 72, before=_f32_bits(1.5)) == _f32_bits(1.5), "rows = 0 is a no-op"


def test_absmax_grid_stride_loop():
    """2 500 x 1024 = 320 000 groups of 8 against the 262 144 one pass of the clamped grid (1024 blocks of 256 lanes) covers."""
    capi, L = _lib()
    x = torch.randn(2500, 1024, generator=_gen(91))
    x[2499, 1023] = 1000.5
    assert _absmax(L, _dev(x), 2500, 1024, 1024) == _f32_bits(1000.5)
    x[2499, 1023] = 0.0
    assert _absmax(L, _dev(x), 2500, 1024, 1024) == _f32_bits(float(x.abs().max()))


@pytest.mark.parametrize("e", [4, 0, -8])
def test_absmax_p8(e):
    """A P8 buffer: |hi| * 2^-e of the largest element, hi = f16(2^e x) - exact in fp32.  The lo halves are no values."""
    capi, L = _lib()
    rows, cols = 40, 256
    x = (100.0 * torch.randn(rows, cols, generator=_gen(92))).float()
    packed = torch.empty(rows, cols, dtype=torch.int32, device="cuda")
    assert L.artalk_op_pack_split_ex(_p(_dev(x)), _p(packed), x.numel(), 0, e, None, None) == 0
    hi = (x.numpy() * np.float32(2.0 ** e)).astype(np.float16).astype(np.float32)
    want = np.float32(np.abs(hi).max()) * np.float32(2.0 ** -e)
    assert _absmax(L, packed, rows, cols, cols, 1, e) == _f32_bits(want)
    # host-packed words whose lo halves hold large fp16 patterns: still the hi halves alone
    words = p8.pack(x.numpy(), e)
    h16 = words.view(np.float16).reshape(rows, cols // 8, 2, 8)
    h16[:, :, 1, :] = np.float16(60000.0)
    assert _absmax(L, _dev(torch.from_numpy(words)), rows, cols, cols, 1, e) == _f32_bits(want)
    # a NaN or an inf in a valid hi half reports inf
    for bad in (np.nan, np.inf):
        y = x.numpy().copy()
        y[rows - 1, cols - 1] = bad
        assert _absmax(L, _dev(torch.from_numpy(p8.pack(y, e))), rows, cols, cols, 1, e) == INF_BITS


@pytest.mark.parametrize("is_p8", [0, 1])
def test_absmax_junk_rows_and_non_finite(is_p8):
    """Rows r with r % 8 >= 6 are layout padding: an inf there is skipped; in a valid row it reports inf, and so does a NaN."""
    capi, L = _lib()
    rows, cols, e = 37, 64, 0
    x = torch.randn(rows, cols, generator=_gen(93))
    junk = torch.arange(rows) % 8 >= 6
    want = float(x[~junk].abs().max()) if not is_p8 else float(np.abs(x[~junk].numpy().astype(np.float16).astype(np.float32)).max())

    def run(t):
        d = _dev(torch.from_numpy(p8.pack(t.numpy(), e))) if is_p8 else _dev(t)
        return _absmax(L, d, rows, cols, cols, is_p8, e, 8, 6)

    y = x.clone()
    y[junk] = float("inf")
    assert run(y) == _f32_bits(want)
    y[junk] = float("nan")
    assert run(y) == _f32_bits(want)
    for r, bad in ((5, float("inf")), (32, float("-inf")), (0, float("nan")), (rows - 1 - 2, float("nan"))):
        assert not bool(junk[r])
        z = y.clone()
        z[r, cols - 1 if r else 0] = bad
        assert run(z) == INF_BITS, (r, bad)


# ---------------------------------------------------------------------------------------------------------------- through the model
@pytest.fixture(scope="module")
def status_model():
    from conftest import get_state_dict
    from artalk_amd.model import BitwiseARModel
    cfg, sd = get_state_dict("tiny")
    m = BitwiseARModel(cfg).eval().to("cuda")
    m.check_finite = False          # the host's recalibration / f32 fall-back would answer a raised bit: here the bits themselves are read
    return m, sd


POISON = [(None, 0, 0), ("logits_head.bias", 5, 1), ("basic_vae.encoder.code_mapping.bias", 31, 2), ("basic_vae.motion_std", 7, 4)]


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("key,index,bit", POISON, ids=["control", "logit_bias", "code_mapping_bias", "motion_std"])
def test_status_bits_through_the_model(status_model, precision, key, index, bit):
    """One NaN in a weight that feeds a decision is laundered into valid-looking bits or codes; the status word must say so.  Weight loading
    accepts a NaN, so the NaN route is taken.  Bit 0: the logit head's bias (a NaN logit in every token); bit 1: the bias of the VAE encoder's
    code mapping (the re-encoder output); bit 2: the motion statistics (the decoded codes).  A clip of two chunks: chunk 0 is decoded
    and re-encoded.  The control reloads the clean weights into the same model and must report 0."""
    from artalk_amd.synth import synth_audio
    m, sd = status_model
    w = dict(sd)
    if key is not None:
        t = sd[key].clone()
        t.view(-1)[index] = float("nan")
        w[key] = t
    m.set_precision(precision)
    m.load_state_dict(w, strict=True)
    out = m.inference_batch([torch.from_numpy(synth_audio(7, 6.0))])[0]
    st = m.status()
    assert out.shape == (150, MD)
    if key is None:
        assert st == 0 and bool(torch.isfinite(out).all())
    else:
        assert st & bit, f"{key}: status {st:#x} lacks bit value {bit}"
