"""The DINO-feature kernels alone (artalk_op_dino_*), one launch each, every output between poisoned guard bands that must stay
poisoned.  The data movements are exact; the two resizes, the normalisation and the LayerNorm stay within the project's allowance for a
float32 kernel: max-abs error <= 4 x e32, e32 being torch's float32 CPU evaluation against its float64 one, with a floor of one float32
ulp of the largest value.  Run with -s for error / e32."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dino_cases as cases
from artalk_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 256
POISON = -7.25e9
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _guarded(n):
    """A device buffer of n floats, NaN inside, between two poisoned bands."""
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf


def _payload(buf, n, what="the kernel"):
    torch.cuda.synchronize()
    whole = buf.cpu()
    assert bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all()), f"{what} wrote outside its output"
    got = whole[GUARD:GUARD + n]
    assert bool(torch.isfinite(got).all()), f"{what} left an output value unwritten"
    return got


def _rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _close(got, f, what):
    """f(dtype) -> the torch CPU statement in that dtype; got within max(4 e32, 1 ulp) of the float64 one."""
    want, got32 = f(torch.float64), f(torch.float32)
    e32 = float((got32.double() - want).abs().max())
    allow = cases.allowance(e32, float(want.abs().max()))
    err = float((got.double().reshape(want.shape) - want).abs().max())
    print(f"{what}: error {err:.2e}, e32 {e32:.2e}, error / e32 {err / e32 if e32 else float('nan'):.2f}, allowance {allow:.2e}")
    assert err <= allow


def _s():
    return capi.current_stream_ptr()


# ---- the two resizes
# shrinking by 3.5, 7, 14, a ratio that is no integer (70 -> 3), enlarging (64 -> 70), and a rectangle
@pytest.mark.parametrize("hi,wi,ho,wo", [(70, 70, 20, 20), (70, 70, 10, 10), (70, 70, 5, 5), (70, 70, 3, 3), (64, 64, 70, 70), (45, 83, 70, 70)])
@pytest.mark.parametrize("channels_last", [0, 1])
def test_resize_aa(hi, wi, ho, wo, channels_last):
    x = torch.rand(3, hi, wi, generator=torch.Generator().manual_seed(hi + wo))
    n = 3 * ho * wo
    buf, xd = _guarded(n), x.cuda()
    assert capi.lib().artalk_op_dino_resize_aa(capi.ptr(xd), capi.ptr(buf[GUARD:]), 3, hi, wi, ho, wo, channels_last, 0, _s()) == capi.OK
    got = _payload(buf, n)
    got = got.reshape(ho, wo, 3).permute(2, 0, 1) if channels_last else got.reshape(3, ho, wo)

    def want(dtype):
        return F.interpolate(x.to(dtype)[None], (ho, wo), mode="bilinear", align_corners=False, antialias=True)[0]
    _close(got, want, f"resize_aa {hi} x {wi} -> {ho} x {wo}")
    # the other reading, no antialias, is far outside when shrinking
    if hi > ho:
        plain = F.interpolate(x.double()[None], (ho, wo), mode="bilinear", align_corners=False)[0]
        assert float((got.double() - plain).abs().max()) > 1e-2


def test_resize_aa_normalized_and_normalize():
    x = torch.rand(3, 33, 47, generator=torch.Generator().manual_seed(1))
    buf, xd = _guarded(3 * 28 * 28), x.cuda()
    assert capi.lib().artalk_op_dino_resize_aa(capi.ptr(xd), capi.ptr(buf[GUARD:]), 3, 33, 47, 28, 28, 0, 1, _s()) == capi.OK

    def norm(t):
        return (t - torch.tensor(MEAN, dtype=t.dtype)[:, None, None]) / torch.tensor(STD, dtype=t.dtype)[:, None, None]
    _close(_payload(buf, 3 * 28 * 28), lambda dt: norm(F.interpolate(x.to(dt)[None], (28, 28), mode="bilinear", antialias=True)[0]), "resize_aa + normalise")
    n = 33 * 47
    buf = _guarded(3 * n)
    assert capi.lib().artalk_op_dino_normalize(capi.ptr(xd), capi.ptr(buf[GUARD:]), n, _s()) == capi.OK
    _close(_payload(buf, 3 * n), lambda dt: norm(x.to(dt)), "normalise")


@pytest.mark.parametrize("hi,ho", [(3, 5), (5, 10), (20, 40), (6, 3)])
def test_resize_ac(hi, ho):
    Cn = 12
    x = _rnd(hi * ho, hi, hi, Cn)
    n = ho * ho * Cn
    buf, xd = _guarded(n), x.cuda()
    assert capi.lib().artalk_op_dino_resize_ac(capi.ptr(xd), capi.ptr(buf[GUARD:]), hi, hi, ho, ho, Cn, _s()) == capi.OK
    got = _payload(buf, n).reshape(ho, ho, Cn)

    def want(dtype, ac=True):
        return F.interpolate(x.to(dtype).permute(2, 0, 1)[None], (ho, ho), mode="bilinear", align_corners=ac)[0].permute(1, 2, 0)
    _close(got, want, f"resize_ac {hi} -> {ho}")
    assert float((got.double() - want(torch.float64, False)).abs().max()) > 1e-2      # align_corners=False is another function


@pytest.mark.parametrize("M,D", [(26, 64), (37, 128), (5, 96), (9, 768)])      # 128 / 768: launch_layernorm's kernels; 64 / 96: the general one
def test_layernorm(M, D):
    x, w, b = _rnd(M, M, D) * 3 + 1, 1 + 0.1 * _rnd(D, D), 0.1 * _rnd(D + 1, D)
    buf = _guarded(M * D)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    assert capi.lib().artalk_op_dino_layernorm(capi.ptr(xd), capi.ptr(buf[GUARD:]), capi.ptr(wd), capi.ptr(bd), M, D, _s()) == capi.OK
    _close(_payload(buf, M * D), lambda dt: F.layer_norm(x.to(dt), (D,), w.to(dt), b.to(dt), 1e-6), f"layernorm {M} x {D}")


# ---- the data movements: exact
@pytest.mark.parametrize("g", [1, 5, 6])
def test_im2col(g):
    S = 14 * g
    img = _rnd(g, 3, S, S)
    n = g * g * 608
    buf, xd = _guarded(n), img.cuda()
    assert capi.lib().artalk_op_dino_im2col(capi.ptr(xd), capi.ptr(buf[GUARD:]), g, _s()) == capi.OK
    cols = F.unfold(img[None], 14, stride=14)[0].transpose(0, 1)      # [g g][3 * 196], channel-major like the conv weight
    want = torch.cat([cols, torch.zeros(g * g, 20)], dim=1)
    assert torch.equal(_payload(buf, n), want.reshape(-1))


@pytest.mark.parametrize("T,D", [(26, 128), (37, 64), (2, 4)])
def test_tokens(T, D):
    patch, cls, pos = _rnd(1, T - 1, D), _rnd(2, D), _rnd(3, T, D)
    buf = _guarded(T * D)
    a, b, c = patch.cuda(), cls.cuda(), pos.cuda()
    assert capi.lib().artalk_op_dino_tokens(capi.ptr(a), capi.ptr(b), capi.ptr(c), capi.ptr(buf[GUARD:]), T, D, _s()) == capi.OK
    assert torch.equal(_payload(buf, T * D), (torch.cat([cls[None], patch]) + pos).reshape(-1))


def test_strip():
    tap = _rnd(4, 26, 128)
    buf, a = _guarded(25 * 128), tap.cuda()
    assert capi.lib().artalk_op_dino_strip(capi.ptr(a), capi.ptr(buf[GUARD:]), 25, 128, _s()) == capi.OK
    assert torch.equal(_payload(buf, 25 * 128), tap[1:].reshape(-1))


@pytest.mark.parametrize("g,s,Co", [(5, 4, 8), (6, 2, 12), (3, 4, 256)])
def test_shuffle_finishes_a_transposed_conv(g, s, Co):
    """GEMM result [g g][s s Co] -> [s g][s g][Co] + bias equals conv_transpose2d, exactly, when the GEMM part is done in torch with
    one product per output (Ci = 1)."""
    x, w, bias = _rnd(1, 1, g, g), _rnd(2, 1, Co, s, s), _rnd(3, Co)
    r = (x.reshape(g * g, 1) * w.permute(0, 2, 3, 1).reshape(1, s * s * Co)).contiguous()      # column (dy s + dx) Co + co
    n = s * g * s * g * Co
    buf = _guarded(n)
    a, b = r.cuda(), bias.cuda()
    assert capi.lib().artalk_op_dino_shuffle(capi.ptr(a), capi.ptr(b), capi.ptr(buf[GUARD:]), g, s, Co, _s()) == capi.OK
    got = _payload(buf, n).reshape(s * g, s * g, Co)
    want = F.conv_transpose2d(x[None], w, None, stride=s)[0].permute(1, 2, 0) + bias
    assert torch.equal(got, want)
    swapped = F.conv_transpose2d(x[None], w.transpose(-1, -2), None, stride=s)[0].permute(1, 2, 0) + bias
    assert not torch.equal(got, swapped)


@pytest.mark.parametrize("g", [5, 6, 9, 2])
def test_gather_s2(g):
    Cn = 8
    Ho = (g - 1) // 2 + 1
    x = _rnd(g, g, g, Cn)
    n = Ho * Ho * 9 * Cn
    buf, a = _guarded(n), x.cuda()
    assert capi.lib().artalk_op_dino_gather_s2(capi.ptr(a), capi.ptr(buf[GUARD:]), g, Cn, _s()) == capi.OK
    cols = F.unfold(x.permute(2, 0, 1)[None], 3, padding=1, stride=2)[0]      # [Cn * 9][Ho Ho], row c 9 + tap
    want = cols.reshape(Cn, 9, Ho * Ho).permute(2, 1, 0).reshape(-1)          # [Ho Ho][tap][c]
    assert torch.equal(_payload(buf, n), want)


@pytest.mark.parametrize("n,Cn", [(25, 256), (9, 1024), (7, 5)])      # widths 259 / 1027 are odd: padded to 264 / 1032
def test_concat(n, Cn):
    img, feat = _rnd(1, n, 3), _rnd(2, n, Cn)
    W = (Cn + 3 + 7) // 8 * 8
    buf = _guarded(n * W)
    a, b = img.cuda(), feat.cuda()
    assert capi.lib().artalk_op_dino_concat(capi.ptr(a), capi.ptr(b), capi.ptr(buf[GUARD:]), n, Cn, _s()) == capi.OK
    assert torch.equal(_payload(buf, n * W), torch.cat([img, feat, torch.zeros(n, W - Cn - 3)], dim=1).reshape(-1))


@pytest.mark.parametrize("n", [4, 1028, 256 * 4 * 3])
def test_add_relu(n):
    a, b = _rnd(1, n), _rnd(2, n)
    s, r = _guarded(n), _guarded(n)
    ad, bd = a.cuda(), b.cuda()
    L = capi.lib()
    assert L.artalk_op_dino_add_relu(capi.ptr(ad), capi.ptr(bd), capi.ptr(s[GUARD:]), capi.ptr(r[GUARD:]), n, _s()) == capi.OK
    assert torch.equal(_payload(s, n), a + b) and torch.equal(_payload(r, n), torch.relu(a + b))
    r = _guarded(n)
    assert L.artalk_op_dino_add_relu(capi.ptr(ad), None, None, capi.ptr(r[GUARD:]), n, _s()) == capi.OK
    assert torch.equal(_payload(r, n), torch.relu(a))
    assert L.artalk_op_dino_add_relu(capi.ptr(ad), None, None, capi.ptr(r[GUARD:]), n + 1, _s()) == capi.EINVAL
    assert L.artalk_op_dino_add_relu(None, None, None, capi.ptr(r[GUARD:]), n, _s()) == capi.EINVAL


@pytest.mark.parametrize("n,Cn,D", [(1600, 16, 128), (33, 40, 64), (5, 3, 0)])      # 33 x 40: partial tiles both ways; D = 0: no token
def test_output(n, Cn, D):
    x, tok = _rnd(1, n, Cn), _rnd(2, max(D, 1))
    out, f1 = _guarded(n * Cn), _guarded(max(D, 1))
    a, b = x.cuda(), tok.cuda()
    rc = capi.lib().artalk_op_dino_output(capi.ptr(a), capi.ptr(out[GUARD:]), n, Cn, capi.ptr(b) if D else None, capi.ptr(f1[GUARD:]), D, _s())
    assert rc == capi.OK
    assert torch.equal(_payload(out, n * Cn), x.t().reshape(-1))
    if D:
        assert torch.equal(_payload(f1, D), tok)
