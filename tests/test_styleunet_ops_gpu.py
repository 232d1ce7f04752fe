"""The StyleUNet conv kernel and resampler alone (artalk_op_conv2d, artalk_op_resample2) against the float64 restatement of one conv
(tests/styleunet_ref.py).  Allowance, as for the mesh renderer and the splat rasteriser: max-abs error <= 4 x e32, where e32 is the
max-abs difference between the restatement in float32 and in float64 on the CPU for the same case, with a floor of one float32 ulp of
the case's largest output magnitude.  Run with -s for the error / e32 ratio of every case."""
import math

import numpy as np
import pytest
import torch

from artalk_amd import capi
from styleunet_ref import conv2d, resample

pytestmark = pytest.mark.gpu

FACTOR = 4.0
GUARD = 256
POISON = -7.25e9
# (Cin, Cout, k, B, H, W)
CASES = [(16, 16, 3, 1, 40, 24), (32, 16, 1, 2, 33, 17), (64, 32, 3, 2, 16, 16), (512, 512, 3, 3, 4, 4), (32, 3, 1, 2, 32, 32),
         (16, 32, 3, 1, 1, 1), (17, 5, 3, 1, 7, 9)]
SWITCHES = ("in_scale", "out_scale", "gain", "noise", "noise_shared", "bias", "lrelu", "sft", "residual")


def _cl(t):
    """(B, C, H, W) float64 -> channels-last float32 on the device"""
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def _inputs(case, on, seed=0, ring=False):
    Cin, Cout, k, B, H, W = case
    g = torch.Generator().manual_seed(1000 * seed + Cin + 7 * Cout + 13 * H)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()      # float32-exact values: both sides read the same numbers
    x = rnd(B, Cin, H, W)
    if ring:
        inner = torch.zeros(H, W, dtype=torch.bool)
        inner[1:-1, 1:-1] = True
        x[:, :, inner] = 0.0
    a = dict(x=x, w=rnd(Cout, Cin, k, k) / math.sqrt(Cin * k * k))
    if "in_scale" in on:
        a["in_scale"] = 1.0 + 0.3 * rnd(B, Cin)
    if "out_scale" in on:
        a["out_scale"] = 1.0 + 0.3 * rnd(B, Cout)
    if "gain" in on:
        a["gain"] = float(np.float32(math.sqrt(2.0)))
    if "noise" in on or "noise_shared" in on:
        a["noise"] = rnd(1 if "noise_shared" in on else B, 1, H, W)
        a["noise_weight"] = rnd(1) * 0.5
    if "bias" in on:
        a["bias"] = rnd(Cout) * 0.3
    if "lrelu" in on:
        a["slope"] = 0.2
    if "sft" in on:
        a["sft_scale"], a["sft_shift"] = 1.0 + 0.3 * rnd(B, Cout, H, W), rnd(B, Cout, H, W)
    if "residual" in on:
        a["residual"] = rnd(B, Cout, H, W)
    return a


def _gpu(case, a):
    Cin, Cout, k, B, H, W = case
    L = capi.lib()
    n = B * H * W * Cout
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float32, device="cuda")
    out = buf[GUARD:GUARD + n]
    out.fill_(float("nan"))
    dev = lambda t: None if t is None else t.float().contiguous().cuda()
    x, w = _cl(a["x"]), a["w"].permute(2, 3, 1, 0).contiguous().float().cuda()
    keep = dict(ins=dev(a.get("in_scale")), outs=dev(a.get("out_scale")), noise=dev(a.get("noise")), nw=dev(a.get("noise_weight")),
                bias=dev(a.get("bias")), sc=None if "sft_scale" not in a else _cl(a["sft_scale"]),
                sh=None if "sft_shift" not in a else _cl(a["sft_shift"]), res=None if "residual" not in a else _cl(a["residual"]))
    nstride = 0 if keep["noise"] is None or keep["noise"].shape[0] == 1 else H * W
    rc = L.artalk_op_conv2d(capi.ptr(x), H * W * Cin, capi.ptr(w), capi.ptr(out), B, H, W, Cin, Cout, k, capi.ptr(keep["ins"]),
                            capi.ptr(keep["outs"]), a.get("gain", 1.0), capi.ptr(keep["noise"]), nstride, capi.ptr(keep["nw"]),
                            capi.ptr(keep["bias"]), 1 if "slope" in a else 0, capi.ptr(keep["sc"]), capi.ptr(keep["sh"]),
                            capi.ptr(keep["res"]), capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()
    whole = buf.cpu()
    assert bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all()), "the kernel wrote outside its output"
    got = whole[GUARD:GUARD + n].reshape(B, H, W, Cout).permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all()), "an output value was not written"
    return got.double()


def _check(tag, case, a):
    with torch.no_grad():
        want = conv2d(**a)
        a32 = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}
        e32 = float((conv2d(**a32).double() - want).abs().max())
    got = _gpu(case, a)
    err = float((got - want).abs().max())
    ulp = float(np.spacing(np.float32(want.abs().max())))
    allowed = max(FACTOR * e32, ulp)
    print(f"{tag} {case}: max-abs error {err:.3e}, e32 {e32:.3e}, error / e32 {err / max(e32, 1e-300):.2f}, ulp floor {ulp:.2e}")
    assert err <= allowed, f"{tag} {case}: error {err:.3e} > allowed {allowed:.3e} (e32 {e32:.3e})"
    return got, want


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_plain_conv(case):
    _check("plain", case, _inputs(case, ()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_every_switch_together(case):
    on = set(SWITCHES) - {"noise_shared"}
    _check("all", case, _inputs(case, on, seed=1))
    _check("all, shared noise", case, _inputs(case, set(SWITCHES) - {"noise"}, seed=2))


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("case", [CASES[2], CASES[6]], ids=lambda c: "x".join(map(str, c)))
def test_each_switch_alone(case, switch):
    a = _inputs(case, {switch}, seed=3)
    got, _ = _check(switch, case, a)
    plain = conv2d(a["x"], a["w"])
    assert float((got - plain).abs().max()) > 1e-3, f"{switch} changed nothing"


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[6]], ids=lambda c: "x".join(map(str, c)))
def test_borders(case):
    """An input that is non-zero only on the outermost ring: every output value near an edge depends on the zero padding."""
    a = _inputs(case, (), seed=4, ring=True)
    got, want = _check("ring", case, a)
    H, W = case[4], case[5]
    if H > 4 and W > 4:
        assert float(want[:, :, 2:-2, 2:-2].abs().max()) == 0.0 and float(got[:, :, 2:-2, 2:-2].abs().max()) == 0.0


def test_shared_input_image():
    """x_bstride = 0: one image for every sample (the decoder's constant input), told apart by the input scale."""
    case = (32, 16, 3, 3, 4, 4)
    a = _inputs(case, {"in_scale"}, seed=5)
    a["x"] = a["x"][:1].expand(3, -1, -1, -1).contiguous()
    want = conv2d(**a)
    L = capi.lib()
    x, w, s = _cl(a["x"][:1]), a["w"].permute(2, 3, 1, 0).contiguous().float().cuda(), a["in_scale"].float().cuda()
    out = torch.full((3, 4, 4, 16), float("nan"), device="cuda")
    rc = L.artalk_op_conv2d(capi.ptr(x), 0, capi.ptr(w), capi.ptr(out), 3, 4, 4, 32, 16, 3, capi.ptr(s), None, 1.0, None, 0, None, None, 0,
                            None, None, None, capi.current_stream_ptr())
    assert rc == capi.OK
    got = out.cpu().permute(0, 3, 1, 2).double()
    e32 = float((conv2d(a["x"].float(), a["w"].float(), in_scale=a["in_scale"].float()).double() - want).abs().max())
    assert float((got - want).abs().max()) <= max(FACTOR * e32, float(np.spacing(np.float32(want.abs().max()))))


@pytest.mark.parametrize("B,C,H,W,up", [(2, 4, 4, 4, 1), (2, 4, 8, 8, 0), (1, 5, 4, 6, 1), (1, 5, 6, 4, 0), (3, 3, 1, 1, 1)])
def test_resample(B, C, H, W, up):
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.randn(B, C, H, W, generator=g).double()
    want = resample(x, bool(up))
    e32 = float((resample(x.float(), bool(up)).double() - want).abs().max())
    n = want.numel()
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float32, device="cuda")
    xd = _cl(x)
    rc = capi.lib().artalk_op_resample2(capi.ptr(xd), capi.ptr(buf[GUARD:]), B, H, W, C, up, capi.current_stream_ptr())
    assert rc == capi.OK
    whole = buf.cpu()
    assert bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all())
    got = whole[GUARD:GUARD + n].reshape(B, want.shape[2], want.shape[3], C).permute(0, 3, 1, 2).double()
    err = float((got - want).abs().max())
    ulp = float(np.spacing(np.float32(want.abs().max())))
    print(f"resample {'x2' if up else 'x0.5'} {(B, C, H, W)}: max-abs error {err:.3e}, e32 {e32:.3e}")
    assert err <= max(FACTOR * e32, ulp)
