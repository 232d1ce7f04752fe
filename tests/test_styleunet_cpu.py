"""StyleUNet upsampler without a GPU: the float64 restatement (tests/styleunet_ref.py) against the fixtures made from the reference's
own module (tools/make_golden_styleunet.py), deliberately wrong variants, the state-dict manifest, and every refusal of the Python
wrapper and of the C ABI that fires before the device is touched."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from artalk_amd import capi
from artalk_amd import styleunet as su
from styleunet_ref import Variant, styleunet_forward

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ((8, 3), (16, 2), (64, 1))
GPU_FACTOR = 4.0      # the allowance of tests/test_styleunet_gpu.py: 4 x e32

WRONG = {
    "align_corners": Variant(align_corners=True),
    "no_gain": Variant(gain=False),
    "no_demod": Variant(demod=False),
    "sft_swapped": Variant(sft_swapped=True),
    "no_noise": Variant(noise=False),
    "slope_0.01": Variant(slope=0.01),
    "rgb_skip_not_upsampled": Variant(rgb_skip_upsampled=False),
}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "styleunet_ref.npz"))


@pytest.fixture(scope="module")
def runs(gold):
    """Per size: the state dict, the input, the restatement's float64 outputs and e32 (computed once, shared, read only)."""
    out = {}
    with torch.no_grad():
        for S, B in CASES:
            sd = su.synth_state_dict(S, seed=int(gold["seed"]))
            x = torch.from_numpy(gold[f"x_{S}"]).double()
            assert x.shape == (B, 32, S, S)
            pre = styleunet_forward(sd, x, activation=False)
            act = styleunet_forward(sd, x, activation=True)
            e32 = float((styleunet_forward(sd, x.float(), activation=True).double() - act).abs().max())
            out[S] = dict(sd=sd, x=x, pre=pre, act=act, e32=e32)
    return out


@pytest.mark.parametrize("S", [c[0] for c in CASES])
def test_restatement_equals_golden(gold, runs, S):
    for name in ("pre", "act"):
        want = torch.from_numpy(gold[f"{name}_{S}"])
        rel = float((runs[S][name] - want).abs().max() / want.abs().max())
        print(f"out_size {S} {name}: restatement vs reference float64, relative error {rel:.2e}")
        assert rel <= 1e-10


@pytest.mark.parametrize("S", [c[0] for c in CASES])
def test_fixtures_are_not_saturated(gold, S):
    std = float(gold[f"pre_{S}"].std())
    assert 0.05 <= std <= 20.0, std
    x = gold[f"x_{S}"]
    assert 0.0 <= x.min() and x.max() < 1.0


@pytest.mark.parametrize("which", sorted(WRONG))
@pytest.mark.parametrize("S", [c[0] for c in CASES])
def test_wrong_variants_miss_golden(gold, runs, S, which):
    r = runs[S]
    with torch.no_grad():
        got = styleunet_forward(r["sd"], r["x"], activation=True, v=WRONG[which])
    err = float((got - torch.from_numpy(gold[f"act_{S}"])).abs().max())
    allowance = GPU_FACTOR * r["e32"]
    print(f"out_size {S} {which}: error {err:.3e} = {err / allowance:.0f} x the GPU allowance {allowance:.2e}")
    assert err > 100.0 * allowance


def test_manifest_equals_reference():
    want = json.load(open(os.path.join(GOLD, "styleunet_manifest.json")))
    assert sorted(want) == ["16", "512", "64", "8"]
    for S in (8, 16, 64, 512):
        mine = [[k, list(s)] for k, s in su.state_dict_manifest(S)]
        assert mine == want[str(S)], S
    assert len(want["512"]) == 285
    net = su.StyleUNet(16, 16, 32, 3)
    assert net.state_dict_manifest() == su.state_dict_manifest(16)


def test_synth_state_dict_is_keyed_by_name():
    a, b = su.synth_state_dict(8), su.synth_state_dict(16)
    for k in ("final_linear.weight", "stylegan_decoder.style_conv1.modulated_conv.weight", "stylegan_decoder.noises.noise0"):
        assert torch.equal(a[k], b[k])
    assert not torch.equal(a["final_linear.bias"], su.synth_state_dict(8, seed=1)["final_linear.bias"])
    assert float(a["stylegan_decoder.style_conv1.weight"].abs()) > 0      # the noise path is live
    assert abs(float(a["stylegan_decoder.style_conv1.modulated_conv.modulation.bias"].mean()) - 1.0) < 0.05


def test_constructor_refusals():
    with pytest.raises(NotImplementedError):
        su.StyleUNet(256, 512, 32, 3)
    with pytest.raises(NotImplementedError):
        su.StyleUNet(512, 512, 32, 3, num_style_feat=256)
    with pytest.raises(NotImplementedError):
        su.StyleUNet(512, 512, 32, 3, num_mlp=4)
    for bad in (4, 2048, 48):
        with pytest.raises(ValueError):
            su.StyleUNet(bad, bad, 32, 3)
    net = su.StyleUNet(512, 512, 32, 3)
    assert net.eval() is net and net.num_layers == 15
    with pytest.raises(RuntimeError):
        net.to("cpu")


def test_load_state_dict_refusals():
    sd = su.synth_state_dict(8)
    net = su.StyleUNet(8, 8, 32, 3)
    extra = dict(sd, bogus=torch.zeros(1))
    with pytest.raises(RuntimeError, match="Unexpected key in state_dict: bogus"):
        net.load_state_dict(extra)
    wrong = dict(sd)
    wrong["final_linear.bias"] = torch.zeros(3)
    with pytest.raises(RuntimeError, match="size mismatch for final_linear.bias"):
        net.load_state_dict(wrong)
    less = {k: v for k, v in sd.items() if k != "toRGB.0.weight"}
    with pytest.raises(RuntimeError, match=r"Missing key\(s\) in state_dict: toRGB.0.weight"):
        net.load_state_dict(less)
    assert net.load_state_dict(sd) is net


def test_forward_refusals():
    net = su.StyleUNet(8, 8, 32, 3)
    net.load_state_dict(su.synth_state_dict(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 32, 8, 8))
    with pytest.raises(ValueError):
        net(torch.zeros(32, 8, 8))
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 32, 4, 4))
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 32, 8, 16))


def _handle(S=8):
    L = capi.lib()
    h = C.c_void_p()
    assert L.artalk_styleunet_create(0, 32, 3, S, C.byref(h)) == capi.OK
    return L, h


def test_capi_refusals_before_the_device_is_touched():
    L = capi.lib()
    h = C.c_void_p()
    assert L.artalk_styleunet_create(0, 32, 3, 8, None) == capi.EINVAL
    for size in (4, 2048, 24, 0, -8):
        assert L.artalk_styleunet_create(0, 32, 3, size, C.byref(h)) == capi.EINVAL
        assert b"out_size" in L.artalk_styleunet_last_error(None)
    assert L.artalk_styleunet_create(0, 0, 3, 8, C.byref(h)) == capi.EINVAL
    assert L.artalk_styleunet_create(0, 32, 0, 8, C.byref(h)) == capi.EINVAL
    assert L.artalk_styleunet_create(-1, 32, 3, 8, C.byref(h)) == capi.EINVAL
    for f in (L.artalk_styleunet_finalize, ):
        assert f(None) == capi.EINVAL
    assert L.artalk_styleunet_forward(None, None, 1, None, None, 1, None, None) == capi.EINVAL
    assert L.artalk_styleunet_set_slab(None, 1) == capi.EINVAL
    assert L.artalk_styleunet_last_error(None) is not None
    L.artalk_styleunet_destroy(None)

    L, h = _handle(8)
    try:
        z = torch.zeros(512)
        one = (C.c_int64 * 1)(512)
        assert L.artalk_styleunet_set_tensor(h, b"bogus", capi.ptr(z), 1, one) == capi.EKEY
        assert L.artalk_styleunet_last_error(h) == b"Unexpected key in state_dict: bogus"
        assert L.artalk_styleunet_set_tensor(h, b"conv_body_first.bias", capi.ptr(z), 1, one) == capi.EINVAL
        assert L.artalk_styleunet_last_error(h) == b"size mismatch for conv_body_first.bias"
        assert L.artalk_styleunet_set_tensor(h, b"final_linear.bias", capi.ptr(z), 1, one) == capi.OK
        assert L.artalk_styleunet_set_tensor(h, None, capi.ptr(z), 1, one) == capi.EINVAL
        assert L.artalk_styleunet_finalize(h) == capi.EMISSING
        msg = L.artalk_styleunet_last_error(h).decode()
        assert msg.startswith("Missing key(s) in state_dict: conv_body_first.weight, conv_body_first.bias") and msg.endswith(", ...")
        assert "final_linear.bias" not in msg
        assert L.artalk_styleunet_forward(h, capi.ptr(z), 1, None, None, 1, capi.ptr(z), None) == capi.ESTATE
        assert L.artalk_styleunet_set_slab(h, -1) == capi.EINVAL
        assert L.artalk_styleunet_set_slab(h, 65) == capi.EINVAL
        assert L.artalk_styleunet_set_slab(h, 2) == 2
        assert L.artalk_styleunet_set_slab(h, 0) == 64
    finally:
        L.artalk_styleunet_destroy(h)
    # the default slab shrinks with the workspace a frame needs
    L, h = _handle(512)
    try:
        assert 1 <= L.artalk_styleunet_set_slab(h, 0) < 64
    finally:
        L.artalk_styleunet_destroy(h)


def test_op_conv2d_refusals_before_the_device_is_touched():
    L = capi.lib()
    p = C.c_void_p(4096)      # never dereferenced: every call below is refused

    def call(x=p, xb=0, w=p, out=p, B=1, H=4, W=4, Cin=16, Cout=16, k=3, noise=None, nb=0, nw=None, sc=None, sh=None):
        return L.artalk_op_conv2d(x, xb, w, out, B, H, W, Cin, Cout, k, None, None, 1.0, noise, nb, nw, None, 0, sc, sh, None, None)

    assert call(x=None) == capi.EINVAL and call(w=None) == capi.EINVAL and call(out=None) == capi.EINVAL
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(Cin=0), dict(Cout=0), dict(k=2), dict(k=5), dict(xb=4 * 4 * 16 - 1)):
        assert call(**kw) == capi.EINVAL, kw
    assert call(noise=p) == capi.EINVAL                   # noise without its weight
    assert call(noise=p, nw=p, nb=15) == capi.EINVAL      # samples would overlap
    assert call(sc=p) == capi.EINVAL and call(sh=p) == capi.EINVAL
    assert L.artalk_op_resample2(None, p, 1, 4, 4, 3, 1, None) == capi.EINVAL
    assert L.artalk_op_resample2(p, p, 1, 3, 4, 3, 0, None) == capi.EINVAL      # x0.5 needs even sizes


def test_new_symbols_are_exported():
    L = capi.lib()
    for name in ("artalk_styleunet_create", "artalk_styleunet_set_tensor", "artalk_styleunet_finalize", "artalk_styleunet_forward",
                 "artalk_styleunet_set_slab", "artalk_styleunet_destroy", "artalk_styleunet_last_error", "artalk_op_conv2d",
                 "artalk_op_resample2"):
        assert name in capi.SYMBOLS and hasattr(L, name), name
