"""StyleUNet upsampler on the GPU (artalk_amd.styleunet, artalk_styleunet_*) against the float64 restatement of its definition
(tests/styleunet_ref.py) on the golden inputs.  Allowance, as for the mesh renderer and the splat rasteriser: max-abs error <= 4 x e32,
e32 being the max-abs difference between the restatement in float32 and in float64 on the CPU for the same case, with a floor of one
float32 ulp of the case's largest output magnitude.  Run with -s for the error / e32 ratio per case; the measured ratios are in README.md."""
import os

import numpy as np
import pytest
import torch

from artalk_amd import styleunet as su
from styleunet_ref import draw_noise, styleunet_forward

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ((8, 3), (16, 2), (64, 1))
FACTOR = 4.0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "styleunet_ref.npz"))


@pytest.fixture(scope="module")
def nets(gold):
    """Per size: the loaded device module, the state dict and the golden input (made once, shared, read only)."""
    out = {}
    for S, B in CASES:
        sd = su.synth_state_dict(S, seed=int(gold["seed"]))
        net = su.StyleUNet(S, S, 32, 3, activation=True).eval().to("cuda:0")
        net.load_state_dict(sd, strict=True)
        out[S] = dict(net=net, sd=sd, x=torch.from_numpy(gold[f"x_{S}"]))
    return out


@pytest.fixture(scope="module")
def refs(nets):
    """Per size: the pre-sigmoid restatement in float64 and float32 on the stored noise."""
    out = {}
    with torch.no_grad():
        for S, r in nets.items():
            out[S] = (styleunet_forward(r["sd"], r["x"].double(), return_pre=True), styleunet_forward(r["sd"], r["x"].float(), return_pre=True))
    return out


def _compare(tag, got, want64, want32):
    e32 = float((want32.double() - want64).abs().max())
    err = float((got.double().cpu() - want64).abs().max())
    ulp = float(np.spacing(np.float32(want64.abs().max())))
    allowed = max(FACTOR * e32, ulp)
    print(f"{tag}: max-abs error {err:.3e}, e32 {e32:.3e}, error / e32 {err / e32:.2f} (allowed {FACTOR:.0f}), ulp floor {ulp:.2e}")
    assert bool(torch.isfinite(got).all())
    assert err <= allowed, f"{tag}: error {err:.3e} > allowed {allowed:.3e}"


@pytest.mark.parametrize("activation", [True, False])
@pytest.mark.parametrize("S", [c[0] for c in CASES])
def test_golden_cases(gold, nets, refs, S, activation):
    r = nets[S]
    r["net"].activation = activation
    try:
        got = r["net"](r["x"].cuda(), randomize_noise=False)
    finally:
        r["net"].activation = True
    p64, p32 = refs[S]
    if activation:
        p64, p32 = torch.sigmoid(p64), torch.sigmoid(p32)
    # the restatement is the oracle; that it equals the reference's own float64 run is tests/test_styleunet_cpu.py
    assert float((p64 - torch.from_numpy(gold[("act_" if activation else "pre_") + str(S)])).abs().max()) < 1e-9
    assert got.shape == p64.shape and got.dtype == torch.float32
    _compare(f"out_size {S} activation {activation}", got, p64, p32)


def test_randomized_noise_follows_the_torch_seed(nets):
    S, B = 16, 2
    r = nets[S]
    x = r["x"].cuda()
    torch.manual_seed(1234)
    got = r["net"](x, randomize_noise=True)
    torch.manual_seed(1234)
    noise = [n.cpu() for n in draw_noise(B, r["net"].num_layers, x.device)]
    assert float(noise[0].std()) > 0.3 and not torch.equal(noise[0][0], noise[0][1])
    with torch.no_grad():
        w64 = styleunet_forward(r["sd"], r["x"].double(), noise=noise)
        w32 = styleunet_forward(r["sd"], r["x"].float(), noise=noise)
    _compare("out_size 16 drawn noise", got, w64, w32)
    stored = r["net"](x, randomize_noise=False)
    assert float((stored - got).abs().max()) > 1e-3      # the drawn noise was used
    torch.manual_seed(1234)
    assert torch.equal(r["net"](x, randomize_noise=True), got)


def test_bit_identity_across_runs(nets):
    for S in (8, 64):
        r = nets[S]
        x = r["x"].cuda()
        a = r["net"](x, randomize_noise=False)
        b = r["net"](x, randomize_noise=False)
        assert torch.equal(a, b), S


def test_bit_identity_across_slabs_and_calls(nets):
    S, B = 8, 3
    r = nets[S]
    net, x = r["net"], r["x"].cuda()
    torch.manual_seed(7)
    noise = draw_noise(B, net.num_layers, x.device)      # per-sample noise: a slab must read its own frames' images
    try:
        whole = net(x, noise=noise)
        for slab in (1, 2, B):
            assert net.set_slab(slab) == slab
            assert torch.equal(net(x, noise=noise), whole), f"slab {slab}"
            assert torch.equal(net(x, randomize_noise=False)[1:], net(x[1:], randomize_noise=False)), f"slab {slab}"
    finally:
        net.set_slab(0)
    two = torch.cat([net(x[:2], noise=[n[:2] for n in noise]), net(x[2:], noise=[n[2:] for n in noise])])
    assert torch.equal(two, whole)
    assert not torch.equal(whole[0], whole[1])


def test_forward_refusals_on_the_device(nets):
    net = nets[8]["net"]
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 32, 16, 16, device="cuda"))
    with pytest.raises(ValueError):
        net(torch.zeros(1, 31, 8, 8, device="cuda"))
    with pytest.raises(ValueError):
        net(torch.zeros(1, 32, 8, 8, device="cuda"), noise=[torch.zeros(1, 1, 4, 4, device="cuda")])
    assert net(torch.zeros(0, 32, 8, 8, device="cuda")).shape == (0, 3, 8, 8)
