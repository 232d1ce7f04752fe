"""The whole StyleUNet upsampler in the bf16x3 and bf16 modes against the float64 statement of the mode's network definition
(tests/styleunet_prec_ref.py on top of tests/styleunet_ref.py) on the golden inputs, under the project's rule applied per mode:
max-abs error <= 4 x e32_m, e32_m being the distance between the mode's definition in float32 and in float64 on the CPU, with a floor
of one float32 ulp.  At network level e32_m is dominated by operand-rounding flips - the float32 and the float64 network feed slightly
different activations into the bf16 rounding of the next conv (measured on the CPU: 2.2e-6 .. 8.8e-5 for bf16x3, 1.4e-3 .. 7.6e-2 for
bf16) - so this bar is wide: the tests that tell a wrong kernel from a right one are the kernel-level ones
(tests/test_styleunet_prec_ops_gpu.py, with tests/test_styleunet_prec_cpu.py for what their bar separates).  Here the modes are checked
end to end, with the properties of the module: bit identity across runs, slabs and calls, and that switching touches nothing else.
Run with -s for the error / e32_m ratio per case."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from artalk_amd import capi
from artalk_amd import styleunet as su
from styleunet_prec_ref import allowance, styleunet_forward_mode
from styleunet_ref import draw_noise

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ((8, 3), (16, 2), (64, 1))
MODES = ("bf16x3", "bf16")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "styleunet_ref.npz"))


@pytest.fixture(scope="module")
def nets(gold):
    """Per size: the loaded device module (f32 until a test switches it, and f32 again when the test ends), the state dict, the golden
    input and the f32 mode's output taken before the first switch."""
    out = {}
    for S, B in CASES:
        sd = su.synth_state_dict(S, seed=int(gold["seed"]))
        net = su.StyleUNet(S, S, 32, 3, activation=True).eval().to("cuda:0")
        net.load_state_dict(sd, strict=True)
        x = torch.from_numpy(gold[f"x_{S}"])
        out[S] = dict(net=net, sd=sd, x=x, f32=net(x.cuda(), randomize_noise=False).cpu())
    return out


@pytest.fixture(scope="module")
def refs(nets):
    """Per (size, mode): the pre-sigmoid definition in float64 and float32 on the stored noise (computed once, shared, read only)."""
    out = {}
    with torch.no_grad():
        for S, r in nets.items():
            for mode in MODES:
                out[S, mode] = (styleunet_forward_mode(mode, r["sd"], r["x"].double(), return_pre=True),
                                styleunet_forward_mode(mode, r["sd"], r["x"].float(), return_pre=True))
    return out


def _in_mode(net, mode):
    class _Ctx:
        def __enter__(self):
            net.set_precision(mode)

        def __exit__(self, *exc):
            net.set_precision("f32")
    return _Ctx()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("activation", [True, False])
@pytest.mark.parametrize("S", [c[0] for c in CASES])
def test_golden_cases(nets, refs, S, activation, mode):
    r = nets[S]
    r["net"].activation = activation
    try:
        with _in_mode(r["net"], mode):
            got = r["net"](r["x"].cuda(), randomize_noise=False)
    finally:
        r["net"].activation = True
    p64, p32 = refs[S, mode]
    if activation:
        p64, p32 = torch.sigmoid(p64), torch.sigmoid(p32)
    allowed, e32 = allowance(p64, p32)
    err = float((got.double().cpu() - p64).abs().max())
    print(f"{mode} out_size {S} activation {activation}: max-abs error {err:.3e}, e32_m {e32:.3e}, error / e32_m {err / e32:.2f}")
    assert got.shape == p64.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert err <= allowed, f"error {err:.3e} > allowed {allowed:.3e}"


@pytest.mark.parametrize("mode", MODES)
def test_bit_identity_across_runs_slabs_and_calls(nets, mode):
    S, B = 8, 3
    r = nets[S]
    net, x = r["net"], r["x"].cuda()
    torch.manual_seed(7)
    noise = draw_noise(B, net.num_layers, x.device)      # per-sample noise: a slab must read its own frames' images
    with _in_mode(net, mode):
        try:
            whole = net(x, noise=noise)
            assert torch.equal(net(x, noise=noise), whole)
            for slab in (1, 2, B):
                assert net.set_slab(slab) == slab
                assert torch.equal(net(x, noise=noise), whole), f"slab {slab}"
        finally:
            net.set_slab(0)
        two = torch.cat([net(x[:2], noise=[n[:2] for n in noise]), net(x[2:], noise=[n[2:] for n in noise])])
        assert torch.equal(two, whole)
        assert not torch.equal(whole[0], whole[1])
    big = nets[64]
    with _in_mode(big["net"], mode):
        xb = big["x"].cuda()
        assert torch.equal(big["net"](xb, randomize_noise=False), big["net"](xb, randomize_noise=False))


@pytest.mark.parametrize("S", [c[0] for c in CASES])
def test_switching_changes_the_conv_arithmetic_and_nothing_else(nets, S):
    r = nets[S]
    net, x = r["net"], r["x"].cuda()
    L = capi.lib()

    def dims():
        v = [C.c_int(-1) for _ in range(5)]
        dev = L.artalk_styleunet_dims(net._h, *[C.byref(i) for i in v])
        return (dev,) + tuple(i.value for i in v)

    handle, before = net._h.value, dims()
    outs = {}
    for mode in MODES:
        with _in_mode(net, mode):
            assert net.precision == mode and L.artalk_styleunet_get_precision(net._h) == su.PRECISIONS[mode]
            assert net._h.value == handle and dims() == before
            outs[mode] = net(x, randomize_noise=False).cpu()
        assert not torch.equal(outs[mode], r["f32"]), f"{mode} gave the f32 mode's bits"
        # back in f32: the bits taken before the first switch
        assert net.precision == "f32" and torch.equal(net(x, randomize_noise=False).cpu(), r["f32"])
    assert not torch.equal(outs["bf16x3"], outs["bf16"])
    d3, d1 = float((outs["bf16x3"] - r["f32"]).abs().max()), float((outs["bf16"] - r["f32"]).abs().max())
    print(f"out_size {S}: max-abs distance from the f32 mode, bf16x3 {d3:.3e}, bf16 {d1:.3e}")
    assert d3 < d1


def test_precision_survives_load_state_dict(nets):
    r = nets[8]
    net = su.StyleUNet(8, 8, 32, 3).eval()
    net.set_precision("bf16x3")      # before the device: remembered, packed by finalize
    net.to("cuda:0").load_state_dict(r["sd"])
    x = r["x"].cuda()
    with _in_mode(r["net"], "bf16x3"):
        want = r["net"](x, randomize_noise=False)
    assert net.precision == "bf16x3" and torch.equal(net(x, randomize_noise=False), want)
    net.load_state_dict(r["sd"])      # new weights, a new handle: the mode stays
    assert net.precision == "bf16x3" and torch.equal(net(x, randomize_noise=False), want)


def test_timing_covers_the_launches_of_every_mode(nets):
    """artalk_styleunet_set_timing times the bf16 launches as it times the f32 ones: the same launches, one event pair each."""
    r = nets[8]
    net, x = r["net"], r["x"].cuda()
    L = capi.lib()
    seen = {}
    try:
        assert L.artalk_styleunet_set_timing(net._h, 1) == capi.OK
        for mode in ("f32",) + MODES:
            net.set_precision(mode)
            net(x, randomize_noise=False)
            conv, total = C.c_double(0), C.c_double(0)
            assert L.artalk_styleunet_get_timing(net._h, C.byref(conv), C.byref(total)) == capi.OK
            n = L.artalk_styleunet_get_launch_timing(net._h, None, None, 0)
            ms, geom = (C.c_double * n)(), (C.c_int32 * (5 * n))()
            assert L.artalk_styleunet_get_launch_timing(net._h, ms, geom, n) == n
            assert n > 0 and all(v > 0 for v in ms) and 0 < conv.value <= total.value
            assert abs(sum(ms) - conv.value) <= 1e-6 * conv.value
            seen[mode] = list(geom)
            assert all(geom[5 * i] == 3 and geom[5 * i + 1] in (4, 8) and geom[5 * i + 4] in (1, 3) for i in range(n))
    finally:
        L.artalk_styleunet_set_timing(net._h, 0)
        net.set_precision("f32")
    assert seen["bf16x3"] == seen["f32"] and seen["bf16"] == seen["f32"]
    want = [k for k, s in su.state_dict_manifest(8) if len(s) >= 4 and k.endswith(".weight") and not k.startswith("toRGB") and "constant_input" not in k and "noises" not in k]
    assert len(seen["f32"]) == 5 * len(want)
