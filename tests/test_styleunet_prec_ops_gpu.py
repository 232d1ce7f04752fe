"""The StyleUNet conv kernel in the bf16x3 and bf16 modes alone (artalk_op_conv2d_ex, precision 1 and 2) against the float64 statement of
the mode's definition (tests/styleunet_prec_ref.py).  Allowance, the project's rule applied per mode: max-abs error <= 4 x e32_m, where
e32_m is the max-abs difference between the mode's definition in float32 and in float64 on the CPU for the same case (computed here,
from the definition and never from the kernel), with a floor of one float32 ulp of the case's largest output magnitude.  What this bar
tells apart - every dropped product, skipped rounding and the exact fp32 kernel miss it by more than 2 x - is
tests/test_styleunet_prec_cpu.py.  Run with -s for the error / e32_m ratio of every case; the measured ranges are in DESIGN.md."""
import pytest
import torch

from artalk_amd import capi
from styleunet_prec_ref import CASES, SWITCHES, allowance, case_id, conv2d_mode, inputs

pytestmark = pytest.mark.gpu

MODES = {"bf16x3": 1, "bf16": 2}
GUARD = 256
POISON = -7.25e9


def _cl(t):
    """(B, C, H, W) float64 -> channels-last float32 on the device"""
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def _gpu(case, a, precision, x_bstride=None, x=None, entry="ex"):
    Cin, Cout, k, B, H, W = case
    L = capi.lib()
    n = B * H * W * Cout
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.float32, device="cuda")
    out = buf[GUARD:GUARD + n]
    out.fill_(float("nan"))
    dev = lambda t: None if t is None else t.float().contiguous().cuda()
    x = _cl(a["x"]) if x is None else x
    w = a["w"].permute(2, 3, 1, 0).contiguous().float().cuda()
    keep = dict(ins=dev(a.get("in_scale")), outs=dev(a.get("out_scale")), noise=dev(a.get("noise")), nw=dev(a.get("noise_weight")),
                bias=dev(a.get("bias")), sc=None if "sft_scale" not in a else _cl(a["sft_scale"]),
                sh=None if "sft_shift" not in a else _cl(a["sft_shift"]), res=None if "residual" not in a else _cl(a["residual"]))
    nstride = 0 if keep["noise"] is None or keep["noise"].shape[0] == 1 else H * W
    args = [capi.ptr(x), H * W * Cin if x_bstride is None else x_bstride, capi.ptr(w), capi.ptr(out), B, H, W, Cin, Cout, k,
            capi.ptr(keep["ins"]), capi.ptr(keep["outs"]), a.get("gain", 1.0), capi.ptr(keep["noise"]), nstride, capi.ptr(keep["nw"]),
            capi.ptr(keep["bias"]), 1 if "slope" in a else 0, capi.ptr(keep["sc"]), capi.ptr(keep["sh"]), capi.ptr(keep["res"])]
    if entry == "ex":
        rc = L.artalk_op_conv2d_ex(*args, precision, capi.current_stream_ptr())
    else:
        rc = L.artalk_op_conv2d(*args, capi.current_stream_ptr())
    assert rc == capi.OK
    torch.cuda.synchronize()
    whole = buf.cpu()
    assert bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all()), "the kernel wrote outside its output"
    got = whole[GUARD:GUARD + n].reshape(B, H, W, Cout).permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all()), "an output value was not written"
    return got


def _check(tag, mode, case, a):
    with torch.no_grad():
        want = conv2d_mode(mode, **a)
        a32 = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}
        allowed, e32 = allowance(want, conv2d_mode(mode, **a32))
    got = _gpu(case, a, MODES[mode]).double()
    err = float((got - want).abs().max())
    print(f"{mode} {tag} {case}: max-abs error {err:.3e}, e32_m {e32:.3e}, error / e32_m {err / max(e32, 1e-300):.2f}, allowed {allowed:.2e}")
    assert err <= allowed, f"{mode} {tag} {case}: error {err:.3e} > allowed {allowed:.3e} (e32_m {e32:.3e})"
    return got, want


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_plain_conv(case, mode):
    _check("plain", mode, case, inputs(case, ()))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_switch_together(case, mode):
    _check("all", mode, case, inputs(case, set(SWITCHES) - {"noise_shared"}, seed=1))
    _check("all, shared noise", mode, case, inputs(case, set(SWITCHES) - {"noise"}, seed=2))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("case", [CASES[2], CASES[6]], ids=case_id)
def test_each_switch_alone(case, switch, mode):
    a = inputs(case, {switch}, seed=3)
    got, _ = _check(switch, mode, case, a)
    plain = conv2d_mode(mode, a["x"], a["w"])
    assert float((got.double() - plain).abs().max()) > 1e-3, f"{switch} changed nothing"


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[6], CASES[8]], ids=case_id)
def test_borders(case, mode):
    """An input that is non-zero only on the outermost ring: every output value near an edge depends on the zero padding."""
    a = inputs(case, (), seed=4, ring=True)
    got, want = _check("ring", mode, case, a)
    H, W = case[4], case[5]
    if H > 4 and W > 4:
        assert float(want[:, :, 2:-2, 2:-2].abs().max()) == 0.0 and float(got[:, :, 2:-2, 2:-2].abs().max()) == 0.0


@pytest.mark.parametrize("mode", sorted(MODES))
def test_shared_input_image(mode):
    """x_bstride = 0: one image for every sample (the decoder's constant input), told apart by the input scale."""
    case = (32, 16, 3, 3, 4, 4)
    a = inputs(case, {"in_scale"}, seed=5)
    a["x"] = a["x"][:1].expand(3, -1, -1, -1).contiguous()
    with torch.no_grad():
        want = conv2d_mode(mode, **a)
        allowed, e32 = allowance(want, conv2d_mode(mode, a["x"].float(), a["w"].float(), in_scale=a["in_scale"].float()))
    got = _gpu(case, a, MODES[mode], x_bstride=0, x=_cl(a["x"][:1])).double()
    err = float((got - want).abs().max())
    print(f"{mode} shared image: max-abs error {err:.3e}, e32_m {e32:.3e}, error / e32_m {err / e32:.2f}")
    assert err <= allowed
    assert not torch.equal(got[0], got[1])


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", [CASES[3], CASES[6], CASES[7]], ids=case_id)
def test_bit_identity_across_runs_and_batch_splits(case, mode):
    """Two runs give the same bits, and B = 3 in one call gives the bits of three calls with B = 1: the tile never depends on B."""
    Cin, Cout, k, _, H, W = case
    case3 = (Cin, Cout, k, 3, H, W)
    a = inputs(case3, set(SWITCHES) - {"noise_shared"}, seed=6)
    whole = _gpu(case3, a, MODES[mode])
    assert torch.equal(_gpu(case3, a, MODES[mode]), whole)
    per_sample = ("x", "in_scale", "out_scale", "noise", "sft_scale", "sft_shift", "residual")
    parts = []
    for b in range(3):
        ab = {key: (v[b:b + 1] if key in per_sample else v) for key, v in a.items()}
        parts.append(_gpu((Cin, Cout, k, 1, H, W), ab, MODES[mode]))
    assert torch.equal(torch.cat(parts), whole)
    assert not torch.equal(whole[0], whole[1])


@pytest.mark.parametrize("case", [CASES[2], CASES[6]], ids=case_id)
def test_precision_0_is_the_fp32_kernel(case):
    a = inputs(case, set(SWITCHES) - {"noise_shared"}, seed=7)
    f32 = _gpu(case, a, 0, entry="plain")
    assert torch.equal(_gpu(case, a, 0), f32)
    for mode in MODES.values():
        assert not torch.equal(_gpu(case, a, mode), f32)
