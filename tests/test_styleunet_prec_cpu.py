"""The StyleUNet precision modes without a GPU: every refusal of the new entry points that fires before the device is touched, the
Python name checks, and what the GPU allowance of tests/test_styleunet_prec_ops_gpu.py can tell apart - for every conv case and both
modes, each deliberately wrong variant of the mode's definition (tests/styleunet_prec_ref.py) misses that allowance by more than 2 x,
the exact fp32 convolution included: a mode that silently runs the old kernel fails the GPU test."""
import ctypes as C

import pytest
import torch

from artalk_amd import capi
from artalk_amd import styleunet as su
from artalk_amd.gaga import GAGAvatar
from styleunet_prec_ref import CASES, WRONG, allowance, case_id, conv2d_mode, inputs


def _handle(S=8):
    L = capi.lib()
    h = C.c_void_p()
    assert L.artalk_styleunet_create(0, 32, 3, S, C.byref(h)) == capi.OK
    return L, h


def test_new_symbols_are_exported():
    L = capi.lib()
    for name in ("artalk_styleunet_set_precision", "artalk_styleunet_get_precision", "artalk_op_conv2d_ex", "artalk_styleunet_get_launch_timing"):
        assert name in capi.SYMBOLS and hasattr(L, name), name


def test_set_precision_refusals_and_host_only_before_finalize():
    L = capi.lib()
    assert L.artalk_styleunet_set_precision(None, 1) == capi.EINVAL
    assert L.artalk_styleunet_get_precision(None) == capi.EINVAL
    L, h = _handle(8)
    try:
        assert L.artalk_styleunet_get_precision(h) == 0
        for bad in (-1, 3, 17):
            assert L.artalk_styleunet_set_precision(h, bad) == capi.EINVAL
            assert b"precision" in L.artalk_styleunet_last_error(h)
            assert L.artalk_styleunet_get_precision(h) == 0
        for mode in (1, 2, 0, 1):      # no device here: before finalize the mode is only remembered
            assert L.artalk_styleunet_set_precision(h, mode) == capi.OK
            assert L.artalk_styleunet_get_precision(h) == mode
        assert L.artalk_styleunet_get_launch_timing(None, None, None, 0) == capi.EINVAL
        assert L.artalk_styleunet_get_launch_timing(h, None, None, 0) == 0      # no timed call yet
        fin, slab = C.c_int(-1), C.c_int(-1)
        assert L.artalk_styleunet_dims(h, None, None, None, C.byref(fin), C.byref(slab)) == 0
        assert fin.value == 0 and slab.value == 64
    finally:
        L.artalk_styleunet_destroy(h)


def test_op_conv2d_ex_refusals_before_the_device_is_touched():
    L = capi.lib()
    p = C.c_void_p(4096)      # never dereferenced: every call below is refused

    def call(x=p, xb=0, w=p, out=p, B=1, H=4, W=4, Cin=16, Cout=16, k=3, noise=None, nb=0, nw=None, sc=None, sh=None, prec=1):
        return L.artalk_op_conv2d_ex(x, xb, w, out, B, H, W, Cin, Cout, k, None, None, 1.0, noise, nb, nw, None, 0, sc, sh, None, prec, None)

    for prec in (0, 1, 2):
        assert call(x=None, prec=prec) == capi.EINVAL and call(w=None, prec=prec) == capi.EINVAL and call(out=None, prec=prec) == capi.EINVAL
        for kw in (dict(B=0), dict(H=0), dict(W=0), dict(Cin=0), dict(Cout=0), dict(k=2), dict(k=5), dict(xb=4 * 4 * 16 - 1)):
            assert call(prec=prec, **kw) == capi.EINVAL, kw
        assert call(noise=p, prec=prec) == capi.EINVAL
        assert call(noise=p, nw=p, nb=15, prec=prec) == capi.EINVAL
        assert call(sc=p, prec=prec) == capi.EINVAL and call(sh=p, prec=prec) == capi.EINVAL
    for prec in (-1, 3, 100):
        assert call(prec=prec) == capi.EINVAL


def test_python_names():
    assert su.PRECISIONS == {"f32": 0, "bf16x3": 1, "bf16": 2}
    net = su.StyleUNet(8, 8, 32, 3)
    assert net.precision == "f32"
    for bad in ("fp32", "bf16x2", "", None, 1):
        with pytest.raises(ValueError):
            net.set_precision(bad)
    assert net.set_precision("bf16x3") is net and net.precision == "bf16x3"      # before .to(device): remembered
    net.load_state_dict(su.synth_state_dict(8))
    assert net.precision == "bf16x3"
    assert net.set_precision("bf16").precision == "bf16"
    assert net.set_precision("f32").precision == "f32"


def test_gaga_passes_the_name_through():
    z = torch.zeros
    av = {"xyz": z(4, 3), "colors": z(4, 32), "opacities": z(4, 1), "scales": z(4, 3), "rotations": z(4, 4), "shapecode": z(300),
          "transform_matrix": z(3, 4)}
    head = GAGAvatar({"a": av}, su.synth_state_dict(8), image_size=8, n_dynamic=4)
    assert head.set_precision("bf16x3") is head and head.upsampler.precision == "bf16x3"
    with pytest.raises(ValueError):
        head.set_precision("half")
    assert head.upsampler.precision == "bf16x3"


@pytest.fixture(scope="module")
def plain():
    """Per case: the plain inputs (made once, shared, read only)."""
    return {c: inputs(c, ()) for c in CASES}


@pytest.mark.parametrize("mode", sorted(WRONG))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_wrong_variants_miss_the_gpu_allowance(plain, case, mode):
    a = plain[case]
    with torch.no_grad():
        want = conv2d_mode(mode, a["x"], a["w"])
        allowed, e32 = allowance(want, conv2d_mode(mode, a["x"].float(), a["w"].float()))
        for name, terms in WRONG[mode].items():
            miss = float((conv2d_mode(mode, a["x"], a["w"], terms=terms) - want).abs().max())
            print(f"{mode} {case} {name}: misses by {miss:.3e} = {miss / allowed:.1f} x the allowance {allowed:.2e} (e32 {e32:.2e})")
            assert miss > 2.0 * allowed, f"{mode} {case} {name}: {miss:.3e} is within 2 x the allowance {allowed:.3e}"
