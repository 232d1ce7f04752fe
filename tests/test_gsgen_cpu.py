"""The Gaussian generators without a GPU: the float64 restatement (tests/gsgen_ref.py) against the fixtures made from the reference's
own classes (tools/make_golden_gsgen.py), the host-only plane geometry of the C ABI, deliberately wrong variants, the state-dict
manifest, and every refusal of the Python class and of the C ABI that fires before the device is touched."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import gsgen_cases as cases
import gsgen_ref
from artalk_amd import capi
from artalk_amd import gsgen

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(cases.CASES)
# variant -> the attributes it touches
WRONG = {
    "channel_sigmoid": ("colors",), "row_rotation": ("rotations",), "l1_plus": ("xyz",), "no_scale": ("scales",),
    "sincos_swapped": ("colors",), "linspace_up": ("xyz",), "relu_last": ("colors",), "leaky": ("colors",),
}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "gsgen_ref.npz"))


def test_cases_are_the_goldens(gold):
    assert int(gold["seed"]) == cases.SEED
    for name in NAMES:
        f0, f1 = cases.features(name)
        assert np.array_equal(gold[f"{name}_f_feature0"], f0) and np.array_equal(gold[f"{name}_f_feature1"], f1)
        assert np.array_equal(gold[f"{name}_transform_matrix"], cases.transform_matrix(name))
        assert gold[f"{name}_xyz"].shape == (cases.n_gaussians(name), 3) and cases.CASES[name][4] >= 5


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_golden(gold, name):
    r = cases.reference_run(name)
    for k in cases.ATTRS:
        want = torch.from_numpy(gold[f"{name}_{k}"])
        rel = float((r["want"][k] - want).abs().max() / want.abs().max())
        print(f"case {name} {k}: restatement vs reference float64, relative error {rel:.2e}")
        assert r["want"][k].shape == want.shape and rel <= 1e-12
    V = cases.CASES[name][0]
    assert float(r["want"]["xyz"][:V].abs().max()) == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_planes(gold, name):
    """The restatement equals the reference's build_points_planes, and artalk_gsgen_planes stays within the float32 allowance of it."""
    P = cases.CASES[name][4]
    tm = cases.transform_matrix(name)
    want, wdir, wenc = (torch.from_numpy(gold[f"{name}_{k}"]) for k in ("plane_points", "plane_dirs", "direnc"))
    pts64, d64 = gsgen_ref.planes(P, tm, torch.float64)
    assert float((pts64 - want).abs().max() / want.abs().max()) <= 1e-12 and torch.equal(d64, wdir)
    pts32, d32 = gsgen_ref.planes(P, tm, torch.float32)
    e32 = float((pts32.double() - want).abs().max())
    enc32 = float((gsgen_ref.direnc(d32).double() - wenc).abs().max())
    pts, d, enc = gsgen.planes(tm, P)
    err, err_enc = float((pts.double() - want).abs().max()), float((enc.double() - wenc).abs().max())
    print(f"case {name}: plane points error {err:.2e} (e32 {e32:.2e}), direnc error {err_enc:.2e} (e32 {enc32:.2e})")
    assert err <= cases.allowance(e32, float(want.abs().max()))
    assert err_enc <= cases.allowance(enc32, float(wenc.abs().max()))
    assert torch.equal(d.double(), wdir)


@pytest.mark.parametrize("which", sorted(WRONG))
@pytest.mark.parametrize("name", NAMES)
def test_wrong_variants_miss_golden(gold, name, which):
    assert which in gsgen_ref.VARIANTS
    r = cases.reference_run(name)
    with torch.no_grad():
        got = gsgen_ref.generate(r["sd"], r["f0"], r["f1"], r["tm"], torch.float64, variant=which)
    for k in WRONG[which]:
        err = float((got[k] - torch.from_numpy(gold[f"{name}_{k}"])).abs().max())
        print(f"case {name} {which} {k}: error {err:.3e} = {err / r['allow'][k]:.0f} x the GPU allowance {r['allow'][k]:.2e}")
        assert err >= 100.0 * r["allow"][k]


def test_manifest_at_the_reference_sizes():
    want = json.load(open(os.path.join(GOLD, "gsgen_manifest.json")))
    got = [[k, list(s)] for k, s in gsgen.state_dict_manifest(*cases.REFERENCE_DIMS)]
    assert got == want
    sd = gsgen.synth_state_dict(*cases.CASES["A"], seed=3)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == gsgen.state_dict_manifest(*cases.CASES["A"])
    again = gsgen.synth_state_dict(*cases.CASES["A"], seed=3)
    assert all(torch.equal(sd[k], again[k]) for k in sd)


def test_exported_symbols():
    L = capi.lib()
    for s in ("artalk_gsgen_create", "artalk_gsgen_set_tensor", "artalk_gsgen_finalize", "artalk_gsgen_planes", "artalk_gsgen_generate",
              "artalk_gsgen_set_timing", "artalk_gsgen_get_timing", "artalk_gsgen_dims", "artalk_gsgen_destroy", "artalk_gsgen_last_error",
              "artalk_op_conv2d_relu", "artalk_op_gs_local_input", "artalk_op_gs_global_input", "artalk_op_gs_concat_dir",
              "artalk_op_gs_local_attr", "artalk_op_gs_global_attr"):
        assert hasattr(L, s) and s in capi.SYMBOLS


# ---- refusals of the C ABI, all before the device is touched
def _create(dims=(50, 16, 48, 16, 6)):
    h = C.c_void_p()
    assert capi.lib().artalk_gsgen_create(0, *dims, C.byref(h)) == capi.OK
    return h


@pytest.mark.parametrize("dims,word", [((0, 16, 48, 16, 6), "V"), ((50, 16, 47, 16, 6), "multiple of 4"), ((50, 16, 48, 15, 6), "even"),
                                       ((50, 16, 48, 16, 2), "P"), ((50, 0, 48, 16, 6), "Dh"), ((50, 16, 48, 16, 5000), "P")])
def test_create_refuses_sizes(dims, word):
    L = capi.lib()
    h = C.c_void_p()
    assert L.artalk_gsgen_create(0, *dims, C.byref(h)) == capi.EINVAL and not h.value
    assert word in L.artalk_gsgen_last_error(None).decode()


def test_c_abi_refusals():
    L = capi.lib()
    assert L.artalk_gsgen_create(0, 50, 16, 48, 16, 6, None) == capi.EINVAL
    h = C.c_void_p()
    assert L.artalk_gsgen_create(-1, 50, 16, 48, 16, 6, C.byref(h)) == capi.EINVAL
    for f, args in ((L.artalk_gsgen_set_tensor, (None, b"head_base", None, 0, None)), (L.artalk_gsgen_finalize, (None,)),
                    (L.artalk_gsgen_generate, (None,) * 10), (L.artalk_gsgen_set_timing, (None, 1)), (L.artalk_gsgen_get_timing, (None, None, None)),
                    (L.artalk_gsgen_dims, (None,) * 7)):
        assert f(*args) == capi.EINVAL and "NULL" in L.artalk_gsgen_last_error(None).decode()
    L.artalk_gsgen_destroy(None)
    h = _create()
    try:
        v, p, fin = C.c_int32(), C.c_int32(), C.c_int32(7)
        assert L.artalk_gsgen_dims(h, C.byref(v), None, None, None, C.byref(p), C.byref(fin)) == 0 and (v.value, p.value, fin.value) == (50, 6, 0)
        x = torch.zeros(50, 16)
        shape = (C.c_int64 * 2)(50, 16)
        assert L.artalk_gsgen_set_tensor(h, None, capi.ptr(x), 2, shape) == capi.EINVAL
        assert L.artalk_gsgen_set_tensor(h, b"head_base", None, 2, shape) == capi.EINVAL
        assert L.artalk_gsgen_set_tensor(h, b"head_bass", capi.ptr(x), 2, shape) == capi.EKEY
        assert L.artalk_gsgen_last_error(h).decode() == "Unexpected key in state_dict: head_bass"
        assert L.artalk_gsgen_set_tensor(h, b"head_base", capi.ptr(x), 2, (C.c_int64 * 2)(16, 50)) == capi.EINVAL
        assert L.artalk_gsgen_last_error(h).decode() == "size mismatch for head_base"
        assert L.artalk_gsgen_set_tensor(h, b"head_base", capi.ptr(x), 1, (C.c_int64 * 1)(800)) == capi.EINVAL
        assert L.artalk_gsgen_set_tensor(h, b"head_base", capi.ptr(x), 2, shape) == capi.OK
        assert L.artalk_gsgen_finalize(h) == capi.EMISSING
        msg = L.artalk_gsgen_last_error(h).decode()
        assert msg.startswith("Missing key(s) in state_dict: gs_generator_g.feature_layers.0.weight, gs_generator_g.feature_layers.0.bias, ")
        assert msg.endswith(", ...") and msg.count(",") == 8 and "head_base" not in msg
        one = (C.c_void_p * 1)(1)      # never read: the call order is checked first
        assert L.artalk_gsgen_generate(h, one, one, one, one, one, one, one, one, None) == capi.ESTATE
        assert "before artalk_gsgen_finalize" in L.artalk_gsgen_last_error(h).decode()
    finally:
        L.artalk_gsgen_destroy(h)


def test_planes_and_ops_refuse_before_the_device():
    L = capi.lib()
    tm = torch.from_numpy(cases.transform_matrix("A")).contiguous()
    out = torch.empty(36, 3)
    assert L.artalk_gsgen_planes(None, 6, capi.ptr(out), None, None) == capi.EINVAL
    assert L.artalk_gsgen_planes(capi.ptr(tm), 2, capi.ptr(out), None, None) == capi.EINVAL
    bad = tm.clone()
    bad[1, 2] = float("nan")
    assert L.artalk_gsgen_planes(capi.ptr(bad), 6, capi.ptr(out), None, None) == capi.EINVAL
    assert "finite" in L.artalk_gsgen_last_error(None).decode()
    assert L.artalk_gsgen_planes(capi.ptr(tm), 6, None, None, None) == capi.OK
    one = C.c_void_p(16)      # never read
    assert L.artalk_op_conv2d_relu(None, 0, one, one, 1, 4, 4, 8, 8, 3, None, 1, None) == capi.EINVAL
    assert L.artalk_op_conv2d_relu(one, 0, one, one, 1, 4, 4, 8, 8, 2, None, 1, None) == capi.EINVAL
    assert L.artalk_op_conv2d_relu(one, 10, one, one, 1, 4, 4, 8, 8, 3, None, 1, None) == capi.EINVAL
    assert L.artalk_op_gs_local_input(None, one, one, 16, 6, None) == capi.EINVAL
    assert L.artalk_op_gs_local_input(one, one, one, 0, 6, None) == capi.EINVAL
    assert L.artalk_op_gs_global_input(one, None, one, 50, 16, 48, None) == capi.EINVAL
    assert L.artalk_op_gs_global_input(one, one, one, 0, 16, 48, None) == capi.EINVAL
    assert L.artalk_op_gs_concat_dir(one, one, None, 50, 16, None) == capi.EINVAL
    assert L.artalk_op_gs_concat_dir(one, one, one, 50, 0, None) == capi.EINVAL
    assert L.artalk_op_gs_local_attr(one, None, 6, 1, 0, one, one, one, one, one, None) == capi.EINVAL
    assert L.artalk_op_gs_local_attr(one, capi.ptr(tm), 6, 0, 0, one, one, one, one, one, None) == capi.EINVAL
    assert L.artalk_op_gs_local_attr(one, capi.ptr(tm), 2, 1, 0, one, one, one, one, one, None) == capi.EINVAL
    assert L.artalk_op_gs_local_attr(one, capi.ptr(tm), 6, 1, -1, one, one, one, one, one, None) == capi.EINVAL
    assert L.artalk_op_gs_local_attr(one, capi.ptr(bad), 6, 1, 0, one, one, one, one, one, None) == capi.EINVAL
    assert L.artalk_op_gs_global_attr(one, one, one, None, 50, one, one, one, one, one, None) == capi.EINVAL
    assert L.artalk_op_gs_global_attr(one, one, one, one, 0, one, one, one, one, one, None) == capi.EINVAL


# ---- refusals of the Python class
def test_python_refusals():
    with pytest.raises(ValueError, match="multiple of 4"):
        gsgen.GSGenerators(50, 16, 47, 16, 6)
    with pytest.raises(ValueError, match="even"):
        gsgen.GSGenerators(50, 16, 48, 15, 6)
    with pytest.raises(ValueError, match="at least 3"):
        gsgen.GSGenerators(50, 16, 48, 16, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gsgen.GSGenerators(50, 16, 48, 16, 6, device="cpu")
    with pytest.raises(ValueError, match="transform_matrix"):
        gsgen.planes(torch.zeros(3, 3), 6)
    g = gsgen.GSGenerators(*cases.CASES["A"])
    assert g.n_gaussians == cases.n_gaussians("A")
    sd = g.synth_state_dict(seed=cases.SEED)
    f0, f1 = (torch.from_numpy(t) for t in cases.features("A"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.build_avatar(f0, f1, cases.transform_matrix("A"), torch.zeros(300))

    def fails(d):
        with pytest.raises(RuntimeError) as e:
            g.load_state_dict(d)
        return str(e.value)

    assert "Unexpected key in state_dict: gs_generator_l2.gaussian_conv.0.bias" in fails(dict(sd, **{"gs_generator_l2.gaussian_conv.0.bias": torch.zeros(8)}))
    assert "size mismatch for head_base" in fails(dict(sd, head_base=torch.zeros(50, 17)))
    part = {k: v for k, v in sd.items() if not k.startswith("gs_generator_l1.")}
    part.update({"base_model.x": torch.zeros(1), "upsampler.conv_body_first.weight": torch.zeros(1), "percep_loss.w": torch.zeros(1)})
    msg = fails(part)
    assert msg.startswith("Error(s) in loading state_dict for GSGenerators:") and "Missing key(s) in state_dict: gs_generator_l1.gaussian_conv.0.weight" in msg
    assert "Unexpected" not in msg and g._h is None


def test_add_avatar():
    import gaga_cases
    from artalk_amd import styleunet as su
    from artalk_amd.gaga import GAGAvatar
    head = GAGAvatar({"a": gaga_cases.avatar()}, su.synth_state_dict(gaga_cases.S), image_size=gaga_cases.S, n_dynamic=gaga_cases.V)
    b = gaga_cases.avatar(seed=9)
    b["xyz"] = b["xyz"][None]      # the reference's batch axis
    head.add_avatar("b", b)
    assert torch.equal(head.all_gagavatar_id["b"]["xyz"], b["xyz"][0])
    head.set_avatar_id("b")
    head._uploaded = "b"
    head.add_avatar("a", gaga_cases.avatar(seed=4))
    assert head._uploaded == "b"
    head.add_avatar("b", gaga_cases.avatar(seed=5))
    assert head._uploaded is None and head._tracked_name == "b"
    with pytest.raises(ValueError, match="lacks 'scales'"):
        head.add_avatar("c", {k: v for k, v in b.items() if k != "scales"})
    assert "c" not in head.all_gagavatar_id
