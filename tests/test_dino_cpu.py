"""DINOBase without a GPU: the float64 restatement (tests/dino_ref.py) against the fixtures made from the reference's own module
(tools/make_golden_dino.py), what float32 loses by itself, deliberately wrong readings, the state-dict manifest, and every refusal of the
C ABI, of the Python class and of the engine's keywords.  Run with -s for the figures."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import dino_cases as cases
import dino_ref
from artalk_amd import capi
from artalk_amd import dino

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXACT = 1e-11      # float64 against float64: two implementations of the same sums (the largest value is about 15)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "dino_ref.npz")), np.load(os.path.join(GOLD, "dino_ref_taps.npz"))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_restatement_equals_the_reference(name, gold):
    r = cases.reference_run(name)
    for k in cases.OUTPUTS:
        want = gold[0][f"{name}_{k}"]
        d = float(np.abs(r["want"][k].numpy() - want).max())
        print(f"case {name} {k}: restatement - reference {d:.2e} (largest value {float(np.abs(want).max()):.2f}); e32 {r['e32'][k]:.2e}")
        assert want.dtype == np.float64 and d <= EXACT
        assert 0.05 <= float(np.abs(want).max()) <= 50 and 1e-8 < r["e32"][k] < 1e-3
    assert float((gold[0][f"{name}_plane"] == 0).mean()) <= 0.01
    if name == "A":
        stride = int(gold[1]["rn0_channel_stride"])
        for i in range(4):
            assert float(np.abs(r["want"][f"tap{i}"].numpy() - gold[1][f"A_tap{i}"]).max()) <= EXACT
            rn = r["want"][f"rn{i}"].numpy()
            assert float(np.abs((rn[..., ::stride] if i == 0 else rn) - gold[1][f"A_rn{i}"]).max()) <= EXACT


@pytest.mark.parametrize("which", list(dino_ref.VARIANTS))
def test_a_wrong_reading_leaves_the_allowance(which):
    """Each misreading moves the output it touches by far more than a kernel may differ from the fixture.  'first_four' needs a depth
    above 4 to be another reading at all, so it is judged on case A; the class token is only in the global vector."""
    key = "glob" if which == "cls_global" else "plane"
    for name in ("A",) if which == "first_four" else list(cases.CASES):
        r = cases.reference_run(name)
        with torch.no_grad():
            got = dino_ref.forward(r["sd"], r["image"], r["dims"], torch.float64, variant=which)
        factor = float((got[key] - r["want"][key]).abs().max()) / r["allow"][key]
        print(f"{which} ({dino_ref.VARIANTS[which]}), case {name}: {key} off by {factor:.1e} x the allowance")
        assert factor > 100


def test_manifest():
    m = json.load(open(os.path.join(GOLD, "dino_manifest.json")))
    ours = [[k, list(s)] for k, s in dino.state_dict_manifest(*cases.REFERENCE_DIMS)]
    assert m["state_dict"] == ours and m["cases"] == {k: list(v) for k, v in cases.CASES.items()}
    # the head's keys, order and shapes are those of the reference's own module
    assert [x for x in ours if not x[0].startswith("dino_model.")] == m["head_state_dict"]
    assert len(m["reference_sha256"]) == 64
    sd = dino.synth_state_dict(*cases.CASES["B"], seed=3)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == dino.state_dict_manifest(*cases.CASES["B"])
    again = dino.synth_state_dict(*cases.CASES["B"], seed=3)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert not torch.equal(sd["output_conv.weight"], dino.synth_state_dict(*cases.CASES["B"], seed=4)["output_conv.weight"])
    assert dino.level_sizes(37) == (148, 74, 37, 19) and dino.level_sizes(6) == (24, 12, 6, 3)


def test_symbols():
    L = capi.lib()
    for s in capi.SYMBOLS:
        if "dino" in s:
            assert hasattr(L, s), s
    assert sum("dino" in s for s in capi.SYMBOLS) == 23


def _create(*dims):
    h = C.c_void_p()
    return capi.lib().artalk_dino_create(0, *dims, C.byref(h)), h


@pytest.mark.parametrize("dims,word", [
    ((128, 3, 2, 5, 16), "depth"), ((128, 4, 1, 5, 16), "64 or 32"), ((128, 4, 8, 5, 16), "64 or 32"), ((100, 4, 2, 5, 16), "multiple of 32"),
    ((128, 4, 2, 1, 16), "grid"), ((128, 4, 2, 65, 16), "grid"), ((128, 4, 2, 5, 0), "output_dim"), ((128, 4, 0, 5, 16), "64 or 32")])
def test_create_refuses(dims, word):
    rc, h = _create(*dims)      # (vit_dim, depth, heads, grid, output_dim)
    assert rc == capi.EINVAL and not h.value
    assert word in capi.lib().artalk_dino_last_error(None).decode()


def test_c_abi_refusals():
    L = capi.lib()
    assert L.artalk_dino_create(0, 128, 4, 2, 5, 16, None) == capi.EINVAL
    h = C.c_void_p()
    assert L.artalk_dino_create(-1, 128, 4, 2, 5, 16, C.byref(h)) == capi.EINVAL
    for f, args in ((L.artalk_dino_set_tensor, (None, b"output_conv.bias", None, 0, None)), (L.artalk_dino_finalize, (None,)),
                    (L.artalk_dino_forward, (None, None, 70, 70, None, None, None)), (L.artalk_dino_prepare_image, (None, None, 1, 1, None, None)),
                    (L.artalk_dino_read, (None, b"tap0", None, 0, None)), (L.artalk_dino_set_timing, (None, 1)),
                    (L.artalk_dino_get_timing, (None, None, None)), (L.artalk_dino_dims, (None,) * 7)):
        assert f(*args) == capi.EINVAL and "NULL" in L.artalk_dino_last_error(None).decode()
    L.artalk_dino_destroy(None)
    rc, h = _create(64, 4, 2, 6, 16)
    assert rc == capi.OK
    try:
        v, g, fin = C.c_int32(), C.c_int32(), C.c_int32(-1)
        assert L.artalk_dino_dims(h, C.byref(v), None, None, C.byref(g), None, C.byref(fin)) == 0 and (v.value, g.value, fin.value) == (64, 6, 0)
        x = torch.zeros(38 * 64)
        one = capi.ptr(x)
        sh = (C.c_int64 * 1)(16)
        assert L.artalk_dino_set_tensor(h, None, one, 1, sh) == capi.EINVAL
        assert L.artalk_dino_set_tensor(h, b"output_conv.bias", None, 1, sh) == capi.EINVAL
        assert L.artalk_dino_set_tensor(h, b"output_conv.bios", one, 1, sh) == capi.EKEY
        assert L.artalk_dino_last_error(h).decode() == "Unexpected key in state_dict: output_conv.bios"
        assert L.artalk_dino_set_tensor(h, b"dino_model.register_tokens", one, 1, sh) == capi.EKEY      # register tokens are not built
        assert L.artalk_dino_set_tensor(h, b"output_conv.bias", one, 1, (C.c_int64 * 1)(17)) == capi.EINVAL
        assert L.artalk_dino_last_error(h).decode() == "size mismatch for output_conv.bias"
        assert L.artalk_dino_set_tensor(h, b"output_conv.bias", one, 1, sh) == capi.OK
        # a pos_embed of another grid: 26 positions (5 x 5) where 6 x 6 takes 37
        assert L.artalk_dino_set_tensor(h, b"dino_model.pos_embed", one, 3, (C.c_int64 * 3)(1, 26, 64)) == capi.EINVAL
        msg = L.artalk_dino_last_error(h).decode()
        assert "pos_embed" in msg and "37" in msg and "not interpolated" in msg
        assert L.artalk_dino_set_tensor(h, b"dino_model.pos_embed", one, 3, (C.c_int64 * 3)(1, 37, 64)) == capi.OK
        assert L.artalk_dino_finalize(h) == capi.EMISSING
        msg = L.artalk_dino_last_error(h).decode()
        assert msg.startswith("Missing key(s) in state_dict: dino_model.cls_token, dino_model.patch_embed.proj.weight") and msg.endswith(", ...")
        assert "mask_token" not in msg      # accepted, unused, may be absent
        # the image: 14 x grid = 84 a side, square; refused on the host, whatever the state of the handle
        assert L.artalk_dino_forward(h, one, 84, 98, one, one, None) == capi.EINVAL and "square" in L.artalk_dino_last_error(h).decode()
        assert L.artalk_dino_forward(h, one, 70, 70, one, one, None) == capi.EINVAL
        msg = L.artalk_dino_last_error(h).decode()
        assert "84 x 84" in msg and "70 x 70" in msg and "not interpolated" in msg
        for args in ((None, 84, 84, one, one), (one, 84, 84, None, one), (one, 84, 84, one, None)):
            assert L.artalk_dino_forward(h, *args, None) == capi.EINVAL and "NULL" in L.artalk_dino_last_error(h).decode()
        assert L.artalk_dino_forward(h, one, 84, 84, one, one, None) == capi.ESTATE
        assert "before artalk_dino_finalize" in L.artalk_dino_last_error(h).decode()
        assert L.artalk_dino_read(h, b"tap0", one, 1, None) == capi.ESTATE
        assert L.artalk_dino_prepare_image(h, None, 4, 4, one, None) == capi.EINVAL
        assert L.artalk_dino_prepare_image(h, one, 0, 4, one, None) == capi.EINVAL
    finally:
        L.artalk_dino_destroy(h)


def test_op_entry_points_refuse_before_the_device():
    L = capi.lib()
    x = torch.zeros(64)
    p = capi.ptr(x)
    odd = C.c_void_p(x.data_ptr() + 4)
    assert L.artalk_op_dino_resize_aa(None, p, 3, 4, 4, 2, 2, 0, 0, None) == capi.EINVAL
    assert L.artalk_op_dino_resize_aa(p, p, 3, 4, 4, 0, 2, 0, 0, None) == capi.EINVAL
    assert L.artalk_op_dino_resize_aa(p, p, 4, 4, 4, 2, 2, 0, 1, None) == capi.EINVAL      # normalisation is for 3 channels
    assert L.artalk_op_dino_normalize(p, None, 4, None) == capi.EINVAL
    assert L.artalk_op_dino_im2col(p, p, 0, None) == capi.EINVAL
    assert L.artalk_op_dino_tokens(p, p, p, p, 5, 6, None) == capi.EINVAL
    assert L.artalk_op_dino_tokens(p, p, p, odd, 5, 8, None) == capi.EINVAL
    assert L.artalk_op_dino_layernorm(p, p, p, None, 5, 8, None) == capi.EINVAL
    assert L.artalk_op_dino_layernorm(p, p, p, p, 5, 6, None) == capi.EINVAL
    assert L.artalk_op_dino_strip(p, p, 0, 8, None) == capi.EINVAL
    assert L.artalk_op_dino_shuffle(p, p, p, 5, 9, 8, None) == capi.EINVAL
    assert L.artalk_op_dino_shuffle(p, p, p, 5, 2, 6, None) == capi.EINVAL
    assert L.artalk_op_dino_gather_s2(p, odd, 5, 8, None) == capi.EINVAL
    assert L.artalk_op_dino_concat(p, None, p, 4, 8, None) == capi.EINVAL
    assert L.artalk_op_dino_resize_ac(p, p, 3, 3, 5, 5, 6, None) == capi.EINVAL
    assert L.artalk_op_dino_add_relu(p, None, None, p, 6, None) == capi.EINVAL
    assert L.artalk_op_dino_output(p, None, 4, 4, None, None, 0, None) == capi.EINVAL
    assert L.artalk_op_dino_output(p, p, 4, 4, p, None, 4, None) == capi.EINVAL


def test_python_class_refusals():
    with pytest.raises(ValueError, match="depth"):
        dino.DINOBase(16, 128, 3, 2, 5)
    with pytest.raises(ValueError, match="64 or 32"):
        dino.DINOBase(16, 128, 4, 8, 5)
    with pytest.raises(ValueError, match="positive int"):
        dino.DINOBase(16, 128.0, 4, 2, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dino.DINOBase(16, 128, 4, 2, 5, device="cpu")
    m = dino.DINOBase(16, 64, 4, 2, 6)
    assert (m.image_size, m.plane) == (84, 48) and m.state_dict_manifest() == dino.state_dict_manifest(16, 64, 4, 2, 6)
    with pytest.raises(RuntimeError, match="load_state_dict"):
        m.forward(torch.zeros(3, 84, 84))
    with pytest.raises(RuntimeError, match="load_state_dict"):
        m.prepare_image(torch.zeros(3, 84, 84))
    # load_state_dict gathers the library's messages in torch's wording; these fail before the device is touched
    sd = {"output_conv.bias": torch.zeros(16), "output_conv.bios": torch.zeros(16), "layer_rn.0.weight": torch.zeros(256, 259, 3, 2)}
    with pytest.raises(RuntimeError) as e:
        m.load_state_dict(sd)
    msg = str(e.value)
    assert "Error(s) in loading state_dict for DINOBase" in msg and "Unexpected key in state_dict: output_conv.bios" in msg
    assert "size mismatch for layer_rn.0.weight" in msg
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({"output_conv.bias": torch.zeros(16)})
    # a whole checkpoint: base_model.* is used, the other known prefixes are ignored, anything else is refused
    whole = {"base_model.output_conv.bias": torch.zeros(16), "head_base": torch.zeros(3, 3), "upsampler.x": torch.zeros(1),
             "gs_generator_g.y": torch.zeros(1), "percep_loss.z": torch.zeros(1), "harmo_encoder.f": torch.zeros(1), "stranger": torch.zeros(1)}
    with pytest.raises(RuntimeError) as e:
        m.load_state_dict(whole)
    assert "Unexpected key in state_dict: stranger" in str(e.value) and "head_base" not in str(e.value) and "upsampler" not in str(e.value)
    assert m._h is None


def test_engine_keywords(tmp_path):
    from artalk_amd.engine import ARTAvatarInferEngine
    from artalk_amd.gaga import GAGAvatar
    stub = types.SimpleNamespace(cfg=None)      # an already loaded model: the constructor loads nothing
    with pytest.raises(NotImplementedError, match="pack"):      # as before
        ARTAvatarInferEngine(load_gaga=True)
    with pytest.raises(NotImplementedError, match="pack"):
        ARTAvatarInferEngine(load_gaga=True, gaga_tracked={}, model=stub)
    with pytest.raises(ValueError, match="gaga_tracked"):
        ARTAvatarInferEngine(load_gaga=True, gaga_ckpt={"head_base": torch.zeros(2, 2)}, model=stub)
    with pytest.raises(ValueError, match="lacks"):      # the keywords are accepted; the dict is not a checkpoint
        ARTAvatarInferEngine(load_gaga=True, gaga_ckpt={"head_base": torch.zeros(2, 2)}, gaga_tracked={"a": {}}, gaga_flame="flame", model=stub)
    # a file that needs pickle is refused with a message that says to pass the dict
    path = tmp_path / "tracked.pt"
    torch.save({"a": {"image": types.SimpleNamespace(x=1)}}, path)
    with pytest.raises(ValueError, match="pass the dict"):
        ARTAvatarInferEngine(load_gaga=True, gaga_ckpt={"head_base": torch.zeros(2, 2)}, gaga_tracked=str(path), model=stub)
    torch.save([1, 2], path)
    with pytest.raises(ValueError, match="not a dict"):
        ARTAvatarInferEngine(load_gaga=True, gaga_ckpt=str(path), gaga_tracked={"a": {}}, model=stub)
    with pytest.raises(ValueError, match="tracked"):
        GAGAvatar.from_checkpoint({"head_base": torch.zeros(2, 2), "base_model.dino_model.pos_embed": torch.zeros(1, 26, 64),
                                   "base_model.dino_model.cls_token": torch.zeros(1, 1, 64), "base_model.output_conv.weight": torch.zeros(16, 256, 3, 3)}, {})
    with pytest.raises(ValueError, match="image"):
        GAGAvatar._check_tracked("a", {"image": torch.zeros(4, 4), "transform_matrix": torch.zeros(3, 4), "shapecode": [0.0]})
