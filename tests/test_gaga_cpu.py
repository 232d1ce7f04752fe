"""The GAGAvatar head without a GPU: exported symbols, every refusal that fires before the device is touched, the pack format, the
engine's wiring, and the host camera function against the float64 restatement (tests/gaga_ref.py).

Camera allowance, the project's convention: every entry within max(4 x e32, 1 ulp), where e32 is the largest difference between the
restatement evaluated in float32 and in float64 for the same case and 1 ulp is one float32 unit of the output's largest magnitude.

An ``artalk_gaga`` object borrows an ``artalk_flame`` handle, which cannot be made without a device, so the object's own refusals
(N < V, bad indices, a watermark larger than S, T < 0, a short stride, no avatar, an upsampler that is not finalized) are exercised
through ``artalk_op_gaga_check``, the host function the entry points themselves call; tests/test_gaga_gpu.py repeats them on a real
object."""
import ctypes as C

import numpy as np
import pytest
import torch

import gaga_cases as gc
import gaga_ref as ref
from artalk_amd import capi
from artalk_amd import gaga
from artalk_amd import styleunet as su

FACTOR = 4.0
NEW_SYMBOLS = ("artalk_gaga_create", "artalk_gaga_set_avatar", "artalk_gaga_set_forehead", "artalk_gaga_set_watermark",
               "artalk_gaga_reset_state", "artalk_gaga_set_slab", "artalk_gaga_render", "artalk_gaga_destroy", "artalk_gaga_last_error",
               "artalk_gaga_cameras", "artalk_op_gaga_flame_inputs", "artalk_op_gaga_forehead", "artalk_op_gaga_means",
               "artalk_op_gaga_finish", "artalk_op_gaga_check", "artalk_flame_dims", "artalk_styleunet_dims")


def test_new_symbols_are_exported():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS and hasattr(L, name), name


# ------------------------------------------------------------------------------------------------ refusals
def _check(V=64, S=16, N=136, idx=(1, 2), wm=(0, 0), T=1, stride=106, avatar=1, finalized=1):
    L = capi.lib()
    arr = (C.c_int32 * max(len(idx), 1))(*idx)
    msg = C.create_string_buffer(256)
    rc = L.artalk_op_gaga_check(V, S, N, arr, len(idx), wm[0], wm[1], T, stride, avatar, finalized, msg, 256)
    return rc, msg.value.decode()


def test_object_refusals_are_host_checks():
    assert _check() == (capi.OK, "")
    for kw, code, word in ((dict(N=63), capi.EINVAL, "at least V"), (dict(idx=(1, 64)), capi.EINVAL, "outside"),
                           (dict(idx=(1, -1)), capi.EINVAL, "outside"), (dict(idx=(5, 9, 5)), capi.EINVAL, "twice"),
                           (dict(wm=(17, 4)), capi.EINVAL, "does not fit"), (dict(wm=(4, 17)), capi.EINVAL, "does not fit"),
                           (dict(T=-1), capi.EINVAL, "T must not be negative"), (dict(stride=105), capi.EINVAL, "at least 106"),
                           (dict(avatar=0), capi.EINVAL, "no avatar"), (dict(finalized=0), capi.ESTATE, "not finalized")):
        rc, msg = _check(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    assert _check(N=64, wm=(16, 16), T=0, idx=())[0] == capi.OK
    # the reference's list passes: 68 distinct indices, the largest 3913
    assert _check(V=3914, N=3914, idx=tuple(range(3846, 3914)))[0] == capi.OK


def test_capi_refusals_before_the_device_is_touched():
    L = capi.lib()
    p = C.c_void_p(4096)      # never dereferenced: every call below is refused
    h = C.c_void_p()
    assert L.artalk_gaga_create(0, None, p, p, 64, 400, 16, C.byref(h)) == capi.EINVAL
    assert b"NULL" in L.artalk_gaga_last_error(None)
    assert L.artalk_gaga_create(0, p, None, p, 64, 400, 16, C.byref(h)) == capi.EINVAL
    assert L.artalk_gaga_create(0, p, p, None, 64, 400, 16, C.byref(h)) == capi.EINVAL
    assert L.artalk_gaga_create(0, p, p, p, 64, 400, 16, None) == capi.EINVAL
    assert L.artalk_gaga_create(-1, p, p, p, 64, 400, 16, C.byref(h)) == capi.EINVAL
    assert L.artalk_gaga_create(0, p, p, p, 0, 400, 16, C.byref(h)) == capi.EINVAL
    assert L.artalk_gaga_create(0, p, p, p, 64, 99, 16, C.byref(h)) == capi.EINVAL
    assert L.artalk_gaga_create(0, p, p, p, 64, 400, 0, C.byref(h)) == capi.EINVAL
    assert h.value is None
    assert L.artalk_gaga_set_avatar(None, 64, p, p, p, p, p, p, p) == capi.EINVAL
    assert L.artalk_gaga_set_forehead(None, p, 1) == capi.EINVAL
    assert L.artalk_gaga_set_watermark(None, p, 1, 1) == capi.EINVAL
    assert L.artalk_gaga_reset_state(None) == capi.EINVAL
    assert L.artalk_gaga_set_slab(None, 1) == capi.EINVAL
    assert L.artalk_gaga_render(None, p, 106, 1, None, None, 1, p, None) == capi.EINVAL
    assert L.artalk_gaga_last_error(None) == b"handle is NULL"
    L.artalk_gaga_destroy(None)
    assert L.artalk_flame_dims(None, None, None, None) == capi.EINVAL
    assert L.artalk_styleunet_dims(None, None, None, None, None, None) == capi.EINVAL
    # a StyleUNet handle before finalize says so
    u = C.c_void_p()
    assert L.artalk_styleunet_create(0, 32, 3, 16, C.byref(u)) == capi.OK
    try:
        dims = [C.c_int(-1) for _ in range(5)]
        assert L.artalk_styleunet_dims(u, *[C.byref(d) for d in dims]) == 0
        assert [d.value for d in dims[:4]] == [32, 3, 16, 0] and dims[4].value >= 1
    finally:
        L.artalk_styleunet_destroy(u)


def test_op_refusals_before_the_device_is_touched():
    L = capi.lib()
    p = C.c_void_p(4096)
    fi = L.artalk_op_gaga_flame_inputs
    assert fi(None, 106, p, 400, 1, p, p, None) == capi.EINVAL and fi(p, 106, p, 400, 1, None, p, None) == capi.EINVAL
    assert fi(p, 106, p, 400, 1, p, None, None) == capi.EINVAL and fi(p, 105, p, 400, 1, p, p, None) == capi.EINVAL
    assert fi(p, 106, None, 400, 1, p, p, None) == capi.EINVAL and fi(p, 106, p, 99, 1, p, p, None) == capi.EINVAL
    assert fi(p, 106, p, 400, 0, p, p, None) == capi.EINVAL
    fh = L.artalk_op_gaga_forehead
    assert fh(None, p, 1, 1, 8, p, p, None) == capi.EINVAL and fh(p, None, 1, 1, 8, p, p, None) == capi.EINVAL
    assert fh(p, p, 1, 1, 8, None, p, None) == capi.EINVAL and fh(p, p, 1, 1, 8, p, None, None) == capi.EINVAL
    assert fh(p, p, -1, 1, 8, p, p, None) == capi.EINVAL and fh(p, p, 1, -1, 8, p, p, None) == capi.EINVAL
    assert fh(p, p, 9, 1, 8, p, p, None) == capi.EINVAL
    assert fh(p, None, 0, 3, 8, p, p, None) == capi.OK      # K = 0: nothing to do, nothing launched
    me = L.artalk_op_gaga_means
    assert me(None, p, p, 1, 4, 8, None) == capi.EINVAL and me(p, None, p, 1, 4, 8, None) == capi.EINVAL
    assert me(p, p, None, 1, 4, 8, None) == capi.EINVAL and me(p, p, p, 0, 4, 8, None) == capi.EINVAL
    assert me(p, p, p, 1, 8, 7, None) == capi.EINVAL
    fin = L.artalk_op_gaga_finish
    assert fin(None, 1, 16, None, 0, 0, None) == capi.EINVAL and fin(p, 0, 16, None, 0, 0, None) == capi.EINVAL
    assert fin(p, 1, 0, None, 0, 0, None) == capi.EINVAL and fin(p, 1, 16, p, 17, 4, None) == capi.EINVAL
    assert fin(p, 1, 16, p, 4, 17, None) == capi.EINVAL and fin(p, 1, 16, p, 0, 4, None) == capi.EINVAL
    cam = L.artalk_gaga_cameras
    z = torch.zeros(16)
    assert cam(None, 3, 1, capi.ptr(z), capi.ptr(z), capi.ptr(z), None) == capi.EINVAL
    assert cam(capi.ptr(z), 3, 1, None, capi.ptr(z), capi.ptr(z), None) == capi.EINVAL
    assert cam(capi.ptr(z), 3, 1, capi.ptr(z), None, capi.ptr(z), None) == capi.EINVAL
    assert cam(capi.ptr(z), 2, 1, capi.ptr(z), capi.ptr(z), capi.ptr(z), None) == capi.EINVAL
    assert cam(capi.ptr(z), 3, -1, capi.ptr(z), capi.ptr(z), capi.ptr(z), None) == capi.EINVAL
    assert cam(capi.ptr(z), 3, 0, capi.ptr(z), capi.ptr(z), capi.ptr(z), None) == capi.OK


# ------------------------------------------------------------------------------------------------ Python surface
@pytest.fixture(scope="module")
def head():
    return gaga.GAGAvatar({"a": gc.avatar(), "b": gc.avatar(seed=3)}, su.synth_state_dict(gc.S), water_mark=gc.water_mark(),
                          image_size=gc.S, n_dynamic=gc.V, forehead_indices=gc.FOREHEAD)


def test_pack_round_trip_and_refusals(head, tmp_path):
    path = str(tmp_path / "pack.pt")
    head.save(path)
    again = gaga.GAGAvatar.load(path, forehead_indices=gc.FOREHEAD)
    assert sorted(again.all_gagavatar_id) == ["a", "b"] and again.image_size == gc.S and again.n_dynamic == gc.V
    assert torch.equal(again.all_gagavatar_id["b"]["colors"], head.all_gagavatar_id["b"]["colors"])
    assert torch.equal(again._water_mark, head._water_mark)
    pack = torch.load(path, weights_only=True)
    assert pack["format"] == "artalk-gaga-avatars/1"
    torch.save(dict(pack, format="artalk-gaga-avatars/2"), path)
    with pytest.raises(ValueError, match="format"):
        gaga.GAGAvatar.load(path)
    torch.save({k: v for k, v in pack.items() if k != "n_dynamic"}, path)
    with pytest.raises(ValueError, match="n_dynamic"):
        gaga.GAGAvatar.load(path)
    torch.save([1, 2], path)
    with pytest.raises(ValueError, match="format"):
        gaga.GAGAvatar.load(path)


def test_avatar_ids_and_constructor_refusals(head):
    with pytest.raises(KeyError):
        head.set_avatar_id("nobody.jpg")
    head.set_avatar_id("b")
    assert head._tracked_name == "b"
    sd = su.synth_state_dict(gc.S)
    few = {k: (v[:gc.V - 1] if k in gaga.AVATAR_FIELDS else v) for k, v in gc.avatar().items()}
    with pytest.raises(ValueError, match="fewer"):
        gaga.GAGAvatar({"a": few}, sd, image_size=gc.S, n_dynamic=gc.V)
    with pytest.raises(ValueError, match="lacks"):
        gaga.GAGAvatar({"a": {k: v for k, v in gc.avatar().items() if k != "scales"}}, sd, image_size=gc.S, n_dynamic=gc.V)
    with pytest.raises(ValueError, match="does not fit"):
        gaga.GAGAvatar({"a": gc.avatar()}, sd, water_mark=torch.zeros(4, 17, 4), image_size=gc.S, n_dynamic=gc.V)
    with pytest.raises(ValueError, match="twice"):
        gaga.GAGAvatar({"a": gc.avatar()}, sd, image_size=gc.S, n_dynamic=gc.V, forehead_indices=[1, 1])
    with pytest.raises(ValueError):
        gaga.GAGAvatar({"a": gc.avatar()}, sd, image_size=gc.S, n_dynamic=gc.V, forehead_indices=[gc.V])
    with pytest.raises(RuntimeError, match="Missing key"):
        gaga.GAGAvatar({"a": gc.avatar()}, {k: v for k, v in sd.items() if k != "final_linear.bias"}, image_size=gc.S, n_dynamic=gc.V)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.render_clip(gc.motion_codes(), None)
    with pytest.raises(ValueError):
        head.render_clip(torch.zeros(3, 105), None)
    with pytest.raises(RuntimeError):
        head.to("cpu")


def test_engine_wiring_without_a_device(head):
    from artalk_amd.engine import ARTAvatarInferEngine
    with pytest.raises(NotImplementedError, match="pack"):
        ARTAvatarInferEngine(load_gaga=True)
    import types
    stub = types.SimpleNamespace(cfg=None)      # an already loaded model: the constructor loads nothing
    eng = ARTAvatarInferEngine(load_gaga=True, gaga=head, gaga_flame="flame", model=stub)
    assert eng.GAGAvatar is head and eng.GAGAvatar_flame == "flame"
    with pytest.raises(KeyError):
        eng.rendering(None, torch.zeros(2, 106), shape_id="nobody.jpg")
    plain = ARTAvatarInferEngine(model=stub)
    assert plain.GAGAvatar is None
    with pytest.raises(NotImplementedError):      # nothing plugged in: as before
        plain.rendering(None, torch.zeros(2, 106), shape_id="a")
    with pytest.raises(NotImplementedError):
        plain.rendering(None, torch.zeros(2, 106))


# ------------------------------------------------------------------------------------------------ cameras
def _allowance(want64, want32):
    e32 = float(np.abs(want32.astype(np.float64) - want64).max())
    ulp = float(np.spacing(np.float32(np.abs(want64).max())))
    return max(FACTOR * e32, ulp), e32, ulp


def _lib_cameras(codes, tm):
    view, proj, cam = gaga.camera_matrices(torch.as_tensor(np.asarray(codes, dtype=np.float32)), torch.tensor(tm))
    return view.numpy(), proj.numpy(), cam.numpy()


@pytest.mark.parametrize("name", sorted(gc.CAMERA_CASES) + ["random"])
def test_cameras_against_the_float64_restatement(name):
    codes = gc.random_codes() if name == "random" else np.array([gc.CAMERA_CASES[name]], dtype=np.float32)
    before = codes.copy()
    got = _lib_cameras(codes, gc.TRANSFORM)
    assert np.array_equal(codes, before)      # the codes are not modified (the reference flips two signs in place)
    w64 = ref.cameras(codes, gc.TRANSFORM, np.float64)
    w32 = ref.cameras(codes, gc.TRANSFORM, np.float32)
    for what, g, a, b in zip(("view", "proj", "cam"), got, w64, w32):
        allow, e32, ulp = _allowance(a, b)
        err = float(np.abs(g.astype(np.float64) - a).max())
        print(f"{name} {what}: error {err:.3e}, e32 {e32:.3e}, ulp {ulp:.3e}, allowance {allow:.3e}")
        assert err <= allow, (name, what, err, allow)
    assert np.array_equal(got[2][:, :, 3], np.broadcast_to(np.asarray(gc.TRANSFORM, dtype=np.float32)[:, 3], got[2][:, :, 3].shape))


def test_zero_rotation_is_exact():
    view, proj, cam = _lib_cameras([[0.0, 0.0, 0.0]], gc.TRANSFORM)
    assert np.array_equal(cam[0, :, :3], np.diag([-1.0, 1.0, -1.0]).astype(np.float32))
    t = np.asarray(gc.TRANSFORM, dtype=np.float32)[:, 3]
    want_view = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [-t[0], -t[1], t[2], 1]], dtype=np.float32)
    assert np.array_equal(view[0], want_view)
    assert proj[0, 0, 0] == 12.0 and proj[0, 1, 1] == -12.0 and proj[0, 2, 3] == -1.0


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_quarter_turns_by_hand(axis):
    cam = _lib_cameras([gc.CAMERA_CASES[f"quarter_{axis}"]], gc.TRANSFORM)[2]
    # float32(pi / 2) misses pi / 2 by 4.4e-8: that much of cos shows up where the exact matrix holds a zero
    assert float(np.abs(cam[0, :, :3] - ref.QUARTER_TURNS[axis]).max()) <= 1e-7
    assert float(np.abs(ref.cameras([gc.CAMERA_CASES[f"quarter_{axis}"]], gc.TRANSFORM)[2][0, :, :3] - ref.QUARTER_TURNS[axis]).max()) <= 1e-7


WRONG = {"no_sign_flip": ref.Variant(flip=False), "no_transpose": ref.Variant(transpose=False), "diag_on_the_right": ref.Variant(diag_left=False),
         "initial_trans": ref.Variant(own_translation=False)}


@pytest.mark.parametrize("which", sorted(WRONG))
def test_wrong_variants_are_told_apart(which):
    codes = gc.random_codes()
    right = ref.cameras(codes, gc.TRANSFORM, np.float64)
    right32 = ref.cameras(codes, gc.TRANSFORM, np.float32)
    wrong = ref.cameras(codes, gc.TRANSFORM, np.float64, WRONG[which])
    got = _lib_cameras(codes, gc.TRANSFORM)
    for g, a, b, w in zip(got, right, right32, wrong):
        allow = _allowance(a, b)[0]
        miss = float(np.abs(w - a).max())
        print(f"{which}: the variant misses the oracle by {miss:.3e} = {miss / allow:.0f} x the allowance")
        assert miss > 100.0 * allow
        assert float(np.abs(g.astype(np.float64) - w).max()) > 100.0 * allow      # and the library is not the variant


# ------------------------------------------------------------------------------------------------ the statements the GPU tests rely on
def test_ema_and_blend_statements_agree_and_exclude_an_fma():
    g = np.random.default_rng(0)
    pts = g.standard_normal((40, 68, 3)).astype(np.float32)
    a, sa = ref.ema_numpy(pts)
    verts = torch.from_numpy(pts)
    b, sb = ref.ema_torch(verts, list(range(68)))
    assert np.array_equal(a, b.numpy()) and np.array_equal(sa, sb[0].numpy())
    c, _ = ref.ema_fma_numpy(pts)
    differ = float((a[1] != c[1]).mean())
    print(f"an FMA variant differs in {100 * differ:.0f} % of the values after one step")
    assert differ > 0.05
    img = torch.from_numpy((g.standard_normal((2, 3, 16, 16)) * 0.8 + 0.5).astype(np.float32))
    wm = gc.water_mark()
    assert np.array_equal(ref.finish_torch(img, wm).numpy(), ref.finish_numpy(img.numpy(), wm.numpy()))
    assert np.array_equal(ref.finish_torch(img).numpy(), ref.finish_numpy(img.numpy()))


def test_the_small_head_is_not_an_empty_image():
    """The condition of tests/test_gaga_gpu.py, checked here with the splat restatement: frame 0 of the small head covers at least a
    quarter of the pixels."""
    from flame_oracle import flame_forward
    from splat_ref import splat_ref
    av, m = gc.avatar(), gc.motion_codes()
    pose = torch.cat([torch.zeros(1, 3), m[:1, 103:106]], dim=1)
    verts = flame_forward(gc.flame_asset(), av["shapecode"][None], m[:1, :100], pose, scale=5.0)[0].numpy()
    means = np.concatenate([verts, av["xyz"][gc.V:].numpy()])
    view, proj, _ = _lib_cameras(m[:1, 100:103].numpy(), av["transform_matrix"].numpy())
    r = splat_ref(means, av["colors"].numpy(), av["opacities"].numpy(), av["scales"].numpy(), av["rotations"].numpy(), view[0], proj[0],
                  1.0 / 12.0, 1.0 / 12.0, gc.S, gc.S, dtype=np.float32)
    share = float((np.abs(r["image"]).max(axis=0) > 1e-3).mean())
    print(f"frame 0: {100 * share:.0f} % of the pixels are covered")
    assert share >= 0.25
