"""The avatar-head objects keep their device memory across calls (csrc/device_mem.h): an object that has grown, shrunk and been used
again must give the bits a fresh object gives.  For artalk_flame, artalk_splat and artalk_gaga, on the smallest entries of the case
tables: one long-lived object is called at size a, at b > a (a regrow), then at a again, and every output word of each call is compared
with a fresh object's output for the same input.  The splat and gaga objects repeat one call with stage timing on: the same bits, and
stage sums that are finite, non-negative and positive for every stage that ran."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import flame_cases as fc
import gaga_cases as gc
from artalk_amd import capi
from artalk_amd import gaga
from artalk_amd import splat
from artalk_amd import styleunet as su
from artalk_amd.flame import FLAMEModel
from splat_cases import case, case_refs
from test_splat_gpu import _abi

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _dirty_device_memory():
    """Hand the runtime a block full of NaNs back, so that a scratch buffer that is not zeroed where it must be has a chance to show."""
    junk = torch.full((16 << 20,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    del junk
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------- artalk_flame
def test_flame_regrown_scratch_gives_a_fresh_objects_bits():
    """V = 4, NB = 400: K is padded to 416 and the 16 padding columns of the betas operand are never written - they read zero because
    the scratch is zero-filled, which the regrow from 2 to 5 frames must do again.  T goes 2, 5, 2."""
    c = fc.BY_NAME["V4-T5"]
    assert (c.n_shape + c.n_exp) % 32 != 0 and c.D == 5
    x = fc.make_inputs(c)

    def call(fm, rows):
        fm.neck_pose = x.neck[rows]
        out = fm(shape_params=x.shape[rows], expression_params=x.exp[rows], pose_params=x.pose[rows], eye_pose_params=x.eyes[rows])
        torch.cuda.synchronize()
        return _bits(out)

    def model():
        return FLAMEModel(n_shape=c.n_shape, n_exp=c.n_exp, scale=c.scale, no_lmks=True, flame_ckpt=fc.asset(c.V))

    steps = (slice(0, 2), slice(0, 5), slice(3, 5))
    want = [call(model(), rows) for rows in steps]
    assert not torch.equal(want[0], want[2])
    live = model()
    for rows, w in zip(steps, want):
        _dirty_device_memory()
        got = call(live, rows)
        assert torch.isfinite(got.view(torch.float32)).all()
        assert torch.equal(got, w), f"frames {rows}: the long-lived object differs from a fresh one"


# ---------------------------------------------------------------------------------------------------------------------- artalk_splat
def _pairs(name):
    """(tile, Gaussian) pairs of a case's frame, from the oracle's tile rectangles (tests/splat_ref.py, on the CPU)"""
    rect = case_refs(name)[0]["rect"]
    return int(((rect[:, 1] - rect[:, 0]) * (rect[:, 3] - rect[:, 2])).sum())


def _splat_timing(h):
    L = capi.lib()
    st, pairs, frames = (C.c_double * 6)(), C.c_longlong(), C.c_int()
    assert L.artalk_splat_get_timing(h, st, 6, C.byref(pairs), C.byref(frames)) == 6
    return list(st), pairs.value, frames.value


def test_splat_regrown_buffers_give_a_fresh_objects_bits():
    """n1 (1 Gaussian), then n257 (257: a second workgroup, and far more than 1.25 x the pairs, so the key buffers outgrow their slack),
    then n1 again, all 40 x 56."""
    a, b = "n1", "n257"
    pa, pb = _pairs(a), _pairs(b)
    print(f"pairs per frame: {a} {pa}, {b} {pb}")
    assert pa >= 1 and pb > 1.25 * pa
    steps = (a, b, a)
    want = [_abi([case(n)])[:2] for n in steps]
    L = capi.lib()
    h = C.c_void_p()
    assert L.artalk_splat_create(0, C.byref(h)) == capi.OK
    try:
        for n, (img, radii) in zip(steps, want):
            got_img, got_radii, _, _ = _abi([case(n)], h=h)
            assert np.array_equal(got_img.view(np.int32), img.view(np.int32)) and np.array_equal(got_radii, radii), n
            st, pairs, frames = _splat_timing(h)
            assert pairs == _pairs(n) and frames == 1 and st == [0.0] * 6      # timing is off
        assert L.artalk_splat_set_timing(h, 1) == capi.OK
        got_img, got_radii, _, _ = _abi([case(b)], h=h)
        assert np.array_equal(got_img.view(np.int32), want[1][0].view(np.int32)) and np.array_equal(got_radii, want[1][1])
        st, pairs, _ = _splat_timing(h)
        print("splat stage ms:", ["%.4f" % v for v in st])
        assert pairs == pb and all(math.isfinite(v) and v > 0.0 for v in st)      # N > 0 and pairs > 0: all six stages ran
        assert L.artalk_splat_set_timing(h, 0) == capi.OK
    finally:
        L.artalk_splat_destroy(h)


# ----------------------------------------------------------------------------------------------------------------------- artalk_gaga
def _big_avatar():
    """gaga_cases.avatar with 40 more static Gaussians, inside the image"""
    av = gc.avatar(seed=3, n=gc.N + 40)
    av["xyz"][gc.N:] = av["xyz"][gc.V:gc.V + 40] + 0.05
    return av


def test_gaga_regrown_scratch_gives_a_fresh_objects_bits():
    """T goes 2, 5, 2 and N 136, 176, 136 (set_avatar with more Gaussians), and the watermark is replaced before every call.  The fresh
    objects come first, each on fresh FLAME and splat objects; then one head, its FLAME model and its rasteriser live through all three."""
    L = capi.lib()
    sd = su.synth_state_dict(gc.S)
    unet = su.StyleUNet(gc.S, gc.S, 32, 3)
    unet.load_state_dict(sd)
    unet.to("cuda")
    avatars = {"a": gc.avatar(), "big": _big_avatar()}
    marks = {"m1": gc.water_mark(), "m2": gc.water_mark(h=7, w=16, seed=6)}
    codes = gc.motion_codes().cuda()
    steps = (("a", "m1", codes[:2]), ("big", "m2", codes), ("a", "m1", codes[3:]))

    def flame():
        return FLAMEModel(300, 100, scale=5.0, no_lmks=True, flame_ckpt=gc.flame_asset())

    def head_for(mark):
        head = gaga.GAGAvatar(avatars, unet, water_mark=marks[mark], image_size=gc.S, n_dynamic=gc.V, forehead_indices=gc.FOREHEAD)
        head.set_slab(0)
        return head

    want = []
    for av, mark, m in steps:
        splat.release()
        head = head_for(mark)
        head.set_avatar_id(av)
        want.append(_bits(head.render_clip(m, flame(), randomize_noise=False)))
        head._release()
    assert not torch.equal(want[0], want[2])

    splat.release()
    live, fm = head_for("m1"), flame()
    for (av, mark, m), w in zip(steps, want):
        live.set_avatar_id(av)
        if live._h is not None:
            wm = marks[mark]
            assert L.artalk_gaga_set_watermark(live._h, capi.ptr(wm), int(wm.shape[1]), int(wm.shape[2])) == capi.OK
        live.reset_motion_state()      # a fresh object starts without an EMA state
        h_before = live._h.value if live._h is not None else None
        _dirty_device_memory()
        got = _bits(live.render_clip(m, fm, randomize_noise=False))
        assert h_before is None or live._h.value == h_before, "the library object was replaced"
        assert torch.equal(got, w), f"avatar {av}, T = {m.shape[0]}: the long-lived head differs from a fresh one"
    # the second call again, with stage timing on
    av, mark, m = steps[1]
    live.set_avatar_id(av)
    assert L.artalk_gaga_set_watermark(live._h, capi.ptr(marks[mark]), 7, 16) == capi.OK
    live.reset_motion_state()
    assert L.artalk_gaga_set_timing(live._h, 1) == capi.OK
    got = _bits(live.render_clip(m, fm, randomize_noise=False))
    st = (C.c_double * 5)()
    assert L.artalk_gaga_get_timing(live._h, st, 5) == 5
    assert L.artalk_gaga_set_timing(live._h, 0) == capi.OK
    print("gaga stage ms:", ["%.4f" % v for v in st])
    assert torch.equal(got, want[1])
    assert all(math.isfinite(v) and v > 0.0 for v in st)      # one slab, forehead indices set: all five stages ran
    live._release()
