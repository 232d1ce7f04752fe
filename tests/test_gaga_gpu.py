"""The GAGAvatar head end to end on the small head of tests/gaga_cases.py (S = 16, 64 vertices, 136 Gaussians, 8 forehead vertices, a
5 x 8 watermark, T = 5 in slabs of 2, 2 and 1): one ``render_clip`` call against the chain of the project's own public pieces -
FLAMEModel -> the torch float32 EMA -> cameras -> the splat rasteriser -> StyleUNet.forward -> torch clamp / blend.  Each piece is
checked against its own oracle elsewhere (tests/test_flame.py, test_splat_gpu.py, test_styleunet_gpu.py, test_gaga_cpu.py,
test_gaga_ops_gpu.py) and each is bit-identical for any split of the frames, so the comparison here is exact: bit for bit."""
import ctypes as C
import json
import os
import types

import pytest
import torch

import gaga_cases as gc
import gaga_ref as ref
from artalk_amd import capi
from artalk_amd import gaga
from artalk_amd import splat
from artalk_amd import styleunet as su
from artalk_amd.flame import FLAMEModel

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Rig:
    def __init__(self):
        self.flame = FLAMEModel(300, 100, scale=5.0, no_lmks=True, flame_ckpt=gc.flame_asset())
        self.sd = su.synth_state_dict(gc.S)
        self.unet = su.StyleUNet(gc.S, gc.S, 32, 3)
        self.unet.load_state_dict(self.sd)
        self.unet.to("cuda")
        self.avatars = {"a": gc.avatar(), "b": gc.avatar(seed=3)}
        self.mark = gc.water_mark()
        self.head = gaga.GAGAvatar(self.avatars, self.sd, water_mark=self.mark, image_size=gc.S, n_dynamic=gc.V,
                                   forehead_indices=gc.FOREHEAD)
        self.head.set_slab(gc.SLAB)
        self.head.set_avatar_id("a")
        self.codes = gc.motion_codes().cuda()
        self.splat_images = None

    def chain(self, codes, state=None, noise=None, avatar="a"):
        """-> (frames (T, 3, S, S) on the CPU, EMA state (1, K, 3)) through separate public calls."""
        av = self.avatars[avatar]
        T = codes.shape[0]
        pose = torch.cat([torch.zeros(T, 3, device="cuda"), codes[:, 103:106]], dim=1)
        verts = self.flame(shape_params=av["shapecode"][None].expand(T, -1), expression_params=codes[:, :100], pose_params=pose)
        verts, state = ref.ema_torch(verts.cpu(), gc.FOREHEAD, state)
        means = torch.cat([verts.cuda(), av["xyz"][gc.V:].cuda()[None].expand(T, -1, -1)], dim=1)
        view, proj, _ = gaga.camera_matrices(codes[:, 100:103].cpu(), av["transform_matrix"])
        attr = splat._device_attr
        images, _ = splat._render(T, gc.S, gc.S, attr(means, "xyz", (3,), T), attr(av["colors"].cuda()[None], "colors", (32,), T),
                                  attr(av["opacities"].cuda()[None], "opacities", (), T), attr(av["scales"].cuda()[None], "scales", (3,), T),
                                  attr(av["rotations"].cuda()[None], "rotations", (4,), T), view.contiguous(), proj.contiguous(),
                                  1.0 / 12.0, 1.0 / 12.0, 1.0, None)
        self.splat_images = images
        rgb = self.unet(images, randomize_noise=False, noise=noise)
        return ref.finish_torch(rgb.cpu(), self.mark), state


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    r.want, r.want_state = r.chain(r.codes)      # computed once, shared, read only
    r.share = float((r.splat_images.abs().amax(dim=1) > 1e-3).float().mean())
    return r


def _fresh(rig, slab=gc.SLAB, avatar="a"):
    rig.head.set_slab(slab)
    rig.head.set_avatar_id(avatar)
    rig.head.reset_motion_state()
    return rig.head


def test_the_chain_is_not_an_empty_image(rig):
    print(f"the chain's splat image covers {100 * rig.share:.0f} % of the pixels")
    assert rig.share >= 0.25
    assert float(rig.want.std()) > 0.01 and 0.0 <= float(rig.want.min()) and float(rig.want.max()) <= 1.0
    assert not torch.equal(rig.want_state[0], rig.chain(rig.codes[:1])[1][0])      # the EMA moved the forehead after frame 0


def test_render_clip_equals_the_chain(rig):
    head = _fresh(rig)
    before = rig.codes.clone()
    got = head.render_clip(rig.codes, rig.flame, randomize_noise=False)
    assert head.slab_in_force() == gc.SLAB
    assert got.shape == (gc.T_CLIP, 3, gc.S, gc.S) and got.is_cuda
    assert torch.equal(_bits(got), _bits(rig.want))
    assert torch.equal(_bits(rig.codes), _bits(before)), "motion_codes was modified"


def test_explicit_noise_equals_the_chain(rig):
    g = torch.Generator(device="cuda").manual_seed(4)
    noise = [torch.randn(gc.T_CLIP, 1, su.noise_resolution(i), su.noise_resolution(i), device="cuda", generator=g)
             for i in range(su.num_noise_layers(gc.S))]
    want, _ = rig.chain(rig.codes, noise=noise)
    got = _fresh(rig).render_clip(rig.codes, rig.flame, noise=noise)
    assert torch.equal(_bits(got), _bits(want))
    assert not torch.equal(_bits(got), _bits(rig.want))      # the noise is live
    shared = [n[:1] for n in noise]
    assert torch.equal(_bits(_fresh(rig).render_clip(rig.codes, rig.flame, noise=shared)), _bits(rig.chain(rig.codes, noise=shared)[0]))


def test_randomize_noise_draws_once_per_slab(rig):
    head = _fresh(rig)
    torch.manual_seed(21)
    got = head.render_clip(rig.codes, rig.flame, randomize_noise=True)
    torch.manual_seed(21)
    parts = [[torch.empty(n, 1, su.noise_resolution(i), su.noise_resolution(i), device="cuda").normal_() for i in range(su.num_noise_layers(gc.S))]
             for n in (2, 2, 1)]
    noise = [torch.cat([p[i] for p in parts]) for i in range(su.num_noise_layers(gc.S))]
    assert torch.equal(_bits(got), _bits(rig.chain(rig.codes, noise=noise)[0]))
    assert 0.0 <= float(got.min()) and float(got.max()) <= 1.0


@pytest.mark.parametrize("slab", (1, 5))
def test_slab_sizes_give_the_same_bits(rig, slab):
    got = _fresh(rig, slab).render_clip(rig.codes, rig.flame, randomize_noise=False)
    assert rig.head.slab_in_force() == slab
    assert torch.equal(_bits(got), _bits(rig.want))


def test_the_ema_carries_over_calls_and_resets(rig):
    head = _fresh(rig)
    first = head.render_clip(rig.codes, rig.flame, randomize_noise=False)
    second = head.render_clip(rig.codes, rig.flame, randomize_noise=False)      # continues from the first call's state
    want_second, _ = rig.chain(rig.codes, state=rig.want_state)
    assert torch.equal(_bits(first), _bits(rig.want)) and torch.equal(_bits(second), _bits(want_second))
    assert not torch.equal(_bits(second), _bits(first))
    head.reset_motion_state()
    parts = torch.cat([head.render_clip(rig.codes[:2], rig.flame, randomize_noise=False),
                       head.render_clip(rig.codes[2:], rig.flame, randomize_noise=False)])
    assert torch.equal(_bits(parts), _bits(rig.want)), "2 + 3 frames differ from 5"
    head.reset_motion_state()
    assert torch.equal(_bits(head.render_clip(rig.codes, rig.flame, randomize_noise=False)), _bits(rig.want)), "reset did not restart the EMA"


def test_set_avatar_id_keeps_the_ema(rig):
    head = _fresh(rig)
    head.render_clip(rig.codes[:2], rig.flame, randomize_noise=False)
    head.set_avatar_id("b")
    got = head.render_clip(rig.codes[2:], rig.flame, randomize_noise=False)
    _, state = rig.chain(rig.codes[:2])
    want, _ = rig.chain(rig.codes[2:], state=state, avatar="b")
    assert torch.equal(_bits(got), _bits(want))
    assert not torch.equal(_bits(got), _bits(rig.chain(rig.codes[2:], avatar="b")[0])), "the state was reset"
    with pytest.raises(KeyError):
        head.set_avatar_id("nobody.jpg")


def test_two_step_form_and_empty_clip(rig):
    head = _fresh(rig)
    batch = head.build_forward_batch(rig.codes, rig.flame)
    assert batch["t_transform"].shape == (gc.T_CLIP, 3, 4)
    assert torch.equal(_bits(head.forward_expression(batch, randomize_noise=False)), _bits(rig.want))
    assert head.render_clip(rig.codes[:0], rig.flame).shape == (0, 3, gc.S, gc.S)
    wide = torch.zeros(gc.T_CLIP, 120, device="cuda")      # a row stride above 106
    wide[:, :106] = rig.codes
    head.reset_motion_state()
    assert torch.equal(_bits(head.render_clip(wide[:, :106], rig.flame, randomize_noise=False)), _bits(rig.want))


def test_engine_rendering(rig):
    from artalk_amd.engine import ARTAvatarInferEngine
    eng = ARTAvatarInferEngine(load_gaga=True, gaga=rig.head, gaga_flame=rig.flame, model=types.SimpleNamespace(cfg=None))
    _fresh(rig)
    got = eng.rendering(None, rig.codes, shape_id="a")
    assert got.shape == (gc.T_CLIP, 3, 16, 16) and 0.0 <= float(got.min()) and float(got.max()) <= 1.0
    torch.manual_seed(8)
    _fresh(rig)
    a = eng.rendering(None, rig.codes, shape_id="a")
    torch.manual_seed(8)
    _fresh(rig)
    assert torch.equal(_bits(a), _bits(rig.head.render_clip(rig.codes, rig.flame)))
    later = ARTAvatarInferEngine(model=types.SimpleNamespace(cfg=None))
    later.GAGAvatar, later.GAGAvatar_flame = rig.head, rig.flame      # plugged in afterwards, like flame_model
    assert later.rendering(None, rig.codes, shape_id="b").shape == (gc.T_CLIP, 3, 16, 16)


def test_refusals_on_a_real_object(rig):
    L = capi.lib()
    head = _fresh(rig)
    head.render_clip(rig.codes[:1], rig.flame, randomize_noise=False)      # the library object exists
    h, av = head._h, rig.avatars["a"]
    p = lambda t: capi.ptr(t)
    short = (h, gc.V - 1, p(av["xyz"]), p(av["colors"]), p(av["opacities"]), p(av["scales"]), p(av["rotations"]), p(av["shapecode"]),
             p(av["transform_matrix"]))
    assert L.artalk_gaga_set_avatar(*short) == capi.EINVAL and b"at least V" in L.artalk_gaga_last_error(h)
    for idx in ((1, gc.V), (2, 2), (-1,)):
        arr = (C.c_int32 * len(idx))(*idx)
        assert L.artalk_gaga_set_forehead(h, arr, len(idx)) == capi.EINVAL
    wm = torch.zeros(4, 17, 4)
    assert L.artalk_gaga_set_watermark(h, p(wm), 17, 4) == capi.EINVAL and b"does not fit" in L.artalk_gaga_last_error(h)
    out = torch.empty(1, 3, gc.S, gc.S, device="cuda")
    s = capi.current_stream_ptr()
    assert L.artalk_gaga_render(h, p(rig.codes), 106, -1, None, None, 1, p(out), s) == capi.EINVAL
    assert L.artalk_gaga_render(h, p(rig.codes), 105, 1, None, None, 1, p(out), s) == capi.EINVAL
    assert L.artalk_gaga_render(h, None, 106, 1, None, None, 1, p(out), s) == capi.EINVAL
    assert L.artalk_gaga_render(h, p(rig.codes), 106, 1, None, None, 1, None, s) == capi.EINVAL
    assert L.artalk_gaga_set_slab(h, 65) == capi.EINVAL and L.artalk_gaga_set_slab(h, -1) == capi.EINVAL
    # none of the refused calls changed the object
    head.reset_motion_state()
    assert torch.equal(_bits(head.render_clip(rig.codes, rig.flame, randomize_noise=False)), _bits(rig.want))
    # a second object on the same borrowed handles: no avatar yet, then an upsampler that was never finalized
    sp = splat._handle(torch.device("cuda", 0))
    g2 = C.c_void_p()
    assert L.artalk_gaga_create(0, rig.flame._h, sp, rig.unet._h, gc.V, 400, gc.S, C.byref(g2)) == capi.OK
    try:
        assert L.artalk_gaga_render(g2, p(rig.codes), 106, 1, None, None, 1, p(out), s) == capi.EINVAL
        assert b"no avatar" in L.artalk_gaga_last_error(g2)
        assert L.artalk_gaga_render(g2, p(rig.codes), 106, 0, None, None, 1, p(out), s) == capi.EINVAL      # refused before T == 0 is looked at
    finally:
        L.artalk_gaga_destroy(g2)
    for bad in ((gc.V + 1, 400, gc.S), (gc.V, 300, gc.S), (gc.V, 400, 32)):
        assert L.artalk_gaga_create(0, rig.flame._h, sp, rig.unet._h, *bad, C.byref(g2)) == capi.EINVAL
    raw = C.c_void_p()
    assert L.artalk_styleunet_create(0, 32, 3, gc.S, C.byref(raw)) == capi.OK
    try:
        assert L.artalk_gaga_create(0, rig.flame._h, sp, raw, gc.V, 400, gc.S, C.byref(g2)) == capi.OK
        try:
            full = (g2, gc.N) + short[2:]
            assert L.artalk_gaga_set_avatar(*full) == capi.OK
            assert L.artalk_gaga_render(g2, p(rig.codes), 106, 1, None, None, 1, p(out), s) == capi.ESTATE
            assert b"not finalized" in L.artalk_gaga_last_error(g2)
        finally:
            L.artalk_gaga_destroy(g2)
    finally:
        L.artalk_styleunet_destroy(raw)


def test_default_forehead_is_the_reference_list(rig):
    """On a mesh with more than 3913 vertices the library smooths the reference's 68 vertices unless told otherwise
    (tests/golden/gaga_forehead_indices.json holds the list): same bits as the explicit list, other bits than no list."""
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaga_forehead_indices.json")))["forehead_indices"]
    assert len(want) == 68 and len(set(want)) == 68 and max(want) == 3913
    from artalk_amd.flame import synthetic_flame_asset
    V = 5023
    flame = FLAMEModel(300, 100, scale=5.0, no_lmks=True, flame_ckpt=synthetic_flame_asset())
    small = rig.avatars["a"]
    g = torch.Generator().manual_seed(6)
    pick = torch.randint(0, gc.N, (V,), generator=g)
    av = {k: (small[k][pick] if k in gaga.AVATAR_FIELDS else small[k]) for k in small}
    codes = gc.motion_codes(T=3).cuda()
    outs = {}
    for name, idx in (("default", None), ("explicit", want), ("none", [])):
        head = gaga.GAGAvatar({"a": av}, rig.unet, image_size=gc.S, n_dynamic=V, forehead_indices=idx)
        outs[name] = head.render_clip(codes, flame, randomize_noise=False)
    assert torch.equal(_bits(outs["default"]), _bits(outs["explicit"]))
    assert not torch.equal(_bits(outs["default"]), _bits(outs["none"]))
    assert torch.equal(_bits(outs["default"][0]), _bits(outs["none"][0]))      # the very first frame is left as it is
