"""8-bit frames out of the GAGAvatar head, on the small head of tests/gaga_cases.py as tests/test_gaga_gpu.py's rig builds it (S = 16,
T = 5, the stored noise buffers): ``render_clip(out=f)`` - one ``artalk_gaga_render_u8`` call, the fused finish-and-pack kernel per slab,
no fp32 clip - must be byte-equal to ``pack_frames(render_clip(), f)``, whose two halves are checked elsewhere (test_gaga_gpu.py:
the float clip bit for bit; test_frames_ops_gpu.py: the pack against the integer restatement)."""
import types

import pytest
import torch

import gaga_cases as gc
from artalk_amd import capi
from artalk_amd import frames
from artalk_amd import gaga
from test_gaga_gpu import Rig

pytestmark = pytest.mark.gpu

FORMATS = ("rgb24", "yuv420p")


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    r.head.set_slab(gc.SLAB)
    r.head.reset_motion_state()
    r.float_clip = r.head.render_clip(r.codes, r.flame, randomize_noise=False)      # computed once, shared, read only
    r.want = {f: frames.pack_frames(r.float_clip, f).cpu() for f in FORMATS}
    return r


def _fresh(rig, slab=gc.SLAB):
    rig.head.set_slab(slab)
    rig.head.set_avatar_id("a")
    rig.head.reset_motion_state()
    return rig.head


def test_the_clip_is_not_flat(rig):
    for f in FORMATS:
        assert tuple(rig.want[f].shape) == frames.frame_shape(f, gc.T_CLIP, gc.S, gc.S) and rig.want[f].dtype == torch.uint8
        assert float(rig.want[f].float().std()) > 5.0
    assert int(rig.want["rgb24"].max()) > 200 and int(rig.want["yuv420p"][:, :gc.S].min()) >= 16


@pytest.mark.parametrize("slab", (1, gc.SLAB, 3, 0))      # T = 5 in slabs of 1; 2, 2, 1; 3, 2; and one (the default)
@pytest.mark.parametrize("fmt", FORMATS)
def test_render_clip_out_equals_render_then_pack(rig, fmt, slab):
    head = _fresh(rig, slab)
    got = head.render_clip(rig.codes, rig.flame, randomize_noise=False, out=fmt)
    assert head.slab_in_force() == slab if slab else head.slab_in_force() >= gc.T_CLIP
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == rig.want[fmt].shape
    assert torch.equal(got.cpu(), rig.want[fmt])


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_copy_equals_the_device_result(rig, fmt):
    head = _fresh(rig)
    got = head.render_clip(rig.codes, rig.flame, randomize_noise=False, out=fmt, host=True)      # three slabs, three copies
    assert not got.is_cuda and got.is_pinned() and got.dtype == torch.uint8
    assert torch.equal(got, rig.want[fmt])
    dev = _fresh(rig).render_clip(rig.codes, rig.flame, randomize_noise=False, out=fmt)
    assert torch.equal(got, dev.cpu())
    again = _fresh(rig, 1).render_clip(rig.codes, rig.flame, randomize_noise=False, out=fmt, host=True)      # five copies
    assert torch.equal(again, got)


def test_the_ema_advances_alike_in_a_float_and_an_8_bit_head(rig):
    a = _fresh(rig)
    b = gaga.GAGAvatar(rig.avatars, rig.unet, water_mark=rig.mark, image_size=gc.S, n_dynamic=gc.V, forehead_indices=gc.FOREHEAD)
    b.set_slab(3)
    b.set_avatar_id("a")
    clips = (rig.codes, rig.codes[1:4])
    floats = [a.render_clip(m, rig.flame, randomize_noise=False) for m in clips]
    assert not torch.equal(floats[0][1:4], floats[1]), "the EMA state did not carry over to the second clip"
    for i, (m, fmt) in enumerate(zip(clips, FORMATS)):
        got = b.render_clip(m, rig.flame, randomize_noise=False, out=fmt)
        assert torch.equal(got, frames.pack_frames(floats[i], fmt)), f"clip {i} ({fmt}) differs"
    # and on from there, the other way round: the 8-bit head's state feeds a float clip
    assert torch.equal(b.render_clip(rig.codes[:2], rig.flame, randomize_noise=False).view(torch.int32),
                       a.render_clip(rig.codes[:2], rig.flame, randomize_noise=False).view(torch.int32))
    b._release()


@pytest.mark.parametrize("fmt", FORMATS)
def test_an_empty_clip(rig, fmt):
    head = _fresh(rig)
    got = head.render_clip(rig.codes[:0], rig.flame, out=fmt)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == frames.frame_shape(fmt, 0, gc.S, gc.S)
    host = head.render_clip(rig.codes[:0], rig.flame, out=fmt, host=True)
    assert not host.is_cuda and host.dtype == torch.uint8 and tuple(host.shape) == frames.frame_shape(fmt, 0, gc.S, gc.S)


def test_two_step_form_passes_out_through(rig):
    head = _fresh(rig)
    batch = head.build_forward_batch(rig.codes, rig.flame)
    assert torch.equal(head.forward_expression(batch, randomize_noise=False, out="yuv420p").cpu(), rig.want["yuv420p"])


def test_explicit_noise_reaches_the_8_bit_path(rig):
    from artalk_amd import styleunet as su
    g = torch.Generator(device="cuda").manual_seed(4)
    noise = [torch.randn(gc.T_CLIP, 1, su.noise_resolution(i), su.noise_resolution(i), device="cuda", generator=g)
             for i in range(su.num_noise_layers(gc.S))]
    want = frames.pack_frames(_fresh(rig).render_clip(rig.codes, rig.flame, noise=noise), "rgb24")
    got = _fresh(rig, 3).render_clip(rig.codes, rig.flame, noise=noise, out="rgb24")      # the slab's slice of a per-frame noise
    assert torch.equal(got, want) and not torch.equal(got.cpu(), rig.want["rgb24"])


def test_engine_rendering_head_branch(rig):
    from artalk_amd.engine import ARTAvatarInferEngine
    eng = ARTAvatarInferEngine(load_gaga=True, gaga=rig.head, gaga_flame=rig.flame, model=types.SimpleNamespace(cfg=None))
    for fmt in FORMATS:
        torch.manual_seed(8)
        _fresh(rig)
        got = eng.rendering(None, rig.codes, shape_id="a", output=fmt)
        torch.manual_seed(8)
        _fresh(rig)
        want = frames.pack_frames(eng.rendering(None, rig.codes, shape_id="a"), fmt)
        assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got, want)
    with pytest.raises(ValueError, match="unknown frame format"):
        eng.rendering(None, rig.codes, shape_id="a", output="nv12")


def test_engine_rendering_mesh_branch():
    from artalk_amd.engine import ARTAvatarInferEngine
    from artalk_amd.flame import FLAMEModel, synthetic_flame_asset
    from artalk_amd.render import RenderMesh
    from conftest import get_gpu_model
    eng = ARTAvatarInferEngine.__new__(ARTAvatarInferEngine)
    eng.ARTalk, eng.device, eng.style_motion, eng.clip_length, eng.fix_pose = get_gpu_model("tiny"), "cuda", None, 40, False
    eng.flame_model = FLAMEModel(n_shape=300, n_exp=100, scale=1.0, no_lmks=True, flame_ckpt=synthetic_flame_asset())
    eng.mesh_renderer = RenderMesh(32, faces=eng.flame_model.get_faces(), scale=1.0)
    pred = gc.motion_codes(T=3).cuda()
    audio = torch.zeros(1)
    images = eng.rendering(audio, pred)
    assert images.shape == (3, 3, 32, 32) and float(images.std()) > 0.01
    for fmt in FORMATS:
        got = eng.rendering(audio, pred, output=fmt)
        assert got.dtype == torch.uint8 and tuple(got.shape) == frames.frame_shape(fmt, 3, 32, 32)
        assert torch.equal(got, frames.pack_frames(images, fmt))
    eng.mesh_renderer = None
    with pytest.raises(ValueError, match="mesh_renderer"):
        eng.rendering(audio, pred, output="rgb24")


def test_refusals_on_a_real_object(rig):
    L = capi.lib()
    head = _fresh(rig)
    with pytest.raises(ValueError, match="unknown frame format"):
        head.render_clip(rig.codes, rig.flame, out="nv12")
    with pytest.raises(ValueError, match="host=True"):
        head.render_clip(rig.codes, rig.flame, out="float", host=True)
    with pytest.raises(ValueError, match="host=True"):
        head.render_clip(rig.codes, rig.flame, host=True)
    head.render_clip(rig.codes[:1], rig.flame, randomize_noise=False)      # the library object exists
    h, p, s = head._h, capi.ptr, capi.current_stream_ptr()
    out = torch.empty(1, gc.S, gc.S, 3, dtype=torch.uint8, device="cuda")
    for fmt in (0, 3, -1):
        assert L.artalk_gaga_render_u8(h, p(rig.codes), 106, 1, None, None, 1, fmt, p(out), None, s) == capi.EINVAL
        assert b"unknown frame format" in L.artalk_gaga_last_error(h)
    assert L.artalk_gaga_render_u8(h, p(rig.codes), 106, 1, None, None, 1, capi.FRAMES_RGB24, None, None, s) == capi.EINVAL
    assert L.artalk_gaga_render_u8(h, None, 106, 1, None, None, 1, capi.FRAMES_RGB24, p(out), None, s) == capi.EINVAL
    assert L.artalk_gaga_render_u8(h, p(rig.codes), 106, -1, None, None, 1, capi.FRAMES_RGB24, p(out), None, s) == capi.EINVAL
    assert L.artalk_gaga_render_u8(h, p(rig.codes), 105, 1, None, None, 1, capi.FRAMES_YUV420P, p(out), None, s) == capi.EINVAL
    # none of the refused calls changed the object
    head.reset_motion_state()
    assert torch.equal(head.render_clip(rig.codes, rig.flame, randomize_noise=False, out="rgb24").cpu(), rig.want["rgb24"])
