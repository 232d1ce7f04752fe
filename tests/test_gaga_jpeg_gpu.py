"""JPEG out of the GAGAvatar head and the engine, on the small head of tests/gaga_cases.py as tests/test_gaga_gpu.py's rig builds it (S = 16,
T = 5): ``out="jpeg"`` renders in pieces of the slab in force and encodes each piece on the device, and must be byte-equal to
``encode_jpeg`` of the ``out="rgb24"`` frames of the unsplit call, whose two halves are checked elsewhere (test_gaga_frames_gpu.py: the
rgb24 frames; test_jpeg_ops_gpu.py: the encoder against the numpy restatement)."""
import types

import pytest
import torch

import gaga_cases as gc
import jpeg_ref
from artalk_amd import frames
from artalk_amd import gaga
from artalk_amd import styleunet as su
from test_gaga_gpu import Rig

pytestmark = pytest.mark.gpu

JPEG = dict(quality=90, subsampling="444")


def _noise(T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(T, 1, su.noise_resolution(i), su.noise_resolution(i), device="cuda", generator=g) for i in range(su.num_noise_layers(gc.S))]


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    r.noise = _noise(gc.T_CLIP, 4)
    r.head.reset_motion_state()
    r.rgb = r.head.render_clip(r.codes, r.flame, noise=r.noise, out="rgb24")      # computed once, shared, read only
    r.next_rgb = r.head.render_clip(r.codes[:2], r.flame, randomize_noise=False, out="rgb24")      # what follows the clip: shows the EMA state
    r.want = frames.split_jpeg(*frames.encode_jpeg(r.rgb, **JPEG))
    return r


def _fresh(rig, slab=gc.SLAB):
    rig.head.set_slab(slab)
    rig.head.set_avatar_id("a")
    rig.head.reset_motion_state()
    return rig.head


def test_the_streams_are_the_restatements(rig):
    assert rig.want == [jpeg_ref.encode(x, 90, "444") for x in rig.rgb.cpu().numpy()]
    assert len(set(rig.want)) == gc.T_CLIP and float(rig.rgb.float().std()) > 5.0


@pytest.mark.parametrize("host", (False, True))
@pytest.mark.parametrize("slab", (1, gc.SLAB, 3, 0))      # T = 5 in pieces of 1; 2, 2, 1; 3, 2; and one (the default)
def test_render_clip_jpeg_equals_render_then_encode(rig, slab, host):
    head = _fresh(rig, slab)
    data, sizes = head.render_clip(rig.codes, rig.flame, noise=rig.noise, out="jpeg", jpeg=JPEG, host=host)
    assert data.dtype == torch.uint8 and sizes.dtype == torch.int64
    assert tuple(data.shape) == (gc.T_CLIP, frames.jpeg_default_cap(gc.S, gc.S)) and tuple(sizes.shape) == (gc.T_CLIP,)
    assert (data.is_pinned() and sizes.is_pinned() and not data.is_cuda) if host else (data.is_cuda and sizes.is_cuda)
    assert frames.split_jpeg(data, sizes) == rig.want
    # the EMA state afterwards is the unsplit call's: the frames that follow are the same
    assert torch.equal(head.render_clip(rig.codes[:2], rig.flame, randomize_noise=False, out="rgb24"), rig.next_rgb)


def test_render_clip_jpeg_options_and_refusals(rig):
    head = _fresh(rig)
    data, sizes = head.render_clip(rig.codes[:2], rig.flame, noise=[n[:2] for n in rig.noise], out="jpeg", jpeg=dict(cap=4000))
    assert tuple(data.shape) == (2, 4000)
    assert frames.split_jpeg(data, sizes) == frames.split_jpeg(*frames.encode_jpeg(rig.rgb[:2]))      # quality 90, 4:2:0: the defaults
    data, sizes = _fresh(rig).render_clip(rig.codes[:0], rig.flame, out="jpeg")
    assert tuple(data.shape) == (0, frames.jpeg_default_cap(gc.S, gc.S)) and tuple(sizes.shape) == (0,)
    for bad in (dict(quality=0), dict(subsampling="422"), dict(cap=100), dict(colour=1)):
        with pytest.raises(ValueError):
            head.render_clip(rig.codes, rig.flame, out="jpeg", jpeg=bad)
    with pytest.raises(ValueError, match="jpeg= goes with"):
        head.render_clip(rig.codes, rig.flame, out="rgb24", jpeg=JPEG)
    with pytest.raises(ValueError, match="unknown frame format"):
        frames.format_code("jpeg")


AVATAR_OF = ("a", "b", "a")
COUNTS = (2, 2, 1)      # three interleaved streams, time-major 00 10 20 01 11: the second piece of 2 is (20, 01), a round cut in half


@pytest.mark.parametrize("host", (False, True))
@pytest.mark.parametrize("order", ("time", "stream"))
def test_render_streams_jpeg_equals_the_rgb24_call(rig, order, host):
    codes = gc.motion_codes(T=3 * 4, seed=31).reshape(3, 4, 106).cuda()
    noise = _noise(sum(COUNTS), 9)
    results = {}
    for out in ("rgb24", "jpeg"):
        head = gaga.GAGAvatar(rig.avatars, rig.unet, water_mark=rig.mark, image_size=gc.S, n_dynamic=gc.V, forehead_indices=gc.FOREHEAD)
        head.set_slab(2)
        streams = [head.open_stream(a) for a in AVATAR_OF]
        kw = dict(jpeg=JPEG, host=host) if out == "jpeg" else {}
        results[out] = head.render_streams(streams, codes, rig.flame, counts=COUNTS, order=order, noise=noise, out=out, **kw)
        # the streams' EMA states afterwards: the frames that follow
        results[out + " next"] = head.render_streams(streams, codes, rig.flame, counts=(1, 1, 1), firsts=(2, 2, 1), randomize_noise=False, out="rgb24")[0]
    (data, sizes), index = results["jpeg"]
    rgb, rgb_index = results["rgb24"]
    assert torch.equal(index, rgb_index) and index.tolist() == [list(p) for p in zip(*gaga.GAGAvatar.plan_frames(COUNTS, order)[1:])]
    assert (data.is_pinned() and not data.is_cuda) if host else data.is_cuda
    got, want = frames.split_jpeg(data, sizes), frames.split_jpeg(*frames.encode_jpeg(rgb, **JPEG))
    for t, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"frame {t} (stream {index[t, 0]}, its frame {index[t, 1]}, {order})"
    assert len(got) == sum(COUNTS) and len(set(got)) == sum(COUNTS)
    assert torch.equal(results["jpeg next"], results["rgb24 next"])


def test_engine_rendering_head_branch(rig):
    from artalk_amd.engine import ARTAvatarInferEngine
    eng = ARTAvatarInferEngine(load_gaga=True, gaga=rig.head, gaga_flame=rig.flame, model=types.SimpleNamespace(cfg=None))
    torch.manual_seed(8)
    _fresh(rig)
    data, sizes = eng.rendering(None, rig.codes, shape_id="a", output="jpeg", jpeg=JPEG)
    torch.manual_seed(8)
    _fresh(rig)
    want = frames.encode_jpeg(eng.rendering(None, rig.codes, shape_id="a", output="rgb24"), **JPEG)
    assert data.is_cuda and frames.split_jpeg(data, sizes) == frames.split_jpeg(*want)


def test_engine_rendering_mesh_branch(tmp_path):
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
    rgb = eng.rendering(audio, pred, output="rgb24")
    for jpeg in (None, JPEG, dict(quality=50, cap=frames.jpeg_bound(32, 32))):
        data, sizes = eng.rendering(audio, pred, output="jpeg", jpeg=jpeg)
        q, ss, cap = frames.jpeg_options(jpeg)
        assert data.is_cuda and tuple(data.shape) == (3, cap or frames.jpeg_default_cap(32, 32))
        got = frames.split_jpeg(data, sizes)
        assert got == frames.split_jpeg(*frames.encode_jpeg(rgb, quality=q, subsampling=ss))
        assert got == [jpeg_ref.encode(x, q, ss) for x in rgb.cpu().numpy()]
    path = tmp_path / "clip.mjpeg"
    assert frames.write_mjpeg(path, data, sizes) == 3 and frames.read_mjpeg(path) == got
    eng.mesh_renderer = None
    with pytest.raises(ValueError, match="mesh_renderer"):
        eng.rendering(audio, pred, output="jpeg")
