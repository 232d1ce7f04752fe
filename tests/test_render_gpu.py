"""Mesh renderer on the GPU (artalk_render_*, artalk_amd.render.RenderMesh) against the numpy restatement of its definition
(tests/render_ref.py, float64).  float32 may decide a pixel differently only where the reference itself is within rounding of a
decision (``ambiguous``: an edge within 1e-4 of the pixel centre in barycentric units, or two covering depths within 1e-5); everywhere
else the face index must be equal.  Colours are held to 4 x the error the same formulas make in float32 numpy.

Measured on an MI355X (max-abs colour error on a 0..255 scale, kernel / float32 numpy; ambiguous share), table in DESIGN.md section 5:
sphere S=64 1.692e-4 / 1.692e-4 (0.057 %), S=96 3.663e-4 / 3.663e-4 (0.072 %), S=1 3.678e-5 / 2.281e-5 (0), S=50 1.288e-4 / 1.288e-4
(0.093 %), custom camera 7.895e-5 / 9.288e-5 (0.024 %), clipping 2.941e-5 / 2.941e-5 (0.046 %), whole-image faces 2.516e-5 / 4.552e-5."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from artalk_amd import capi
from render_ref import ambiguous, default_transform, jittered_sphere, render_ref

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 0.01      # share of all pixels the ambiguity mask may take
COLOUR_FACTOR = 4.0       # kernel colour error <= this x the float32 numpy error


@functools.lru_cache(maxsize=None)
def _sphere():
    return jittered_sphere(T=5)      # frames 0..2 are the 3-frame mesh of the reference tests; 5 frames for the batching test


@functools.lru_cache(maxsize=None)
def _sphere_ref(S, T, dtype, camera=None):
    verts, faces = _sphere()
    kw = {} if camera is None else dict(transform=_camera_20deg(), focal=8.0)
    return render_ref(verts[:T], faces, S, dtype=dtype, **kw)


def _camera_20deg():
    a = np.deg2rad(20.0)
    ry = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    M = default_transform()
    M[:, :3] = ry @ M[:, :3]
    return M


def _render(verts, faces, S, slab=0, **kw):
    from artalk_amd.render import RenderMesh
    r = RenderMesh(S, faces=faces)
    r.slab_frames = slab
    rgb, alpha, p2f = r.forward(torch.from_numpy(np.ascontiguousarray(verts)).cuda(), return_pix_to_face=True, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), alpha.cpu().numpy(), p2f.cpu().numpy()


def _check(tag, got, r64, r32, cap=AMBIGUOUS_CAP):
    """The checks every comparison with the reference shares.  Returns (ambiguous share, kernel colour error, float32 numpy error)."""
    rgb, alpha, p2f = got
    assert rgb.shape == r64["rgb"].shape and alpha.shape == r64["alpha"].shape and p2f.shape == r64["pix_to_face"].shape
    assert rgb.dtype == np.float32 and alpha.dtype == np.float32 and p2f.dtype == np.int32
    amb = ambiguous(r64)
    share = float(amb.mean())
    ok = ~amb
    covered = ok & (r64["pix_to_face"] >= 0)
    m3 = np.broadcast_to(covered[:, None], rgb.shape)
    yard = float(np.abs(r32["rgb"].astype(np.float64) - r64["rgb"])[m3].max()) if covered.any() else 0.0
    err = float(np.abs(rgb.astype(np.float64) - r64["rgb"])[m3].max()) if covered.any() else 0.0
    print(f"{tag}: ambiguous share {share:.4%} of {amb.size} pixels, colour max-abs error kernel {err:.3e} / float32 numpy {yard:.3e} "
          f"(bound {COLOUR_FACTOR:g} x = {COLOUR_FACTOR * yard:.3e}) on {int(covered.sum())} covered pixels")
    if cap is not None:
        assert share <= cap, f"{tag}: the ambiguity mask covers {share:.3%} of the pixels"
    bad = ok & (p2f != r64["pix_to_face"])
    assert not bad.any(), f"{tag}: {int(bad.sum())} unambiguous pixels with another face, first {np.argwhere(bad)[:4].tolist()}"
    assert np.array_equal(alpha[:, 0][ok], r64["alpha"][:, 0][ok].astype(np.float32))
    # background: exactly white, transparent, -1
    bg = p2f == -1
    assert (rgb[np.broadcast_to(bg[:, None], rgb.shape)] == 255.0).all() and (alpha[:, 0][bg] == 0.0).all()
    assert (alpha[:, 0][~bg] == 1.0).all() and (p2f >= -1).all()
    assert err <= COLOUR_FACTOR * yard, f"{tag}: colour error {err:.3e} above {COLOUR_FACTOR:g} x the float32 numpy error {yard:.3e}"
    return share, err, yard


@pytest.mark.parametrize("S", [64, 96])
def test_against_float64(S):
    verts, faces = _sphere()
    got = _render(verts[:3], faces, S)
    r64, r32 = _sphere_ref(S, 3, np.float64), _sphere_ref(S, 3, np.float32)
    assert np.array_equal(r32["pix_to_face"][~ambiguous(r64)], r64["pix_to_face"][~ambiguous(r64)])      # the yardstick decides alike
    _check(f"sphere S={S}", got, r64, r32)
    assert (got[2] >= 0).mean() > 0.25      # the sphere fills a third of the image


@pytest.mark.parametrize("S", [1, 50])
def test_odd_sizes(S):
    verts, faces = _sphere()
    got = _render(verts[:3], faces, S)
    _check(f"sphere S={S}", got, _sphere_ref(S, 3, np.float64), _sphere_ref(S, 3, np.float32))


# One triangle per case, under the default camera (NDC = (-12 x / Z, 12 y / Z), Z = 2 - z): a plain one in view, one wholly outside, one
# across each image border, one with a vertex behind the camera, one of zero area (collinear) and one that names a vertex twice.
def _clip_mesh():
    def tri(ndc, z=0.0):
        return [[-x * (2.0 - z) / 12.0, y * (2.0 - z) / 12.0, z] for x, y in ndc]
    v = []
    v += tri([(0.5, 0.4), (-0.45, 0.3), (0.1, -0.55)], 0.0)            # 0: in view
    v += tri([(2.1, 0.2), (3.0, 0.4), (2.5, 1.0)], 0.1)                # 1: wholly outside (left of the image)
    v += tri([(0.7, 0.1), (1.6, 0.3), (0.8, 0.62)], 0.2)               # 2: across the left border (x = +1)
    v += tri([(-0.7, -0.1), (-1.7, -0.3), (-0.8, -0.6)], 0.3)          # 3: across the right border
    v += tri([(0.1, 0.7), (-0.33, 1.8), (-0.4, 0.8)], 0.4)             # 4: across the top border (y = +1)
    v += tri([(0.3, -0.7), (0.0, -5.0), (-0.4, -0.8)], 0.5)            # 5: across the bottom border, far out
    v += [[0.05, 0.02, 0.6], [-0.06, 0.03, 0.6], [0.0, 0.0, 3.0]]      # 6: third vertex behind the camera (Z = -1)
    v += tri([(0.6, 0.0), (0.0, 0.0), (-0.6, 0.0)], 0.7)               # 7: zero area (all on y = 0)
    faces = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(8)] + [[0, 0, 1]]      # 8: a vertex named twice
    return np.array([v], dtype=np.float32), np.array(faces, dtype=np.int32)


def test_clipping_and_guard_bands():
    verts, faces = _clip_mesh()
    S, T, PAD = 33, 2, 4096
    verts = np.concatenate([verts, verts * np.float32(0.9)])      # second frame: everything scaled towards the origin
    V, F = verts.shape[1], faces.shape[0]
    L = capi.lib()
    h = C.c_void_p()
    assert L.artalk_render_create(0, V, F, faces.ctypes.data_as(C.c_void_p), S, 1.0, C.byref(h)) == capi.OK
    try:
        n = T * S * S
        rgb = torch.full((PAD + 3 * n + PAD,), -7.5, dtype=torch.float32, device="cuda")
        alpha = torch.full((PAD + n + PAD,), -7.5, dtype=torch.float32, device="cuda")
        p2f = torch.full((PAD + n + PAD,), -77, dtype=torch.int32, device="cuda")
        vd = torch.from_numpy(verts).cuda()
        rc = L.artalk_render_mesh(h, capi.ptr(vd), T, None, 0.0, capi.ptr(rgb[PAD:]), capi.ptr(alpha[PAD:]), capi.ptr(p2f[PAD:]),
                                  capi.current_stream_ptr())
        assert rc == capi.OK, L.artalk_render_last_error(h).decode()
        torch.cuda.synchronize()
        for buf, poison, size in ((rgb, -7.5, 3 * n), (alpha, -7.5, n), (p2f, -77, n)):
            assert (buf[:PAD] == poison).all() and (buf[PAD + size:] == poison).all(), "guard band written"
            assert (buf[PAD:PAD + size] != poison).all(), "output not fully written"
        got = (rgb[PAD:PAD + 3 * n].reshape(T, 3, S, S).cpu().numpy(), alpha[PAD:PAD + n].reshape(T, 1, S, S).cpu().numpy(),
               p2f[PAD:PAD + n].reshape(T, S, S).cpu().numpy())
        # every refusal of artalk_render_mesh, with a live handle; nothing may be written
        before = rgb.clone()
        for args in ((None, T, capi.ptr(rgb[PAD:]), capi.ptr(alpha[PAD:])), (capi.ptr(vd), T, None, capi.ptr(alpha[PAD:])),
                     (capi.ptr(vd), T, capi.ptr(rgb[PAD:]), None), (capi.ptr(vd), -1, capi.ptr(rgb[PAD:]), capi.ptr(alpha[PAD:]))):
            assert L.artalk_render_mesh(h, args[0], args[1], None, 0.0, args[2], args[3], None, capi.current_stream_ptr()) == capi.EINVAL
            assert L.artalk_render_last_error(h).decode()
        rgb.fill_(-7.5)
        assert L.artalk_render_mesh(h, capi.ptr(vd), 0, None, 0.0, capi.ptr(rgb[PAD:]), capi.ptr(alpha[PAD:]), None,
                                    capi.current_stream_ptr()) == capi.OK      # T = 0: a successful no-op
        torch.cuda.synchronize()
        assert (rgb == -7.5).all() and before.shape == rgb.shape
        assert L.artalk_render_set_slab(h, 10 ** 6) == capi.EINVAL and L.artalk_render_set_slab(h, -1) == capi.EINVAL
    finally:
        L.artalk_render_destroy(h)
    r64, r32 = render_ref(verts, faces, S), render_ref(verts, faces, S, dtype=np.float32)
    _check("clipping", got, r64, r32, cap=None)
    seen = set(np.unique(got[2]).tolist())
    assert seen == {-1, 0, 2, 3, 4, 5}, seen      # never the outside (1), behind-camera (6) or zero-area (7, 8) faces
    for f in (2, 3, 4, 5):      # each border triangle reaches its border
        rows, cols = np.nonzero(got[2][0] == f)
        assert {2: cols.min() == 0, 3: cols.max() == S - 1, 4: rows.min() == 0, 5: rows.max() == S - 1}[f], f


def test_tie_break_lower_index_wins():
    """Two faces with identical vertices: equal depth on every pixel, the lower index is drawn - also when it is not the first to arrive
    (face 3 repeats face 1) and when the twin is built from other vertex indices with the same coordinates (face 2 vs face 0)."""
    a = [[-0.1, 0.09, 0.0], [0.11, 0.1, 0.02], [0.0, -0.12, 0.05]]
    b = [[-0.03, 0.11, -0.1], [0.12, -0.05, -0.1], [-0.11, -0.08, -0.12]]
    verts = np.array([a + b + a], dtype=np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [3, 4, 5]], dtype=np.int32)
    S = 40
    rgb, alpha, p2f = _render(verts, faces, S)
    r64 = render_ref(verts, faces, S)
    assert set(np.unique(p2f).tolist()) == {-1, 0, 1}
    assert (r64["gap"][r64["pix_to_face"] >= 0] == 0).all()          # every covered pixel is a tie in the reference
    clear = r64["min_w"] >= 1e-4
    assert np.array_equal(p2f[clear], r64["pix_to_face"][clear]) and (p2f == 0).sum() > 50 and (p2f == 1).sum() > 50


def test_whole_image_faces():
    """The 9 976 random faces of the synthetic FLAME asset: almost every face spans the image, every pixel is covered thousands of
    times.  A rasteriser that walks faces per thread, or one workgroup's share of them in sequence, does not finish this in test time."""
    from artalk_amd.flame import FLAMEModel, synthetic_flame_asset
    fm = FLAMEModel(n_shape=300, n_exp=100, scale=1.0, no_lmks=True, flame_ckpt=synthetic_flame_asset())
    g = torch.Generator().manual_seed(5)
    vd = fm(shape_params=0.5 * torch.randn(1, 300, generator=g), expression_params=0.5 * torch.randn(1, 100, generator=g),
            pose_params=0.1 * torch.randn(1, 6, generator=g))
    verts, faces = vd.cpu().numpy(), fm.get_faces().numpy().astype(np.int32)
    assert faces.shape == (9976, 3)
    S = 32
    got = _render(verts, faces, S)
    r64, r32 = render_ref(verts, faces, S, detail=True), render_ref(verts, faces, S, dtype=np.float32)
    share, _, _ = _check("whole-image faces", got, r64, r32, cap=None)      # thousands of edges and depths per pixel: no cap here
    assert share < 0.9, "no unambiguous pixel left to compare"
    # on EVERY pixel, ambiguous or not: the face drawn comes within 1e-4 of covering the pixel in float64, and is not deeper (beyond
    # 1e-5) than the nearest face that covers it clearly
    p2f = got[2].reshape(-1)
    assert (p2f >= 0).all()
    px = np.arange(S * S)
    wmin, pz = r64["wmin"][0], r64["pz"][0]
    assert (wmin[p2f, px] > -1e-4).all()
    nearest_clear = np.where(wmin > 1e-4, pz, np.inf).min(axis=0)
    assert (pz[p2f, px] <= nearest_clear + 1e-5).all()


def test_determinism_and_batching():
    verts, faces = _sphere()
    S = 64
    whole = _render(verts, faces, S, slab=2)            # T = 5 in slabs of 2, 2 and 1 frames
    again = _render(verts, faces, S, slab=2)
    default = _render(verts, faces, S)                   # one slab
    for a, b, c in zip(whole, again, default):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    for t in range(5):
        one = _render(verts[t:t + 1], faces, S)
        for a, b in zip(whole, one):
            assert np.array_equal(a[t:t + 1], b), t
    assert not np.array_equal(whole[2][0], whole[2][1])      # the frames do differ
    r64 = _sphere_ref(S, 3, np.float64)
    assert np.array_equal(whole[2][:3][~ambiguous(r64)], r64["pix_to_face"][~ambiguous(r64)])


def test_custom_camera():
    verts, faces = _sphere()
    S = 64
    M = _camera_20deg()
    got = _render(verts[:3], faces, S, transform_matrix=torch.from_numpy(M)[None].float(), focal_length=8.0)
    r64, r32 = _sphere_ref(S, 3, np.float64, "20deg"), _sphere_ref(S, 3, np.float32, "20deg")
    _check("custom camera", got, r64, r32)
    assert not np.array_equal(got[2], _render(verts[:3], faces, S)[2])
    # one camera per frame goes frame by frame and gives the same bits
    per_frame = _render(verts[:3], faces, S, transform_matrix=torch.from_numpy(M)[None].float().repeat(3, 1, 1), focal_length=torch.tensor(8.0))
    for a, b in zip(got, per_frame):
        assert np.array_equal(a, b)


def test_engine_rendering_returns_images_with_a_renderer():
    """inference.py:59-72, :83: with a FLAME model and a mesh renderer plugged in, ``rendering`` returns the stack of frames."""
    from artalk_amd.engine import ARTAvatarInferEngine
    from artalk_amd.flame import FLAMEModel, synthetic_flame_asset
    from artalk_amd.render import RenderMesh
    from artalk_amd.synth import synth_audio
    from conftest import get_gpu_model
    eng = ARTAvatarInferEngine.__new__(ARTAvatarInferEngine)
    eng.ARTalk, eng.device, eng.style_motion, eng.clip_length, eng.fix_pose = get_gpu_model("tiny"), "cuda", None, 40, False
    eng.flame_model = FLAMEModel(n_shape=300, n_exp=100, scale=1.0, no_lmks=True, flame_ckpt=synthetic_flame_asset())
    eng.mesh_renderer = None
    audio = torch.from_numpy(synth_audio(3, 4.0))
    pred = eng.inference(audio)
    verts = eng.rendering(audio, pred)
    assert verts.shape == (40, 5023, 3)                       # no renderer: the vertices, as before
    eng.mesh_renderer = RenderMesh(32, faces=eng.flame_model.get_faces(), scale=1.0)
    images = eng.rendering(audio, pred, shape_id="mesh")
    assert images.shape == (40, 3, 32, 32) and images.is_cuda and images.dtype == torch.float32
    assert images.min().item() >= 0.0 and images.max().item() <= 1.0
    want = RenderMesh(32, faces=eng.flame_model.get_faces(), n_verts=5023).forward(verts)[0] / 255
    assert torch.equal(images, want)
    assert images.std().item() > 0.01
