"""Gaussian splat rasteriser, the part that needs no GPU: the header and the library agree on the symbols, every refusal of the C ABI
and of the Python surface comes back with its message before a device is touched, the numpy oracle (tests/splat_ref.py) reproduces a
hand-computed isotropic Gaussian and tells six wrong readings of the definition apart, the committed case table keeps its ambiguity
cap with float32 numpy deciding like float64, and ``build_camera_matrices`` gives hand-written matrices."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from artalk_amd import capi
from splat_cases import AMBIGUOUS_CAP, TABLE, camera, case, case_refs, hand_case, near_threshold, run_ref, share_and_yardstick
from splat_ref import NUM_CHANNELS, VARIANTS, build_camera

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLAT_SYMBOLS = ["artalk_splat_create", "artalk_splat_render", "artalk_splat_destroy", "artalk_splat_last_error", "artalk_splat_set_timing",
                 "artalk_splat_get_timing"]


def test_header_declares_and_library_exports_the_splat_symbols():
    text = open(os.path.join(REPO, "include", "artalk_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = capi.lib()
    for name in SPLAT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/artalk_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in capi.SYMBOLS
    assert "utils_renderer.py:6" in text and "WAITS ONCE" in text and "unpinned" in text


def _render(h, N=4, T=1, H=8, W=8, n_cams=1, tanx=0.5, tany=0.5, null=(), strides=(0, 0, 0, 0, 0)):
    """artalk_splat_render with host buffers standing in for device pointers: only for calls that are refused before the device is
    touched."""
    L = capi.lib()
    buf = np.zeros(4096, dtype=np.float32)
    p = {k: (None if k in null else buf.ctypes.data_as(C.c_void_p))
         for k in ("means", "colors", "opac", "scales", "rots", "view", "proj", "out", "radii")}
    rc = L.artalk_splat_render(h, N, T, H, W, p["means"], strides[0], p["colors"], strides[1], p["opac"], strides[2], p["scales"], strides[3],
                               p["rots"], strides[4], p["view"], p["proj"], n_cams, tanx, tany, 1.0, None, p["out"], p["radii"], None)
    return rc, L.artalk_splat_last_error(h).decode()


def test_refusals_without_gpu():
    L = capi.lib()
    rc, msg = _render(None)
    assert rc == capi.EINVAL and "NULL" in msg
    assert L.artalk_splat_create(0, None) == capi.EINVAL and "out" in L.artalk_splat_last_error(None).decode()
    h = C.c_void_p()
    assert L.artalk_splat_create(-1, C.byref(h)) == capi.EINVAL and not h.value and "device_id" in L.artalk_splat_last_error(None).decode()
    assert L.artalk_splat_set_timing(None, 1) == capi.EINVAL and L.artalk_splat_get_timing(None, None, 0, None, None) == capi.EINVAL
    L.artalk_splat_destroy(None)      # a no-op


def test_render_refusals_with_a_handle():
    """The argument checks of artalk_splat_render on a live handle: creating one does not touch the device, nor does a refused call."""
    L = capi.lib()
    h = C.c_void_p()
    assert L.artalk_splat_create(0, C.byref(h)) == capi.OK and h.value
    try:
        for kw, word in ((dict(N=-1), "N"), (dict(T=-1), "T"), (dict(H=0), "H"), (dict(H=4097), "H"), (dict(W=0), "W"), (dict(W=4097), "W"),
                         (dict(T=3, n_cams=2), "n_cams"), (dict(n_cams=0), "n_cams"), (dict(tanx=0.0), "tanfov"), (dict(tany=-1.0), "tanfov"),
                         (dict(tanx=float("nan")), "tanfov"), (dict(null=("out",)), "out"), (dict(null=("radii",)), "radii"),
                         (dict(null=("means",)), "means"), (dict(null=("colors",)), "colors"), (dict(null=("opac",)), "opacities"),
                         (dict(null=("scales",)), "scales"), (dict(null=("rots",)), "rotations"), (dict(null=("view",)), "viewmatrix"),
                         (dict(null=("proj",)), "projmatrix"), (dict(strides=(0, -32, 0, 0, 0)), "stride")):
            rc, msg = _render(h, **kw)
            assert rc == capi.EINVAL and word in msg, (kw, rc, msg)
        assert _render(h, T=0, n_cams=0)[0] == capi.OK and _render(h, T=0)[0] == capi.OK      # T = 0: a successful no-op
    finally:
        L.artalk_splat_destroy(h)


def test_python_refusals_without_gpu():
    from artalk_amd.splat import GaussianRasterizationSettings, GaussianRasterizer, build_camera_matrices, render_gaussian
    assert GaussianRasterizationSettings._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                                                     "projmatrix", "sh_degree", "campos", "prefiltered", "debug")
    eye = torch.eye(4)
    rs = GaussianRasterizationSettings(image_height=8, image_width=8, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(32), scale_modifier=1.0,
                                       viewmatrix=eye, projmatrix=eye, sh_degree=0, campos=torch.zeros(3), prefiltered=False, debug=False)
    r = GaussianRasterizer(raster_settings=rs)
    assert r.raster_settings is rs and r.to("cuda") is r
    n = 5
    kw = dict(means3D=torch.zeros(n, 3), means2D=torch.zeros(n, 3), opacities=torch.ones(n, 1), colors_precomp=torch.zeros(n, 32),
              scales=torch.ones(n, 3), rotations=torch.zeros(n, 4))
    with pytest.raises(NotImplementedError, match="harmonics"):
        r(**dict(kw, shs=torch.zeros(n, 16, 3), colors_precomp=None))
    with pytest.raises(NotImplementedError, match="covariance"):
        r(**dict(kw, cov3D_precomp=torch.zeros(n, 6)))
    with pytest.raises(ValueError, match="colors_precomp"):
        r(**dict(kw, colors_precomp=None))
    with pytest.raises(ValueError, match="scales"):
        r(**dict(kw, scales=None))
    with pytest.raises(ValueError, match="means3D"):
        r(**dict(kw, means3D=torch.zeros(n, 2)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(**kw)
    gs = dict(xyz=torch.zeros(2, n, 3), colors=torch.zeros(2, n, 32), opacities=torch.ones(2, n, 1), scales=torch.ones(2, n, 3),
              rotations=torch.zeros(2, n, 4))
    cam = torch.zeros(2, 3, 4)
    params = dict(focal_x=12.0, focal_y=12.0, size=(8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_gaussian(gs, cam, params)
    with pytest.raises(NotImplementedError):
        render_gaussian(gs, cam, params, sh_degree=3)
    with pytest.raises(ValueError, match="cam_params"):
        render_gaussian(gs, cam)
    with pytest.raises(ValueError, match="xyz"):
        render_gaussian(dict(gs, xyz=torch.zeros(3, n, 3)), cam, params)
    with pytest.raises(ValueError, match=r"\(B, 3, 4\)"):
        build_camera_matrices(torch.zeros(2, 4, 4), 12.0, 12.0)


def test_build_camera_matrices_against_hand_written_matrices():
    from artalk_amd.splat import build_camera_matrices
    # a quarter turn about y (x -> z, z -> -x as rows of R) and a translation; focal 12 horizontally, 6 vertically
    M = torch.tensor([[[0.0, 0.0, 1.0, 0.5], [0.0, 1.0, 0.0, -0.25], [-1.0, 0.0, 0.0, 2.0]]])
    view, proj, pos = build_camera_matrices(M, 12.0, 6.0)
    want_view = torch.tensor([[0.0, 0.0, 1.0, 0.0], [0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [-0.5, 0.25, 2.0, 1.0]])
    assert view.shape == (1, 4, 4) and torch.equal(view[0], want_view)
    a, b = 100.0 / 99.99, -1.0 / 99.99      # z_far / (z_far - z_near), -z_far z_near / (z_far - z_near)
    # a point p maps to (p, 1) . view = t, then to (12 t.x, 6 t.y, a t.z + b, t.z)
    want_proj = torch.tensor([[0.0, 0.0, a, 1.0], [0.0, -6.0, 0.0, 0.0], [12.0, 0.0, 0.0, 0.0], [-6.0, 1.5, 2.0 * a + b, 2.0]])
    assert torch.allclose(proj[0], want_proj, rtol=0, atol=2e-6), proj[0]
    assert torch.equal(pos, torch.tensor([[0.5, -0.25, 2.0]]))
    p = torch.tensor([0.1, 0.2, 0.3, 1.0])
    t = p @ view[0]
    assert torch.allclose(t, torch.tensor([0.3 - 0.5, -0.2 + 0.25, 0.1 + 2.0, 1.0]), atol=1e-7)
    h = p @ proj[0]
    assert torch.allclose(h, torch.tensor([12.0 * t[0], 6.0 * t[1], a * t[2] + b, t[2]]), atol=1e-5)
    # the numpy restatement the oracle uses is the same thing
    V, P = build_camera(M[0].numpy(), 12.0, 6.0)
    assert np.allclose(V, view[0].numpy(), atol=1e-7) and np.allclose(P, proj[0].numpy(), atol=2e-6)


# ---------------------------------------------------------------------------------------------- the oracle against a hand computation
# One isotropic Gaussian (scale s, identity rotation) on the optical axis at depth z under a camera without rotation: J V^T is
# diag(fx / z, fy / z) up to sign, so cov = (fx s / z)^2 + 0.3 on both axes with no cross term, and alpha(d) = o exp(-d^2 / (2 cov)).
def test_oracle_against_a_hand_computed_isotropic_gaussian():
    H = W = 24
    s, o, z = 0.3, 0.8, 3.0
    cam = camera(2.0, 2.0, z)
    c = hand_case([[0.0, 0.0, 0.0]], o, s, H, W, cam=cam, bg=np.full(NUM_CHANNELS, 0.25))
    r = run_ref(c)
    fx = W / (2.0 * 0.5)
    cov = (fx * s / z) ** 2 + 0.3
    pre = r["pre"]
    assert np.allclose(pre["conic"][0], [1.0 / cov, 0.0, 1.0 / cov], rtol=1e-6, atol=1e-12)      # (float32 inputs: s is not exactly 0.3)
    assert np.allclose(pre["centre"][0], [(W - 1) / 2.0, (H - 1) / 2.0], atol=1e-6) and abs(pre["depth"][0] - z) < 1e-12
    lam = cov + math.sqrt(0.1)      # mid = cov, det = cov^2: the floor of 0.1 under the root is what counts
    assert r["radii"][0] == math.ceil(3.0 * math.sqrt(lam)) == 8
    # centre 11.5 +- 8 -> tiles int(3.5 / 16) .. int((19.5 + 15) / 16) = 0 .. 2, which is also the image's 2 tiles
    assert r["rect"][0].tolist() == [0, 2, 0, 2]
    col = c["colors"][0].astype(np.float64)
    o32 = float(c["opacities"][0])
    for (py, px) in ((11, 11), (12, 14), (11, 18), (3, 20), (0, 0), (23, 5)):
        d2 = (11.5 - px) ** 2 + (11.5 - py) ** 2
        alpha = min(0.99, o32 * math.exp(-d2 / (2.0 * cov)))
        if alpha < 1.0 / 255.0:
            want = np.full(NUM_CHANNELS, 0.25)
            assert r["count"][py, px] == 0
        else:
            want = col * alpha + (1.0 - alpha) * 0.25
            assert r["count"][py, px] == 1
        assert np.allclose(r["image"][:, py, px], want, rtol=0, atol=1e-6), (py, px)
    assert r["count"][0, 0] == 0 and r["count"][11, 18] == 1      # both branches were taken, the second tile column too
    r32 = run_ref(c, dtype=np.float32)
    assert r32["image"].dtype == np.float32 and np.array_equal(r32["radii"], r["radii"]) and np.array_equal(r32["rect"], r["rect"])
    assert np.abs(r32["image"] - r["image"]).max() < 1e-5


def test_oracle_tells_wrong_variants_apart():
    c = case("opaque_stack")
    good = run_ref(c)
    assert len(VARIANTS) >= 6
    assert (good["stop_margin"] < np.inf).any() and good["T"][16, 16] < 0.01 and good["count"][16, 16] <= 3      # the centre stops at the third of the stack
    assert abs(good["pre"]["centre"][5] - [20.0, 10.0]).max() < 1e-6      # (the 1e-7 under the division)
    for variant in VARIANTS:
        bad = run_ref(c, variant=variant)
        diff = float(np.abs(bad["image"] - good["image"]).max())
        assert diff > 1e-3, f"variant {variant} renders the same image (max difference {diff:.2e})"
    # and the float32 yardstick stays far inside that distance
    assert np.abs(run_ref(c, dtype=np.float32)["image"] - good["image"]).max() < 1e-4


@pytest.mark.parametrize("name", sorted(TABLE))
def test_case_table_keeps_its_cap_and_float32_decides_alike(name):
    c = case(name)
    r64, r32 = case_refs(name)
    assert not near_threshold(r64["pre"]).any()
    assert np.array_equal(r32["radii"], r64["radii"]) and np.array_equal(r32["rect"], r64["rect"])
    amb, share, yard = share_and_yardstick(r64, r32)
    print(f"{name}: N {c['means'].shape[0]}, {c['H']} x {c['W']}, drawn {int((r64['radii'] > 0).sum())}, ambiguous share {share:.3%}, "
          f"float32 numpy error {yard:.3e} on values up to {np.abs(r64['image']).max():.2f}, most Gaussians on a pixel {int(r64['count'].max())}")
    assert share <= AMBIGUOUS_CAP, f"{name}: the ambiguity mask covers {share:.3%} of the pixels"
    ok = ~amb
    assert np.array_equal(r32["count"][ok], r64["count"][ok]), "float32 numpy blends another number of Gaussians on an unambiguous pixel"
    assert yard < 1e-4
    if c["means"].shape[0] >= 255:
        assert (r64["radii"] > 0).sum() > 0.3 * c["means"].shape[0] and r64["count"].max() >= 5
    if name == "one_tile_600":
        in_tile = (r64["rect"][:, 0] <= 1) & (r64["rect"][:, 1] > 1) & (r64["rect"][:, 2] <= 1) & (r64["rect"][:, 3] > 1)
        assert in_tile.sum() > 512 and r64["T"][16:32, 16:32].min() > 1e-3      # three batches, and the walk reaches the last
    if name == "whole_image":
        assert r64["rect"][0].tolist() == [0, 4, 0, 3] and r64["radii"][0] > 56
    if name == "culled_and_drawn":
        assert r64["radii"][:6].tolist() == [0] * 6 and (r64["radii"][6:] > 0).all()
