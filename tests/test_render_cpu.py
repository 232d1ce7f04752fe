"""Mesh renderer, the part that needs no GPU: every refusal of the C ABI and of the Python class comes back with its error and its
message before a device is touched, the numpy reference (tests/render_ref.py) renders a hand-computed triangle, and the header and
the library agree on the new symbols."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from artalk_amd import capi
from render_ref import ambiguous, render_ref, uv_sphere

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDER_SYMBOLS = ["artalk_render_create", "artalk_render_mesh", "artalk_render_destroy", "artalk_render_last_error"]


def test_header_declares_and_library_exports_the_render_symbols():
    text = open(os.path.join(REPO, "include", "artalk_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = capi.lib()
    for name in RENDER_SYMBOLS + ["artalk_render_set_slab"]:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/artalk_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in capi.SYMBOLS
    assert "renderer_utils.py:55-85" in text and "unpinned" in text


def _create(V, F, faces, S, scale=1.0, out=True):
    L = capi.lib()
    h = C.c_void_p()
    fp = None if faces is None else np.ascontiguousarray(faces, dtype=np.int32).ctypes.data_as(C.c_void_p)
    rc = L.artalk_render_create(0, V, F, fp, S, scale, C.byref(h) if out else None)
    return rc, L.artalk_render_last_error(None).decode(), h


def test_create_refusals_without_gpu():
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    for args, word in (((0, 1, tri, 8), "V"), ((-3, 1, tri, 8), "V"), ((3, 0, tri, 8), "F"), ((3, -1, tri, 8), "F"),
                       ((3, 1, tri, 0), "image_size"), ((3, 1, tri, -5), "image_size"), ((3, 1, None, 8), "faces_host")):
        rc, msg, h = _create(*args)
        assert rc == capi.EINVAL and word in msg and not h.value, (args[:2], args[3], rc, msg)
    rc, msg, h = _create(3, 1, np.array([[0, 1, 3]], dtype=np.int32), 8)
    assert rc == capi.EINVAL and "face 0" in msg and "3" in msg and not h.value, msg
    rc, msg, h = _create(5, 2, np.array([[0, 1, 2], [4, -1, 2]], dtype=np.int32), 8)
    assert rc == capi.EINVAL and "face 1" in msg and "-1" in msg and not h.value, msg
    rc, msg, _ = _create(3, 1, tri, 8, out=False)
    assert rc == capi.EINVAL and "out" in msg


def test_render_mesh_and_set_slab_refuse_a_null_handle_without_gpu():
    L = capi.lib()
    buf = np.zeros(16, dtype=np.float32).ctypes.data_as(C.c_void_p)
    assert L.artalk_render_mesh(None, buf, 1, None, 0.0, buf, buf, None, None) == capi.EINVAL
    assert "NULL" in L.artalk_render_last_error(None).decode()
    assert L.artalk_render_set_slab(None, 1) == capi.EINVAL
    L.artalk_render_destroy(None)      # a no-op


def test_python_refusals_without_gpu():
    from artalk_amd.render import RenderMesh
    tri = np.array([[0, 1, 2]], dtype=np.int64)
    with pytest.raises(NotImplementedError):
        RenderMesh(32, obj_filename="head_template.obj")
    with pytest.raises(NotImplementedError, match="Must have faces"):
        RenderMesh(32)
    with pytest.raises(ValueError, match="integer"):
        RenderMesh(32.5, faces=tri)
    with pytest.raises(ValueError, match="image_size"):
        RenderMesh(0, faces=tri, n_verts=3)
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        RenderMesh(32, faces=np.zeros((4, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="face 0 has vertex index 2"):
        RenderMesh(32, faces=tri, n_verts=2)
    with pytest.raises(ValueError, match="V must be positive"):
        RenderMesh(32, faces=tri, n_verts=0)
    r = RenderMesh(32.0, faces=torch.from_numpy(tri), scale=1.0, n_verts=3)      # the reference's arguments; an ndarray works as well
    assert r.image_size == 32 and r.to("cuda") is r and r.faces.shape == (1, 3)
    assert RenderMesh(16, faces=tri).faces.dtype == torch.int32                  # renderer_utils.py:38
    with pytest.raises(NotImplementedError, match="pytorch3d"):
        r.forward(torch.zeros(1, 3, 3), cameras=object())
    with pytest.raises(ValueError):
        r.forward(torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.forward(torch.zeros(1, 3, 3))


# ---------------------------------------------------------------------------------------------- the reference against a hand computation
# One triangle in the plane z = 0 under the default camera (view = (-x, y, 2 - z), focal 12): NDC = (-6 x, 6 y), every depth 2, so the
# perspective correction is the identity.  NDC vertices (0.9, 0.9), (0.9, -1.0), (-1.0, 0.9): covered is x < 0.9, y < 0.9, x + y > -0.1.
# The winding makes the normal +z, towards the camera at (0, 0, 2).
TRI_NDC = [(0.9, 0.9), (0.9, -1.0), (-1.0, 0.9)]
TRI = np.array([[[-x / 6.0, y / 6.0, 0.0] for x, y in TRI_NDC]])


def _phong_by_hand(P):
    """The shading formula in scalar arithmetic, normal (0, 0, 1), camera centre (0, 0, 2), light (0, 1, 3)."""
    d = [0.0 - P[0], 1.0 - P[1], 3.0 - P[2]]
    n = math.sqrt(sum(x * x for x in d))
    d = [x / n for x in d]
    c = d[2]
    v = [0.0 - P[0], 0.0 - P[1], 2.0 - P[2]]
    n = math.sqrt(sum(x * x for x in v))
    v = [x / n for x in v]
    r = [-d[0], -d[1], -d[2] + 2.0 * c]
    a = max(sum(x * y for x, y in zip(v, r)), 0.0) if c > 0 else 0.0
    return [255.0 * ((0.5 + 0.3 * max(c, 0.0)) * k / 255.0 + 0.2 * 0.6 * a ** 10) for k in (142.0, 179.0, 247.0)]


def test_reference_renders_a_hand_computed_triangle():
    faces = np.array([[0, 1, 2]])
    r = render_ref(TRI, faces, 4)
    # pixel centres at 0.75, 0.25, -0.25, -0.75 (index 0..3; column 0 is the LEFT = +x side, row 0 the top = +y side)
    want = np.array([[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0]], dtype=bool)
    assert np.array_equal(r["pix_to_face"][0] == 0, want)
    assert np.array_equal(r["pix_to_face"][0] == -1, ~want)
    assert np.array_equal(r["alpha"][0, 0], want.astype(np.float64))
    assert (r["rgb"][0][:, ~want] == 255.0).all()
    assert not ambiguous(r).any() and np.isinf(r["gap"]).all()      # one face: no second depth
    # the nearest edge of pixel (row 3, column 0) = (0.75, -0.75) is x + y = -0.1: w = 0.1 / 1.9 of the way in
    assert abs(r["min_w"][0, 3, 0] - 0.1 / 1.9) < 1e-12
    for (row, col) in ((1, 1), (0, 3), (2, 0)):
        x, y = 1 - (2 * col + 1) / 4, 1 - (2 * row + 1) / 4
        assert np.allclose(r["rgb"][0, :, row, col], _phong_by_hand([-x / 6.0, y / 6.0, 0.0]), rtol=0, atol=1e-11), (row, col)
    # the centre pixel of the image (S = 1: NDC (0, 0), the point (0, 0, 0)): d = (0, 1, 3) / sqrt 10, c = a = 3 / sqrt 10, a^10 = 0.9^5
    c1 = render_ref(TRI, faces, 1)
    lit, spec = 0.5 + 0.3 * 3 / math.sqrt(10.0), 0.12 * 0.9 ** 5
    assert np.allclose(c1["rgb"][0, :, 0, 0], [lit * 142 + 255 * spec, lit * 179 + 255 * spec, lit * 247 + 255 * spec], rtol=0, atol=1e-11)
    assert c1["pix_to_face"][0, 0, 0] == 0 and c1["alpha"][0, 0, 0, 0] == 1.0
    # the same in float32 (the yardstick arithmetic of the GPU tests): same coverage, colours to float32 accuracy
    r32 = render_ref(TRI.astype(np.float32), faces, 4, dtype=np.float32)
    assert r32["rgb"].dtype == np.float32 and np.array_equal(r32["pix_to_face"], r["pix_to_face"])
    assert np.abs(r32["rgb"] - r["rgb"]).max() < 1e-3


def test_reference_conventions():
    """Back faces are drawn (no culling), depth picks the nearer face, a custom camera moves the image the way its matrix says."""
    faces = np.array([[0, 1, 2], [3, 5, 4]])      # the same triangle 0.1 nearer to the camera, wound the other way
    near = TRI[0] + np.array([0.0, 0.0, 0.1])
    r = render_ref(np.concatenate([TRI[0], near])[None], faces, 4)
    assert set(np.unique(r["pix_to_face"])) == {-1, 1}
    assert (r["gap"][r["pix_to_face"] == 1] > 0.09).all()
    # back-facing: the normal points away from the light, only the ambient term is left
    assert np.allclose(r["rgb"][0, :, 0, 0], [0.5 * 142, 0.5 * 179, 0.5 * 247], atol=1e-12)
    # T = (0.05, 0, 2) shifts the view by +0.05 in x: NDC x grows by 0.3 (the image moves left), covered is now x + y > 0.2, which
    # drops the four pixels on x + y = 0
    M = np.array([[-1.0, 0, 0, 0.05], [0, 1.0, 0, 0], [0, 0, -1.0, 2.0]])
    s = render_ref(TRI, np.array([[0, 1, 2]]), 4, transform=M)
    want = np.array([[1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], dtype=bool)
    assert np.array_equal(s["pix_to_face"][0] == 0, want)
    # focal 6 halves the NDC triangle: (0.45, 0.45), (0.45, -0.5), (-0.5, 0.45) holds the pixel centres (0.25, +-0.25) and (-0.25, 0.25)
    h = render_ref(TRI, np.array([[0, 1, 2]]), 4, focal=6.0)
    want = np.array([[0, 0, 0, 0], [0, 1, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0]], dtype=bool)
    assert np.array_equal(h["pix_to_face"][0] == 0, want)
    v, f = uv_sphere()
    assert v.shape == (408, 3) and f.shape == (768, 3)
