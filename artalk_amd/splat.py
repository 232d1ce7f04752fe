"""Device stand-in for the CUDA extension ``diff_gaussian_rasterization_32d`` that the reference's GAGAvatar head imports
(``app/GAGAvatar/utils_renderer.py:6``): ``GaussianRasterizationSettings`` and ``GaussianRasterizer`` with the extension's call
surface, and ``render_gaussian`` / ``build_camera_matrices`` with the reference's, on top of ``artalk_splat_*``
(``include/artalk_hip.h``, ``csrc/splat.hip``).  Forward only (the reference renders under ``torch.no_grad``), 32 feature channels,
precomputed colours, no spherical harmonics.  What is computed is written out in DESIGN.md ("Gaussian splat rasteriser"); parity with
the CUDA extension itself is unpinned.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import torch

from . import capi

NUM_CHANNELS = 32


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


_handles = {}      # device index -> library handle: the reference builds a rasteriser object per frame, the buffers live here


def _handle(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    h = _handles.get(idx)
    if h is None:
        L = capi.lib()
        h = C.c_void_p()
        rc = L.artalk_splat_create(int(idx), C.byref(h))
        if rc != capi.OK:
            raise RuntimeError("artalk_splat_create failed: " + L.artalk_splat_last_error(None).decode())
        _handles[idx] = h
    return h


def release():
    """Free the per-device handles and their buffers (they are kept for the life of the process otherwise)."""
    L = capi.lib()
    for h in _handles.values():
        L.artalk_splat_destroy(h)
    _handles.clear()


def _host_mats(m, what):
    m = torch.as_tensor(m).detach().to(dtype=torch.float32, device="cpu").reshape(-1, 4, 4).contiguous()
    if m.shape[0] < 1:
        raise ValueError(f"{what} must hold at least one 4 x 4 matrix")
    return m


def _device_attr(t, what, shape_tail, frames):
    """(frames or 1, N, *shape_tail) contiguous fp32 view of an attribute and its frame stride in elements."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"the splat rasteriser runs on the GPU: {what} must be a CUDA tensor (there is no CPU fallback)")
    t = t.detach().float()
    n_tail = 1
    for s in shape_tail:
        n_tail *= s
    t = t.reshape(t.shape[0], -1, *shape_tail) if frames is not None else t.reshape(1, -1, *shape_tail)
    t = t.contiguous()
    if frames is not None and t.shape[0] not in (1, frames):
        raise ValueError(f"{what} must hold 1 or {frames} frames, got {t.shape[0]}")
    stride = 0 if t.shape[0] == 1 else t.shape[1] * n_tail
    return t, stride


def _render(T, H, W, means, colors, opac, scales, rots, view, proj, tanfovx, tanfovy, scale_modifier, bg):
    """One library call.  Attributes: (tensor, frame stride) pairs from _device_attr; view / proj: host (1 or T, 4, 4)."""
    dev = means[0].device
    N = int(means[0].shape[1])
    for t, what, tail in ((colors, "colors_precomp", NUM_CHANNELS), (opac, "opacities", 1), (scales, "scales", 3), (rots, "rotations", 4)):
        if t[0].device != dev:
            raise RuntimeError(f"{what} lives on {t[0].device}, means3D on {dev}")
        if int(t[0].shape[1]) != N:
            raise ValueError(f"{what} holds {int(t[0].shape[1])} Gaussians, means3D {N}")
    if view.shape[0] != proj.shape[0] or view.shape[0] not in (1, T):
        raise ValueError(f"viewmatrix and projmatrix must hold 1 or {T} cameras each, got {view.shape[0]} and {proj.shape[0]}")
    if bg is not None:
        bg = torch.as_tensor(bg).detach().to(dtype=torch.float32, device=dev).reshape(-1)
        if bg.numel() < NUM_CHANNELS:
            raise ValueError(f"bg must hold {NUM_CHANNELS} values, got {bg.numel()}")
        bg = bg[:NUM_CHANNELS].contiguous()      # the extension reads the first 32 floats of whatever it is handed
    out = torch.empty(T, NUM_CHANNELS, H, W, dtype=torch.float32, device=dev)
    radii = torch.empty(T, N, dtype=torch.int32, device=dev)
    L = capi.lib()
    with torch.cuda.device(dev):
        h = _handle(dev)
        rc = L.artalk_splat_render(h, N, T, int(H), int(W), capi.ptr(means[0]), means[1], capi.ptr(colors[0]), colors[1],
                                   capi.ptr(opac[0]), opac[1], capi.ptr(scales[0]), scales[1], capi.ptr(rots[0]), rots[1],
                                   capi.ptr(view), capi.ptr(proj), int(view.shape[0]), float(tanfovx), float(tanfovy), float(scale_modifier),
                                   capi.ptr(bg), capi.ptr(out), capi.ptr(radii), capi.current_stream_ptr())
    if rc == capi.EINVAL:
        raise ValueError("artalk_splat_render refused: " + L.artalk_splat_last_error(h).decode())
    if rc != capi.OK:
        raise RuntimeError("artalk_splat_render failed: " + L.artalk_splat_last_error(h).decode())
    return out, radii


class GaussianRasterizer:
    def __init__(self, raster_settings):
        self.raster_settings = raster_settings

    def to(self, device):
        return self

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    @torch.no_grad()
    def forward(self, means3D, means2D=None, opacities=None, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        """One frame: means3D (N, 3), opacities (N,) or (N, 1), colors_precomp (N, 32), scales (N, 3), rotations (N, 4) as
        (r, x, y, z) -> (colour (32, H, W), radii (N,) int32).  ``means2D`` only carries gradients in the extension: ignored."""
        if shs is not None:
            raise NotImplementedError("spherical harmonics are not built: pass colors_precomp= (the reference does, utils_renderer.py:37)")
        if cov3D_precomp is not None:
            raise NotImplementedError("a precomputed 3D covariance is not built: pass scales= and rotations=")
        if colors_precomp is None:
            raise ValueError("colors_precomp is required")
        if scales is None or rotations is None:
            raise ValueError("scales and rotations are required")
        if opacities is None:
            raise ValueError("opacities is required")
        rs = self.raster_settings
        if not isinstance(means3D, torch.Tensor) or means3D.dim() != 2 or means3D.shape[-1] != 3:
            raise ValueError("means3D must be a (N, 3) tensor")
        means = _device_attr(means3D, "means3D", (3,), None)
        N = int(means[0].shape[1])
        if colors_precomp.dim() != 2 or colors_precomp.shape[-1] != NUM_CHANNELS:
            raise ValueError(f"colors_precomp must be (N, {NUM_CHANNELS}), got {tuple(colors_precomp.shape)}")
        if opacities.numel() != N:
            raise ValueError(f"opacities holds {opacities.numel()} values, means3D {N} Gaussians")
        out, radii = _render(1, rs.image_height, rs.image_width, means,
                             _device_attr(colors_precomp, "colors_precomp", (NUM_CHANNELS,), None),
                             _device_attr(opacities, "opacities", (), None), _device_attr(scales, "scales", (3,), None),
                             _device_attr(rotations, "rotations", (4,), None), _host_mats(rs.viewmatrix, "viewmatrix")[:1],
                             _host_mats(rs.projmatrix, "projmatrix")[:1], rs.tanfovx, rs.tanfovy, rs.scale_modifier, rs.bg)
        return out[0], radii[0]


def build_camera_matrices(cam_matrix, focal_x, focal_y, z_near=0.01, z_far=100.0):
    """cam_matrix (B, 3, 4) = [R | t] -> (viewmatrix (B, 4, 4), full projection (B, 4, 4), camera position (B, 3)), in the row-vector
    convention the rasteriser reads: rows 0..2 of the view matrix are R, row 3 is t, and the x and y columns are negated; a focal length
    f is in NDC units (tan(fov / 2) = 1 / f); the projection maps view z to w and [z_near, z_far] to [0, 1]."""
    if cam_matrix.shape[-2:] != (3, 4):
        raise ValueError(f"cam_matrix must be (B, 3, 4), got {tuple(cam_matrix.shape)}")
    B = cam_matrix.shape[0]
    view = cam_matrix.new_zeros(B, 4, 4)
    view[:, :3, :3] = cam_matrix[:, :, :3]
    view[:, 3, :3] = cam_matrix[:, :, 3]
    view[:, 3, 3] = 1.0
    view[:, :, :2] = -view[:, :, :2]
    fov_x, fov_y = 2.0 * math.atan(1.0 / focal_x), 2.0 * math.atan(1.0 / focal_y)
    proj_t = cam_matrix.new_zeros(4, 4)      # the projection, already transposed for row vectors
    proj_t[0, 0] = 1.0 / math.tan(fov_x / 2.0)
    proj_t[1, 1] = 1.0 / math.tan(fov_y / 2.0)
    proj_t[2, 2] = z_far / (z_far - z_near)
    proj_t[3, 2] = -(z_far * z_near) / (z_far - z_near)
    proj_t[2, 3] = 1.0
    return view, view @ proj_t, cam_matrix[:, :, 3]


@torch.no_grad()
def render_gaussian(gs_params, cam_matrix, cam_params=None, sh_degree=0, bg_color=None):
    """utils_renderer.py:10-47 in one library call over the whole batch: gs_params holds 'xyz' (B, N, 3), 'colors' (B, N, 32),
    'opacities' (B, N, 1), 'scales' (B, N, 3) and 'rotations' (B, N, 4); cam_matrix (B, 3, 4); cam_params 'focal_x', 'focal_y' and
    'size' = (H, W).  Returns the reference's dict: 'images' (B, 32, H, W), 'radii' (B, N) int32 and 'viewspace_points' (zeros: it
    only carries gradients there).  The reference hands the whole (B, 32) ``bg_color`` to every frame and the extension reads its
    first 32 floats, so row 0 is every frame's background here too."""
    if cam_params is None:
        raise ValueError("cam_params is required: focal_x, focal_y and size")
    if sh_degree != 0:
        raise NotImplementedError("spherical harmonics are not built (the reference calls with sh_degree=0)")
    B = int(cam_matrix.shape[0])
    H, W = int(cam_params["size"][0]), int(cam_params["size"][1])
    focal_x, focal_y = float(cam_params["focal_x"]), float(cam_params["focal_y"])
    points = gs_params["xyz"]
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[-1] != 3 or points.shape[0] != B:
        raise ValueError(f"gs_params['xyz'] must be ({B}, N, 3)")
    view, proj, _ = build_camera_matrices(cam_matrix.detach().float().cpu(), focal_x, focal_y)
    means = _device_attr(points, "xyz", (3,), B)
    images, radii = _render(B, H, W, means, _device_attr(gs_params["colors"], "colors", (NUM_CHANNELS,), B),
                            _device_attr(gs_params["opacities"], "opacities", (), B), _device_attr(gs_params["scales"], "scales", (3,), B),
                            _device_attr(gs_params["rotations"], "rotations", (4,), B), view.contiguous(), proj.contiguous(),
                            1.0 / focal_x, 1.0 / focal_y, 1.0, bg_color)
    return {"images": images, "radii": radii, "viewspace_points": torch.zeros_like(points)}
