"""Device stand-in for the reference's ``RenderMesh`` (``app/flame_model/renderer_utils.py:23-85``), which wraps pytorch3d's
rasteriser and ``HardPhongShader``.  pytorch3d has no ROCm build, so the mesh branch of ``inference.py:59-72`` cannot run there;
this class takes the same constructor and ``forward`` arguments and rasterises and shades on the GPU through ``artalk_render_*``
(``include/artalk_hip.h``, ``csrc/render.hip``).  What it computes is written out in DESIGN.md ("Mesh renderer"); parity with
pytorch3d itself is unpinned.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import capi


class RenderMesh:
    def __init__(self, image_size, obj_filename=None, faces=None, scale=1.0, n_verts=None):
        """Arguments of the reference class, plus ``n_verts``: the vertex count the faces index into.  Without it the device
        object is created on the first ``forward``, from the vertices it is given."""
        if int(image_size) != image_size:
            # the reference resizes to ``ori_size`` at the end (mode='area'); only the identity resize is built
            raise ValueError(f"image_size must be an integer, got {image_size!r}")
        if not 1 <= int(image_size) <= 16384:
            raise ValueError(f"image_size must be in 1..16384, got {image_size!r}")
        self.ori_size = image_size
        self.image_size = int(image_size)
        self.scale = float(scale)
        if obj_filename is not None:
            raise NotImplementedError("loading an .obj needs pytorch3d.io.load_obj; pass faces= (FLAMEModel.get_faces())")
        if faces is None:
            raise NotImplementedError("Must have faces.")
        if isinstance(faces, torch.Tensor):
            self.faces = faces
            faces = faces.detach().cpu().numpy()
        else:
            faces = np.asarray(faces)
            self.faces = torch.tensor(faces.astype(np.int32))
        if faces.ndim != 2 or faces.shape[1] != 3:
            raise ValueError(f"faces must be (F, 3), got {tuple(faces.shape)}")
        self._faces32 = np.ascontiguousarray(faces.astype(np.int32))
        self.n_verts = None
        self.slab_frames = 0          # frames per pass over the per-pixel key buffer; 0 = the library's default
        self._h = None
        self._device = None
        if n_verts is not None:
            self._check(int(n_verts))
            self.n_verts = int(n_verts)

    def _check(self, n_verts):
        """The refusals of artalk_render_create, from the library itself (host only: no device is touched for a refusal)."""
        if n_verts <= 0 or self._faces32.shape[0] == 0 or self._faces32.min() < 0 or self._faces32.max() >= n_verts:
            self._create(n_verts, 0)      # raises with the library's message

    def _create(self, n_verts, device_index):
        L = capi.lib()
        h = C.c_void_p()
        f = self._faces32
        rc = L.artalk_render_create(int(device_index), int(n_verts), int(f.shape[0]), f.ctypes.data_as(C.c_void_p), self.image_size,
                                    self.scale, C.byref(h))
        if rc != capi.OK:
            raise ValueError("artalk_render_create failed: " + L.artalk_render_last_error(None).decode())
        return h

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None:
                capi.lib().artalk_render_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def to(self, device):
        return self

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    @torch.no_grad()
    def forward(self, vertices, cameras=None, transform_matrix=None, focal_length=None, return_pix_to_face=False):
        """renderer_utils.py:55-85: vertices (N, V, 3) -> (images * 255 (N, 3, S, S), alpha (N, 1, S, S)), all N frames in one call.
        ``transform_matrix``: (3, 4), (1, 3, 4), or (N, 3, 4) with one camera per frame; ``focal_length`` defaults to 12 as for the
        default camera.  ``return_pix_to_face=True`` appends the (N, S, S) int32 face index per pixel (-1: background)."""
        if cameras is not None:
            raise NotImplementedError("cameras= is a pytorch3d object; pass transform_matrix= and focal_length=")
        if not isinstance(vertices, torch.Tensor) or vertices.dim() != 3 or vertices.shape[-1] != 3:
            raise ValueError("vertices must be a (N, V, 3) tensor")
        if not vertices.is_cuda:
            raise RuntimeError("RenderMesh renders on the GPU: vertices must be a CUDA tensor (there is no CPU fallback)")
        n, V = int(vertices.shape[0]), int(vertices.shape[1])
        if self.n_verts is not None and V != self.n_verts:
            raise ValueError(f"vertices have {V} points, the renderer was built for {self.n_verts}")
        mats = None
        if transform_matrix is not None:
            mats = torch.as_tensor(transform_matrix).detach().float().cpu().reshape(-1, 3, 4).contiguous()
            if mats.shape[0] not in (1, n):
                raise ValueError(f"transform_matrix must hold 1 or {n} cameras, got {mats.shape[0]}")
        focal = 0.0 if focal_length is None else float(torch.as_tensor(focal_length).reshape(-1)[0])
        dev = vertices.device
        if self._h is None:
            self._h = self._create(V, dev.index or 0)
            self.n_verts, self._device = V, dev
        elif dev != self._device:
            raise RuntimeError(f"the renderer lives on {self._device}, vertices on {dev}")
        L = capi.lib()
        if L.artalk_render_set_slab(self._h, int(self.slab_frames)) < 0:
            raise ValueError("artalk_render_set_slab failed: " + L.artalk_render_last_error(self._h).decode())
        S = self.image_size
        verts = vertices.float().contiguous()
        rgb = torch.empty(n, 3, S, S, dtype=torch.float32, device=dev)
        alpha = torch.empty(n, 1, S, S, dtype=torch.float32, device=dev)
        p2f = torch.empty(n, S, S, dtype=torch.int32, device=dev) if return_pix_to_face else None
        with torch.cuda.device(dev):
            if mats is None or mats.shape[0] == 1:
                calls = [(0, n, None if mats is None else mats[0])]
            else:
                calls = [(i, 1, mats[i]) for i in range(n)]
            for t0, cnt, m in calls:
                if cnt == 0:
                    continue
                rc = L.artalk_render_mesh(self._h, capi.ptr(verts[t0:]), cnt, capi.ptr(m), focal, capi.ptr(rgb[t0:]), capi.ptr(alpha[t0:]),
                                          None if p2f is None else capi.ptr(p2f[t0:]), capi.current_stream_ptr())
                if rc != capi.OK:
                    raise RuntimeError("artalk_render_mesh failed: " + L.artalk_render_last_error(self._h).decode())
        return (rgb, alpha, p2f) if return_pix_to_face else (rgb, alpha)
