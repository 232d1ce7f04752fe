"""Device stand-in for the reference's ``DINOBase`` (``app/GAGAvatar/modules/dino_base.py``, ``models.py:63-110``): the tracked photo of
an identity comes in, the two features ``artalk_amd.gsgen.GSGenerators.build_avatar`` takes go out - the feature plane
``(output_dim, 8 grid, 8 grid)`` and the global vector ``(vit_dim,)`` - from one library call on top of ``artalk_dino_*``
(``include/artalk_hip.h``, ``csrc/dino.hip``).  What is computed is written out in DESIGN.md section 5 ("DINO features").  Forward only,
exact fp32, one image per call.

Only synthetic weights are checked.  Unpinned: parity on the real ``GAGAvatar.pt``, the upstream DINOv2 checkpoint's key names (taken
from the published module layout, whose source was not at hand) and torchvision's resize (its tensor path,
``F.interpolate(mode="bilinear", align_corners=False, antialias=True)``, is the definition used).  Not built: position-embedding
interpolation, register tokens, batches, lower-precision modes, ``only_global`` / ``output_size``.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import capi
from ._intake import load_tensors
from .weights import _rng

PATCH, HIDDEN, PROJ = 14, 256, (256, 512, 1024, 1024)
PREFIX = "base_model."
IGNORED_PREFIXES = ("head_base", "gs_generator_", "upsampler.", "percep_loss", "harmo_encoder.")      # of a whole GAGAvatar checkpoint
STAGES = ("gemm", "attention", "conv", "rest")


def _check_dims(output_dim, vit_dim, depth, heads, grid):
    for name, v in (("output_dim", output_dim), ("vit_dim", vit_dim), ("depth", depth), ("heads", heads), ("grid", grid)):
        if not isinstance(v, int) or v < 1:
            raise ValueError(f"{name} must be a positive int, got {v!r}")
    if depth < 4:
        raise ValueError(f"depth must be at least 4 (the head taps the last four blocks), got {depth}")
    if vit_dim % heads or vit_dim // heads not in (64, 32):
        raise ValueError(f"the head width vit_dim / heads must be 64 or 32, got {vit_dim} / {heads}")
    if vit_dim % 32 or vit_dim > 4096:
        raise ValueError(f"vit_dim must be a multiple of 32 up to 4096, got {vit_dim}")
    if grid < 2 or grid > 64:
        raise ValueError(f"grid must be in 2..64, got {grid}")
    if output_dim > 1024:
        raise ValueError(f"output_dim must be at most 1024, got {output_dim}")


def level_sizes(grid):
    """Side of the four pyramid levels, fine to coarse: 4 g, 2 g, g, (g - 1) // 2 + 1 (37 -> 148, 74, 37, 19)."""
    return 4 * grid, 2 * grid, grid, (grid - 1) // 2 + 1


def state_dict_manifest(output_dim=256, vit_dim=768, depth=12, heads=12, grid=37):
    """[(name, shape)] of the module, in the order of the reference module's ``state_dict()`` (without the ``base_model.`` prefix)."""
    _check_dims(output_dim, vit_dim, depth, heads, grid)
    D, G = vit_dim, grid * grid
    m = [("dino_model.cls_token", (1, 1, D)), ("dino_model.pos_embed", (1, 1 + G, D)), ("dino_model.mask_token", (1, D)),
         ("dino_model.patch_embed.proj.weight", (D, 3, PATCH, PATCH)), ("dino_model.patch_embed.proj.bias", (D,))]

    def wb(name, shape, bias=True):
        m.append((name + ".weight", shape))
        if bias:
            m.append((name + ".bias", (shape[0],)))

    for i in range(depth):
        b = f"dino_model.blocks.{i}."
        wb(b + "norm1", (D,))
        wb(b + "attn.qkv", (3 * D, D))
        wb(b + "attn.proj", (D, D))
        m.append((b + "ls1.gamma", (D,)))
        wb(b + "norm2", (D,))
        wb(b + "mlp.fc1", (4 * D, D))
        wb(b + "mlp.fc2", (D, 4 * D))
        m.append((b + "ls2.gamma", (D,)))
    wb("dino_model.norm", (D,))
    for i, c in enumerate(PROJ):
        wb(f"projects.{i}", (c, D, 1, 1))
    wb("resize_layers.0", (PROJ[0], PROJ[0], 4, 4))
    wb("resize_layers.1", (PROJ[1], PROJ[1], 2, 2))
    wb("resize_layers.3", (PROJ[3], PROJ[3], 3, 3))
    for i, c in enumerate(PROJ):
        wb(f"layer_rn.{i}", (HIDDEN, c + 3, 3, 3), bias=False)
    for i in range(4):
        wb(f"refinenet.{i}.out_conv", (HIDDEN, HIDDEN, 1, 1))
        for u in (1, 2):
            for c in (1, 2):
                wb(f"refinenet.{i}.resConfUnit{u}.conv{c}", (HIDDEN, HIDDEN, 3, 3))
    wb("output_conv", (output_dim, HIDDEN, 3, 3))
    return m


def synth_state_dict(output_dim=256, vit_dim=768, depth=12, heads=12, grid=37, seed=0):
    """Name-keyed deterministic weights that keep taps and outputs of order 1: matrices and kernels N(0, 1) * sqrt(2 / fan_in) (the second
    conv of a residual unit and the 1 x 1 ``out_conv`` at half of that, so that the four fusion stages do not pile up), LayerNorm weights
    and LayerScale gammas 1 + N(0, 0.1), biases N(0, 0.1), ``pos_embed`` / ``cls_token`` / ``mask_token`` N(0, 0.5)."""
    sd = {}
    for name, shape in state_dict_manifest(output_dim, vit_dim, depth, heads, grid):
        z = _rng("dino." + name, seed).standard_normal(int(np.prod(shape)), dtype=np.float32)
        if name.endswith(("cls_token", "pos_embed", "mask_token")):
            a = z * np.float32(0.5)
        elif name.endswith(".gamma") or (name.endswith(".weight") and len(shape) == 1):
            a = np.float32(1.0) + z * np.float32(0.1)
        elif name.endswith(".bias"):
            a = z * np.float32(0.1)
        else:
            if name.startswith("resize_layers.0") or name.startswith("resize_layers.1"):
                fan_in = shape[0]      # ConvTranspose2d [Cin][Cout][k][k] with k = s: one tap per output pixel
            else:
                fan_in = int(np.prod(shape[1:]))
            scale = math.sqrt(2.0 / fan_in)
            if name.endswith("conv2.weight") or "out_conv" in name:
                scale *= 0.5
            a = z * np.float32(scale)
        sd[name] = torch.from_numpy(a.reshape(shape).copy())
    return sd


class DINOBase:
    """``DINOBase(output_dim=256, vit_dim=768, depth=12, heads=12, grid=37, device="cuda")``: ``base_model`` of the reference's
    ``GAGAvatar``.  The device is first touched by ``load_state_dict``."""

    def __init__(self, output_dim=256, vit_dim=768, depth=12, heads=12, grid=37, device="cuda"):
        _check_dims(output_dim, vit_dim, depth, heads, grid)
        self.output_dim, self.vit_dim, self.depth, self.heads, self.grid = output_dim, vit_dim, depth, heads, grid
        self.image_size, self.plane = PATCH * grid, 8 * grid
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DINOBase runs on the GPU only (there is no CPU fallback)")
        self._h = None

    def _dims(self):
        return self.output_dim, self.vit_dim, self.depth, self.heads, self.grid

    def state_dict_manifest(self):
        return state_dict_manifest(*self._dims())

    def synth_state_dict(self, seed=0):
        return synth_state_dict(*self._dims(), seed=seed)

    def _err(self):
        return capi.lib().artalk_dino_last_error(self._h).decode()

    def __del__(self):
        try:
            if self._h is not None:
                capi.lib().artalk_dino_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def load_state_dict(self, state_dict, strict=True):
        """Takes the module's own dict or the whole GAGAvatar checkpoint's ``model`` dict: of the latter ``base_model.*`` is used and
        ``head_base``, ``gs_generator_*``, ``upsampler.*``, ``percep_loss*`` and ``harmo_encoder.*`` are ignored.  Other unknown keys,
        missing keys and wrong shapes raise with torch's wording."""
        assert strict, "only strict=True is supported"
        whole = any(k.startswith(PREFIX) for k in state_dict)
        L = capi.lib()
        h = C.c_void_p()
        if L.artalk_dino_create(self.device.index or 0, self.vit_dim, self.depth, self.heads, self.grid, self.output_dim, C.byref(h)) != capi.OK:
            raise RuntimeError("artalk_dino_create failed: " + L.artalk_dino_last_error(None).decode())
        errors = []

        def own():      # of the whole checkpoint: the module's keys, their prefix stripped
            for key, val in state_dict.items():
                if not whole:
                    yield key, val
                elif key.startswith(PREFIX):
                    yield key[len(PREFIX):], val
                elif not key.startswith(IGNORED_PREFIXES):
                    errors.append("Unexpected key in state_dict: " + key)
        try:
            load_tensors(L, "dino", h, own(), errors)
            if errors:
                raise RuntimeError("Error(s) in loading state_dict for DINOBase:\n\t" + "\n\t".join(errors[:12]))
        except BaseException:
            L.artalk_dino_destroy(h)
            raise
        if self._h is not None:
            L.artalk_dino_destroy(self._h)
        self._h = h
        return self

    def _loaded(self):
        if self._h is None:
            raise RuntimeError("DINOBase before load_state_dict")

    @torch.no_grad()
    def prepare_image(self, image, size=None):
        """``image`` (3, h, w) in [0, 1], on the CPU or the device, a leading batch axis of 1 allowed -> (1, 3, S, S) on the device,
        S = 14 grid: the reference's ``torchvision.transforms.functional.resize(image, (518, 518), antialias=True)``.  ``size``: None
        or S (another size would need interpolated position embeddings, which are not built)."""
        self._loaded()
        S = self.image_size
        if size is not None and tuple(np.atleast_1d(size).tolist()) not in ((S,), (S, S)):
            raise ValueError(f"size must be {S} (14 x grid; position embeddings are not interpolated), got {size!r}")
        if not isinstance(image, torch.Tensor):
            image = torch.as_tensor(np.asarray(image))
        if image.dim() == 4 and image.shape[0] == 1:
            image = image[0]
        if image.dim() != 3 or image.shape[0] != 3:
            raise ValueError(f"image must be (3, h, w) (or with a leading batch axis of 1), got {tuple(image.shape)}")
        if image.is_cuda and (image.device.index or 0) != (self.device.index or 0):
            raise RuntimeError(f"image lives on {image.device}, the weights on {self.device}")
        image = image.detach().float().contiguous()
        dev = torch.device("cuda", self.device.index or 0)
        out = torch.empty(1, 3, S, S, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = capi.lib().artalk_dino_prepare_image(self._h, capi.ptr(image), int(image.shape[1]), int(image.shape[2]), capi.ptr(out),
                                                      capi.current_stream_ptr())
        if rc == capi.EINVAL:
            raise ValueError("artalk_dino_prepare_image refused: " + self._err())
        if rc != capi.OK:
            raise RuntimeError("artalk_dino_prepare_image failed: " + self._err())
        return out

    @torch.no_grad()
    def forward(self, images):
        """``images`` (1, 3, S, S) or (3, S, S) in [0, 1] on the device -> (f_feature0 (1, output_dim, P, P), f_feature1 (1, vit_dim)),
        P = 8 grid, on the device."""
        self._loaded()
        if not isinstance(images, torch.Tensor):
            raise ValueError("images must be a tensor")
        if not images.is_cuda:
            raise RuntimeError("DINOBase runs on the GPU: images must be a CUDA tensor (there is no CPU fallback)")
        if (images.device.index or 0) != (self.device.index or 0):
            raise RuntimeError(f"images lives on {images.device}, the weights on {self.device}")
        if images.dim() == 4:
            if images.shape[0] != 1:
                raise ValueError(f"one image per call: the batch axis must be 1, got {images.shape[0]}")
            images = images[0]
        if images.dim() != 3 or images.shape[0] != 3:
            raise ValueError(f"images must be (1, 3, S, S) or (3, S, S), got {tuple(images.shape)}")
        x = images.detach().float().contiguous()
        P = self.plane
        f0 = torch.empty(1, self.output_dim, P, P, dtype=torch.float32, device=x.device)
        f1 = torch.empty(1, self.vit_dim, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            rc = capi.lib().artalk_dino_forward(self._h, capi.ptr(x), int(x.shape[1]), int(x.shape[2]), capi.ptr(f0), capi.ptr(f1),
                                                capi.current_stream_ptr())
        if rc == capi.EINVAL:
            raise ValueError("artalk_dino_forward refused: " + self._err())
        if rc != capi.OK:
            raise RuntimeError("artalk_dino_forward failed: " + self._err())
        return f0, f1

    __call__ = forward

    def read(self, what):
        """An intermediate of the last ``forward`` on the current stream: ``tap0`` .. ``tap3`` (grid, grid, vit_dim), the normed patch
        tokens of the last four blocks; ``rn0`` .. ``rn3`` (H, H, 256), the ``layer_rn`` outputs, channels last."""
        self._loaded()
        if what[:3] == "tap":
            shape = (self.grid, self.grid, self.vit_dim)
        elif what[:2] == "rn" and what[2:] in ("0", "1", "2", "3"):
            H = level_sizes(self.grid)[int(what[2:])]
            shape = (H, H, HIDDEN)
        else:
            raise ValueError("what must be tap0..tap3 or rn0..rn3")
        dev = torch.device("cuda", self.device.index or 0)
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = capi.lib().artalk_dino_read(self._h, what.encode(), capi.ptr(out), out.numel(), capi.current_stream_ptr())
        if rc != capi.OK:
            raise ValueError("artalk_dino_read refused: " + self._err())
        return out

    def set_timing(self, enable):
        self._loaded()
        capi.lib().artalk_dino_set_timing(self._h, int(bool(enable)))

    def timing(self):
        """({stage: ms}, whole call ms) of the last ``forward`` made with timing on; the stages are ``STAGES``."""
        self._loaded()
        st, total = (C.c_double * len(STAGES))(), C.c_double()
        capi.lib().artalk_dino_get_timing(self._h, st, C.byref(total))
        return dict(zip(STAGES, st)), total.value
