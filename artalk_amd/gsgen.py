"""Device stand-in for the Gaussian generators of the reference's ``GAGAvatar`` (``app/GAGAvatar/models.py:65-87``, ``141-233``,
``236-252``): ``LinearGSGenerator``, the two ``ConvGSGenerator``s, ``build_points_planes``, the direction encoding and the assembly of
``_gs_params``.  The two DINO features of an identity come in, the avatar dict ``artalk_amd.gaga.GAGAvatar`` takes goes out, from one
library call on top of ``artalk_gsgen_*`` (``include/artalk_hip.h``, ``csrc/gsgen.hip``).  What is computed is written out in DESIGN.md
section 5 ("Gaussian generators").  Forward only, exact fp32, one avatar per call.

DINOv2 and its DPT head, which make the two features, are ``artalk_amd.dino.DINOBase``.  Only synthetic weights are checked: parity on real GAGAvatar
checkpoints is unpinned, and so is the reading of pytorch3d's ``HarmonicEmbedding`` (pytorch3d was not at hand).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import capi
from ._intake import load_tensors
from .gaga import AVATAR_FIELDS
from .weights import _rng

DIR_DIM, CONV_OUT, HEAD_HIDDEN = 27, 41, 128
HEADS = (("color", 32), ("opacity", 1), ("scale", 3), ("rotation", 4))
IGNORED_PREFIXES = ("base_model.", "upsampler.", "percep_loss", "harmo_encoder.")      # of a whole GAGAvatar checkpoint


def _check_dims(n_verts, head_dim, global_dim, feat_dim, plane):
    for name, v in (("n_verts", n_verts), ("head_dim", head_dim), ("global_dim", global_dim), ("feat_dim", feat_dim), ("plane", plane)):
        if not isinstance(v, int) or v < 1:
            raise ValueError(f"{name} must be a positive int, got {v!r}")
    if (head_dim + global_dim) % 4:
        raise ValueError(f"head_dim + global_dim must be a multiple of 4, got {head_dim} + {global_dim}")
    if feat_dim % 2:
        raise ValueError(f"feat_dim must be even, got {feat_dim}")
    if plane < 3:
        raise ValueError(f"plane must be at least 3, got {plane}")


def state_dict_manifest(n_verts=5023, head_dim=256, global_dim=768, feat_dim=256, plane=296):
    """[(name, shape)] of ``head_base`` and the three generators, in the order of the reference module's ``state_dict()``."""
    _check_dims(n_verts, head_dim, global_dim, feat_dim, plane)
    hid, chid = (head_dim + global_dim) // 4, feat_dim // 2
    m = [("head_base", (n_verts, head_dim))]

    def linear(name, cin, cout):
        m.append((name + ".weight", (cout, cin)))
        m.append((name + ".bias", (cout,)))

    def conv(name, cin, cout, k):
        m.append((name + ".weight", (cout, cin, k, k)))
        m.append((name + ".bias", (cout,)))

    g = "gs_generator_g."
    for i in range(4):
        linear(g + f"feature_layers.{2 * i}", hid if i else head_dim + global_dim, hid)
    for head, width in HEADS:
        linear(g + f"{head}_layers.0", hid + DIR_DIM, HEAD_HIDDEN)
        linear(g + f"{head}_layers.2", HEAD_HIDDEN, width)
    for l in range(2):
        n = f"gs_generator_l{l}.gaussian_conv."
        conv(n + "0", feat_dim + DIR_DIM, chid, 3)
        conv(n + "2", chid, chid, 3)
        conv(n + "4", chid, chid, 3)
        conv(n + "6", chid, CONV_OUT, 1)
    return m


def synth_state_dict(n_verts=5023, head_dim=256, global_dim=768, feat_dim=256, plane=296, seed=0):
    """Name-keyed deterministic weights: ``head_base`` N(0, 1) (its init in the reference), weights N(0, 1) * sqrt(2 / fan_in) (inputs of
    standard deviation 1 keep pre-activations of order 1 through the ReLUs), biases N(0, 0.1)."""
    sd = {}
    for name, shape in state_dict_manifest(n_verts, head_dim, global_dim, feat_dim, plane):
        z = _rng("gsgen." + name, seed).standard_normal(int(np.prod(shape)), dtype=np.float32)
        if name == "head_base":
            a = z
        elif name.endswith(".bias"):
            a = z * np.float32(0.1)
        else:
            a = z * np.float32(math.sqrt(2.0 / int(np.prod(shape[1:]))))
        sd[name] = torch.from_numpy(a.reshape(shape).copy())
    return sd


def planes(transform_matrix, plane=296):
    """``artalk_gsgen_planes`` (host only): the avatar's (3, 4) ``transform_matrix`` -> (plane_points (plane^2, 3), plane_dirs (3,),
    direnc (27,)): ``build_points_planes`` and the harmonic encoding of its direction, evaluated in double and rounded once."""
    tm = torch.as_tensor(transform_matrix).detach().to(dtype=torch.float32, device="cpu")
    if tuple(tm.shape[-2:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"transform_matrix must be (3, 4), got {tuple(tm.shape)}")
    tm = tm.reshape(-1, tm.shape[-2], 4)[0][:3].contiguous()
    pts, d, enc = torch.empty(max(int(plane), 0) ** 2, 3), torch.empty(3), torch.empty(DIR_DIM)
    L = capi.lib()
    if L.artalk_gsgen_planes(capi.ptr(tm), int(plane), capi.ptr(pts), capi.ptr(d), capi.ptr(enc)) != capi.OK:
        raise ValueError("artalk_gsgen_planes refused: " + L.artalk_gsgen_last_error(None).decode())
    return pts, d, enc


class GSGenerators:
    """``GSGenerators(n_verts=5023, head_dim=256, global_dim=768, feat_dim=256, plane=296, device="cuda")``: ``head_base``,
    ``gs_generator_g``, ``gs_generator_l0`` and ``gs_generator_l1`` of the reference's ``GAGAvatar``.  The device is first touched by
    ``load_state_dict``."""

    def __init__(self, n_verts=5023, head_dim=256, global_dim=768, feat_dim=256, plane=296, device="cuda"):
        _check_dims(n_verts, head_dim, global_dim, feat_dim, plane)
        self.n_verts, self.head_dim, self.global_dim, self.feat_dim, self.plane = n_verts, head_dim, global_dim, feat_dim, plane
        self.n_gaussians = n_verts + 2 * plane * plane
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GSGenerators runs on the GPU only (there is no CPU fallback)")
        self._h = None

    def _dims(self):
        return self.n_verts, self.head_dim, self.global_dim, self.feat_dim, self.plane

    def state_dict_manifest(self):
        return state_dict_manifest(*self._dims())

    def synth_state_dict(self, seed=0):
        return synth_state_dict(*self._dims(), seed=seed)

    def planes(self, transform_matrix):
        return planes(transform_matrix, self.plane)

    def _err(self):
        return capi.lib().artalk_gsgen_last_error(self._h).decode()

    def __del__(self):
        try:
            if self._h is not None:
                capi.lib().artalk_gsgen_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def load_state_dict(self, state_dict, strict=True):
        """Takes the generators' own dict or the whole GAGAvatar checkpoint's ``model`` dict: ``head_base`` and ``gs_generator_*`` are
        used; ``base_model.*``, ``upsampler.*``, ``percep_loss*`` and ``harmo_encoder.*`` (a buffer of constants in some pytorch3d
        versions) are ignored.  Other unknown keys, missing keys and wrong shapes raise with torch's wording."""
        assert strict, "only strict=True is supported"
        L = capi.lib()
        h = C.c_void_p()
        if L.artalk_gsgen_create(self.device.index or 0, *self._dims(), C.byref(h)) != capi.OK:
            raise RuntimeError("artalk_gsgen_create failed: " + L.artalk_gsgen_last_error(None).decode())
        try:
            errors = load_tensors(L, "gsgen", h, ((k, v) for k, v in state_dict.items() if not k.startswith(IGNORED_PREFIXES)))
            if errors:
                raise RuntimeError("Error(s) in loading state_dict for GSGenerators:\n\t" + "\n\t".join(errors[:12]))
        except BaseException:
            L.artalk_gsgen_destroy(h)
            raise
        if self._h is not None:
            L.artalk_gsgen_destroy(self._h)
        self._h = h
        return self

    def _feature(self, name, t, shape):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
        if not t.is_cuda:
            raise RuntimeError(f"GSGenerators runs on the GPU: {name} must be a CUDA tensor (there is no CPU fallback)")
        if (t.device.index or 0) != (self.device.index or 0):
            raise RuntimeError(f"{name} lives on {t.device}, the weights on {self.device}")
        if t.dim() == len(shape) + 1 and t.shape[0] == 1:      # the reference's batch axis
            t = t[0]
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape} (or with a leading batch axis of 1), got {tuple(t.shape)}")
        return t.detach().float().contiguous()

    @torch.no_grad()
    def build_avatar(self, f_feature0, f_feature1, transform_matrix, shapecode, device="cpu"):
        """``f_feature0`` (feat_dim, plane, plane) and ``f_feature1`` (global_dim,) on the device - what the reference's ``base_model``
        returns, a leading batch axis of 1 allowed - and the identity's tracked ``transform_matrix`` / ``shapecode`` -> the avatar dict
        ``GAGAvatar`` takes: xyz, colors, opacities, scales, rotations (N rows each), shapecode, transform_matrix.  On the CPU by
        default (``device="cuda"``: the five arrays stay on the device)."""
        P = self.plane
        f0 = self._feature("f_feature0", f_feature0, (self.feat_dim, P, P))
        f1 = self._feature("f_feature1", f_feature1, (self.global_dim,))
        if self._h is None:
            raise RuntimeError("GSGenerators.build_avatar before load_state_dict")
        tm = torch.as_tensor(transform_matrix).detach().to(dtype=torch.float32, device="cpu")
        if tuple(tm.shape[-2:]) not in ((3, 4), (4, 4)):
            raise ValueError(f"transform_matrix must be (3, 4), got {tuple(tm.shape)}")
        tm = tm.reshape(-1, tm.shape[-2], 4)[0][:3].contiguous()
        out = {k: torch.empty(self.n_gaussians, w, dtype=torch.float32, device=f0.device) for k, w in AVATAR_FIELDS.items()}
        with torch.cuda.device(f0.device):
            rc = capi.lib().artalk_gsgen_generate(self._h, capi.ptr(f0), capi.ptr(f1), capi.ptr(tm), *[capi.ptr(out[k]) for k in AVATAR_FIELDS],
                                                  capi.current_stream_ptr())
        if rc == capi.EINVAL:
            raise ValueError("artalk_gsgen_generate refused: " + self._err())
        if rc != capi.OK:
            raise RuntimeError("artalk_gsgen_generate failed: " + self._err())
        if torch.device(device).type != "cuda":
            out = {k: v.cpu() for k, v in out.items()}
        out["shapecode"] = torch.as_tensor(shapecode).detach().to(dtype=torch.float32, device="cpu").reshape(-1).contiguous()
        out["transform_matrix"] = tm
        return out

    def set_timing(self, enable):
        if self._h is None:
            raise RuntimeError("load_state_dict first")
        capi.lib().artalk_gsgen_set_timing(self._h, int(bool(enable)))

    def timing(self):
        """(conv kernel ms, whole call ms) of the last call made with timing on."""
        conv, total = C.c_double(), C.c_double()
        capi.lib().artalk_gsgen_get_timing(self._h, C.byref(conv), C.byref(total))
        return conv.value, total.value
