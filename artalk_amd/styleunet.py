"""Device stand-in for the reference's ``StyleUNet`` (``app/GAGAvatar/modules/style_unet.py``), the upsampler that turns the
32-channel splat image of the GAGAvatar head into RGB: a U-Net encoder whose up path feeds SFT conditions into a StyleGAN2 decoder.
Forward only, exact fp32 by default (``set_precision``: the convolutions in bf16x3 or bf16), all frames of a call in one library call on
top of ``artalk_styleunet_*`` (``include/artalk_hip.h``, ``csrc/styleunet.hip``, ``csrc/styleunet_bf16.hip``).  What is computed is
written out in DESIGN.md ("StyleUNet upsampler").  Only synthetic weights are checked: parity on real GAGAvatar checkpoints is
unpinned.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import capi
from ._intake import load_tensors
from .weights import _rng

UNET_CHANNELS = {4: 256, 8: 256, 16: 256, 32: 256, 64: 128, 128: 64, 256: 32, 512: 16, 1024: 8}
DECODER_CHANNELS = {s: 2 * c for s, c in UNET_CHANNELS.items()}
STYLE_FEAT, NUM_MLP = 512, 8
PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16": 2}      # the modes of artalk_styleunet_set_precision


def _check_size(out_size):
    if not isinstance(out_size, int) or out_size < 8 or out_size > 1024 or out_size & (out_size - 1):
        raise ValueError(f"out_size must be a power of two in 8..1024, got {out_size!r}")
    return int(math.log2(out_size))


def num_noise_layers(out_size):
    return (_check_size(out_size) - 2) * 2 + 1


def noise_resolution(layer):
    return 2 ** ((layer + 5) // 2)


def state_dict_manifest(out_size, in_dim=32, out_dim=3):
    """[(name, shape)] in the order of the reference module's ``state_dict()`` (in_size == out_size)."""
    log_size = _check_size(out_size)
    ch, dch, F = UNET_CHANNELS, DECODER_CHANNELS, STYLE_FEAT
    m = []

    def conv(name, cin, cout, k, bias=True):
        m.append((name + ".weight", (cout, cin, k, k)))
        if bias:
            m.append((name + ".bias", (cout,)))

    def resblock(name, cin, cout):
        conv(name + ".conv1", cin, cin, 3)
        conv(name + ".conv2", cin, cout, 3)
        conv(name + ".skip", cin, cout, 1, bias=False)

    def modconv(name, cin, cout, k):
        m.append((name + ".weight", (1, cout, cin, k, k)))
        m.append((name + ".modulation.weight", (cin, F)))
        m.append((name + ".modulation.bias", (cin,)))

    def styleconv(name, cin, cout):
        m.append((name + ".weight", (1,)))
        m.append((name + ".bias", (1, cout, 1, 1)))
        modconv(name + ".modulated_conv", cin, cout, 3)

    def torgb(name, cin):
        m.append((name + ".bias", (1, out_dim, 1, 1)))
        modconv(name + ".modulated_conv", cin, out_dim, 1)

    conv("conv_body_first", in_dim, ch[out_size], 1)
    c = ch[out_size]
    for j, i in enumerate(range(log_size, 2, -1)):
        resblock(f"conv_body_down.{j}", c, ch[2 ** (i - 1)])
        c = ch[2 ** (i - 1)]
    conv("final_conv", c, ch[4], 3)
    c = ch[4]
    for j, i in enumerate(range(3, log_size + 1)):
        resblock(f"conv_body_up.{j}", c, ch[2 ** i])
        c = ch[2 ** i]
    for j, i in enumerate(range(3, log_size + 1)):
        conv(f"toRGB.{j}", ch[2 ** i], 3, 1)
    m.append(("final_linear.weight", (F, ch[4] * 16)))
    m.append(("final_linear.bias", (F,)))
    d = "stylegan_decoder."
    for j in range(NUM_MLP):
        m.append((d + f"style_mlp.{2 * j + 1}.weight", (F, F)))
        m.append((d + f"style_mlp.{2 * j + 1}.bias", (F,)))
    m.append((d + "constant_input.weight", (1, dch[4], 4, 4)))
    styleconv(d + "style_conv1", dch[4], dch[4])
    torgb(d + "to_rgb1", dch[4])
    c = dch[4]
    for j, i in enumerate(range(3, log_size + 1)):
        styleconv(d + f"style_convs.{2 * j}", c, dch[2 ** i])
        styleconv(d + f"style_convs.{2 * j + 1}", dch[2 ** i], dch[2 ** i])
        c = dch[2 ** i]
    for j, i in enumerate(range(3, log_size + 1)):
        torgb(d + f"to_rgbs.{j}", dch[2 ** i])
    for layer in range((log_size - 2) * 2 + 1):
        r = noise_resolution(layer)
        m.append((d + f"noises.noise{layer}", (1, 1, r, r)))
    for which in ("condition_scale", "condition_shift"):
        for j, i in enumerate(range(3, log_size + 1)):
            conv(f"{which}.{j}.0", ch[2 ** i], ch[2 ** i], 3)
            conv(f"{which}.{j}.2", ch[2 ** i], 2 * ch[2 ** i], 3)
    return m


def _is_noise_strength(name, shape):
    return tuple(shape) == (1,) and name.endswith(".weight")


def synth_state_dict(out_size, in_dim=32, out_dim=3, seed=0):
    """Name-keyed deterministic weights: conv / Linear weights N(0, 1) / sqrt(fan_in), biases N(0, 0.1), modulation biases
    1 + N(0, 0.1), noise strengths N(0, 0.1) (the default init of 0 would hide the noise path), noise buffers and the constant
    input N(0, 1)."""
    sd = {}
    for name, shape in state_dict_manifest(out_size, in_dim, out_dim):
        g = _rng("styleunet." + name, seed)
        z = g.standard_normal(int(np.prod(shape)), dtype=np.float32)
        if ".noises." in name or name.endswith("constant_input.weight"):
            a = z
        elif _is_noise_strength(name, shape):
            a = z * np.float32(0.1)
        elif name.endswith("modulation.bias"):
            a = np.float32(1.0) + z * np.float32(0.1)
        elif name.endswith(".bias"):
            a = z * np.float32(0.1)
        else:
            fan_in = int(np.prod(shape[-3:])) if len(shape) >= 4 else int(shape[-1])
            a = z * np.float32(1.0 / math.sqrt(fan_in))
        sd[name] = torch.from_numpy(a.reshape(shape).copy())
    return sd


class StyleUNet:
    """``StyleUNet(in_size, out_size, in_dim, out_dim)`` with the reference's constructor arguments, ``load_state_dict`` and
    ``forward(x, randomize_noise=True)``: (B, in_dim, S, S) -> (B, out_dim, S, S) on the device."""

    def __init__(self, in_size, out_size, in_dim, out_dim, num_style_feat=512, num_mlp=8, activation=True):
        if in_size != out_size:
            raise NotImplementedError(f"in_size ({in_size}) != out_size ({out_size}) is not built (the GAGAvatar head uses 512 / 512)")
        if num_style_feat != STYLE_FEAT or num_mlp != NUM_MLP:
            raise NotImplementedError(f"only num_style_feat={STYLE_FEAT} and num_mlp={NUM_MLP} (the reference's defaults) are built")
        _check_size(out_size)
        if in_dim < 1 or out_dim < 1:
            raise ValueError("in_dim and out_dim must be positive")
        self.in_size, self.out_size, self.in_dim, self.out_dim = int(in_size), int(out_size), int(in_dim), int(out_dim)
        self.activation = bool(activation)
        self.num_layers = num_noise_layers(out_size)
        self._device = None
        self._h = None
        self._loaded = False
        self._pending = None
        self._precision = "f32"

    # ---- precision of the convolutions ----
    @property
    def precision(self):
        return self._precision

    def set_precision(self, name):
        """``"f32"`` (the default, exact fp32), ``"bf16x3"`` (three bf16 MFMA products per operand pair: within a few 1e-5 of fp32 on the
        synthetic weights) or ``"bf16"`` (one product: a throughput mode, grey levels off).  DESIGN.md section 5, "Precision modes".
        Accepted at any time: before the weights are on the device it is remembered, and it survives ``load_state_dict``."""
        if name not in PRECISIONS:
            raise ValueError(f"precision must be one of {', '.join(PRECISIONS)}, got {name!r}")
        if self._h is not None:
            self._apply_precision(name)
        self._precision = name
        return self

    def _apply_precision(self, name):
        if capi.lib().artalk_styleunet_set_precision(self._h, PRECISIONS[name]) != capi.OK:
            raise RuntimeError("artalk_styleunet_set_precision failed: " + self._err())

    # ---- torch.nn.Module look-alikes ----
    def eval(self):
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("StyleUNet runs on the GPU only (there is no CPU fallback)")
        if self._h is not None and self._loaded and (device.index or 0) != (self._device.index or 0):
            raise RuntimeError("the weights live on " + str(self._device) + ": load them again after moving")
        self._device = device
        if self._pending is not None:
            sd, self._pending = self._pending, None
            self.load_state_dict(sd)
        return self

    def cuda(self):
        return self.to("cuda")

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    def state_dict_manifest(self):
        return state_dict_manifest(self.out_size, self.in_dim, self.out_dim)

    def _err(self):
        return capi.lib().artalk_styleunet_last_error(self._h).decode()

    def __del__(self):
        try:
            if self._h is not None:
                capi.lib().artalk_styleunet_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def load_state_dict(self, state_dict, strict=True):
        assert strict, "only strict=True is supported"
        if self._device is None:      # the reference loads on the CPU and moves afterwards: keep the dict until .to(device)
            self._check_names(state_dict)
            self._pending = dict(state_dict)
            return self
        L = capi.lib()
        if self._h is not None:
            L.artalk_styleunet_destroy(self._h)
            self._h, self._loaded = None, False
        h = C.c_void_p()
        rc = L.artalk_styleunet_create(self._device.index or 0, self.in_dim, self.out_dim, self.out_size, C.byref(h))
        if rc != capi.OK:
            raise RuntimeError("artalk_styleunet_create failed: " + L.artalk_styleunet_last_error(None).decode())
        self._h = h
        self._apply_precision(self._precision)      # host only before finalize: the mode is remembered, finalize packs for it
        errors = load_tensors(L, "styleunet", self._h, state_dict.items())
        if errors:
            raise RuntimeError("Error(s) in loading state_dict for StyleUNet:\n\t" + "\n\t".join(errors[:12]))
        self._loaded = True
        return self

    def _check_names(self, state_dict):
        want = dict(self.state_dict_manifest())
        errors = [f"Unexpected key in state_dict: {k}" for k in state_dict if k not in want]
        errors += [f"size mismatch for {k}" for k, v in state_dict.items() if k in want and tuple(v.shape) != tuple(want[k])]
        missing = [k for k in want if k not in state_dict]
        if missing:
            errors.append("Missing key(s) in state_dict: " + ", ".join(missing[:8]) + (", ..." if len(missing) > 8 else ""))
        if errors:
            raise RuntimeError("Error(s) in loading state_dict for StyleUNet:\n\t" + "\n\t".join(errors[:12]))

    def set_slab(self, frames):
        """Frames per pass over the workspace (0: the default chosen at create time); returns the slab in force."""
        if self._h is None:
            raise RuntimeError("load_state_dict on a device first")
        rc = capi.lib().artalk_styleunet_set_slab(self._h, int(frames))
        if rc < 0:
            raise ValueError("artalk_styleunet_set_slab refused: " + self._err())
        return rc

    @torch.no_grad()
    def forward(self, x, randomize_noise=True, noise=None):
        """x (B, in_dim, S, S) fp32 on the device -> (B, out_dim, S, S).  ``randomize_noise=True`` draws one (B, 1, h, w) normal image
        per style conv with torch's generator, as the reference does; ``False`` uses the stored ``noises.noise{i}`` buffers.
        ``noise`` (a list of ``num_layers`` device tensors, (B or 1, 1, h, w)) overrides both."""
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError("x must be a (B, C, H, W) tensor")
        if x.shape[-1] != self.out_size or x.shape[-2] != self.out_size:
            raise NotImplementedError(f"x is {x.shape[-2]} x {x.shape[-1]}: only inputs of out_size ({self.out_size}) are built")
        if not x.is_cuda:
            raise RuntimeError("StyleUNet runs on the GPU: x must be a CUDA tensor (there is no CPU fallback)")
        if not self._loaded:
            raise RuntimeError("StyleUNet.forward before load_state_dict on a device")
        if x.shape[1] != self.in_dim:
            raise ValueError(f"x has {x.shape[1]} channels, the module {self.in_dim}")
        if (x.device.index or 0) != (self._device.index or 0):
            raise RuntimeError(f"x lives on {x.device}, the weights on {self._device}")
        x = x.detach().float().contiguous()
        B = int(x.shape[0])
        out = torch.empty(B, self.out_dim, self.out_size, self.out_size, dtype=torch.float32, device=x.device)
        if B == 0:
            return out
        L = capi.lib()
        with torch.cuda.device(x.device):
            if noise is None and randomize_noise:
                noise = [torch.empty(B, 1, noise_resolution(i), noise_resolution(i), device=x.device).normal_()
                         for i in range(self.num_layers)]
            ptrs = strides = None
            if noise is not None:
                if len(noise) != self.num_layers:
                    raise ValueError(f"noise must hold {self.num_layers} tensors")
                keep = []
                for i, n in enumerate(noise):
                    r = noise_resolution(i)
                    if not n.is_cuda or tuple(n.shape[1:]) != (1, r, r) or n.shape[0] not in (1, B):
                        raise ValueError(f"noise[{i}] must be a CUDA tensor of shape (1 or {B}, 1, {r}, {r})")
                    keep.append(n.detach().float().contiguous())
                ptrs = (C.c_void_p * self.num_layers)(*[t.data_ptr() for t in keep])
                strides = (C.c_int64 * self.num_layers)(*[0 if t.shape[0] == 1 else t.shape[2] * t.shape[3] for t in keep])
            rc = L.artalk_styleunet_forward(self._h, capi.ptr(x), B, ptrs, strides, int(self.activation), capi.ptr(out),
                                            capi.current_stream_ptr())
        if rc == capi.EINVAL:
            raise ValueError("artalk_styleunet_forward refused: " + self._err())
        if rc != capi.OK:
            raise RuntimeError("artalk_styleunet_forward failed: " + self._err())
        return out
