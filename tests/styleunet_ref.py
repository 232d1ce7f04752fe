"""Torch-CPU restatement of the StyleUNet upsampler from DESIGN.md ("StyleUNet upsampler"), in whatever dtype the input has
(float64 for the oracle, float32 for the e32 yardstick).  ``Variant`` holds one switch per arithmetic choice so that deliberately wrong
variants can be built.  Not a product path: the tests import it, nothing under artalk_amd/ does."""
from dataclasses import dataclass
import math

import torch
import torch.nn.functional as F

from artalk_amd.styleunet import noise_resolution


@dataclass(frozen=True)
class Variant:
    align_corners: bool = False      # True: the resamplers sample with align_corners=True
    gain: bool = True                # False: no sqrt(2) after a style conv
    demod: bool = True               # False: no demodulation
    sft_swapped: bool = False        # True: out * shift + scale
    noise: bool = True               # False: the noise term is dropped
    slope: float = 0.2               # LeakyReLU slope
    rgb_skip_upsampled: bool = True  # False: the to-RGB skip is pixel-repeated instead of bilinearly upsampled


def lrelu(x, slope=0.2):
    return torch.where(x >= 0, x, x * slope)


def _up_axis(x, dim):
    n = x.shape[dim]
    i = torch.arange(n, device=x.device)
    prev, nxt = x.index_select(dim, (i - 1).clamp(min=0)), x.index_select(dim, (i + 1).clamp(max=n - 1))
    even = 0.25 * prev + 0.75 * x      # output 2 i     samples at i - 0.25
    odd = 0.75 * x + 0.25 * nxt        # output 2 i + 1 samples at i + 0.25
    shape = list(x.shape)
    shape[dim] = 2 * n
    return torch.stack([even, odd], dim=dim + 1).reshape(shape)


def resample(x, up, v=Variant()):
    """(B, C, H, W) -> x2 (up) or x0.5 bilinear, align_corners=False: weights 0.25 / 0.75 with edge clamping, or the 2 x 2 mean."""
    if v.align_corners:
        return F.interpolate(x, scale_factor=2 if up else 0.5, mode="bilinear", align_corners=True)
    if up:
        return _up_axis(_up_axis(x, 2), 3)
    return 0.25 * (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])


def conv2d(x, w, in_scale=None, out_scale=None, gain=None, noise=None, noise_weight=None, bias=None, slope=None,
           sft_scale=None, sft_shift=None, residual=None):
    """The conv kernel's contract: x (B, Cin, H, W), w (Cout, Cin, k, k), zero padding k // 2, then in order: per-(sample, Cout) scale,
    gain, + noise_weight * noise (B or 1, 1, H, W), + bias (Cout), LeakyReLU, SFT out * scale + shift, + residual."""
    if in_scale is not None:
        x = x * in_scale[:, :, None, None]
    out = F.conv2d(x, w, padding=w.shape[-1] // 2)
    if out_scale is not None:
        out = out * out_scale[:, :, None, None]
    if gain is not None:
        out = out * gain
    if noise is not None:
        out = out + noise_weight * noise
    if bias is not None:
        out = out + bias.reshape(1, -1, 1, 1)
    if slope is not None:
        out = lrelu(out, slope)
    if sft_scale is not None:
        out = out * sft_scale + sft_shift
    if residual is not None:
        out = out + residual
    return out


def styleunet_forward(sd, x, activation=True, noise=None, v=Variant(), return_pre=False):
    """sd: the module's state dict; x (B, in_dim, S, S); noise: None (the stored buffers) or a list of (B or 1, 1, h, w) tensors."""
    dt = x.dtype
    P = {k: t.to(dt) for k, t in sd.items()}
    S = x.shape[-1]
    L = int(math.log2(S))
    B = x.shape[0]

    def plain(name, t, act=True, residual=None, bias=True):
        return conv2d(t, P[name + ".weight"], bias=P[name + ".bias"] if bias else None, slope=v.slope if act else None, residual=residual)

    def resblock(name, t, up):
        skip = plain(name + ".skip", resample(t, up, v), act=False, bias=False)
        return plain(name + ".conv2", resample(plain(name + ".conv1", t), up, v), residual=skip)

    # ---- U-Net encoder and up path ----
    feat = plain("conv_body_first", x)
    skips = []
    for i in range(L - 2):
        feat = resblock(f"conv_body_down.{i}", feat, up=False)
        skips.insert(0, feat)
    feat = plain("final_conv", feat)
    code = feat.reshape(B, -1) @ P["final_linear.weight"].t() + P["final_linear.bias"]
    conds = []
    for i in range(L - 2):
        feat = resblock(f"conv_body_up.{i}", feat + skips[i], up=True)
        for which in ("condition_scale", "condition_shift"):
            conds.append(plain(f"{which}.{i}.2", plain(f"{which}.{i}.0", feat), act=False))

    # ---- style path ----
    d = "stylegan_decoder."
    lat = code * torch.rsqrt((code * code).mean(dim=1, keepdim=True) + 1e-8)
    for j in range(8):
        lat = lrelu(lat @ P[d + f"style_mlp.{2 * j + 1}.weight"].t() + P[d + f"style_mlp.{2 * j + 1}.bias"], 0.2)

    def modulated(name, t, demod):
        w = P[name + ".weight"][0]
        s = lat @ P[name + ".modulation.weight"].t() + P[name + ".modulation.bias"]
        dmod = None
        if demod and v.demod:
            dmod = torch.rsqrt((s * s) @ (w * w).sum(dim=(2, 3)).t() + 1e-8)
        return w, s, dmod

    def styleconv(name, t, layer, sft=None):
        w, s, dmod = modulated(name + ".modulated_conv", t, True)
        nz = (P[d + f"noises.noise{layer}"] if noise is None else noise[layer].to(dt)) if v.noise else None
        sc, sh = (None, None) if sft is None else (sft[1], sft[0]) if v.sft_swapped else sft
        return conv2d(t, w, in_scale=s, out_scale=dmod, gain=math.sqrt(2.0) if v.gain else None, noise=nz,
                      noise_weight=P[name + ".weight"], bias=P[name + ".bias"], slope=v.slope, sft_scale=sc, sft_shift=sh)

    def torgb(name, t, skip):
        w, s, _ = modulated(name + ".modulated_conv", t, False)
        if skip is not None:
            skip = resample(skip, True, v) if v.rgb_skip_upsampled else skip.repeat_interleave(2, 2).repeat_interleave(2, 3)
        return conv2d(t, w, in_scale=s, bias=P[name + ".bias"], residual=skip)

    # ---- StyleGAN2 decoder with SFT ----
    out = P[d + "constant_input.weight"].expand(B, -1, -1, -1)
    out = styleconv(d + "style_conv1", out, 0)
    skip = torgb(d + "to_rgb1", out, None)
    for j in range(L - 2):
        out = styleconv(d + f"style_convs.{2 * j}", resample(out, True, v), 1 + 2 * j, sft=(conds[2 * j], conds[2 * j + 1]))
        out = styleconv(d + f"style_convs.{2 * j + 1}", out, 2 + 2 * j)
        skip = torgb(d + f"to_rgbs.{j}", out, skip)
    if return_pre:
        return skip
    return torch.sigmoid(skip) if activation else skip


def draw_noise(B, num_layers, device):
    """The draws of StyleUNet.forward(randomize_noise=True), in its order."""
    return [torch.empty(B, 1, noise_resolution(i), noise_resolution(i), device=device).normal_() for i in range(num_layers)]
