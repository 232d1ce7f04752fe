#!/usr/bin/env python
"""Writes tests/golden/dino_ref.npz, dino_ref_taps.npz and dino_manifest.json from the reference's own DINOBase.

    python tools/make_golden_dino.py --reference /path/to/ARTalk

app/GAGAvatar/modules/dino_base.py is imported at run time from the checkout, with stand-ins for what it cannot import here:

  torchvision      Normalize and transforms.functional.resize, the latter written with torch's F.interpolate(mode="bilinear",
                   align_corners=False, antialias=True) - torchvision's own tensor path (unpinned: torchvision was not at hand)
  torch.hub.load   a small adapter around transformers.Dinov2Model, an independent implementation of the same network (the upstream
                   DINOv2 source is fetched by torch.hub and was not at hand), with attn_implementation="eager" and image_size =
                   14 grid so that nothing is interpolated.  It offers get_intermediate_layers(x, n) - the last n blocks' outputs through
                   the final norm, the class token stripped - and blocks[0].attn.qkv.in_features.

The synthetic dict (artalk_amd.dino.synth_state_dict, named after the facebookresearch module) is mapped onto the HF module by splitting
qkv into query / key / value.  The whole module runs on the CPU in float64 on the case table of tests/dino_cases.py.  A fixture whose
outputs are not of order 1 is refused.  Run once, on a CPU; no test imports the reference or transformers.  All outputs hold data only."""
import argparse
import hashlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import dino_cases as cases      # noqa: E402
from artalk_amd.dino import state_dict_manifest, synth_state_dict      # noqa: E402

MAX_RANGE = (0.05, 50.0)
ZERO_SHARE = 0.01
TAPS_CASE = "A"
RN0_STRIDE = 4      # channels of rn0 kept in the taps fixture (the committed-file size limit)


class _Normalize(nn.Module):
    def __init__(self, mean, std):
        super().__init__()
        self.mean, self.std = list(mean), list(std)

    def forward(self, x):
        mean = torch.as_tensor(self.mean, dtype=x.dtype, device=x.device)[:, None, None]
        std = torch.as_tensor(self.std, dtype=x.dtype, device=x.device)[:, None, None]
        return (x - mean) / std


def _resize(img, size, antialias=True):
    lead = img.dim() == 3
    out = F.interpolate(img[None] if lead else img, tuple(size), mode="bilinear", align_corners=False, antialias=bool(antialias))
    return out[0] if lead else out


class _Adapter(nn.Module):
    """What dino_base.py uses of torch.hub's dinov2_vitb14, on top of transformers.Dinov2Model."""

    def __init__(self, vit_dim, depth, heads, grid):
        super().__init__()
        cfg = Dinov2Config(hidden_size=vit_dim, num_hidden_layers=depth, num_attention_heads=heads, mlp_ratio=4, image_size=14 * grid,
                           patch_size=14, layer_norm_eps=1e-6, hidden_act="gelu", qkv_bias=True, use_swiglu_ffn=False,
                           attn_implementation="eager")
        self.hf = Dinov2Model(cfg)
        qkv = types.SimpleNamespace(in_features=vit_dim)
        self.blocks = [types.SimpleNamespace(attn=types.SimpleNamespace(qkv=qkv))]

    def get_intermediate_layers(self, x, n=1):
        hs = self.hf(pixel_values=x, output_hidden_states=True).hidden_states      # the embeddings, then every block's output
        return tuple(self.hf.layernorm(h)[:, 1:] for h in hs[-n:])

    def load_facebook(self, sd, depth, D):
        """sd: the dino_model.* part of the synthetic dict, keys without that prefix."""
        m = {"embeddings.cls_token": sd["cls_token"], "embeddings.mask_token": sd["mask_token"], "embeddings.position_embeddings": sd["pos_embed"],
             "embeddings.patch_embeddings.projection.weight": sd["patch_embed.proj.weight"],
             "embeddings.patch_embeddings.projection.bias": sd["patch_embed.proj.bias"],
             "layernorm.weight": sd["norm.weight"], "layernorm.bias": sd["norm.bias"]}
        for i in range(depth):
            b, h = f"blocks.{i}.", f"encoder.layer.{i}."
            for j, part in enumerate(("query", "key", "value")):
                m[h + f"attention.attention.{part}.weight"] = sd[b + "attn.qkv.weight"][j * D:(j + 1) * D]
                m[h + f"attention.attention.{part}.bias"] = sd[b + "attn.qkv.bias"][j * D:(j + 1) * D]
            for ours, theirs in (("norm1", "norm1"), ("norm2", "norm2"), ("attn.proj", "attention.output.dense"), ("mlp.fc1", "mlp.fc1"),
                                 ("mlp.fc2", "mlp.fc2")):
                m[h + theirs + ".weight"], m[h + theirs + ".bias"] = sd[b + ours + ".weight"], sd[b + ours + ".bias"]
            m[h + "layer_scale1.lambda1"], m[h + "layer_scale2.lambda1"] = sd[b + "ls1.gamma"], sd[b + "ls2.gamma"]
        self.hf.load_state_dict(m, strict=True)


def reference_module(checkout):
    global Dinov2Config, Dinov2Model
    from transformers import Dinov2Config, Dinov2Model      # before the torchvision stand-in: transformers probes for the real package
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.Normalize = _Normalize
    tv.transforms.functional = types.ModuleType("torchvision.transforms.functional")
    tv.transforms.functional.resize = _resize
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms, "torchvision.transforms.functional": tv.transforms.functional})
    path = os.path.join(checkout, "app", "GAGAvatar", "modules", "dino_base.py")
    spec = importlib.util.spec_from_file_location("gaga_dino_base", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, hashlib.sha256(open(path, "rb").read()).hexdigest()


def build(mod, dims, sd, dtype):
    od, D, depth, heads, g = dims
    saved = torch.hub.load
    torch.hub.load = lambda *a, **k: _Adapter(D, depth, heads, g)
    try:
        ref = mod.DINOBase(output_dim=od)
    finally:
        torch.hub.load = saved
    ref.dino_model.load_facebook({k[len("dino_model."):]: v for k, v in sd.items() if k.startswith("dino_model.")}, depth, D)
    res = ref.load_state_dict({k: v for k, v in sd.items() if not k.startswith("dino_model.")}, strict=False)
    assert not res.unexpected_keys and all(k.startswith("dino_model.") for k in res.missing_keys), res
    return ref.to(dtype).eval()


def run(ref, img, dtype):
    """The module's two outputs, and through hooks the four taps (g, g, D) and the four layer_rn outputs (H, H, 256)."""
    taps, rns = [], []
    orig = ref.dino_model.get_intermediate_layers

    def tapped(x, n=1):
        out = orig(x, n)
        taps.extend(out)
        return out
    ref.dino_model.get_intermediate_layers = tapped
    hooks = [l.register_forward_hook(lambda m, i, o: rns.append(o)) for l in ref.layer_rn]
    try:
        plane, glob = ref(torch.from_numpy(img).to(dtype)[None])
    finally:
        ref.dino_model.get_intermediate_layers = orig
        for h in hooks:
            h.remove()
    g = img.shape[-1] // 14
    return dict(plane=plane[0], glob=glob[0], taps=[t[0].reshape(g, g, -1) for t in taps], rn=[r[0].permute(1, 2, 0).contiguous() for r in rns])


def check_fixture(name, out):
    for k in cases.OUTPUTS:
        big = float(out[k].abs().max())
        print(f"    {name} {k}: max |x| {big:.3f}")
        assert MAX_RANGE[0] <= big <= MAX_RANGE[1], "an output is not of order 1: change the seed or the weight scales"
    zeros = float((out["plane"] == 0).double().mean())
    print(f"    {name} plane: {100 * zeros:.3f} % exact zeros")
    assert zeros <= ZERO_SHARE, "a dead plane: change the seed"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--seed", type=int, default=cases.SEED)
    a = ap.parse_args()
    mod, digest = reference_module(a.reference)
    gold = os.path.join(REPO, "tests", "golden")
    store, taps = {"seed": np.int64(a.seed)}, {"seed": np.int64(a.seed), "rn0_channel_stride": np.int64(RN0_STRIDE)}
    with torch.no_grad():
        for name, dims in cases.CASES.items():
            sd = synth_state_dict(*dims, seed=a.seed)
            img = cases.image(name)
            out = run(build(mod, dims, sd, torch.float64), img, torch.float64)
            out32 = run(build(mod, dims, sd, torch.float32), img, torch.float32)
            print(f"case {name} {dims}: plane {tuple(out['plane'].shape)}")
            check_fixture(name, out)
            for k in cases.OUTPUTS:
                e = float((out32[k].double() - out[k]).abs().max())
                print(f"    {k}: the reference in float32 differs from its float64 run by {e:.2e}")
                store[f"{name}_{k}"] = out[k].numpy()
            if name == TAPS_CASE:
                for i in range(4):
                    taps[f"{name}_tap{i}"] = out["taps"][i].numpy()
                    taps[f"{name}_rn{i}"] = out["rn"][i][..., ::RN0_STRIDE].numpy() if i == 0 else out["rn"][i].numpy()
    np.savez_compressed(os.path.join(gold, "dino_ref.npz"), **store)
    np.savez_compressed(os.path.join(gold, "dino_ref_taps.npz"), **taps)
    manifest = {"reference_file": "app/GAGAvatar/modules/dino_base.py", "reference_sha256": digest, "seed": a.seed,
                "cases": {k: list(v) for k, v in cases.CASES.items()}, "reference_dims": list(cases.REFERENCE_DIMS),
                "state_dict": [[k, list(s)] for k, s in state_dict_manifest(*cases.REFERENCE_DIMS)]}
    # the head's part of the key list comes from the reference's own module (the backbone's names are the published DINOv2 layout)
    saved = torch.hub.load
    torch.hub.load = lambda *a_, **k_: _Adapter(*cases.REFERENCE_DIMS[1:])
    try:
        with torch.device("meta"):
            head = mod.DINOBase(output_dim=cases.REFERENCE_DIMS[0])
    finally:
        torch.hub.load = saved
    manifest["head_state_dict"] = [[k, list(v.shape)] for k, v in head.state_dict().items() if not k.startswith("dino_model.")]
    with open(os.path.join(gold, "dino_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
