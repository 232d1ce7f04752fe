#!/usr/bin/env python
"""Writes tests/golden/styleunet_ref.npz and tests/golden/styleunet_manifest.json from the reference's own StyleUNet.

    python tools/make_golden_styleunet.py --reference /path/to/ARTalk

The reference module is imported at run time from the checkout (through a stub package around modules/style_clean.py and
modules/style_unet.py, so that the rest of the GAGAvatar head and its dependencies are not needed), loaded with
artalk_amd.styleunet.synth_state_dict and run on the CPU in float64 with randomize_noise=False.  Run once, on a CPU; no test imports the
reference.  Both outputs hold data only."""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from artalk_amd.styleunet import synth_state_dict      # noqa: E402

CASES = ((8, 3), (16, 2), (64, 1))      # (out_size, B)
MANIFEST_SIZES = (8, 16, 64, 512)
IN_DIM, OUT_DIM = 32, 3
STD_RANGE = (0.05, 20.0)


def reference_class(checkout):
    pkg = types.ModuleType("gaga_modules")
    pkg.__path__ = [os.path.join(checkout, "app", "GAGAvatar", "modules")]
    sys.modules["gaga_modules"] = pkg
    return importlib.import_module("gaga_modules.style_unet").StyleUNet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    StyleUNet = reference_class(a.reference)
    gold = os.path.join(REPO, "tests", "golden")
    out = {"seed": np.int64(a.seed)}
    with torch.no_grad():
        for S, B in CASES:
            sd = synth_state_dict(S, IN_DIM, OUT_DIM, seed=a.seed)
            net = StyleUNet(in_size=S, out_size=S, in_dim=IN_DIM, out_dim=OUT_DIM, activation=False).double().eval()
            net.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
            x32 = np.random.Generator(np.random.SFC64(1000 + S)).random((B, IN_DIM, S, S), dtype=np.float32)
            x = torch.from_numpy(x32).double()      # stored as float32 (exact in float64): keeps the file under the size limit
            pre = net(x, randomize_noise=False)
            std = float(pre.std())
            print(f"out_size {S} B {B}: pre-sigmoid std {std:.4f}, range [{float(pre.min()):.3f}, {float(pre.max()):.3f}]")
            assert STD_RANGE[0] <= std <= STD_RANGE[1], "saturated or dead fixture: change the seed"
            out[f"x_{S}"] = x32
            out[f"pre_{S}"] = pre.numpy()
            out[f"act_{S}"] = torch.sigmoid(pre).numpy()
            f32 = StyleUNet(in_size=S, out_size=S, in_dim=IN_DIM, out_dim=OUT_DIM, activation=True).eval()
            f32.load_state_dict(sd, strict=True)
            e = float((f32(x.float(), randomize_noise=False).double() - torch.sigmoid(pre)).abs().max())
            print(f"    the reference in float32 differs from its float64 run by {e:.2e} after the sigmoid")
    np.savez_compressed(os.path.join(gold, "styleunet_ref.npz"), **out)
    manifest = {}
    for S in MANIFEST_SIZES:
        with torch.device("meta"):
            net = StyleUNet(in_size=S, out_size=S, in_dim=IN_DIM, out_dim=OUT_DIM)
        manifest[str(S)] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    with open(os.path.join(gold, "styleunet_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
