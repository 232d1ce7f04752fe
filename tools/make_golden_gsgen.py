#!/usr/bin/env python
"""Writes tests/golden/gsgen_ref.npz and tests/golden/gsgen_manifest.json from the reference's own Gaussian generators.

    python tools/make_golden_gsgen.py --reference /path/to/ARTalk

app/GAGAvatar/models.py is imported at run time from the checkout, with stand-ins for the modules it imports but the generators do not
need (pytorch3d.*, torchvision, the sibling modules and utils_renderer).  Its LinearGSGenerator and ConvGSGenerator are loaded with
artalk_amd.gsgen.synth_state_dict and run on the CPU in float64 on the case table of tests/gsgen_cases.py, and so is its
build_points_planes (through a view of torch whose float32 requests give float64, so that only its float32 linspace values stay
float32's); the direction encoding comes from the restatement (tests/gsgen_ref.py), pytorch3d not being at hand.  Run once, on a CPU; no
test imports the reference.  Both outputs hold data only."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))

import gsgen_cases as cases      # noqa: E402
import gsgen_ref      # noqa: E402
from artalk_amd.gsgen import synth_state_dict      # noqa: E402

STD_RANGE = (0.05, 20.0)
NORM_FLOOR = 0.05      # of the case's median norm


def reference_module(checkout):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    stub("pytorch3d").__path__ = []
    stub("pytorch3d.transforms", axis_angle_to_matrix=None)
    stub("pytorch3d.renderer").__path__ = []
    stub("pytorch3d.renderer.implicit").__path__ = []
    stub("pytorch3d.renderer.implicit.harmonic_embedding", HarmonicEmbedding=None)
    if "torchvision" not in sys.modules:
        stub("torchvision")
    pkg = stub("gaga_app")
    pkg.__path__ = [os.path.join(checkout, "app", "GAGAvatar")]
    stub("gaga_app.modules", DINOBase=None, StyleUNet=None)
    stub("gaga_app.utils_renderer", render_gaussian=None)
    return importlib.import_module("gaga_app.models")


class _Float64Torch:
    """torch, except that tensors asked for in float32 come in float64 (a float32 linspace keeps float32's values)."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def linspace(*a, dtype=None, **k):
        return torch.linspace(*a, dtype=torch.float32, **k).double()

    @staticmethod
    def tensor(data, dtype=None, **k):
        return torch.tensor(data, dtype=torch.float64, **k)


def run_reference(models, dims, sd, f0, f1, tm, enc, dtype):
    """The five arrays as forward_expression assembles them (models.py:65-87), from the reference's classes."""
    V, Dh, Dg, C, P = dims
    cast = lambda t: t.to(dtype)
    gen_g = models.LinearGSGenerator(in_dim=Dh + Dg, dir_dim=27).to(dtype).eval()
    gen_g.load_state_dict({k[len("gs_generator_g."):]: cast(v) for k, v in sd.items() if k.startswith("gs_generator_g.")}, strict=True)
    inp = torch.cat([cast(sd["head_base"])[None], cast(f1)[None, None].expand(-1, V, -1)], dim=-1)
    parts = [gen_g(inp, cast(enc)[None])]
    parts[0]["xyz"] = inp.new_zeros((1, V, 3))
    hidden = torch.cat([gen_g.feature_layers(inp), cast(enc)[None, None].expand(-1, V, -1)], dim=-1)
    pre = {"g": {h: getattr(gen_g, h + "_layers")(hidden)[0] for h in ("color", "opacity", "scale", "rotation")}}
    if dtype == torch.float64:
        saved, models.torch = models.torch, _Float64Torch()
        try:
            pl = models.build_points_planes(P, cast(tm))
        finally:
            models.torch = saved
    else:
        pl = models.build_points_planes(P, tm)
    for l, sign in ((0, 1.0), (1, -1.0)):
        gen = models.ConvGSGenerator(in_dim=C, dir_dim=27).to(dtype).eval()
        gen.load_state_dict({k[len(f"gs_generator_l{l}."):]: cast(v) for k, v in sd.items() if k.startswith(f"gs_generator_l{l}.")},
                            strict=True)
        pre[l] = gen.gaussian_conv(torch.cat([cast(f0)[None], cast(enc)[None, :, None, None].expand(-1, -1, P, P)], dim=1))
        r = gen(cast(f0)[None], cast(enc)[None])
        r["xyz"] = pl["plane_points"][None] + sign * r["positions"] * pl["plane_dirs"][None, None]
        parts.append(r)
    out = {k: torch.cat([p[k] for p in parts], dim=1)[0] for k in cases.ATTRS}
    return out, pl, pre


def check_fixture(name, pre, dims):
    """Refuses a fixture whose sigmoids saturate or die, or whose normalisations sit where a float32 run amplifies its own error."""
    for l in (0, 1):
        o = pre[l][0]
        for what, sl in (("opacity", slice(32, 33)), ("scale", slice(33, 36)), ("position", slice(40, 41)), ("colour", slice(0, 32))):
            std = float(o[sl].std())
            print(f"    {name} l{l} {what}: pre-sigmoid std {std:.3f}")
            assert STD_RANGE[0] <= std <= STD_RANGE[1], "saturated or dead fixture: change the seed"
        nrm = o[36:40].norm(dim=0).reshape(-1)
        print(f"    {name} l{l} rotation norms: min {float(nrm.min()):.3f}, median {float(nrm.median()):.3f}")
        assert float(nrm.min()) >= NORM_FLOOR * float(nrm.median()), "a local rotation norm is close to 0: change the seed"
    for what in ("color", "opacity", "scale"):
        std = float(pre["g"][what].std())
        print(f"    {name} g {what}: pre-sigmoid std {std:.3f}")
        assert STD_RANGE[0] <= std <= STD_RANGE[1], "saturated or dead fixture: change the seed"
    col = pre["g"]["rotation"].norm(dim=0)
    print(f"    {name} g rotation column norms: {[round(float(v), 3) for v in col]}")
    assert float(col.min()) >= NORM_FLOOR * float(col.median()), "a global column norm is close to 0: change the seed"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--seed", type=int, default=cases.SEED)
    a = ap.parse_args()
    models = reference_module(a.reference)
    gold = os.path.join(REPO, "tests", "golden")
    store = {"seed": np.int64(a.seed)}
    with torch.no_grad():
        for name, dims in cases.CASES.items():
            V, Dh, Dg, C, P = dims
            sd = synth_state_dict(*dims, seed=a.seed)
            f0, f1 = (torch.from_numpy(t) for t in cases.features(name))
            tm = torch.from_numpy(cases.transform_matrix(name))
            _, d64 = gsgen_ref.planes(P, tm, torch.float64)
            enc64, enc32 = gsgen_ref.direnc(d64), gsgen_ref.direnc(d64.float())
            out, pl, pre = run_reference(models, dims, sd, f0, f1, tm, enc64, torch.float64)
            out32, _, _ = run_reference(models, dims, sd, f0, f1, tm, enc32, torch.float32)
            print(f"case {name} {dims}: N = {out['xyz'].shape[0]}")
            check_fixture(name, pre, dims)
            for k in cases.ATTRS:
                e = float((out32[k].double() - out[k]).abs().max())
                print(f"    {k}: the reference in float32 differs from its float64 run by {e:.2e} (largest value {float(out[k].abs().max()):.3f})")
                store[f"{name}_{k}"] = out[k].numpy()
            store[f"{name}_plane_points"] = pl["plane_points"].numpy()
            store[f"{name}_plane_dirs"] = pl["plane_dirs"].numpy()
            store[f"{name}_direnc"] = enc64.numpy()
            store[f"{name}_f_feature0"] = f0.numpy()
            store[f"{name}_f_feature1"] = f1.numpy()
            store[f"{name}_transform_matrix"] = tm.numpy()
    np.savez_compressed(os.path.join(gold, "gsgen_ref.npz"), **store)
    V, Dh, Dg, C, P = cases.REFERENCE_DIMS
    with torch.device("meta"):
        mods = (("gs_generator_g.", models.LinearGSGenerator(in_dim=Dh + Dg, dir_dim=27)), ("gs_generator_l0.", models.ConvGSGenerator(in_dim=C, dir_dim=27)),
                ("gs_generator_l1.", models.ConvGSGenerator(in_dim=C, dir_dim=27)))
    manifest = [["head_base", [V, Dh]]] + [[p + k, list(v.shape)] for p, m in mods for k, v in m.state_dict().items()]
    with open(os.path.join(gold, "gsgen_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
