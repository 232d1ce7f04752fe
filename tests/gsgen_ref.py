"""Torch-CPU restatement of the Gaussian generators ("Gaussian generators"), written from that definition and
parameterised by dtype: float64 is what the goldens from the reference's own classes are compared with, float32 gives e32, the error a
float32 evaluation makes by itself.  ``variant`` names one deliberate misreading of the definition (tests/test_gsgen_cpu.py shows that
each of them misses the golden by a wide margin)."""
import torch
import torch.nn.functional as F

VARIANTS = ("channel_sigmoid", "row_rotation", "l1_plus", "no_scale", "sincos_swapped", "linspace_up", "relu_last", "leaky")
HEADS = (("color", "colors"), ("opacity", "opacities"), ("scale", "scales"), ("rotation", "rotations"))


def planes(P, transform, dtype=torch.float64, variant=None):
    """build_points_planes: (plane_points (P P, 3), plane_dirs (3,)).  The linspace is float32's in every dtype, as in the reference."""
    T = torch.as_tensor(transform, dtype=torch.float32).to(dtype)
    u = torch.linspace(1, -1, P, dtype=torch.float32).to(dtype)
    if variant == "linspace_up":
        u = torch.linspace(-1, 1, P, dtype=torch.float32).to(dtype)
    R, t = T[:, :3], T[:, 3]
    d = R @ torch.tensor([0.0, 0.0, 1.0], dtype=dtype)
    origin = -(R @ t)
    dist = (origin * d).sum().abs()
    x, y = torch.meshgrid(u, u, indexing="xy")      # x: the column, the fastest index
    ray = torch.stack([x / 12.0, y / 12.0, torch.ones_like(x)], dim=-1).reshape(-1, 3)
    return origin + dist * (ray @ R.T), d


def direnc(d, variant=None):
    """pytorch3d's HarmonicEmbedding(4) with append_input, omega_0 = 1, logspace (this reading is unpinned: pytorch3d was not at hand)."""
    freq = 2.0 ** torch.arange(4, dtype=d.dtype)
    e = (d[:, None] * freq).reshape(-1)
    s, c = torch.sin(e), torch.cos(e)
    return torch.cat([c, s, d]) if variant == "sincos_swapped" else torch.cat([s, c, d])


def global_attributes(raw, variant=None):
    """The global generator's activations: raw {colors (V, 32), opacities (V, 1), scales (V, 3), rotations (V, 4)} -> the V rows."""
    scale = 1.0 if variant == "no_scale" else 0.05
    colors = raw["colors"].clone()
    colors[:, :3] = torch.sigmoid(colors[:, :3])
    q = raw["rotations"]
    if variant == "row_rotation":
        rot = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    else:      # F.normalize on (1, V, 4) with its default dim = 1: every component over all V rows
        rot = q / q.norm(dim=0, keepdim=True).clamp_min(1e-12)
    return {"xyz": torch.zeros_like(raw["scales"]), "colors": colors, "opacities": torch.sigmoid(raw["opacities"]),
            "scales": torch.sigmoid(raw["scales"]) * scale, "rotations": rot}


def local_attributes(o, pts, d, sign, variant=None):
    """A local generator's per-pixel arithmetic: o (P, P, 41) indexed (y, x, channel), plane points (P P, 3), direction (3,)."""
    scale = 1.0 if variant == "no_scale" else 0.05
    colors = o[..., :32].clone()
    if variant == "channel_sigmoid":
        colors[..., :3] = torch.sigmoid(colors[..., :3])
    else:      # colors[..., :3] on the NCHW tensor: the last axis is the width
        colors[:, :3, :] = torch.sigmoid(colors[:, :3, :])
    q = o[..., 36:40]
    pos = torch.sigmoid(o[..., 40:41]).reshape(-1, 1)
    return {"xyz": pts + sign * pos * d, "colors": colors.reshape(-1, 32), "opacities": torch.sigmoid(o[..., 32:33]).reshape(-1, 1),
            "scales": (torch.sigmoid(o[..., 33:36]) * scale).reshape(-1, 3),
            "rotations": (q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)).reshape(-1, 4)}


def generate(sd, f_feature0, f_feature1, transform, dtype=torch.float64, variant=None, device="cpu"):
    """The avatar's arrays {xyz, colors, opacities, scales, rotations}, (N, width) each, N = V + 2 P P.  ``device``: where the layers
    run (tools/gsgen_bench.py times this restatement in float32 on the GPU); the plane geometry is always worked out on the CPU."""
    w = lambda k: sd[k].to(device=device, dtype=dtype)
    f0 = torch.as_tensor(f_feature0, dtype=torch.float32).to(device=device, dtype=dtype)
    f1 = torch.as_tensor(f_feature1, dtype=torch.float32).to(device=device, dtype=dtype)
    C, P = f0.shape[0], f0.shape[1]
    act = (lambda x: F.leaky_relu(x, 0.2)) if variant == "leaky" else torch.relu
    pts, d = planes(P, transform, dtype, variant)
    enc = direnc(d, variant).to(device)
    pts, d = pts.to(device), d.to(device)
    # ---- global generator
    head_base = w("head_base")
    V = head_base.shape[0]
    h = torch.cat([head_base, f1[None].expand(V, -1)], dim=1)
    g = "gs_generator_g."
    for i in range(4):
        h = F.linear(h, w(g + f"feature_layers.{2 * i}.weight"), w(g + f"feature_layers.{2 * i}.bias"))
        if i < 3 or variant == "relu_last":
            h = act(h)
    h = torch.cat([h, enc[None].expand(V, -1)], dim=1)
    raw = {}
    for head, attr in HEADS:
        t = act(F.linear(h, w(g + f"{head}_layers.0.weight"), w(g + f"{head}_layers.0.bias")))
        raw[attr] = F.linear(t, w(g + f"{head}_layers.2.weight"), w(g + f"{head}_layers.2.bias"))
    out = {k: [v] for k, v in global_attributes(raw, variant).items()}
    # ---- local generators
    x0 = torch.cat([f0, enc[:, None, None].expand(-1, P, P)], dim=0)[None]
    for l in range(2):
        n = f"gs_generator_l{l}.gaussian_conv."
        x = x0
        for i in range(3):
            x = act(F.conv2d(x, w(n + f"{2 * i}.weight"), w(n + f"{2 * i}.bias"), padding=1))
        o = F.conv2d(x, w(n + "6.weight"), w(n + "6.bias"))[0].permute(1, 2, 0)      # (y, x, 41)
        for k, v in local_attributes(o, pts, d, 1.0 if l == 0 or variant == "l1_plus" else -1.0, variant).items():
            out[k].append(v)
    return {k: torch.cat(v, dim=0) for k, v in out.items()}
