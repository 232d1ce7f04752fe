"""Frames per second of the mesh renderer (``artalk_render_mesh``) on one 10 s clip: S = 512, T = 250, a mesh with FLAME's counts.

The mesh is a displaced UV sphere, 116 x 43 segments = 5 104 vertices and 9 976 faces (FLAME: 5 023 and 9 976), about 70 % of the
image height under the default camera, as the head is; every frame displaces it a little differently.  The synthetic FLAME asset is
no use here: its random faces span the whole image.  The LBS call (``artalk_flame_verts``, synthetic asset, T = 250) is timed beside
it, separately: HIP events around each call, warm-up, then rounds that alternate the two; medians.

The only derived floor is the bytes written: 16 B per pixel of image (rgb + alpha) and 8 B per pixel of visibility keys per frame,
about 4 MB + 2 MB at 512 x 512, over the measured streaming rate of the HBM (6.29 TB/s).  The tool prints the achieved fraction.

    python tools/render_bench.py --out profiles/render_bench.json

Prints one JSON line; --out also writes it to a file.  Needs the GPU: without one it fails.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BYTES_PER_S = 6.29e12      # float4 copy, measured on an MI355X


def head_like_mesh(T, seed=0, n_lon=116, n_lat=43, radius=0.7 * 2.0 / 12.0):
    """(T, V, 3) float32 vertices, (F, 3) int32 faces: a sphere filling 70 % of the image height at focal 12 and distance 2, with a
    smooth radial displacement (a few low harmonics) that changes per frame."""
    g = np.random.default_rng(seed)
    lat = np.pi * np.arange(n_lat + 1) / n_lat
    lon = 2.0 * np.pi * np.arange(n_lon) / n_lon
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    d = np.stack([0.8 * np.sin(la) * np.cos(lo), np.cos(la), np.sin(la) * np.sin(lo)], -1).reshape(-1, 3)
    la, lo = la.reshape(-1), lo.reshape(-1)
    amp, ph = 0.03 * g.standard_normal((4, 4)), 2.0 * np.pi * g.random((4, 4))
    verts = np.empty((T,) + d.shape, np.float32)
    for t in range(T):
        r = np.ones_like(la)
        for a in range(4):
            for b in range(4):
                r += amp[a, b] * np.sin((a + 1) * la + ph[a, b] + 0.05 * t) * np.cos(b * lo + ph[b, a])
        verts[t] = radius * r[:, None] * d
    faces = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
            faces += [(a, b, a + n_lon), (b, b + n_lon, a + n_lon)]
    return verts, np.array(faces, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--rounds", type=int, default=9, help="alternations of the LBS call and the render call")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from artalk_amd.flame import FLAMEModel, synthetic_flame_asset
    from artalk_amd.render import RenderMesh

    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs the GPU")
    S, T = args.size, args.frames
    verts_host, faces = head_like_mesh(T)
    verts = torch.from_numpy(verts_host).cuda()
    renderer = RenderMesh(S, faces=faces, n_verts=verts.shape[1])
    fm = FLAMEModel(n_shape=300, n_exp=100, scale=1.0, no_lmks=True, flame_ckpt=synthetic_flame_asset())
    g = torch.Generator().manual_seed(1)
    shape = torch.zeros(T, 300).cuda()
    exp, pose = (0.5 * torch.randn(T, 100, generator=g)).cuda(), (0.1 * torch.randn(T, 6, generator=g)).cuda()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def lbs():
        return fm(shape_params=shape, expression_params=exp, pose_params=pose)

    def render():
        return renderer(verts)

    for _ in range(args.warmup):
        timed(lbs)
        _, (rgb, alpha) = timed(render)
    covered = float(alpha.mean().item())
    lbs_ms, render_ms = [], []
    for _ in range(args.rounds):
        lbs_ms.append(timed(lbs)[0])
        render_ms.append(timed(render)[0])
    r_med, l_med = statistics.median(render_ms), statistics.median(lbs_ms)
    floor_bytes = T * S * S * (16 + 8)
    floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
    res = {
        "workload": f"artalk_render_mesh, S = {S}, T = {T}, {verts.shape[1]} vertices, {faces.shape[0]} faces, displaced sphere covering "
                    f"{covered:.1%} of the pixels; output tensors allocated inside the timed call; HIP events, {args.warmup} warm-up calls, "
                    f"median of {args.rounds} rounds alternating with the LBS call",
        "render_ms": r_med, "render_ms_min": min(render_ms), "render_ms_max": max(render_ms),
        "render_fps": T / r_med * 1e3,
        "lbs_ms": l_med, "lbs_ms_min": min(lbs_ms), "lbs_ms_max": max(lbs_ms), "lbs_fps": T / l_med * 1e3,
        "bytes_written_floor": floor_bytes, "floor_ms_at_6.29TBps": floor_ms, "fraction_of_floor": floor_ms / r_med,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
