"""Frames per second of the Gaussian splat rasteriser (``artalk_splat_render``) at the GAGAvatar head's shape: N = 180 255 Gaussians
(5 023 points and two 296 x 296 planes, ``models.py:31,78-93``), 32 channels, 512 x 512, in front of a camera at the reference's
focal 12 and distance 2.

The scene is synthetic (GAGAvatar's checkpoints are not at hand): a head-sized ellipsoid of 5 023 points and two planes 0.3 wide, the
second a little behind the first, each plane Gaussian about one grid step wide (sigma 1.8 px on screen, radius 6 - 7 px), opacities
0.1 .. 0.9.  Attributes are shared by all frames (stride 0); the means move a little from frame to frame, as the head does.

Rounds alternate a plain call (HIP events around it: the figure that counts) and a call with the library's stage timing on (events
around every stage of every frame, which costs a little); medians over the rounds.  The only derived floor is bytes: 32 x H x W x 4 of
output per frame plus the (tile, Gaussian) pairs' 12 bytes of key and value written once and read once, over the measured streaming
rate of the HBM (6.29 TB/s).  The tool prints the achieved fraction and names the stage that dominates.

    python tools/splat_bench.py --out profiles/splat_bench.json

Prints one JSON line; --out also writes it to a file.  Needs the GPU: without one it fails.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BYTES_PER_S = 6.29e12      # float4 copy, measured on an MI355X
STAGES = ("count_pass", "preprocess", "scan_emit", "sort", "ranges", "blend")
N_POINTS, PLANE = 5023, 296


def gaga_like_scene(T, seed=0):
    """means (T, N, 3), colors (N, 32), opacities (N,), scales (N, 3), rotations (N, 4) float32, N = 5 023 + 2 * 296^2."""
    g = np.random.default_rng(seed)
    d = g.standard_normal((N_POINTS, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    points = d * np.array([0.085, 0.11, 0.09])
    u = (np.arange(PLANE) + 0.5) / PLANE * 0.3 - 0.15
    px, py = np.meshgrid(u, u)
    planes = [np.stack([px.ravel(), py.ravel(), np.full(PLANE * PLANE, z) + 0.004 * g.standard_normal(PLANE * PLANE)], axis=1)
              for z in (0.0, 0.03)]
    means = np.concatenate([points] + planes)
    N = means.shape[0]
    step = 0.3 / PLANE
    scales = np.concatenate([np.full((N_POINTS, 3), 0.003), np.full((N - N_POINTS, 3), 1.15 * step)]) * g.uniform(0.7, 1.3, (N, 3))
    rots = g.standard_normal((N, 4))
    rots /= np.linalg.norm(rots, axis=1, keepdims=True)
    opac = g.uniform(0.1, 0.9, N)
    colors = g.uniform(-1.0, 1.0, (N, 32))
    frames = np.stack([means + 0.002 * np.sin(0.3 * t + means[:, ::-1] * 40.0) for t in range(T)])
    return [a.astype(np.float32) for a in (frames, colors, opac, scales, rots)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9, help="alternations of the plain call and the stage-timed call")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from artalk_amd import capi, splat

    if not torch.cuda.is_available():
        raise SystemExit("splat_bench needs the GPU")
    S, T = args.size, args.frames
    means, colors, opac, scales, rots = [torch.from_numpy(a).cuda() for a in gaga_like_scene(T)]
    N = int(means.shape[1])
    cam = torch.tensor([[[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 2.0]]])
    view, proj, _ = splat.build_camera_matrices(cam, 12.0, 12.0)
    view, proj = view.contiguous(), proj.contiguous()
    out = torch.empty(T, 32, S, S, dtype=torch.float32, device="cuda")
    radii = torch.empty(T, N, dtype=torch.int32, device="cuda")
    L = capi.lib()
    h = splat._handle(torch.device("cuda", torch.cuda.current_device()))

    def call():
        rc = L.artalk_splat_render(h, N, T, S, S, capi.ptr(means), N * 3, capi.ptr(colors), 0, capi.ptr(opac), 0, capi.ptr(scales), 0,
                                   capi.ptr(rots), 0, capi.ptr(view), capi.ptr(proj), 1, 1.0 / 12.0, 1.0 / 12.0, 1.0, None, capi.ptr(out),
                                   capi.ptr(radii), capi.current_stream_ptr())
        if rc != capi.OK:
            raise SystemExit("artalk_splat_render failed: " + L.artalk_splat_last_error(h).decode())

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        timed()
    total_ms, stage_ms = [], []
    pairs, frames = C.c_longlong(0), C.c_int(0)
    for _ in range(args.rounds):
        L.artalk_splat_set_timing(h, 0)
        total_ms.append(timed())
        L.artalk_splat_set_timing(h, 1)
        timed()
        buf = (C.c_double * len(STAGES))()
        L.artalk_splat_get_timing(h, buf, len(STAGES), C.byref(pairs), C.byref(frames))
        stage_ms.append(list(buf))
    L.artalk_splat_set_timing(h, 0)
    med = statistics.median(total_ms)
    stages = {name: statistics.median(r[i] for r in stage_ms) / T for i, name in enumerate(STAGES)}
    pairs_per_frame = pairs.value / max(frames.value, 1)
    drawn = float((radii > 0).float().mean().item())
    floor_bytes = T * (32 * S * S * 4 + pairs_per_frame * 12 * 2)
    floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
    res = {
        "workload": f"artalk_splat_render, N = {N} (5 023 points + two 296 x 296 planes), 32 channels, {S} x {S}, T = {T} frames per call, "
                    f"shared attributes, per-frame means, focal 12 at distance 2, {drawn:.1%} of the Gaussians drawn; output tensors "
                    f"allocated outside the timed call; HIP events, {args.warmup} warm-up calls, median of {args.rounds} rounds alternating "
                    f"with a stage-timed call",
        "ms_per_call": med, "ms_per_call_min": min(total_ms), "ms_per_call_max": max(total_ms),
        "ms_per_frame": med / T, "fps": T / med * 1e3,
        "stage_ms_per_frame": stages, "dominant_stage": max(stages, key=stages.get),
        "pairs_per_frame": pairs_per_frame,
        "bytes_floor_per_call": floor_bytes, "floor_ms_at_6.29TBps": floor_ms, "fraction_of_bytes_floor": floor_ms / med,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
