"""Milliseconds per frame of the GAGAvatar head (``GAGAvatar.render_clip`` = one ``artalk_gaga_render`` call) at the reference's shape:
S = 512, V = 5 023 FLAME vertices, N = 180 255 Gaussians (5 023 + 2 x 296^2), T = 64 frames, stored StyleGAN noise.

Everything is synthetic (neither the FLAME asset nor GAGAvatar's checkpoints are at hand): ``synthetic_flame_asset`` at scale 5, the
upsampler's ``synth_state_dict(512)``, an avatar of two 296 x 296 planes about 1.5 wide around the head with Gaussians one grid step
wide, seen from (0, 0, 5000 / 512) at focal 12, an 82 x 256 watermark, motion codes with a moving head.

Three kinds of call alternate in every round, each between HIP events, medians over the rounds:
  - ``render_clip`` (the figure that counts);
  - ``render_clip`` with the library's stage timing on: the share of inputs + FLAME, forehead + means, splat, upsampler and finish;
  - the same frames through the chain of separate Python calls - FLAMEModel -> torch EMA on the device, frame by frame as the reference
    runs it -> ``render_gaussian`` -> ``StyleUNet`` -> torch clamp / blend: what a user of the pieces had before this call existed.
No target is set.  The one derived expectation is that the new kernels are a small share: they move about 2.2 MB of means and 6 MB of
image per frame against 3.29 ms of upsampler.

    python tools/gaga_bench.py --out profiles/gaga_bench.json

``--precision f32|bf16x3|bf16`` runs the above with the upsampler's convolutions in that mode (the default is f32; the chain's upsampler
is the same module, so it follows).  ``--precision all`` compares the modes instead (no chain): in every round of the one process the
three modes alternate, each with a plain call and a stage-timed call, so the baseline is the f32 mode of the same build in the same rounds.

    python tools/gaga_bench.py --precision all --out profiles/gaga_precision_bench.json

``--output all`` compares the forms in which a clip leaves the head (no chain): in every round of the one process ``float`` (the call
above), ``float+host`` (the same frames, ``.cpu()``, then ``(x * 255).astype(uint8)`` and the transpose in numpy: the reference's
hand-over with the host conversion timed), ``rgb24`` and ``yuv420p`` (``render_clip(out=...)``, device only) and both with ``host=True``
alternate, by the wall clock between device synchronisations, each with a plain call and a stage-timed call whose ``finish`` stage is
the fused clamp / watermark / pack kernel.

    python tools/gaga_bench.py --output all --out profiles/gaga_output_bench.json

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

STAGES = ("inputs_flame", "forehead_means", "splat", "upsampler", "finish")
V, PLANE = 5023, 296
DISTANCE = 5000.0 / 512
FOREHEAD = list(range(3846, 3914))      # 68 vertices (the asset is synthetic: which ones does not matter for the time)


def synthetic_avatar(seed=0):
    import torch
    g = np.random.default_rng(seed)
    N = V + 2 * PLANE * PLANE
    width = 1.46
    u = (np.arange(PLANE) + 0.5) / PLANE * width - width / 2
    px, py = np.meshgrid(u, u)
    xyz = np.zeros((N, 3))
    for i, z in enumerate((0.0, -0.15)):
        lo = V + i * PLANE * PLANE
        xyz[lo:lo + PLANE * PLANE] = np.stack([px.ravel(), py.ravel(), z + 0.02 * g.standard_normal(PLANE * PLANE)], axis=1)
    step = width / PLANE
    scales = np.concatenate([np.full((V, 3), 0.015), np.full((N - V, 3), 1.15 * step)]) * g.uniform(0.7, 1.3, (N, 3))
    rots = g.standard_normal((N, 4))
    rots /= np.linalg.norm(rots, axis=1, keepdims=True)
    tm = np.concatenate([np.diag([-1.0, 1.0, -1.0]), np.array([[0.0], [0.0], [DISTANCE]])], axis=1)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return {"xyz": f(xyz), "colors": f(g.uniform(-1.0, 1.0, (N, 32))), "opacities": f(g.uniform(0.1, 0.9, (N, 1))), "scales": f(scales),
            "rotations": f(rots), "shapecode": f(0.5 * g.standard_normal(300)), "transform_matrix": f(tm)}


def motion(T, seed=1):
    import torch
    g = np.random.default_rng(seed)
    m = np.zeros((T, 106), dtype=np.float32)
    t = np.arange(T)[:, None]
    m[:, :100] = 0.6 * np.sin(0.2 * t + g.uniform(0, 6.28, (1, 100)))
    m[:, 100:103] = 0.12 * np.sin(0.1 * t + g.uniform(0, 6.28, (1, 3)))
    m[:, 103] = 0.1 + 0.1 * np.sin(0.4 * t[:, 0])
    return torch.from_numpy(m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", choices=("f32", "bf16x3", "bf16", "all"), default="f32")
    ap.add_argument("--output", choices=("float", "all"), default="float")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from artalk_amd import capi
    from artalk_amd.flame import FLAMEModel, synthetic_flame_asset
    from artalk_amd.gaga import GAGAvatar, camera_matrices
    from artalk_amd.splat import render_gaussian
    from artalk_amd.styleunet import StyleUNet, synth_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("gaga_bench needs the GPU")
    S, T = args.size, args.frames
    L = capi.lib()
    flame = FLAMEModel(300, 100, scale=5.0, no_lmks=True, flame_ckpt=synthetic_flame_asset())
    sd = synth_state_dict(S)
    av = synthetic_avatar()
    N = int(av["xyz"].shape[0])
    mark = torch.from_numpy(np.random.default_rng(2).random((4, min(82, S), min(256, S)), dtype=np.float32))
    unet = StyleUNet(S, S, 32, 3).eval().to("cuda:0")      # one set of weights: the head and the chain share the module
    unet.load_state_dict(sd)
    head = GAGAvatar({"synthetic": av}, unet, water_mark=mark, image_size=S, n_dynamic=V, forehead_indices=FOREHEAD)
    head.set_avatar_id("synthetic")
    codes = motion(T).cuda()
    dev = {k: v.cuda() for k, v in av.items()}
    dmark = mark.cuda()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    lib_call = lambda: head.render_clip(codes, flame, randomize_noise=False)
    lib_call()      # builds the library object
    slab = head.slab_in_force()
    if args.precision == "all":
        modes = ("f32", "bf16x3", "bf16")
        handle = head._h.value
        frames = {}
        for m in modes:
            head.set_precision(m)
            head.reset_motion_state()
            frames[m] = lib_call()
            for _ in range(args.warmup):
                timed(lib_call)
        call, stage = {m: [] for m in modes}, {m: [] for m in modes}
        st = (C.c_double * len(STAGES))()
        for _ in range(args.rounds):
            for m in modes:
                head.set_precision(m)
                L.artalk_gaga_set_timing(head._h, 0)
                call[m].append(timed(lib_call)[0])
                L.artalk_gaga_set_timing(head._h, 1)
                lib_call()
                L.artalk_gaga_get_timing(head._h, st, len(STAGES))
                stage[m].append(list(st))
        L.artalk_gaga_set_timing(head._h, 0)
        assert head._h.value == handle, "a switch rebuilt the library object"
        f32 = statistics.median(call["f32"])
        res = {
            "workload": f"GAGAvatar.render_clip, S = {S}, V = {V}, N = {N}, T = {T} frames per call in slabs of {slab}, synthetic FLAME asset, "
                        f"avatar and upsampler weights, stored noise, {mark.shape[1]} x {mark.shape[2]} watermark, 68 forehead vertices; HIP "
                        f"events, {args.warmup} warm-up calls per mode, {args.rounds} rounds in one process, each round running the upsampler "
                        f"modes f32, bf16x3, bf16 in turn: a plain call and a stage-timed call",
            "modes": {m: {"ms_per_call": {"median": statistics.median(call[m]), "min": min(call[m]), "max": max(call[m])},
                          "ms_per_frame": statistics.median(call[m]) / T, "frames_per_s": 1e3 * T / statistics.median(call[m]),
                          "speedup_over_f32": f32 / statistics.median(call[m]),
                          "stage_ms_per_frame": {n: statistics.median(s[i] for s in stage[m]) / T for i, n in enumerate(STAGES)},
                          "max_abs_difference_to_f32_frames": float((frames[m] - frames["f32"]).abs().max())} for m in modes},
        }
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    head.set_precision(args.precision)
    if args.output == "all":
        import time
        from artalk_amd.frames import frame_bytes, pack_frames

        def host_hand_over():      # the reference's hand-over (inference.py:83-86), the conversion on one host thread
            x = lib_call().cpu().numpy()
            return np.ascontiguousarray((x * 255.0).astype(np.uint8).transpose(0, 2, 3, 1))

        variants = {"float": lib_call, "float+host": host_hand_over}
        for f in ("rgb24", "yuv420p"):
            variants[f] = lambda f=f: head.render_clip(codes, flame, randomize_noise=False, out=f)
            variants[f + "+host"] = lambda f=f: head.render_clip(codes, flame, randomize_noise=False, out=f, host=True)

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0), out

        head.reset_motion_state()
        ref = lib_call()
        same = {}
        for name, fn in variants.items():      # every variant shows the same frames (the EMA restarts before each)
            head.reset_motion_state()
            out = fn()
            if name == "float":
                same[name] = bool(torch.equal(out, ref))
            elif name == "float+host":      # the reference's cast wraps where ours clamps: the frames are in [0, 1], so none does
                same[name] = bool(np.array_equal(out, pack_frames(ref, "rgb24").cpu().numpy()))
            else:
                same[name] = bool(torch.equal(out.cpu(), pack_frames(ref, name.split("+")[0]).cpu()))
            for _ in range(args.warmup):
                wall(fn)
        ms, stage = {n: [] for n in variants}, {n: [] for n in variants}
        st = (C.c_double * len(STAGES))()
        for _ in range(args.rounds):
            for name, fn in variants.items():
                L.artalk_gaga_set_timing(head._h, 0)
                ms[name].append(wall(fn)[0])
                L.artalk_gaga_set_timing(head._h, 1)
                fn()
                L.artalk_gaga_get_timing(head._h, st, len(STAGES))
                stage[name].append(list(st))
        L.artalk_gaga_set_timing(head._h, 0)
        base = statistics.median(ms["float"])
        per_frame = {name: 12 * S * S if name.startswith("float") else frame_bytes(name.split("+")[0], S, S) for name in variants}

        def entry(name):
            stages = {n: statistics.median(s[i] for s in stage[name]) / T for i, n in enumerate(STAGES)}
            return {"ms_per_frame": {"median": statistics.median(ms[name]) / T, "min": min(ms[name]) / T, "max": max(ms[name]) / T},
                    "frames_per_s": 1e3 * T / statistics.median(ms[name]), "relative_to_float": statistics.median(ms[name]) / base,
                    "bytes_per_frame_out": per_frame[name],
                    "stage_ms_per_frame": stages, "finish_or_pack_share": stages["finish"] / sum(stages.values()),
                    "equals_the_float_frames_packed": same[name]}

        res = {
            "workload": f"GAGAvatar.render_clip by output, upsampler precision {args.precision}, S = {S}, V = {V}, N = {N}, T = {T} frames per call "
                        f"in slabs of {slab}, synthetic FLAME asset, avatar and upsampler weights, stored noise, {mark.shape[1]} x "
                        f"{mark.shape[2]} watermark, 68 forehead vertices; wall clock between device synchronisations (the host variants "
                        f"include host work), {args.warmup} warm-up calls per variant, {args.rounds} rounds in one process, each round running "
                        f"every variant in turn: a plain call and a stage-timed call.  float+host: .cpu(), then (x * 255).astype(uint8) and "
                        f"the transpose in numpy; +host of the 8-bit variants: pinned host tensor filled slab by slab on a copy stream",
            "variants": {name: entry(name) for name in variants},
        }
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    upper = {"state": None}

    def chain():
        pose = torch.cat([codes.new_zeros(T, 3), codes[:, 103:106]], dim=1)
        verts = flame(shape_params=dev["shapecode"][None].expand(T, -1), expression_params=codes[:, :100], pose_params=pose)
        fi = chain.forehead
        for t in range(T):      # the recurrence, frame by frame as the reference runs it
            cur = verts[t:t + 1, fi]
            if upper["state"] is None:
                upper["state"] = cur
            else:
                upper["state"] = 0.98 * upper["state"] + 0.02 * cur
                verts[t:t + 1, fi] = upper["state"]
        cam = camera_matrices(codes[:, 100:103].cpu(), av["transform_matrix"])[2].cuda()
        gs = {"xyz": torch.cat([verts, dev["xyz"][V:][None].expand(T, -1, -1)], dim=1), "colors": dev["colors"][None],
              "opacities": dev["opacities"][None], "scales": dev["scales"][None], "rotations": dev["rotations"][None]}
        images = render_gaussian(gs, cam, head.cam_params)["images"]
        rgb = unet(images, randomize_noise=False).clamp_(0, 1)
        h, w = dmark.shape[-2:]
        a = dmark[3:4] * 0.8
        rgb[..., -h:, -w:] = rgb[..., -h:, -w:] * (1 - a) + dmark[:3] * a
        return rgb

    chain.forehead = torch.tensor(FOREHEAD, dtype=torch.long, device="cuda")
    head.reset_motion_state()
    a = lib_call()
    upper["state"] = None
    b = chain()
    diff = float((a - b).abs().max())
    for _ in range(args.warmup):
        timed(lib_call)
        timed(chain)
    lib_ms, chain_ms, stage_ms = [], [], []
    st = (C.c_double * len(STAGES))()
    for _ in range(args.rounds):
        L.artalk_gaga_set_timing(head._h, 0)
        lib_ms.append(timed(lib_call)[0])
        L.artalk_gaga_set_timing(head._h, 1)
        lib_call()
        L.artalk_gaga_get_timing(head._h, st, len(STAGES))
        stage_ms.append(list(st))
        L.artalk_gaga_set_timing(head._h, 0)
        chain_ms.append(timed(chain)[0])
    med, cmed = statistics.median(lib_ms), statistics.median(chain_ms)
    stages = {n: statistics.median(s[i] for s in stage_ms) / T for i, n in enumerate(STAGES)}
    total = sum(stages.values())
    res = {
        "workload": f"GAGAvatar.render_clip, upsampler precision {args.precision}, S = {S}, V = {V}, N = {N}, T = {T} frames per call in slabs of {slab}, synthetic FLAME asset, avatar "
                    f"and upsampler weights, stored noise, {mark.shape[1]} x {mark.shape[2]} watermark, 68 forehead vertices; codes and frames "
                    f"on the device, output allocated inside the timed call; HIP events, {args.warmup} warm-up calls, median of {args.rounds} "
                    f"rounds alternating the call, the stage-timed call and the chain of separate Python calls",
        "ms_per_call": med, "ms_per_call_min": min(lib_ms), "ms_per_call_max": max(lib_ms), "ms_per_frame": med / T,
        "frames_per_s": 1e3 * T / med,
        "stage_ms_per_frame": stages, "stage_share": {n: v / total for n, v in stages.items()},
        "new_kernels_share": (stages["forehead_means"] + stages["finish"]) / total,
        "chain_ms_per_frame": cmed / T, "chain_ms_per_call_min_max": [min(chain_ms), max(chain_ms)],
        "speedup_over_chain": cmed / med,
        "max_abs_difference_to_chain": diff,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
