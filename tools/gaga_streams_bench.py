"""Live streams through the GAGAvatar head at the reference's shape (S = 512, V = 5 023, N = 180 255, everything synthetic as in
tools/gaga_bench.py): 8 streams on 4 avatars, 25 frames each, 8-bit yuv420p frames handed to the host.

Three variants alternate in every round of the one process, by the wall clock between device synchronisations:
  a  ``render_streams(order="time", out="yuv420p", host=True)``: one call, frame k of every stream before frame k + 1 of any;
  b  the same with ``order="stream"``;
  c  what there was before: one ``GAGAvatar`` per stream (each with its own scratch and its own copy of its avatar) and
     ``render_clip(out="yuv420p", host=True)`` for each in turn.
Recorded: ms per frame (median, min - max over the rounds); for a and b the time from the call's start until frame 0 of the LAST stream
is on the host (a watcher thread polls the frame's last byte in the pinned buffer, which is cleared before the call - the V plane of a
limited-range frame holds no zero - and sleeps 0.2 ms between two looks; in c that frame follows the seven calls before the last
head's, so c's time per call tells it); the device memory in use by a's head against c's eight, from ``torch.cuda.mem_get_info``
around building and warming up each; a's stage split from the library's stage timer.  a and b fill one pinned buffer made before the
rounds, c's eight calls make a pinned tensor each inside the timed region (``render_clip`` has no other form): what those eight
allocations alone cost is timed beside c in every round and reported as c's share, so the gap between a and c can be read without it.
No target is set: the upsampler is 88 % of a frame and is the same code on every path, so the per-frame times should be about equal.

    python tools/gaga_streams_bench.py --out profiles/gaga_streams_bench.json

Prints one JSON line; --out also writes it to a file.  Needs the GPU: without one it fails.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaga_bench import FOREHEAD, STAGES, V, motion, synthetic_avatar      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--avatars", type=int, default=4)
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from artalk_amd import capi
    from artalk_amd.flame import FLAMEModel, synthetic_flame_asset
    from artalk_amd.frames import frame_shape
    from artalk_amd.gaga import GAGAvatar
    from artalk_amd.styleunet import StyleUNet, synth_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("gaga_streams_bench needs the GPU")
    S, n, F = args.size, args.streams, args.frames
    T = n * F
    L = capi.lib()
    flame = FLAMEModel(300, 100, scale=5.0, no_lmks=True, flame_ckpt=synthetic_flame_asset())
    unet = StyleUNet(S, S, 32, 3).eval().to("cuda:0")      # one set of weights for every head
    unet.load_state_dict(synth_state_dict(S))
    avatars = {f"id{k}": synthetic_avatar(seed=k) for k in range(args.avatars)}
    names = [f"id{i % args.avatars}" for i in range(n)]
    N = int(avatars["id0"]["xyz"].shape[0])
    mark = torch.from_numpy(np.random.default_rng(2).random((4, min(82, S), min(256, S)), dtype=np.float32))
    codes = torch.stack([motion(F, seed=10 + i) for i in range(n)]).cuda()      # (n, F, 106)
    make = lambda avs: GAGAvatar(avs, unet, water_mark=mark, image_size=S, n_dynamic=V, forehead_indices=FOREHEAD)

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    # ---- a and b: one head, resident avatars, one call
    base = used()
    head = make(avatars).set_resident(args.avatars)
    streams = [head.open_stream(a) for a in names]
    buf = torch.empty(frame_shape("yuv420p", T, S, S), dtype=torch.uint8, pin_memory=True)
    flat = buf.view(T, -1).numpy()

    def one_call(order):
        target = {"time": n - 1, "stream": (n - 1) * F}[order]      # frame 0 of the last stream
        flat[target, -1] = 0
        seen = {}

        def watch():
            while "stop" not in seen:
                if flat[target, -1] != 0:
                    seen["t"] = time.perf_counter()
                    return
                time.sleep(2e-4)

        th = threading.Thread(target=watch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        th.start()
        head.render_streams(streams, codes, flame, order=order, randomize_noise=False, out="yuv420p", host=True, host_buffer=buf)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        seen["stop"] = True
        th.join()
        return 1e3 * (t1 - t0), 1e3 * (seen.get("t", t1) - t0)

    for _ in range(args.warmup):
        one_call("time")
        one_call("stream")
    slab = head.stream_slab_in_force()
    mem_a = used() - base

    # ---- c: one head per stream
    base_c = used()
    heads = [make({a: avatars[a]}) for a in names]
    for h, a in zip(heads, names):
        h.set_avatar_id(a)

    def per_stream():
        return [h.render_clip(codes[i], flame, randomize_noise=False, out="yuv420p", host=True) for i, h in enumerate(heads)]

    for _ in range(args.warmup):
        per_stream()
    mem_c = used() - base_c

    # the same bytes on both paths (the EMA restarts before each)
    for st in streams:
        st.reset()
    for h in heads:
        h.reset_motion_state()
    one_call("stream")
    want = torch.cat(per_stream())
    same = bool(torch.equal(buf, want))

    def pinned_alone():      # the eight pinned result tensors c's calls make, and nothing else
        return [torch.empty(frame_shape("yuv420p", F, S, S), dtype=torch.uint8, pin_memory=True) for _ in heads]

    ms = {"a": [], "b": [], "c": [], "pinned": []}
    first = {"a": [], "b": []}
    stage = []
    st = (C.c_double * len(STAGES))()
    for _ in range(args.rounds):
        for key, order in (("a", "time"), ("b", "stream")):
            total, t_first = one_call(order)
            ms[key].append(total)
            first[key].append(t_first)
        ms["c"].append(wall(per_stream)[0])
        ms["pinned"].append(wall(pinned_alone)[0])
        L.artalk_gaga_set_timing(head._h, 1)
        one_call("time")
        L.artalk_gaga_get_timing(head._h, st, len(STAGES))
        L.artalk_gaga_set_timing(head._h, 0)
        stage.append(list(st))

    def entry(key):
        e = {"ms_per_frame": {"median": statistics.median(ms[key]) / T, "min": min(ms[key]) / T, "max": max(ms[key]) / T},
             "ms_per_call": statistics.median(ms[key])}
        if key in first:
            e["ms_until_frame_0_of_the_last_stream_is_on_the_host"] = {"median": statistics.median(first[key]), "min": min(first[key]),
                                                                        "max": max(first[key])}
        return e

    stages = {k: statistics.median(s[i] for s in stage) / T for i, k in enumerate(STAGES)}
    res = {
        "workload": f"{n} streams on {args.avatars} avatars, {F} frames each, S = {S}, V = {V}, N = {N}, synthetic FLAME asset, avatars and "
                    f"upsampler weights (f32), stored noise, {mark.shape[1]} x {mark.shape[2]} watermark, 68 forehead vertices, yuv420p frames "
                    f"to pinned host memory; slabs of {slab}; wall clock between device synchronisations, {args.warmup} warm-up calls per "
                    f"variant, {args.rounds} rounds in one process, each round running a, b and c in turn and a stage-timed a",
        "variants": {"a_render_streams_time": entry("a"), "b_render_streams_stream": entry("b"), "c_one_head_per_stream_render_clip": entry("c")},
        "a_relative_to_c": statistics.median(ms["a"]) / statistics.median(ms["c"]),
        "c_pinned_allocation_ms_per_frame": {"median": statistics.median(ms["pinned"]) / T, "min": min(ms["pinned"]) / T, "max": max(ms["pinned"]) / T},
        "a_relative_to_c_without_the_allocation": statistics.median(ms["a"]) / (statistics.median(ms["c"]) - statistics.median(ms["pinned"])),
        "a_stage_ms_per_frame": stages,
        "device_bytes": {"a_one_head_resident_avatars": int(mem_a), "c_one_head_per_stream": int(mem_c)},
        "a_and_c_give_the_same_bytes": same,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
