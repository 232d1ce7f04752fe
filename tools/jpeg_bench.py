"""JPEG out at the serving shape: 512 x 512 rgb24 frames, F = 64, quality 90, both subsamplings, on smooth synthetic pictures (sums of
low-frequency waves, a hard-edged stripe pattern and a little noise: what a rendered head looks like to a codec).

Variants alternate in every round of the one process, by the wall clock between device synchronisations (a device variant's window
holds 20 calls, since one takes a fraction of a millisecond; a Pillow variant's holds one pass over the 64 frames):
  a  ``encode_jpeg`` on the device: the streams stay there;
  b  ``encode_jpeg(host=True)``: the slots and sizes in pinned host memory;
  c  what a caller does today: the rgb24 frames to the host, then Pillow's ``Image.save(..., "JPEG")`` per frame, on one thread;
  d  the same on 16 threads.
c and d are skipped, with a note, on a machine without Pillow.  Recorded: ms per frame (median, min - max over the rounds), bytes per
frame, the share of each of the two launches (the encoder's own event timer, in a run of its own each round), and the fraction of the
bytes floor - one read of the rgb24 frame plus one write of its stream at the HBM's measured streaming rate (6.29 TB/s).  b copies whole
slots, ``cap`` bytes a frame: its cap is the largest stream of a's run rounded up to 4 KiB, as a sender that knows its pictures would
choose it, and the default cap (H W 3 + 1024) is timed beside it.  No target is set.

    python tools/jpeg_bench.py --out profiles/jpeg_bench.json

Prints one JSON line; --out also writes it to a file.  Needs the GPU: without one it fails.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BYTES_PER_S = 6.29e12


def pictures(F, S, device):
    """(F, S, S, 3) uint8 on the device: smooth, colourful, every frame different."""
    import torch
    g = torch.Generator(device=device).manual_seed(5)
    y, x = torch.meshgrid(torch.arange(S, device=device, dtype=torch.float32), torch.arange(S, device=device, dtype=torch.float32), indexing="ij")
    t = torch.arange(F, device=device, dtype=torch.float32)[:, None, None]
    r = 128 + 90 * torch.sin(0.021 * x + 0.3 * t) * torch.cos(0.013 * y)
    gch = 128 + 80 * torch.cos(0.017 * y + 0.005 * x + 0.2 * t)
    b = torch.where(((x + 2 * y + 3 * t) % 97) < 40, 60.0, 200.0) + 0 * t
    img = torch.stack([r, gch, b.expand_as(r)], dim=-1) + 3.0 * torch.randn(F, S, S, 3, device=device, generator=g)
    return img.clamp(0, 255).to(torch.uint8).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20, help="calls of a device variant inside one timed window (a call takes a fraction of a millisecond)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from artalk_amd import frames

    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench needs the GPU")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    S, F, q = args.size, args.frames, args.quality
    rgb = pictures(F, S, "cuda")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def stats(v):
        return {"median": statistics.median(v) / F, "min": min(v) / F, "max": max(v) / F}

    res = {"workload": f"{F} rgb24 frames of {S} x {S}, smooth synthetic pictures, quality {q}; wall clock between device synchronisations, "
                       f"{args.calls} calls per window of a device variant, {args.warmup} warm-up windows per variant, {args.rounds} rounds in one process, each round running every variant in turn "
                       f"and one launch-timed call; ms are per frame",
           "variants": {}}
    for ss in ("420", "444"):
        enc = frames.JpegEncoder(quality=q, subsampling=ss)
        data, sizes = enc.encode(rgb)
        sizes_host = sizes.cpu()
        assert int(sizes_host.min()) > 0
        mean_bytes = float(sizes_host.double().mean())
        tight = (int(sizes_host.max()) + 4095) // 4096 * 4096
        pil_ss = 2 if ss == "420" else 0

        def pillow_one(x):
            out = io.BytesIO()
            Image.fromarray(x).save(out, "JPEG", quality=q, subsampling=pil_ss)
            return out.tell()

        def host_then_pillow(threads):
            host = rgb.cpu().numpy()
            if threads == 1:
                return sum(pillow_one(x) for x in host)
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(threads) as pool:
                return sum(pool.map(pillow_one, host))

        def calls(**kw):      # the pinned results of b are made inside the window, as a caller's would be
            def run():
                for _ in range(args.calls):
                    out = enc.encode(rgb, **kw)
                return out
            return run

        variants = {"a_device": calls(cap=tight), "b_host_tight_cap": calls(cap=tight, host=True), "b_host_default_cap": calls(host=True)}
        per_window = {k: args.calls for k in variants}
        if Image is not None:
            variants["c_pillow_1_thread"] = lambda: host_then_pillow(1)
            variants[f"d_pillow_{args.threads}_threads"] = lambda: host_then_pillow(args.threads)
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        ms = {k: [] for k in variants}
        launches = []
        pillow_bytes = None
        for _ in range(args.rounds):
            for k, fn in variants.items():
                t, out = wall(fn)
                ms[k].append(t / per_window.get(k, 1))
                if k.startswith("c_"):
                    pillow_bytes = out / F
            enc.set_timing(True)
            enc.encode(rgb, cap=tight)
            launches.append(enc.launch_ms())
            enc.set_timing(False)
        rows, pack = (statistics.median(l[i] for l in launches) for i in range(2))
        floor_ms = (S * S * 3 + mean_bytes) / HBM_BYTES_PER_S * 1e3
        entry = {k: stats(v) for k, v in ms.items()}
        entry.update({
            "bytes_per_frame": mean_bytes, "largest_stream": int(sizes_host.max()), "tight_cap": tight, "default_cap": frames.jpeg_default_cap(S, S),
            "launch_ms_per_frame": {"rows_kernel": rows / F, "pack_kernel": pack / F},
            "launch_share": {"rows_kernel": rows / (rows + pack), "pack_kernel": pack / (rows + pack)},
            "bytes_floor_ms_per_frame_at_6.29TBps": floor_ms, "fraction_of_bytes_floor": floor_ms / (statistics.median(ms["a_device"]) / F),
        })
        if Image is not None:
            entry["pillow_bytes_per_frame"] = pillow_bytes
            entry["a_relative_to_pillow_1_thread"] = statistics.median(ms["a_device"]) / statistics.median(ms["c_pillow_1_thread"])
            entry["b_relative_to_pillow_%d_threads" % args.threads] = (statistics.median(ms["b_host_tight_cap"])
                                                                      / statistics.median(ms[f"d_pillow_{args.threads}_threads"]))
        else:
            entry["note"] = "Pillow is not importable on this machine: the host variants c and d were skipped"
        res["variants"][ss] = entry
        enc.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
