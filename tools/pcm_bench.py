"""Live audio in: what feeding raw packets costs.  32 streams of 48 kHz stereo s16 in 20 ms packets (960 frames, 3 840 bytes each), one
4-s block (200 packets a stream) per round, on the tiny model's engine (the front door does not depend on the model's size).

Two variants alternate in every round of the one process, by the wall clock:
  a  ``engine.stream_feed(streams, packets)`` for all 32 streams, 200 times, then one ``LiveAudio.take`` of the 32 blocks and a device
     synchronisation: microseconds per feed = the round's time / 200.  The host's time inside each call (no synchronisation) is
     recorded beside it.
  b  what a caller does today: every packet appended to its stream's host buffer (200 x 32 appends), then per stream one
     ``resample_mean_16k`` of the block's (2, 192 000) float32 signal (int16 -> float32 / 32768 on the host, as ``read_wav`` does) and a
     device synchronisation; the same division by 200.  (b's blocks carry a filter edge every 4 s, which a's do not; the bits are
     compared once, on a block's interior.)
No target is set: a 32-stream push moves about 120 KB in and 40 KB out, so it is bound by launch and copy latency.  Recorded: both
times with their ranges over the rounds (five, or more - up to --max-rounds - while the two ranges overlap), and the share of a 4-s
step (README: 8.2 ms for one stream, 28.6 ms for 32) that a round's 200 feeds add.

    python tools/pcm_bench.py --out profiles/pcm_bench.json

Prints one JSON line; --out also writes it to a file.  Needs the GPU: without one it fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from artalk_amd.audio import resample_mean_16k
    from artalk_amd.config import ARTalkConfig
    from artalk_amd.engine import ARTAvatarInferEngine
    from artalk_amd.model import BitwiseARModel
    from artalk_amd.weights import generate_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("pcm_bench needs the GPU")
    n, sr, nch, pkt, per_block = args.streams, 48000, 2, 960, 200
    cfg = ARTalkConfig.tiny()
    model = BitwiseARModel(cfg).eval().to("cuda:0")
    model.load_state_dict(generate_state_dict(cfg), strict=True)
    eng = ARTAvatarInferEngine(model=model)
    streams = [eng.open_stream(audio=(sr, nch, "s16")) for _ in range(n)]
    audio = eng._audio_of(streams)
    live = eng.live_audio
    g = np.random.default_rng(1)
    # one block's packets per stream, reused every round (the streams just go on)
    pcm = (g.standard_normal((n, per_block * pkt, nch)) * 6000).clip(-32768, 32767).astype("<i2")
    packets = [[pcm[i, k * pkt:(k + 1) * pkt].tobytes() for i in range(n)] for k in range(per_block)]

    def variant_a():
        host = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(per_block):
            h0 = time.perf_counter()
            eng.stream_feed(streams, packets[k])
            host.append(time.perf_counter() - h0)
        blocks = None
        if all(live.ready(a) for a in audio):      # (the first round holds 6 samples less than a block: the filter's latency)
            blocks, _ = live.take(audio)
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / per_block, 1e6 * statistics.median(host), blocks

    def variant_b():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bufs = [bytearray() for _ in range(n)]
        for k in range(per_block):
            for i in range(n):
                bufs[i] += packets[k][i]
        blocks = []
        for i in range(n):
            w = torch.from_numpy((np.frombuffer(bufs[i], dtype="<i2").astype(np.float32) / 32768.0).reshape(-1, nch).T.copy())
            blocks.append(resample_mean_16k(w, sr, "cuda"))
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / per_block, torch.stack(blocks)

    for _ in range(args.warmup):
        variant_a()
        variant_b()
    # the same bits away from b's block edges: every round feeds the same 192 000 frames = 64 000 samples, and a takes whole blocks, so
    # sample i of a's block and of b's read the same frames - except near the edges, where b's filter sees zeros and a's the neighbour block
    _, _, blocks_a = variant_a()
    _, blocks_b = variant_b()
    same = None if blocks_a is None else bool(torch.equal(blocks_a[:, 64:63900], blocks_b[:, 64:63900]))

    a_us, a_host, b_us = [], [], []
    rounds = 0
    while rounds < args.rounds or (rounds < args.max_rounds and max(a_us) >= min(b_us) and max(b_us) >= min(a_us)):
        t, h, _ = variant_a()
        a_us.append(t)
        a_host.append(h)
        b_us.append(variant_b()[0])
        rounds += 1

    def entry(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    a_med = statistics.median(a_us)
    res = {
        "workload": f"{n} streams, {sr} Hz, {nch} channels, s16, packets of {pkt} frames ({pkt * nch * 2} bytes), {per_block} packets a stream "
                    f"per round (one 4-s block); tiny model's engine; wall clock, one device synchronisation at the end of a round; "
                    f"{args.warmup} warm-up round(s), {rounds} rounds in one process, each running a then b",
        "a_stream_feed_us_per_feed_of_all_streams": entry(a_us),
        "a_host_us_inside_one_stream_feed_call": entry(a_host),
        "b_host_accumulation_and_resample_mean_16k_per_stream_us_per_feed": entry(b_us),
        "a_relative_to_b": a_med / statistics.median(b_us),
        "ranges_overlap": bool(max(a_us) >= min(b_us) and max(b_us) >= min(a_us)),
        "a_200_feeds_ms": a_med * per_block / 1e3,
        "a_200_feeds_share_of_a_4s_step": {"of_8.2_ms_one_stream": a_med * per_block / 1e3 / 8.2, "of_28.6_ms_32_streams": a_med * per_block / 1e3 / 28.6},
        "a_and_b_give_the_same_bits_inside_a_block": same,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
