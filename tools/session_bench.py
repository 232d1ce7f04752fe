"""What the session pool costs per step: ``step_sessions`` (gather + chunk step + scatter) against lockstep ``stream_chunk`` (the chunk
step alone) in ONE process, alternating round by round, on bench.py's ``stream_chunk_ms`` workload - the full model, one 4-second block
per stream, pinned host chunk in -> pinned host codes out, synchronous calls - at n = 1 and n = 32 streams.  The yardstick is lockstep
in the same run on the same box, never a number from another run (boxes and runs differ by +-2 %).

    python tools/session_bench.py --rounds 5 --calls 6 --out profiles/sessions_step_ab.json
    python tools/session_bench.py --config tiny --rounds 2 --calls 3        # a quick look

``--variant smooth`` measures the streaming smoother the same way: the engine's ``stream_step(smooth=True)`` (the session step + one
``artalk_session_smooth`` launch, up to 104 frames back per stream) against ``stream_step(smooth=False)`` on sessions of their own, same
process, alternating rounds.  Every timed smooth call is a stream's middle call (100 frames in, 100 out).

    python tools/session_bench.py --variant smooth --rounds 5 --calls 6 --out profiles/sessions_smooth_ab.json

Prints one JSON line; --out also writes it to a file.
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
    ap.add_argument("--config", default="full", choices=["full", "tiny"])
    ap.add_argument("--rounds", type=int, default=5, help="alternations of lockstep and sessions per stream count")
    ap.add_argument("--calls", type=int, default=6, help="timed synchronous calls per mode and round")
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--variant", default="step", choices=["step", "smooth"], help="step: sessions against lockstep; smooth: smooth=True against smooth=False")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from artalk_amd.config import ARTalkConfig
    from artalk_amd.model import BitwiseARModel
    from artalk_amd.synth import synth_audio
    from artalk_amd.weights import generate_state_dict

    cfg = ARTalkConfig.by_name(args.config)
    model = BitwiseARModel(cfg).eval().to("cuda")
    model.load_state_dict(generate_state_dict(cfg), strict=True)
    model.set_precision(args.precision)
    dev = model.device
    spc = cfg.samples_per_chunk
    nmax = max(args.streams)
    model.reserve(nmax, nmax)
    model.reserve_sessions(2 * nmax if args.variant == "smooth" else nmax)
    host_audio = [torch.from_numpy(synth_audio(i, 10.0)) for i in range(min(nmax, 32))]

    def timed(fn):
        ts = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    if args.variant == "smooth":
        from artalk_amd.engine import ARTAvatarInferEngine
        eng = ARTAvatarInferEngine(model=model)
        res = {"workload": f"{args.config} model, {args.precision}: one 4-s block per stream through ARTAvatarInferEngine.stream_step, pinned host chunk "
                           "in -> pinned host frames out, synchronous calls; raw = smooth=False (100 x 106 per stream), smooth = smooth=True "
                           "(the same step + artalk_session_smooth, 104 x 106 per stream copied back)",
               "rounds": args.rounds, "calls_per_round": args.calls, "streams": {}}
        for nb in args.streams:
            chunk_host = torch.stack([host_audio[i % len(host_audio)][:spc] for i in range(nb)]).pin_memory()
            raw_host = torch.empty(nb, 100, cfg.motion_dim).pin_memory()
            smooth_host = torch.empty(nb, 104, cfg.motion_dim).pin_memory()
            plain, smoothed = model.open_sessions([None] * nb), model.open_sessions([None] * nb)

            def raw_call():
                raw_host.copy_(eng.stream_step(plain, chunk_host.to(dev, non_blocking=True)), non_blocking=False)

            def smooth_call():
                smooth_host.copy_(eng.stream_step(smoothed, chunk_host.to(dev, non_blocking=True), smooth=True)[0], non_blocking=False)

            ms = {"raw": [], "smooth": []}
            for r in range(args.rounds + 1):          # round 0 warms up (and is every smoothed stream's first call)
                raw_call()
                t_raw = timed(raw_call)
                smooth_call()
                t_smooth = timed(smooth_call)
                if r:
                    ms["raw"].append(t_raw)
                    ms["smooth"].append(t_smooth)
                assert model.status() == 0 and model._precision == args.precision
            model.close_sessions(plain + smoothed)
            a, b = statistics.median(ms["raw"]), statistics.median(ms["smooth"])
            res["streams"][f"n{nb}"] = {
                "raw_ms_median": round(a, 3), "smooth_ms_median": round(b, 3), "smooth_over_raw": round(b / a, 4),
                "extra_us": round((b - a) * 1e3, 1), "raw_ms_rounds": [round(x, 3) for x in ms["raw"]],
                "smooth_ms_rounds": [round(x, 3) for x in ms["smooth"]],
                "smoother_bytes_moved_per_step": nb * 4 * cfg.motion_dim * (100 + 100 + 2 * 9)}
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return

    res = {"workload": f"{args.config} model, {args.precision}: one 4-s block (100 frames) per stream, pinned host chunk in -> pinned host codes "
                       "out, synchronous calls; lockstep = stream_chunk, sessions = step_sessions (gather + the same chunk step + scatter)",
           "rounds": args.rounds, "calls_per_round": args.calls, "streams": {}}
    for nb in args.streams:
        chunk_host = torch.stack([host_audio[i % len(host_audio)][:spc] for i in range(nb)]).pin_memory()
        out_host = torch.empty(nb, 100, cfg.motion_dim).pin_memory()

        def lockstep_call():
            out_host.copy_(model.stream_chunk(chunk_host.to(dev, non_blocking=True)), non_blocking=False)

        def session_call():
            out_host.copy_(model.step_sessions(sessions, chunk_host.to(dev, non_blocking=True)), non_blocking=False)

        sessions = model.open_sessions([None] * nb)
        ms = {"lockstep": [], "sessions": []}
        for r in range(args.rounds + 1):          # round 0 warms up: graphs captured, allocator settled
            model.stream_begin(nb)                # (a session call ends the lockstep session: it lives in the workspace)
            lockstep_call()
            t_lock = timed(lockstep_call)
            model.stream_end()
            session_call()
            t_sess = timed(session_call)
            if r:
                ms["lockstep"].append(t_lock)
                ms["sessions"].append(t_sess)
            assert model.status() == 0 and model._precision == args.precision
        model.close_sessions(sessions)
        lock, sess = statistics.median(ms["lockstep"]), statistics.median(ms["sessions"])
        res["streams"][f"n{nb}"] = {
            "lockstep_ms_median": round(lock, 3), "sessions_ms_median": round(sess, 3),
            "sessions_over_lockstep": round(sess / lock, 4), "extra_us": round((sess - lock) * 1e3, 1),
            "lockstep_ms_rounds": [round(x, 3) for x in ms["lockstep"]], "sessions_ms_rounds": [round(x, 3) for x in ms["sessions"]],
            "state_bytes_moved_per_step": 2 * nb * 4 * (cfg.embed_dim * 182 + 100 * cfg.code_dim) - nb * 4 * cfg.embed_dim}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
