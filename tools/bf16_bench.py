"""The bf16 precision mode against the f16x3 default, in ONE process on the bench workload (full model, 32 synthetic 10 s clips
resident in HBM, hipGraph decode): the two modes alternate round by round (medians of ms per step and of the stage times of
get_profile), then the bf16 mode's error against the reference's golden fixtures (per-chunk AR-bit flip rate, FLAME max-abs).

    python tools/bf16_bench.py --rounds 5 --steps 3 --out profiles/r06_bf16_bench.json
    python tools/bf16_bench.py --only bf16 --rounds 1 --steps 2 --no-error      # one mode, e.g. under rocprofv3 --kernel-trace --stats

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

ERROR_CASES = ["tiny_4s_s0", "tiny_10s_s1_style", "tiny_6p3s_s2", "full_4s_s2", "full_10s_s1_style", "full_demo_eng1",
               "heavy_tiny_6p3s_s2", "heavy_full_4s_s2"]
PEAK_BF16_TFLOPS = 2500.0     # MI355X dense bf16 MFMA, nominal


def golden_inputs(g, sd):
    import numpy as np
    import torch
    from artalk_amd.synth import synth_audio, synth_style
    gdir = os.path.join(REPO, "tests", "golden")
    if "demo" in g.files:
        q = np.load(os.path.join(gdir, "demo_16k_s16.npz"))[str(g["demo"])]
        audio = torch.from_numpy(q.astype(np.float32) / np.float32(32768.0))
    else:
        audio = torch.from_numpy(synth_audio(int(g["seed"]), float(g["seconds"])))
    style = None
    if bool(g["with_style"]):
        style = torch.from_numpy(synth_style(int(g["seed"]), sd["basic_vae.motion_mean"].numpy(), sd["basic_vae.motion_std"].numpy()))
    return audio, style


def error_table(models):
    import numpy as np
    from artalk_amd.config import ARTalkConfig
    from artalk_amd.model import BitwiseARModel
    from artalk_amd.weights import generate_state_dict
    rows = []
    for case in ERROR_CASES:
        parts = case.split("_")
        profile, name = (parts[0], parts[1]) if parts[0] in ("heavy", "outlier") else ("benign", parts[0])
        key = (name, profile)
        if key not in models:
            cfg = ARTalkConfig.by_name(name)
            sd = generate_state_dict(cfg, profile=profile)
            m = BitwiseARModel(cfg).eval().to("cuda")
            m.load_state_dict(sd, strict=True)
            models[key] = (m, sd)
        m, sd = models[key]
        g = np.load(os.path.join(REPO, "tests", "golden", case + ".npz"))
        audio, style = golden_inputs(g, sd)
        m.set_precision("bf16")
        out = m.inference_batch([audio], [style], return_aux=True)[0].cpu().numpy()
        bits = m.last_aux["bits"][0].cpu().numpy()
        gbits = np.unpackbits(g["bits"], axis=-1)
        flips = (bits != gbits).reshape(bits.shape[0], -1).mean(axis=1)
        err = np.abs(out - g["out"])
        per_chunk = [float(err[j * 100:(j + 1) * 100].max()) for j in range(bits.shape[0])]
        rows.append({"case": case, "status": m.status(), "mode": m._precision, "finite": bool(np.isfinite(out).all()),
                     "flip_rate_per_chunk": [round(float(f), 5) for f in flips], "flame_maxabs_per_chunk": [float(f"{e:.4e}") for e in per_chunk],
                     "flip_rate_clip": round(float((bits != gbits).mean()), 5), "flame_maxabs_clip": float(f"{err.max():.4e}")})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        if key != ("full", "benign") and name == "full":
            del models[key]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two modes")
    ap.add_argument("--steps", type=int, default=3, help="timed steps per mode and round")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--only", default="", choices=["", "f16x3", "bf16"], help="time one mode only")
    ap.add_argument("--no-error", action="store_true", help="skip the error table")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from artalk_amd.config import ARTalkConfig
    from artalk_amd.model import BitwiseARModel
    from artalk_amd.synth import synth_audio
    from artalk_amd.weights import generate_state_dict

    cfg = ARTalkConfig.full()
    sd = generate_state_dict(cfg)
    model = BitwiseARModel(cfg).eval().to("cuda")
    model.load_state_dict(sd, strict=True)
    model.set_graphs(True)
    B = args.batch
    n = int(round(args.seconds * 16000))
    model.reserve(B, B * model.n_chunks(n))
    audio = [torch.from_numpy(synth_audio(i, args.seconds)).cuda() for i in range(B)]
    frames = model.seq_length(n)
    modes = [args.only] if args.only else ["f16x3", "bf16"]
    for mode in modes:                       # warm-up: graphs captured, bf16 copy built
        model.set_precision(mode)
        model.inference_batch(audio)
        model.inference_batch(audio)
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    stages = {m: [] for m in modes}
    for _ in range(args.rounds):
        for mode in modes:
            model.set_precision(mode)
            model.inference_batch(audio)
            torch.cuda.synchronize()
            model.set_profiling(1)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                model.inference_batch(audio, check=False)
            torch.cuda.synchronize()
            ms[mode].append((time.perf_counter() - t0) / args.steps * 1e3)
            stages[mode].append(model.get_profile())
            model.set_profiling(0)
            assert model.status() == 0, f"{mode}: status {model.status()}"
    res = {"workload": f"full model, {B} x {args.seconds:g} s synthetic clips, audio resident, hipGraph decode",
           "rounds": args.rounds, "steps_per_round": args.steps, "modes": {}}
    for mode in modes:
        med = statistics.median(ms[mode])
        st = {k: round(statistics.median(p[k] for p in stages[mode]), 3) for k in stages[mode][0]}
        r = {"ms_per_step_median": round(med, 2), "ms_per_step_rounds": [round(x, 2) for x in ms[mode]],
             "frames_per_s": round(B * frames / (med * 1e-3), 1), "stages_ms_median": st}
        if mode == "bf16" and st.get("dom_ms", 0) > 0:
            tf = st["dom_flop"] / (st["dom_ms"] * 1e-3) / 1e12
            r["dominant_kernel"] = {"kernel": "gemm_bf16_kernel<128,128> register-staged (eager launches)", "tflops": round(tf, 1),
                                    "frac_of_bf16_peak": round(tf / PEAK_BF16_TFLOPS, 4), "peak_tflops": PEAK_BF16_TFLOPS}
        res["modes"][mode] = r
    if len(modes) == 2:
        res["bf16_over_f16x3"] = round(res["modes"]["bf16"]["ms_per_step_median"] / res["modes"]["f16x3"]["ms_per_step_median"], 4)
    if not args.no_error:
        model.set_precision("bf16")
        res["error"] = error_table({("full", "benign"): (model, sd)})
        res["reference_bf16_autocast"] = "BASELINE.md: 1.4-7.6 % AR bits flipped per chunk, 1.3e-2 FLAME max-abs"
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
