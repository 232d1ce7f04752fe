"""Milliseconds per avatar of the Gaussian generators (``GSGenerators.build_avatar`` = one ``artalk_gsgen_generate`` call) at the
reference's shape: V = 5 023 rows of ``head_base`` (256 wide), a 768-wide class token, a (256, 296, 296) feature map, N = 180 255
Gaussians.  Weights and features are synthetic (``synth_state_dict``, standard-normal features): GAGAvatar's checkpoint is not at hand.

Three kinds of call alternate in every round, each between HIP events, medians over the rounds:
  - the library call, outputs on the device (the figure that counts);
  - the same with the library's timing on (it adds event pairs around the conv launches and waits at the end of the call): the conv
    kernels' share of the call, and TF/s on the convs' multiply-adds (counted from the shapes);
  - the float32 restatement (tests/gsgen_ref.py) through PyTorch-ROCm on the same device, weights already there: what a user had
    before this call existed.
No target is set.  ``fraction_of_fp32_mfma_floor`` is the time the convs' multiply-adds would take at 157 TF/s (the fp32 MFMA rate
DESIGN.md uses) over the measured conv time.

    python tools/gsgen_bench.py --out profiles/gsgen_bench.json

Prints one JSON line; --out also writes it to a file.  Needs the GPU: without one it fails.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

DIMS = (5023, 256, 768, 256, 296)
FP32_MFMA_TFLOPS = 157.0


def conv_flops(V, Dh, Dg, C, P):
    """2 x the multiply-adds of every conv launch of one call."""
    hid, chid = (Dh + Dg) // 4, C // 2
    local = P * P * (9 * (C + 27) * chid + 2 * 9 * chid * chid + chid * 41)
    glob = V * ((Dh + Dg) * hid + 3 * hid * hid + 4 * (hid + 27) * 128 + 128 * (32 + 1 + 3 + 4))
    return 2 * (2 * local + glob)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "gsgen_bench.py needs the GPU"
    import gsgen_ref
    from artalk_amd import gsgen

    sd = gsgen.synth_state_dict(*DIMS, seed=0)
    gen = gsgen.GSGenerators(*DIMS).load_state_dict(sd)
    g = torch.Generator().manual_seed(1)
    f0, f1 = torch.randn(DIMS[3], DIMS[4], DIMS[4], generator=g).cuda(), torch.randn(DIMS[2], generator=g).cuda()
    tm = torch.tensor([[-1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 5000.0 / 512]])
    shapecode = torch.zeros(300)
    sd_dev = {k: v.cuda() for k, v in sd.items()}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    ours = lambda: gen.build_avatar(f0, f1, tm, shapecode, device="cuda")
    with torch.no_grad():
        theirs = lambda: gsgen_ref.generate(sd_dev, f0, f1, tm, torch.float32, device="cuda")
        for _ in range(a.warmup):
            ours()
            theirs()
        torch.cuda.synchronize()
        call, conv, total, torch_ms = [], [], [], []
        for _ in range(a.rounds):
            ms, got = timed(ours)
            call.append(ms)
            gen.set_timing(True)
            ours()
            gen.set_timing(False)
            c, t = gen.timing()
            conv.append(c)
            total.append(t)
            ms, want = timed(theirs)
            torch_ms.append(ms)
    diff = {k: float((got[k] - want[k]).abs().max()) for k in ("xyz", "colors", "opacities", "scales", "rotations")}
    flops = conv_flops(*DIMS)
    med = statistics.median
    res = {
        "workload": f"GSGenerators.build_avatar at (V, Dh, Dg, C, P) = {DIMS}, N = {gen.n_gaussians}, synthetic weights and features, features and "
                    f"outputs on the device, output allocated inside the timed call; HIP events, {a.warmup} warm-up calls, median of {a.rounds} rounds "
                    "alternating the library call, the same with its timing on and the float32 torch restatement on the same device",
        "ms_per_avatar": med(call), "ms_per_avatar_min_max": [min(call), max(call)],
        "library_call_ms": med(total), "conv_ms": med(conv), "conv_share_of_call": med(conv) / med(total),
        "conv_gflop": flops / 1e9, "conv_tflops": flops / (med(conv) * 1e-3) / 1e12,
        "fraction_of_fp32_mfma_floor": (flops / (FP32_MFMA_TFLOPS * 1e12)) / (med(conv) * 1e-3),
        "torch_ms_per_avatar": med(torch_ms), "torch_ms_min_max": [min(torch_ms), max(torch_ms)],
        "speedup_over_torch": med(torch_ms) / med(call), "max_abs_difference_to_torch": diff,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
