"""Milliseconds per avatar of the DINO features (``DINOBase.forward`` = one ``artalk_dino_forward`` call) at the reference's shape: a
518 x 518 image, ViT-B/14 (768 wide, 12 blocks, 12 heads, 1 370 tokens), the DPT head up to the (256, 296, 296) feature plane.  Weights
and image are synthetic (``synth_state_dict``, ``--dims`` for another shape): GAGAvatar's checkpoint is not at hand.

Three kinds of call alternate in every round, each between HIP events, medians over the rounds:
  - the library call, outputs on the device (the figure that counts);
  - the same with the library's timing on (it marks the stages with events and waits at the end of the call): the share of the ViT and
    head GEMMs, the attention, the head's convs and everything else;
  - the float32 restatement (tests/dino_ref.py) through PyTorch-ROCm on the same device, weights already there: what a user had before
    this call existed.
No target is set.  ``fraction_of_fp32_mfma_floor`` is the time the multiply-adds of the GEMMs, the attention and the convs (counted from
the shapes) would take at 157 TF/s (the fp32 MFMA rate DESIGN.md uses) over the measured time of those three stages.

    python tools/dino_bench.py --out profiles/dino_bench.json

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

DIMS = (256, 768, 12, 12, 37)
FP32_MFMA_TFLOPS = 157.0
PROJ, HID = (256, 512, 1024, 1024), 256


def flops(od, D, depth, heads, g):
    """2 x the multiply-adds of one call: (the GEMMs, the attention, the stride-1 convs)."""
    G, T = g * g, g * g + 1
    hs = (4 * g, 2 * g, g, (g - 1) // 2 + 1)
    gemm = G * 608 * D + depth * T * (3 * D * D + D * D + 8 * D * D)
    gemm += sum(G * D * c for c in PROJ) + G * 16 * PROJ[0] ** 2 + G * 4 * PROJ[1] ** 2 + hs[3] ** 2 * 9 * PROJ[3] ** 2
    attn = depth * 2 * T * T * D
    conv = sum(h * h * 9 * (c + 3) * HID for h, c in zip(hs, PROJ))
    conv += sum(h * h * 9 * HID * HID * (2 if j == 3 else 4) for j, h in enumerate(hs))      # the residual units (refinenet.0 runs one)
    conv += sum(h * h * HID * HID for h in (hs[2], hs[1], hs[0], 8 * g))                        # out_conv at the next level's size
    conv += (8 * g) ** 2 * 9 * HID * od
    return 2 * gemm, 2 * attn, 2 * conv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", type=int, nargs=5, default=DIMS, metavar=("OUT", "VIT", "DEPTH", "HEADS", "GRID"))
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "dino_bench.py needs the GPU"
    import dino_ref
    from artalk_amd import dino

    dims = tuple(a.dims)
    sd = dino.synth_state_dict(*dims, seed=0)
    net = dino.DINOBase(*dims).load_state_dict(sd)
    S = net.image_size
    img = torch.rand(3, S, S, generator=torch.Generator().manual_seed(1)).cuda()
    sd_dev = {k: v.cuda() for k, v in sd.items()}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    ours = lambda: net.forward(img)
    with torch.no_grad():
        theirs = lambda: dino_ref.forward(sd_dev, img, dims, torch.float32, device="cuda")
        for _ in range(a.warmup):
            ours()
            theirs()
        torch.cuda.synchronize()
        call, total, torch_ms, stages = [], [], [], {k: [] for k in dino.STAGES}
        for _ in range(a.rounds):
            ms, got = timed(ours)
            call.append(ms)
            net.set_timing(True)
            ours()
            net.set_timing(False)
            st, t = net.timing()
            total.append(t)
            for k, v in st.items():
                stages[k].append(v)
            ms, want = timed(theirs)
            torch_ms.append(ms)
    diff = {"plane": float((got[0][0] - want["plane"]).abs().max()), "glob": float((got[1][0] - want["glob"]).abs().max()),
            "largest_plane_value": float(want["plane"].abs().max())}
    fl = dict(zip(("gemm", "attention", "conv"), flops(*dims)))
    med = statistics.median
    st_ms = {k: med(v) for k, v in stages.items()}
    mfma_ms = sum(st_ms[k] for k in fl)
    res = {
        "workload": f"DINOBase.forward at (output_dim, vit_dim, depth, heads, grid) = {dims}: a {S} x {S} image, {dims[4] ** 2 + 1} tokens, a "
                    f"({dims[0]}, {net.plane}, {net.plane}) plane; synthetic weights and image, image and outputs on the device, outputs allocated "
                    f"inside the timed call; HIP events, {a.warmup} warm-up calls, median of {a.rounds} rounds alternating the library call, the "
                    "same with its timing on and the float32 torch restatement on the same device",
        "ms_per_avatar": med(call), "ms_per_avatar_min_max": [min(call), max(call)],
        "library_call_ms": med(total), "stage_ms": st_ms, "stage_share_of_call": {k: v / med(total) for k, v in st_ms.items()},
        "gflop": {k: v / 1e9 for k, v in fl.items()}, "tflops": {k: fl[k] / (st_ms[k] * 1e-3) / 1e12 for k in fl},
        "fraction_of_fp32_mfma_floor": (sum(fl.values()) / (FP32_MFMA_TFLOPS * 1e12)) / (mfma_ms * 1e-3),
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
