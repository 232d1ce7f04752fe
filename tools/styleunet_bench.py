"""Milliseconds per frame of the StyleUNet upsampler (``artalk_styleunet_forward``) at the GAGAvatar head's shape: out_size 512, 32 input
channels, B = 8 frames per call, synthetic weights (``artalk_amd.styleunet.synth_state_dict``), stored noise.

Three kinds of call alternate in every round, each between HIP events, medians over the rounds:
  - the library call (the figure that counts);
  - the library call with its conv timing on (an event pair around every conv launch): the conv kernel's share of the call;
  - the float32 torch restatement of the same arithmetic (tests/styleunet_ref.py) on the same GPU through PyTorch-ROCm, in the same
    process: what a user has without this library.  If it cannot run there, the reason is recorded instead of a number.
The floor is arithmetic: the module's convolutions are 68.45 GMAC per frame, 0.87 ms at the 157 TF/s fp32-MFMA peak.

    python tools/styleunet_bench.py --out profiles/styleunet_bench.json

Prints one JSON line; --out also writes it to a file.  Needs the GPU: without one it fails.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

FP32_MFMA_FLOPS = 157e12


def conv_macs(out_size, in_dim=32, out_dim=3):
    """Multiply-accumulates of every convolution of one frame (the Linears are not counted)."""
    from artalk_amd.styleunet import state_dict_manifest, UNET_CHANNELS
    import math
    log_size = int(math.log2(out_size))
    size = {"conv_body_first": out_size, "final_conv": 4, "stylegan_decoder.style_conv1": 4, "stylegan_decoder.to_rgb1": 4}
    for j in range(log_size - 2):
        down, up = out_size >> j, 8 << j
        size[f"conv_body_down.{j}.conv1"] = down
        size[f"conv_body_down.{j}.conv2"] = size[f"conv_body_down.{j}.skip"] = down // 2
        size[f"conv_body_up.{j}.conv1"] = up // 2
        size[f"conv_body_up.{j}.conv2"] = size[f"conv_body_up.{j}.skip"] = up
        for w in ("condition_scale", "condition_shift"):
            size[f"{w}.{j}.0"] = size[f"{w}.{j}.2"] = up
        size[f"stylegan_decoder.style_convs.{2 * j}"] = size[f"stylegan_decoder.style_convs.{2 * j + 1}"] = up
        size[f"stylegan_decoder.to_rgbs.{j}"] = up
    total = 0
    for name, shape in state_dict_manifest(out_size, in_dim, out_dim):
        if len(shape) < 4 or not name.endswith(".weight") or name.startswith("toRGB") or "constant_input" in name or "noises" in name:
            continue
        key = name[:-len(".weight")].replace(".modulated_conv", "")
        n = 1
        for v in shape:
            n *= v
        total += n * size[key] ** 2
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch-ROCm baseline")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from artalk_amd import capi
    from artalk_amd.styleunet import StyleUNet, synth_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("styleunet_bench needs the GPU")
    S, B = args.size, args.frames
    sd = synth_state_dict(S)
    net = StyleUNet(S, S, 32, 3).eval().to("cuda:0")
    net.load_state_dict(sd)
    L = capi.lib()
    slab = net.set_slab(0)
    x = torch.rand(B, 32, S, S, generator=torch.Generator().manual_seed(0)).cuda()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    lib_call = lambda: net(x, randomize_noise=False)
    torch_call, torch_note = None, None
    if not args.no_torch:
        try:
            from styleunet_ref import styleunet_forward
            sd_dev = {k: v.cuda() for k, v in sd.items()}
            with torch.no_grad():
                ref = styleunet_forward(sd_dev, x)
            diff = float((ref - lib_call()).abs().max())
            torch_call = lambda: styleunet_forward(sd_dev, x)
            torch_note = f"max-abs difference to the library call {diff:.2e}"
        except Exception as e:      # recorded, not hidden: the figure is then missing from the result
            torch_note = f"the torch restatement did not run on this GPU: {type(e).__name__}: {e}"[:300]
    for _ in range(args.warmup):
        timed(lib_call)
        if torch_call:
            with torch.no_grad():
                timed(torch_call)
    lib_ms, conv_ms, timed_ms, torch_ms = [], [], [], []
    cm, tm = C.c_double(0), C.c_double(0)
    for _ in range(args.rounds):
        L.artalk_styleunet_set_timing(net._h, 0)
        lib_ms.append(timed(lib_call))
        L.artalk_styleunet_set_timing(net._h, 1)
        lib_call()
        L.artalk_styleunet_get_timing(net._h, C.byref(cm), C.byref(tm))
        conv_ms.append(cm.value)
        timed_ms.append(tm.value)
        if torch_call:
            with torch.no_grad():
                torch_ms.append(timed(torch_call))
    L.artalk_styleunet_set_timing(net._h, 0)
    med = statistics.median(lib_ms)
    macs = conv_macs(S)
    floor_ms = 2.0 * macs / FP32_MFMA_FLOPS * 1e3
    res = {
        "workload": f"artalk_styleunet_forward, out_size {S}, in_dim 32, B = {B} frames per call in slabs of {slab}, synthetic weights, stored "
                    f"noise, sigmoid on; input and output NCHW on the device, output allocated inside the timed call; HIP events, "
                    f"{args.warmup} warm-up calls, median of {args.rounds} rounds alternating the call, the conv-timed call and the torch call",
        "ms_per_call": med, "ms_per_call_min": min(lib_ms), "ms_per_call_max": max(lib_ms), "ms_per_frame": med / B,
        "conv_gmac_per_frame": macs / 1e9, "fp32_mfma_floor_ms_per_frame": floor_ms, "fraction_of_fp32_mfma_floor": floor_ms / (med / B),
        "conv_tflops": 2.0 * macs * B / (statistics.median(conv_ms) * 1e-3) / 1e12,
        "conv_kernel_ms_per_frame": statistics.median(conv_ms) / B,
        "conv_kernel_share_of_call": statistics.median(c / t for c, t in zip(conv_ms, timed_ms)),
        "torch_rocm_fp32_ms_per_frame": statistics.median(torch_ms) / B if torch_ms else None,
        "torch_rocm_fp32_ms_per_call_min_max": [min(torch_ms), max(torch_ms)] if torch_ms else None,
        "torch_note": torch_note,
        "speedup_over_torch": statistics.median(torch_ms) / med if torch_ms else None,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
