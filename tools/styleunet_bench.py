"""Milliseconds per frame of the StyleUNet upsampler (``artalk_styleunet_forward``) at the GAGAvatar head's shape: out_size 512, 32 input
channels, B = 8 frames per call, synthetic weights (``artalk_amd.styleunet.synth_state_dict``), stored noise.

Three kinds of call alternate in every round, each between HIP events, medians over the rounds:
  - the library call (the figure that counts);
  - the library call with its conv timing on (an event pair around every conv launch): the conv kernel's share of the call;
  - the float32 torch restatement of the same arithmetic (tests/styleunet_ref.py) on the same GPU through PyTorch-ROCm, in the same
    process: what a user has without this library.  If it cannot run there, the reason is recorded instead of a number.
The floor is arithmetic: the module's convolutions are 68.45 GMAC per frame, 0.87 ms at the 157 TF/s fp32-MFMA peak.

    python tools/styleunet_bench.py --out profiles/styleunet_bench.json

``--precision f32|bf16x3|bf16`` runs the above in that mode of the convolutions (the default is f32).  ``--precision all`` compares the
modes instead (no torch call): in every round of the one process the three modes alternate, each with a plain call and a conv-timed
call, so the baseline is the f32 mode of the same build in the same rounds.  Per mode: per-call and conv-only medians with min and max,
the ratio to f32, TF/s counted on the convolutions' multiply-adds, the fraction of the mode's own floor (its 3 or 1 bf16 products per
multiply-add at the 2.5 PF/s bf16-MFMA peak; f32: 157 TF/s) and the conv time per resolution level from the event pairs.

    python tools/styleunet_bench.py --precision all --out profiles/styleunet_precision_bench.json

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
BF16_MFMA_FLOPS = 2.5e15
PRODUCTS = {"f32": 1, "bf16x3": 3, "bf16": 1}      # MFMA products per multiply-add


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


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def compare_modes(args, net, x, L):
    """--precision all: the three modes alternate inside each round."""
    S, B = args.size, args.frames
    modes = ("f32", "bf16x3", "bf16")
    macs = conv_macs(S)

    def timed():
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        net(x, randomize_noise=False)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        for m in modes:
            net.set_precision(m)
            timed()
    call = {m: [] for m in modes}
    conv = {m: [] for m in modes}
    levels = {m: {} for m in modes}      # H -> per round, the summed time of the launches at that resolution
    level_macs = {}
    cm, tm = C.c_double(0), C.c_double(0)
    for _ in range(args.rounds):
        for m in modes:
            net.set_precision(m)
            L.artalk_styleunet_set_timing(net._h, 0)
            call[m].append(timed())
            L.artalk_styleunet_set_timing(net._h, 1)
            net(x, randomize_noise=False)
            L.artalk_styleunet_get_timing(net._h, C.byref(cm), C.byref(tm))
            conv[m].append(cm.value)
            n = L.artalk_styleunet_get_launch_timing(net._h, None, None, 0)
            ms, geom = (C.c_double * n)(), (C.c_int32 * (5 * n))()
            L.artalk_styleunet_get_launch_timing(net._h, ms, geom, n)
            per, mac = {}, {}
            for i in range(n):
                frames, H, cin, cout, k = geom[5 * i:5 * i + 5]
                per[H] = per.get(H, 0.0) + ms[i]
                mac[H] = mac.get(H, 0) + frames * H * H * cin * cout * k * k
            for H, v in per.items():
                levels[m].setdefault(H, []).append(v)
            level_macs = mac
    L.artalk_styleunet_set_timing(net._h, 0)
    net.set_precision("f32")
    assert sum(level_macs.values()) == macs * B, (sum(level_macs.values()), macs * B)
    res = {
        "workload": f"artalk_styleunet_forward, out_size {S}, in_dim 32, B = {B} frames per call, synthetic weights, stored noise, sigmoid on; "
                    f"HIP events, {args.warmup} warm-up calls per mode, {args.rounds} rounds in one process, each round running the modes "
                    f"f32, bf16x3, bf16 in turn: a plain call (ms_per_call) and a conv-timed call (conv_ms_per_call, an event pair around "
                    f"every conv launch); floors: 157 TF/s fp32 MFMA, 2.5 PF/s bf16 MFMA times the mode's products per multiply-add",
        "conv_gmac_per_frame": macs / 1e9, "modes": {},
    }
    f32_call, f32_conv = statistics.median(call["f32"]), statistics.median(conv["f32"])
    for m in modes:
        c, k = statistics.median(call[m]), statistics.median(conv[m])
        floor_ms = 2.0 * macs * PRODUCTS[m] / (FP32_MFMA_FLOPS if m == "f32" else BF16_MFMA_FLOPS) * 1e3
        res["modes"][m] = {
            "ms_per_call": spread(call[m]), "ms_per_frame": c / B, "conv_ms_per_call": spread(conv[m]), "conv_ms_per_frame": k / B,
            "call_speedup_over_f32": f32_call / c, "conv_speedup_over_f32": f32_conv / k,
            "conv_tflops_on_the_macs": 2.0 * macs * B / (k * 1e-3) / 1e12,
            "own_floor_ms_per_frame": floor_ms, "conv_fraction_of_own_floor": floor_ms / (k / B),
            "levels": {str(H): {"conv_ms_per_call": statistics.median(v), "share_of_conv_time": statistics.median(v) / k,
                                "share_of_macs": level_macs[H] / (macs * B),
                                "tflops_on_the_macs": 2.0 * level_macs[H] / (statistics.median(v) * 1e-3) / 1e12}
                       for H, v in sorted(levels[m].items())},
        }
    return res


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch-ROCm baseline")
    ap.add_argument("--precision", choices=("f32", "bf16x3", "bf16", "all"), default="f32")
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
    if args.precision == "all":
        return emit(compare_modes(args, net, x, L), args.out)
    net.set_precision(args.precision)

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
        "workload": f"artalk_styleunet_forward, precision {args.precision}, out_size {S}, in_dim 32, B = {B} frames per call in slabs of {slab}, synthetic weights, stored "
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
    emit(res, args.out)


if __name__ == "__main__":
    main()
