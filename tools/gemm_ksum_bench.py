"""Microseconds per launch of the fp32 MFMA GEMM with its two sum orders - one chain over K (``artalk_op_gemm``) and K summed in blocks of
256 (``artalk_op_gemm_blocked``, what the DINO object launches) - at the two ViT-B shapes the order matters for: fc2 (1370, 768, 3072) and
fc1 (1370, 3072, 768) as (M, N, K), bias in the epilogue, random operands.  Both run the 64 x 64 tile.

Each launch lies between two HIP events on the current stream; the two entry points alternate launch by launch after a warm-up of each,
and the median, minimum and maximum of the launches are reported.  The two results are also compared: the same sums in another order
differ in the last bits only.  No target is set.

    python tools/gemm_ksum_bench.py --out profiles/gemm_ksum_bench.json

Prints one JSON line; --out also writes it to a file.  Needs the GPU: without one it fails.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = ((1370, 768, 3072), (1370, 3072, 768))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.launches >= 20
    import torch
    assert torch.cuda.is_available(), "gemm_ksum_bench.py needs the GPU"
    from artalk_amd import capi
    L = capi.lib()
    entries = {"one_chain": L.artalk_op_gemm, "blocks_of_256": L.artalk_op_gemm_blocked}
    result = {"launches": a.launches, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "shapes": []}
    for M, N, K in SHAPES:
        g = torch.Generator().manual_seed(M + N)
        A = torch.randn(M, K, generator=g).cuda()
        W = (torch.randn(N, K, generator=g) * (2.0 / K) ** 0.5).cuda()
        bias = torch.randn(N, generator=g).cuda()
        out = {k: torch.empty(M, N, device="cuda") for k in entries}
        stream = capi.current_stream_ptr()

        def launch(k):
            rc = entries[k](capi.ptr(A), K, capi.ptr(W), capi.ptr(bias), None, None, capi.ptr(out[k]), M, N, K, 0, stream)
            assert rc == capi.OK, rc
        for _ in range(a.warmup):
            for k in entries:
                launch(k)
        torch.cuda.synchronize()
        times = {k: [] for k in entries}
        for _ in range(a.launches):
            for k in entries:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(k)
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        ref = A.double().cpu() @ W.double().cpu().t() + bias.double().cpu()
        row = {"M": M, "N": N, "K": K, "gflop": 2.0 * M * N * K / 1e9}
        for k in entries:
            t = times[k]
            row[k] = {"us_median": statistics.median(t), "us_min": min(t), "us_max": max(t),
                      "tflops_at_median": 2.0 * M * N * K / statistics.median(t) / 1e6,
                      "max_abs_error": float((out[k].cpu().double() - ref).abs().max())}
        row["max_abs_difference"] = float((out["one_chain"] - out["blocks_of_256"]).abs().max())
        result["shapes"].append(row)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
