#!/usr/bin/env python
"""Per-shape time of the attention kernel (no argument), or with --kernels the time of each of the six f16-split kernel instances of
attention.hip at the shape the model runs it at, with the name of the kernel that ran (artalk_op_attention_rows_cus reports it), so
that a row cannot silently time another kernel.  ARTALK_ATTN_WIDE and ARTALK_ATTN_PP are read once per process: --kernels starts one
child per setting, one after the other, and touches no device itself.  ARTALK_LIB chooses the build, as in tools/ab_bench.sh."""
import ctypes as C, os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {name: rest for name, *rest in [("w2v", 96, 16, 64, 199, 199, 0, 0), ("ar p4", 16, 12, 64, 100, 362, 1, 0), ("ar p3", 16, 12, 64, 50, 262, 1, 0),
                                         ("ar p2", 16, 12, 64, 25, 212, 1, 0), ("ar p1", 16, 12, 64, 5, 187, 1, 0), ("ar p0", 16, 12, 64, 1, 182, 1, 0),
                                         ("vae dec", 16, 8, 64, 200, 200, 0, 100), ("vae enc", 16, 8, 64, 100, 100, 0, 0)]}
# setting of the dispatch switches -> (kernel expected, shape, flags of artalk_op_attention_ex: | 1 l2norm, | 2 f16 split, | 4 P8 rows)
ARMS = {
    "default": ({}, [("attention_f16_pp_kernel", "w2v", 6), ("attention_f16_wide_ar_kernel<1>", "ar p4", 3),
                     ("attention_f16_wide_ar_kernel<1,1,7,128>", "vae dec", 6), ("attention_f16_kernel<1,1>", "vae enc", 6)]),
    "pp0": ({"ARTALK_ATTN_PP": "0"}, [("attention_f16_wide_kernel", "w2v", 6)]),
    "wide0": ({"ARTALK_ATTN_WIDE": "0"}, [("attention_f16_kernel<1,1>", "w2v", 6), ("attention_f16_kernel<1>", "ar p4", 3)]),
}


def per_shape():
    import torch
    from artalk_amd import capi
    L = capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, (B, H, HD, Lq, Lk, l2, split) in SHAPES.items():
        if os.environ.get("ATTN_ONLY") and name not in os.environ["ATTN_ONLY"].split(","):
            continue
        D = H * HD
        Q = torch.randn(B, Lq, D, device="cuda"); K = torch.randn(B, Lk, D, device="cuda"); V = torch.randn(B, Lk, D, device="cuda")
        O = torch.empty(B, Lq, D, device="cuda"); qs = torch.ones(H, device="cuda")
        fl = 4.0 * B * H * Lq * Lk * HD
        line = f"{name:8s} B={B} H={H} Lq={Lq} Lk={Lk}:"
        for mode, tag in ((l2, "fp32 mfma"), (l2 | 2, "f16 split")) + (((2 | 4, "f16 split, P8 in (timing only)"),) if not l2 else ()):
            best = 1e9
            for _ in range(3):
                L.artalk_op_attention(p(Q), p(K), p(V), p(O), B, H, HD, Lq, Lk, 0.125, mode, p(qs), split, s)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    L.artalk_op_attention(p(Q), p(K), p(V), p(O), B, H, HD, Lq, Lk, 0.125, mode, p(qs), split, s)
                e1.record(); torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1) / 10)
            line += f"  {tag} {best*1e3:7.1f} us {fl/best/1e9:6.1f} TF"
        print(line, flush=True)


def per_kernel(arm, reps=500, windows=7):
    """the rows of one setting: median and least time per launch over `windows` windows of `reps` launches (timing only: random words)"""
    import torch
    from artalk_amd import capi
    L = capi.lib()
    for want, shape, flags in ARMS[arm][1]:
        B, H, HD, Lq, Lk, _, split = SHAPES[shape]
        D = H * HD
        Q, K, V = (torch.randn(B, n, D, device="cuda") for n in (Lq, Lk, Lk))
        O = torch.empty(B, Lq, D, device="cuda"); qs = torch.ones(H, device="cuda"); st = torch.zeros(1, dtype=torch.int32, device="cuda")
        used = C.c_int32(-7)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        call = lambda: L.artalk_op_attention_rows_cus(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), B, H, HD, Lq, Lk, 0.125, flags, qs.data_ptr(),
                                                      split, 4, 4, 0, st.data_ptr(), D, D, D, D, Lq * D, Lk * D, Lk * D, Lq * D,
                                                      B * Lq * D, B * Lk * D, B * Lk * D, B * Lq * D, 0, C.byref(used), stream)
        for _ in range(20):
            assert call() == 0
        ran = capi.ATTN_KERNELS.get(used.value, str(used.value))
        assert ran == want, f"{arm}: {shape} ran as {ran}, not {want}"
        times = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record(); torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / reps * 1e3)
        times.sort()
        print(f"{ran:42s} {shape:8s} B={B} H={H} Lq={Lq} Lk={Lk} [{arm}]  median {times[len(times) // 2]:8.2f} us  least {times[0]:8.2f} us", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--arm":
        per_kernel(sys.argv[2])
    elif len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        for arm, (env, _) in ARMS.items():
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm], env=dict(os.environ, **env), timeout=120).returncode
            if rc:
                sys.exit(rc)      # (a child that failed: start nothing more on the device)
    else:
        per_shape()
