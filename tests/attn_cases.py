"""The attention edge cases shared by tests/test_attn_edges_cpu.py (planning, dry run) and tests/test_attn_edges_gpu.py (float64, poison,
bit identity, peaked softmax): one table, every case named for the kernel of attention.hip that plan_attention gives it on a device of
256 compute units.  numpy only; nothing here touches a device.

A case is (kernel, B, H, HD, Lq, Lk, split, flags, cus, kind, out_p8, o_exp):
  flags   the l2norm word of artalk_op_attention_ex: | 1 L2-normalised q and k with a per-head scale, | 2 the f16-split kernels, | 4 P8 rows
  cus     AttnArgs::cus (0: the whole device)
  kind    "randn", or for the peaked-softmax group "peak-random" / "peak-drift" / "peak-drift-rev" with `peak` = the per-head q scale
          (l2norm) or the largest |score| Q is scaled to (P8 rows)
Sizes are the smallest at which an edge exists: B * H = 6 unless a kernel's dispatch or grid arithmetic needs another count.

Where the dispatch does not leave a shape to the kernel one might expect, the case is named for the kernel that does run it:
  * fp32 rows with Lq <= 64 and Lk >= 64 are the short kernel's whatever the f16 flag says, so attention_f16_wide_ar_kernel<1> is reached
    from Lq = 65 on only (its own lower bound Lq > 32 never decides); Lq = 33, 48, 49 are kept here as short-kernel cases;
  * P8 rows with a mask and Lq = Lk = 130 are the two-workgroup wide-AR form's, so the mask set of attention_f16_kernel<1,1> runs at
    Lq = Lk = 65 and 209 (four query blocks, the key loop trimmed at the first)."""
from collections import namedtuple

import numpy as np

KERNELS = ("attention_kernel<64>", "attention_kernel<32>", "attention_short_kernel", "attention_f16_kernel<1>", "attention_f16_kernel<1,1>",
           "attention_f16_wide_kernel", "attention_f16_pp_kernel", "attention_f16_wide_ar_kernel<1>", "attention_f16_wide_ar_kernel<1,1,7,128>")
F32_64, F32_32, SHORT, F16, F16_P8, WIDE, PP, WIDE_AR, WIDE_AR_P8 = range(9)      # ARTALK_ATTN_* of include/artalk_hip.h
# the kernels the code claims bit-identical to the 64-query f16 kernel of the same row format (ARTALK_ATTN_WIDE=0 runs that one)
BIT_IDENTICAL = {WIDE: F16_P8, PP: F16_P8, WIDE_AR_P8: F16_P8, WIDE_AR: F16}
N_CU = 256                  # the device the table is planned for
QKV_EXP = 3                 # site exponent of the P8 q | k | v rows (what the VAE's q|k|v GEMM writes with)

Case = namedtuple("Case", "kernel B H HD Lq Lk split flags cus kind out_p8 o_exp peak")


def _c(kernel, Lq, Lk, flags, B=2, H=3, HD=64, split=0, cus=0, kind="randn", out_p8=0, o_exp=4, peak=0.0):
    return Case(kernel, B, H, HD, Lq, Lk, split, flags, cus, kind, out_p8, o_exp, peak)


def _with_p8_out(cases):
    """every third case of a 64-wide kernel writes O in the P8 format, at the site exponents 4 and 0 in turn"""
    out = []
    for i, c in enumerate(cases):
        out.append(c._replace(out_p8=1, o_exp=(4, 0)[(i // 3) % 2]) if c.HD == 64 and i % 3 == 2 else c)
    return out


def _build():
    t = []
    # attention_kernel<64>: whatever the short kernel does not take (Lq > 64, Lk < 64, or a mask)
    f = [_c(F32_64, Lq, Lk, 0) for Lq in (1, 63, 64, 65, 129) for Lk in (1, 15, 16, 17, 63, 64, 65, 130) if Lq > 64 or Lk < 64]
    t += [c._replace(flags=i & 1) for i, c in enumerate(f)]
    t += [_c(F32_64, L, L, 0, split=s) for L in (65, 130) for s in sorted({1, 16, 40, 64, L - 1})]
    # attention_kernel<32>
    t += [_c(F32_32, Lq, Lk, 0, HD=32) for Lq in (1, 50, 65) for Lk in (1, 17, 64, 65)]
    # attention_short_kernel: 4, 5, 8, 9 and 10 key tiles; B * H = 1, 6, 9 (a surplus workgroup group) and 12; flag bit 1 changes nothing
    bh = ((1, 1), (2, 3), (3, 3), (1, 12))
    i = 0
    for Lq in (1, 15, 16, 17, 33, 64):
        for Lk in (64, 65, 79, 80, 81, 127, 128, 129, 144, 145):
            B, H = bh[(i + i // 4) % 4]
            t.append(_c(SHORT, Lq, Lk, (i + i // 10) % 4, B=B, H=H))
            i += 1
    t += [_c(SHORT, Lq, Lk, fl) for Lq in (33, 48, 49) for Lk, fl in ((65, 2), (193, 3))]      # (not the wide-AR kernel's: see above)
    # attention_f16_kernel<1>: Lk < 64, a mask, or Lq > 112 (or Lk = 64, which the wide-AR kernel leaves)
    f = [_c(F16, Lq, Lk, 2) for Lq in (1, 16, 64, 65, 113, 129) for Lk in (1, 17, 63, 64, 65, 130, 257)
         if (Lk < 64 or Lq > 112 or (Lq > 64 and Lk == 64))]
    t += [c._replace(flags=2 | (i & 1)) for i, c in enumerate(f)]
    t += [_c(F16, L, L, 2, split=s) for L in (65, 130) for s in sorted({1, 16, 40, 64, L - 1})]
    # attention_f16_kernel<1,1>: P8 rows outside (128, 208] queries, or past 256 keys
    t += [_c(F16_P8, Lq, Lk, 6) for Lq in (1, 64, 65, 128, 209) for Lk in (1, 17, 64, 65, 128, 257)]
    t += [_c(F16_P8, L, L, 6, split=s) for L in (65, 209) for s in sorted({1, 16, 40, 64, L - 1})]
    # attention_f16_wide_ar_kernel<1>: the 192-key phase at 191, 192, 193, 384, 385 keys; one to seven waves
    f = [_c(WIDE_AR, Lq, Lk, 2) for Lq in (65, 80, 81, 97, 112) for Lk in (65, 128, 191, 192, 193, 384, 385)]
    t += [c._replace(flags=2 | (i & 1)) for i, c in enumerate(f)]
    # attention_f16_wide_ar_kernel<1,1,7,128>: the 128-key phase, a second workgroup of 1 .. 6 waves
    t += [_c(WIDE_AR_P8, Lq, Lk, 6) for Lq in (129, 144, 208) for Lk in (1, 33, 127, 128, 129, 255, 256)]
    t += [_c(WIDE_AR_P8, L, L, 6, split=s) for L in (129, 200) for s in sorted({1, 64, 100, 112, 113, L - 1})]
    # attention_f16_wide_kernel: 256 heads (what the VAE decoder runs at 32 clips, there with the mask)
    t += [_c(WIDE, Lq, Lk, 6, B=32, H=8) for Lq in (129, 208) for Lk in (1, 31, 32, 33, 64, 97, 128, 255, 256)]
    t += [_c(WIDE, L, L, 6, B=32, H=8, split=s) for L in (129, 200) for s in sorted({64, 100, 128, L - 1})]
    # attention_f16_pp_kernel on 8 compute units: whole rounds (16 heads), one surplus head (17), a ragged last round (23)
    bh = ((2, 8), (17, 1), (1, 23))
    i = 0
    for Lq in (129, 150, 208):
        for Lk in (129, 160, 161, 192, 193, 223, 224):
            B, H = bh[(i + i // 7) % 3]
            t.append(_c(PP, Lq, Lk, 6, B=B, H=H, cus=8))
            i += 1
    return _with_p8_out(t)


def _build_peaked():
    """the peaked-softmax group: the four kernels that normalise q and k with a per-head scale of 20 and 100, the four P8 kernels with
    Q scaled until the largest |score| is 20; random data and keys that drift towards (or away from) a common direction"""
    return [
        _c(F32_64, 65, 385, 1, kind="peak-random", peak=20.0), _c(F32_64, 65, 385, 1, kind="peak-drift", peak=100.0),
        _c(SHORT, 50, 385, 1, kind="peak-drift", peak=20.0), _c(SHORT, 50, 385, 1, kind="peak-random", peak=100.0),
        _c(F16, 129, 385, 3, kind="peak-random", peak=20.0), _c(F16, 129, 385, 3, kind="peak-drift-rev", peak=100.0),
        _c(WIDE_AR, 100, 385, 3, kind="peak-drift", peak=20.0), _c(WIDE_AR, 100, 385, 3, kind="peak-drift", peak=100.0),
        _c(F16_P8, 65, 257, 6, kind="peak-drift", peak=20.0), _c(WIDE_AR_P8, 200, 256, 6, kind="peak-drift-rev", peak=20.0),
        _c(WIDE, 200, 200, 6, B=32, H=8, kind="peak-random", peak=20.0), _c(PP, 199, 199, 6, B=2, H=8, cus=8, kind="peak-drift", peak=20.0),
    ]


CASES = _build()
PEAKED = _build_peaked()
ALL = CASES + PEAKED


def case_id(c):
    s = f"{KERNELS[c.kernel]}-q{c.Lq}-k{c.Lk}-bh{c.B}x{c.H}-f{c.flags}"
    if c.split:
        s += f"-split{c.split}"
    if c.out_p8:
        s += f"-o8e{c.o_exp}"
    if c.kind != "randn":
        s += f"-{c.kind}{c.peak:g}"
    return s


PAD_COLS, PAD_ROWS = 64, 2


def layout(c):
    """The buffers of a case: rows of pitch H * HD + 64, Lq + 2 (Q, O) and Lk + 2 (K, V) rows per clip, and the sizes handed to the entry
    point, which end at the last valid element."""
    D = c.H * c.HD
    ld = D + PAD_COLS
    qbs, kbs = (c.Lq + PAD_ROWS) * ld, (c.Lk + PAD_ROWS) * ld
    return dict(D=D, ld=ld, qbs=qbs, kbs=kbs, qn=(c.B - 1) * qbs + (c.Lq - 1) * ld + D, kn=(c.B - 1) * kbs + (c.Lk - 1) * ld + D)


def scale_of(c):
    return 1.0 if c.flags & 1 else c.HD ** -0.5


def make_inputs(c, index):
    """Q [B, Lq, H * HD], K, V [B, Lk, H * HD] float32, the per-head q scale (l2norm) or None, and the softmax scale of a case.  The same
    bits in every process (numpy's PCG64 seeded by the case's place in ALL)."""
    rng = np.random.default_rng(1000 + index)
    B, H, HD, Lq, Lk = c.B, c.H, c.HD, c.Lq, c.Lk
    Q = rng.standard_normal((B, Lq, H, HD))
    K = rng.standard_normal((B, Lk, H, HD))
    V = rng.standard_normal((B, Lk, H, HD))
    qs = (rng.random(H) * 4 + 1) if c.flags & 1 else None
    if c.kind != "randn":
        if c.kind != "peak-random":
            # keys drift towards a direction u common to a head: the cosine of key j with u rises with j from about 0 to about 0.97, the
            # queries lie close to u: the row maximum rises in every 64-key block and the last block carries the sum (-rev: the first)
            u = rng.standard_normal((B, 1, H, HD))
            u *= 8.0 / np.linalg.norm(u, axis=-1, keepdims=True)
            tj = (0.8 * (np.arange(Lk) + 1.0) / Lk).reshape(1, Lk, 1, 1)
            K = (1.0 - tj) * K + tj * u
            Q = u + 0.3 * Q
            if c.kind == "peak-drift-rev":
                K = K[:, ::-1]
        if c.flags & 1:
            qs = np.full(H, c.peak)
        else:
            s = np.einsum("bqhd,bkhd->bhqk", Q, K) * scale_of(c)
            Q = Q * (c.peak / np.abs(s).max())
    f = lambda x: np.ascontiguousarray(x.reshape(x.shape[0], x.shape[1], H * HD), dtype=np.float32)
    return f(Q), f(K), f(V), (None if qs is None else qs.astype(np.float32)), scale_of(c)
