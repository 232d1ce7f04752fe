// The StyleUNet convolution in the bf16x3 and bf16 precision modes ("Precision modes"): the implicit GEMM of
// styleunet.hip's conv_mfma_kernel - M = B H W pixels, N = Cout, K = k k Cin, same ConvArgs, same fp32 epilogue - on
// v_mfma_f32_32x32x16_bf16.  With a = fl32(x * in_scale), hi(v) = bf16(v) and lo(v) = bf16(v - hi(v)):
//   NP = 3 (bf16x3)   conv(lo(a), hi(w)) + conv(hi(a), lo(w)) + conv(hi(a), hi(w))
//   NP = 1 (bf16)     conv(hi(a), hi(w))
// bf16 has fp32's exponent range, so there is no operand scale, no calibration and no range guard.
//
// Weights come packed once (conv_pack_kernel): planes hi and lo of [Cout][Kp] bf16, K index = tap * Cinp + ci with Cin zero-padded to
// Cinp (a multiple of 8) and K to Kp (a multiple of 32).  Activations stay fp32 in memory: they are read as fp32, scaled, split and
// rounded (v_cvt_pk_bf16_f32) while they are staged into LDS, the 8 threads of a pixel reading 128 consecutive bytes of its row.
// Staging per 32-deep K step as in gemm_bf16.hip: LDS rows of 32 + 8 bf16 (80 bytes: the ds_read_b128 fragment reads of 16
// consecutive rows fall on 16 distinct 4-bank groups), two buffers, one barrier per step; lane (r, h) holds k in
// [16 s + 8 h, 16 s + 8 h + 8) of row r in k-substep s, for both operands.  A group of 8 consecutive k never straddles a tap, so
// any Cin >= 1 takes the same path, and a step may span two taps (Cin = 16).
//
// Summation: every K step (32 deep, NP products) sums from zero inside the MFMA accumulator, 8 steps add up to a block of 256, blocks
// add up - the three levels of conv_mfma_kernel, so that a K of 4608 does not pile its rounding onto one running sum.  The tile
// depends on Cout alone, there are no atomics and no split of K: the K order of an output value is fixed by the layer.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "styleunet_conv.h"

namespace artalk {

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int CB_LD = CB_BK + 8;

__global__ __launch_bounds__(256) void conv_pack_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int Cin, int Cout, int kk, int Cinp,
                                                        int Kp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)Cout * Kp;
    if (i >= n) return;
    const int co = (int)(i / Kp), kidx = (int)(i - (long)co * Kp);
    const int tap = kidx / Cinp, ci = kidx - tap * Cinp;
    const float v = (tap < kk && ci < Cin) ? w[((long)tap * Cin + ci) * Cout + co] : 0.f;
    const __bf16 hv = (__bf16)v;
    out[i] = hv;
    out[n + i] = (__bf16)(v - (float)hv);      // (the difference is exact in fp32)
}

// One workgroup: 128 pixels x 32 NT output channels; wave w owns pixels 32 w .. 32 w + 31 and all NT column tiles.
// VA: Cin % 8 == 0 and 16-byte aligned rows of x and in_scale (vector loads); otherwise element by element.
template <int NT, int NP, bool VA>
__global__ __launch_bounds__(256) void conv_bf16_kernel(ConvArgs a, const __bf16* __restrict__ wp, int Cinp, int Kp) {
    constexpr int NPL = NP == 3 ? 2 : 1;      // operand planes: hi, lo
    constexpr int BN = 32 * NT;
    constexpr int B_PIECES = NPL * BN * 4, B_PER = (B_PIECES + 255) / 256;      // 16-byte pieces of the weight tile
    __shared__ __attribute__((aligned(16))) __bf16 As[2][NPL][CB_BM * CB_LD];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[2][NPL][BN * CB_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const long M = (long)a.B * a.H * a.W;
    const int HW = a.H * a.W;
    const long m0 = (long)blockIdx.x * CB_BM;
    const int n0 = blockIdx.y * BN;
    const int pad = a.k >> 1, kk = a.k * a.k;
    const int nsteps = Kp / CB_BK;

    // this thread's share of the A tile: 4 consecutive k starting at ak of the pixels ap, ap + 32, ap + 64, ap + 96, so that the 8
    // threads of a pixel read 128 consecutive bytes of its row (a group of 4 k never straddles a tap: Cinp % 8 == 0)
    const int ap = t >> 3, ak = (t & 7) * 4;
    int ay[4], ax[4];             // ay far below 0: no such pixel
    const float *xb[4], *sb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long am = m0 + ap + 32 * i;
        int ab = 0;
        ay[i] = -0x40000000; ax[i] = 0;
        if (am < M) { ab = (int)(am / HW); const int rem = (int)(am - (long)ab * HW); ay[i] = rem / a.W; ax[i] = rem - ay[i] * a.W; }
        xb[i] = a.x + (long)ab * a.x_bstride + ((long)ay[i] * a.W + ax[i]) * a.Cin;      // the pixel itself (never read when there is none)
        sb[i] = a.in_scale ? a.in_scale + (long)ab * a.in_scale_ld : nullptr;
    }
    int atap = ak / Cinp, aci = ak - atap * Cinp;      // tap and channel of this thread's k in the next step

    f32x4 ra[4];
    bf16x8_t rb[B_PER];
    auto gload = [&](int step) {
        const int ky = atap / a.k, kx = atap - ky * a.k;
        const long shift = ((long)(ky - pad) * a.W + (kx - pad)) * a.Cin + aci;      // from a pixel to this step's operand: the same for the four
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int yy = ay[i] + ky - pad, xx = ax[i] + kx - pad;
            const bool inb = atap < kk && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (inb) {
                const float* p = xb[i] + shift;
                if (VA) {      // (Cin == Cinp: the four channels lie inside the row)
                    v = *reinterpret_cast<const f32x4*>(p);
                    if (sb[i]) {
                        const f32x4 sv = *reinterpret_cast<const f32x4*>(sb[i] + aci);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = __fmul_rn(v[e], sv[e]);      // one rounded multiply: never fused into the split
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (aci + e < a.Cin) v[e] = sb[i] ? __fmul_rn(p[e], sb[i][aci + e]) : p[e];
                }
            }
            ra[i] = v;
        }
        aci += CB_BK;
        while (aci >= Cinp) { aci -= Cinp; ++atap; }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int p = t + i * 256;
            const int plane = p / (BN * 4), rem = p - plane * (BN * 4), co = n0 + (rem >> 2);
            bf16x8_t v = {};
            if (p < B_PIECES && co < a.Cout) v = *reinterpret_cast<const bf16x8_t*>(wp + ((long)plane * a.Cout + co) * Kp + step * CB_BK + (rem & 3) * 8);
            rb[i] = v;
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bf16x4_t hi, lo;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const __bf16 hv = (__bf16)ra[i][e];      // round to nearest even
                hi[e] = hv;
                if (NP == 3) lo[e] = (__bf16)(ra[i][e] - (float)hv);
            }
            const int at = (ap + 32 * i) * CB_LD + ak;
            *reinterpret_cast<bf16x4_t*>(&As[buf][0][at]) = hi;
            if (NP == 3) *reinterpret_cast<bf16x4_t*>(&As[buf][NPL - 1][at]) = lo;
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int p = t + i * 256;
            const int plane = p / (BN * 4), rem = p - plane * (BN * 4);
            if (p < B_PIECES) *reinterpret_cast<bf16x8_t*>(&Bs[buf][plane][(rem >> 2) * CB_LD + (rem & 3) * 8]) = rb[i];
        }
    };

    f32x16 acc[NT], mid[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc[j][e] = 0.f; mid[j][e] = 0.f; }

    gload(0);
    lstore(0);
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
        const int buf = step & 1;
        if (step + 1 < nsteps) gload(step + 1);
        const int ao = (wave * 32 + r) * CB_LD + h * 8, bo = r * CB_LD + h * 8;
        f32x16 part[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) part[j][e] = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8_t ahi = *reinterpret_cast<const bf16x8_t*>(&As[buf][0][ao + s * 16]);
            bf16x8_t bhi[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) bhi[j] = *reinterpret_cast<const bf16x8_t*>(&Bs[buf][0][bo + j * 32 * CB_LD + s * 16]);
            if (NP == 3) {      // the two small products first
                const bf16x8_t alo = *reinterpret_cast<const bf16x8_t*>(&As[buf][NPL - 1][ao + s * 16]);
#pragma unroll
                for (int j = 0; j < NT; ++j) part[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi[j], part[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const bf16x8_t blo = *reinterpret_cast<const bf16x8_t*>(&Bs[buf][NPL - 1][bo + j * 32 * CB_LD + s * 16]);
                    part[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo, part[j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) part[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi[j], part[j], 0, 0, 0);
        }
        if (step + 1 < nsteps) lstore(buf ^ 1);
#pragma unroll
        for (int j = 0; j < NT; ++j) mid[j] += part[j];
        if ((step & 7) == 7) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                acc[j] += mid[j];
#pragma unroll
                for (int e = 0; e < 16; ++e) mid[j][e] = 0.f;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] += mid[j];

    conv_epilogue<NT>(a, acc, m0, n0, wave, r, h, M, HW);
}

void launch_conv_pack(const float* w, void* packed, int Cin, int Cout, int k, hipStream_t s) {
    const int Cinp = conv_packed_cinp(Cin), Kp = conv_packed_kp(Cin, k);
    const long n = (long)Cout * Kp;
    ARTALK_LAUNCH(conv_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, reinterpret_cast<__bf16*>(packed), Cin, Cout, k * k, Cinp, Kp);
}

// The tile choice depends on Cout alone (never on B), as for the fp32 kernel.
void launch_conv_bf16(const ConvArgs& a, const void* packed, int precision, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if ((long)a.B * a.H * a.W <= 0) return;
    const ConvPlan p = plan_conv(a, precision);
    const bool va = p.va;
    const int Cinp = p.cinp, Kp = p.kp;
    const __bf16* wp = reinterpret_cast<const __bf16*>(packed);
    const dim3 grid(p.gx, p.gy), block(256);
#define CB_GO(NT, NP, VA)                                                                                                  \
    do {                                                                                                                   \
        if (e0) hipExtLaunchKernelGGL((conv_bf16_kernel<NT, NP, VA>), grid, block, 0, s, e0, e1, 0, a, wp, Cinp, Kp);      \
        else ARTALK_LAUNCH((conv_bf16_kernel<NT, NP, VA>), grid, block, 0, s, a, wp, Cinp, Kp);                            \
    } while (0)
#define CB_NP(NT, VA)                                                                                                      \
    do {                                                                                                                   \
        if (precision == CONV_PRECISION_BF16X3) CB_GO(NT, 3, VA); else CB_GO(NT, 1, VA);                                   \
    } while (0)
    if (p.nt == 1) { if (va) CB_NP(1, true); else CB_NP(1, false); }
    else         { if (va) CB_NP(2, true); else CB_NP(2, false); }
#undef CB_NP
#undef CB_GO
}

}  // namespace artalk
