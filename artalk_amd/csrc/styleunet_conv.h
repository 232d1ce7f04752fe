// What the StyleUNet convolution kernels share (styleunet.hip: exact fp32; styleunet_bf16.hip: the bf16x3 and bf16 modes): the
// arguments of one launch, the fp32 epilogue, and the host entry points of the kernels (the fp32 one also serves gsgen.hip).
// Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace artalk {

struct ConvArgs {
    const float* x; long x_bstride;      // [B][H][W][Cin]; elements between two samples (0: one image for every sample)
    const float* w;                      // [k k][Cin][Cout]
    float* out;                          // [B][H][W][Cout]
    int B, H, W, Cin, Cout, k;
    const float* in_scale; long in_scale_ld;      // [B][in_scale_ld >= Cin] or null
    const float* out_scale;              // [B][Cout] or null
    float gain;                          // 1: none
    const float* noise; long noise_bstride; const float* noise_w;      // [B or 1][H][W], one device float; null: none
    const float* bias;                   // [Cout] or null
    int lrelu;
    int relu;                            // plain ReLU, in the slot of the LeakyReLU (0: off; the Gaussian generators, gsgen.hip)
    const float* sft_scale; const float* sft_shift;      // [B][H][W][Cout] or null (both or neither)
    const float* res;                    // [B][H][W][Cout] or null
};

// The epilogue of a 128-pixel x 32 NT-channel workgroup tile whose wave `wave` holds pixels 32 wave .. 32 wave + 31 in 32x32 MFMA
// accumulators: lane (r, h) holds output channel n0 + 32 j + r of pixels 32 wave + 8 q + 4 h + e (register 4 q + e).  In this order:
// output scale (demodulation), gain, noise, bias, LeakyReLU 0.2 or ReLU, SFT and residual, all fp32.
template <int NT>
__device__ __forceinline__ void conv_epilogue(const ConvArgs a, const f32x16 (&acc)[NT], long m0, int n0, int wave, int r, int h, long M, int HW) {
    const float nw = a.noise ? a.noise_w[0] : 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int co = n0 + j * 32 + r;
        if (co >= a.Cout) continue;
        const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const long m = m0 + wave * 32 + 8 * (v >> 2) + 4 * h + (v & 3);
            if (m >= M) continue;
            const int b = (int)(m / HW);
            float o = acc[j][v];
            if (a.out_scale) o *= a.out_scale[(long)b * a.Cout + co];
            if (a.gain != 1.f) o *= a.gain;
            if (a.noise) o += nw * a.noise[(long)b * a.noise_bstride + (m - (long)b * HW)];
            o += bv;
            if (a.lrelu) o = o >= 0.f ? o : o * 0.2f;
            if (a.relu) o = o > 0.f ? o : 0.f;
            const long idx = m * a.Cout + co;
            if (a.sft_scale) o = o * a.sft_scale[idx] + a.sft_shift[idx];
            if (a.res) o += a.res[idx];
            a.out[idx] = o;
        }
    }
}

// Workgroup tiles: pixels x K depth of one step (the N extent is 32 NT).  conv_mfma_kernel (CV_) and conv_bf16_kernel (CB_).
constexpr int CV_BM = 128, CV_BK = 16;
constexpr int CB_BM = 128, CB_BK = 32;

// One exact-fp32 conv (styleunet.hip).  e0 / e1: events around the launch, or null.
void launch_conv(const ConvArgs& a, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// ---- bf16 modes (styleunet_bf16.hip) ----
// A conv weight packed for the bf16 kernels: two planes (hi, then lo) of [Cout][Kp] bf16, the K index being tap * Cinp + ci with Cin
// padded to Cinp (a multiple of 8, one MFMA fragment) and K = k k Cinp padded to Kp (a multiple of 32, one K step); padding is zero.
constexpr int CONV_PRECISION_F32 = 0, CONV_PRECISION_BF16X3 = 1, CONV_PRECISION_BF16 = 2;
static_assert(CB_BK == 32, "conv_packed_kp pads K to one step of conv_bf16_kernel");
inline int conv_packed_cinp(int Cin) { return (Cin + 7) & ~7; }
inline int conv_packed_kp(int Cin, int k) { return (k * k * conv_packed_cinp(Cin) + 31) & ~31; }
inline size_t conv_packed_elems(int Cin, int Cout, int k) { return (size_t)2 * Cout * conv_packed_kp(Cin, k); }      // 2-byte elements

// Which instantiation a launch runs and on what grid: the one choice launch_conv and launch_conv_bf16 switch on (styleunet.hip; host
// only, asked without a device through artalk_op_conv2d_plan).  Of `a` it looks at the shape, x, x_bstride, w, in_scale and
// in_scale_ld; pointers are looked at for presence and alignment, never dereferenced.
//   nt      1 for Cout <= 32, else 2: the tile depends on Cout alone (never on B), so the K order of an output value does not depend
//           on how frames are batched
//   va      vector loads of x and in_scale: Cin % 8 == 0, x and in_scale 16-byte aligned, x_bstride % 4 == 0 and in_scale_ld % 4 == 0
//   vb      fp32 only (-1 in the bf16 modes, which read the packed copy): vector loads of w: Cout % 4 == 0 and w 16-byte aligned
//   np      products per MFMA step: 0 fp32, 3 bf16x3, 1 bf16
//   nsteps  K steps of the main loop: k k ceil(Cin / CV_BK) in fp32, kp / CB_BK in the bf16 modes
//   cinp, kp: the packed weight's paddings (0 in fp32)
struct ConvPlan { int nt, va, vb, np; unsigned gx, gy; int nsteps, cinp, kp; };
ConvPlan plan_conv(const ConvArgs& a, int precision);

// w [k k][Cin][Cout] fp32 -> packed (conv_packed_elems 2-byte elements, 16-byte aligned)
void launch_conv_pack(const float* w, void* packed, int Cin, int Cout, int k, hipStream_t s);
// One conv in mode `precision` (1 or 2) from the packed weight; a.w is not read.  e0 / e1: events around the launch, or null.
void launch_conv_bf16(const ConvArgs& a, const void* packed, int precision, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

}  // namespace artalk
