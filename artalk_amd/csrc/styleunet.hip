// StyleUNet upsampler of the GAGAvatar head, forward only, exact fp32 ("StyleUNet upsampler"): a stand-in for
// app/GAGAvatar/modules/style_unet.py.  Activations are channels-last ([B][H][W][C]) between the two layout kernels at the ends of a
// call, so the K index (tap, ci) of a convolution's implicit GEMM is contiguous in memory; the public tensors are NCHW.
//
//   conv_mfma_kernel   k x k (1 or 3), stride 1, zero padding k / 2: M = B H W pixels, N = Cout, K = k k Cin on
//                      v_mfma_f32_32x32x2f32, with the input scale (modulation) as prologue and, as epilogue in this order, output
//                      scale (demodulation), gain, noise, bias, LeakyReLU 0.2, SFT and residual
//                      (its bf16x3 / bf16 counterpart, selected by artalk_styleunet_set_precision, is styleunet_bf16.hip)
//   resample2_kernel   bilinear x2 (0.25 / 0.75, edges clamped) and x0.5 (2 x 2 mean), align_corners = False
//   linear / normstyle / demod kernels: the GEMV-sized style path, one wave per output value, fixed summation order
//
// No atomics and no split of K anywhere: the K order of every output value is fixed by the layer alone, so results are bit-identical
// from run to run and for any split of the frames over slabs and calls.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "artalk_hip.h"
#include "common.h"
#include "device_mem.h"
#include "styleunet_conv.h"
#include "weight_store.h"

namespace artalk {

// ------------------------------------------------------------------ convolution ------------------------------------------------------
constexpr int CV_LDA = CV_BM + 32;      // pitches = 32 mod 64 banks: the two half-waves of a fragment read (k, k + 1) hit disjoint banks
constexpr int CV_LDB = 96;

// One workgroup: 128 pixels x 32 NT output channels; wave w owns pixels 32 w .. 32 w + 31 and all NT column tiles.  K runs tap by tap
// and, inside a tap, over Cin in chunks of 16, two LDS buffers deep with the next chunk's global loads in flight during the MFMAs.
// VA: Cin % 8 == 0 and 16-byte aligned rows of x (vector loads); VB: Cout % 4 == 0 (vector loads of w).
template <int NT, bool VA, bool VB>
__global__ __launch_bounds__(256) void conv_mfma_kernel(ConvArgs a) {
    __shared__ float As[2][CV_BK * CV_LDA];
    __shared__ float Bs[2][CV_BK * CV_LDB];
    constexpr int BN = 32 * NT;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const long M = (long)a.B * a.H * a.W;
    const int HW = a.H * a.W;
    const long m0 = (long)blockIdx.x * CV_BM;
    const int n0 = blockIdx.y * BN;
    const int pad = a.k >> 1;
    const int nchunk = (a.Cin + CV_BK - 1) / CV_BK;
    const int nsteps = a.k * a.k * nchunk;

    // this thread's share of the A tile: pixel ai, 8 consecutive ci starting at 8 aq
    const int ai = t & (CV_BM - 1), aq = t >> 7;
    const long am = m0 + ai;
    const bool apix = am < M;
    int ab = 0, ay = 0, ax = 0;
    if (apix) { ab = (int)(am / HW); const int rem = (int)(am - (long)ab * HW); ay = rem / a.W; ax = rem - ay * a.W; }
    const float* xb = a.x + (long)ab * a.x_bstride;
    const float* sb = a.in_scale ? a.in_scale + (long)ab * a.in_scale_ld : nullptr;
    // ... and of the B tile: k row bk, 4 consecutive co starting at bc
    constexpr int BQ = BN / 4;
    const int bk = t / BQ, bc = (t % BQ) * 4;
    const bool bthread = t < CV_BK * BQ;

    float ra[8], rb[4];
    auto gload = [&](int step) {
        const int tap = step / nchunk, c0 = (step - tap * nchunk) * CV_BK;
        const int ky = tap / a.k, kx = tap - ky * a.k;
        const int yy = ay + ky - pad, xx = ax + kx - pad;
        const bool inb = apix && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
        const int ci = c0 + aq * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) ra[e] = 0.f;
        if (inb) {
            const float* p = xb + ((long)yy * a.W + xx) * a.Cin + ci;
            if (VA) {
                if (ci < a.Cin) {
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(p), v1 = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { ra[e] = v0[e]; ra[4 + e] = v1[e]; }
                    if (sb) {
                        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sb + ci), s1 = *reinterpret_cast<const f32x4*>(sb + ci + 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { ra[e] *= s0[e]; ra[4 + e] *= s1[e]; }
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (ci + e < a.Cin) ra[e] = sb ? p[e] * sb[ci + e] : p[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) rb[e] = 0.f;
        const int wci = c0 + bk, co = n0 + bc;
        if (bthread && wci < a.Cin) {
            const float* p = a.w + ((long)tap * a.Cin + wci) * a.Cout + co;
            if (VB) {
                if (co < a.Cout) { const f32x4 v = *reinterpret_cast<const f32x4*>(p); rb[0] = v[0]; rb[1] = v[1]; rb[2] = v[2]; rb[3] = v[3]; }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (co + e < a.Cout) rb[e] = p[e];
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int e = 0; e < 8; ++e) As[buf][(aq * 8 + e) * CV_LDA + ai] = ra[e];
        if (bthread) { const f32x4 v = {rb[0], rb[1], rb[2], rb[3]}; *reinterpret_cast<f32x4*>(&Bs[buf][bk * CV_LDB + bc]) = v; }
    };

    // Three levels of partial sums, so that a long K does not pile its rounding onto one running sum (one accumulator over
    // K = 4608 measured 13 x the error of a float32 CPU conv): each 16-wide chunk sums from zero, 16 chunks make a block, blocks add up.
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
        const float* as = &As[buf][h * CV_LDA + wave * 32 + r];
        const float* bs = &Bs[buf][h * CV_LDB + r];
        f32x16 part[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) part[j][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < CV_BK / 2; ++ks) {
            const float av = as[2 * ks * CV_LDA];
#pragma unroll
            for (int j = 0; j < NT; ++j) part[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bs[2 * ks * CV_LDB + j * 32], part[j], 0, 0, 0);
        }
        if (step + 1 < nsteps) lstore(buf ^ 1);
#pragma unroll
        for (int j = 0; j < NT; ++j) mid[j] += part[j];
        if ((step & 15) == 15) {
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

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

ConvPlan plan_conv(const ConvArgs& a, int precision) {
    const long M = (long)a.B * a.H * a.W;
    ConvPlan p{};
    p.nt = a.Cout <= 32 ? 1 : 2;
    p.va = a.Cin % 8 == 0 && aligned16(a.x) && a.x_bstride % 4 == 0 && (!a.in_scale || (aligned16(a.in_scale) && a.in_scale_ld % 4 == 0));
    p.gy = (unsigned)((a.Cout + 32 * p.nt - 1) / (32 * p.nt));
    if (precision == CONV_PRECISION_F32) {
        p.vb = a.Cout % 4 == 0 && aligned16(a.w);
        p.gx = (unsigned)((M + CV_BM - 1) / CV_BM);
        p.nsteps = a.k * a.k * ((a.Cin + CV_BK - 1) / CV_BK);
    } else {
        p.vb = -1;
        p.np = precision == CONV_PRECISION_BF16X3 ? 3 : 1;
        p.gx = (unsigned)((M + CB_BM - 1) / CB_BM);
        p.cinp = conv_packed_cinp(a.Cin); p.kp = conv_packed_kp(a.Cin, a.k);
        p.nsteps = p.kp / CB_BK;
    }
    return p;
}

void launch_conv(const ConvArgs& a, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if ((long)a.B * a.H * a.W <= 0) return;
    const ConvPlan p = plan_conv(a, CONV_PRECISION_F32);
    const bool va = p.va, vb = p.vb;
    const dim3 grid(p.gx, p.gy), block(256);
#define CV_GO(NT, VA, VB)                                                                                              \
    do {                                                                                                               \
        if (e0) hipExtLaunchKernelGGL((conv_mfma_kernel<NT, VA, VB>), grid, block, 0, s, e0, e1, 0, a);                \
        else ARTALK_LAUNCH((conv_mfma_kernel<NT, VA, VB>), grid, block, 0, s, a);                                      \
    } while (0)
    if (p.nt == 1) {
        if (va && vb) CV_GO(1, true, true); else if (va) CV_GO(1, true, false); else if (vb) CV_GO(1, false, true); else CV_GO(1, false, false);
    } else {
        if (va && vb) CV_GO(2, true, true); else if (va) CV_GO(2, true, false); else if (vb) CV_GO(2, false, true); else CV_GO(2, false, false);
    }
#undef CV_GO
}

// ------------------------------------------------------------------ resampling and layout --------------------------------------------
// x [B][H][W][C] -> out [B][2H][2W][C] (up) or [B][H/2][W/2][C]; one thread per output value, C fastest.
__global__ __launch_bounds__(256) void resample2_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H, int W, int C, int up) {
    const int OH = up ? 2 * H : H / 2, OW = up ? 2 * W : W / 2;
    const long n = (long)B * OH * OW * C;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    long p = i / C;
    const int ox = (int)(p % OW); p /= OW;
    const int oy = (int)(p % OH);
    const int b = (int)(p / OH);
    const float* xb = x + (long)b * H * W * C + c;
    if (up) {
        // source coordinate (o + 0.5) / 2 - 0.5, clamped at 0: lower neighbour, weight of the upper one
        const int y0 = oy == 0 ? 0 : (oy - 1) >> 1, x0 = ox == 0 ? 0 : (ox - 1) >> 1;
        const float ly = oy == 0 ? 0.f : (oy & 1) ? 0.25f : 0.75f, lx = ox == 0 ? 0.f : (ox & 1) ? 0.25f : 0.75f;
        const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        const float p00 = xb[((long)y0 * W + x0) * C], p01 = xb[((long)y0 * W + x1) * C];
        const float p10 = xb[((long)y1 * W + x0) * C], p11 = xb[((long)y1 * W + x1) * C];
        out[i] = (1.f - ly) * ((1.f - lx) * p00 + lx * p01) + ly * ((1.f - lx) * p10 + lx * p11);
    } else {
        const float p00 = xb[((long)(2 * oy) * W + 2 * ox) * C], p01 = xb[((long)(2 * oy) * W + 2 * ox + 1) * C];
        const float p10 = xb[((long)(2 * oy + 1) * W + 2 * ox) * C], p11 = xb[((long)(2 * oy + 1) * W + 2 * ox + 1) * C];
        out[i] = 0.5f * (0.5f * p00 + 0.5f * p01) + 0.5f * (0.5f * p10 + 0.5f * p11);
    }
}

__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}

// [B][C][HW] -> [B][HW][C] (one thread per output value)
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, long HW) {
    const long n = (long)B * C * HW;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const long p = i / C;
    const long b = p / HW, q = p - b * HW;
    out[i] = x[(b * C + c) * HW + q];
}

// [B][HW][C] -> [B][C][HW], with the final sigmoid (one thread per output value)
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, long HW, int sigmoid) {
    const long n = (long)B * C * HW;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long q = i % HW;
    const long p = i / HW;
    const int c = (int)(p % C);
    const long b = p / C;
    float v = x[(b * HW + q) * C + c];
    if (sigmoid) v = 1.f / (1.f + expf(-v));
    out[i] = v;
}

// ------------------------------------------------------------------ style path -------------------------------------------------------
// y[b][o] = act(sum_i x[b][i] W[o][i] + bias[o]); one wave per (b, o), lane l sums i = l, l + 64, ... in order, then a butterfly
__global__ __launch_bounds__(256) void linear_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                     float* __restrict__ y, int B, int In, int Out, int lrelu) {
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long)B * Out) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(wid / Out), o = (int)(wid - (long)b * Out);
    const float* xr = x + (long)b * In;
    const float* wr = W + (long)o * In;
    float s = 0.f;
    for (int i = lane; i < In; i += 64) s += xr[i] * wr[i];
    s = wave_sum(s);
    if (lane == 0) {
        s += bias ? bias[o] : 0.f;
        if (lrelu) s = s >= 0.f ? s : s * 0.2f;
        y[wid] = s;
    }
}

// NormStyleCode: y = x rsqrt(mean(x^2) + 1e-8); one wave per sample
__global__ __launch_bounds__(64) void normstyle_kernel(const float* __restrict__ x, float* __restrict__ y, int n) {
    const float* xr = x + (long)blockIdx.x * n;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) s += xr[i] * xr[i];
    s = wave_sum(s);
    const float k = rsqrtf(s / (float)n + 1e-8f);
    for (int i = threadIdx.x; i < n; i += 64) y[(long)blockIdx.x * n + i] = xr[i] * k;
}

// d[b][co] = rsqrt(sum_ci s[b][ci]^2 wsq[co][ci] + 1e-8), wsq = sum over the taps of W^2; s rows are ld apart; one wave per (b, co)
__global__ __launch_bounds__(256) void demod_kernel(const float* __restrict__ s, long ld, const float* __restrict__ wsq, float* __restrict__ d,
                                                    int B, int Cin, int Cout) {
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long)B * Cout) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(wid / Cout), co = (int)(wid - (long)b * Cout);
    const float* sr = s + (long)b * ld;
    const float* wr = wsq + (long)co * Cin;
    float acc = 0.f;
    for (int i = lane; i < Cin; i += 64) acc += sr[i] * sr[i] * wr[i];
    acc = wave_sum(acc);
    if (lane == 0) d[wid] = rsqrtf(acc + 1e-8f);
}

static inline unsigned blocks256(long n) { return (unsigned)((n + 255) / 256); }
static inline unsigned waves4(long n) { return (unsigned)((n + 3) / 4); }      // workgroups of four waves, one wave per output value

// One launcher per kernel, each with its grid: SuRun and the artalk_op_su_* entry points both launch through these, so the grid a
// kernel-level test runs is the grid the network runs.
static void launch_linear(const float* x, const float* W, const float* bias, float* y, int B, int In, int Out, int lrelu, hipStream_t s) {
    ARTALK_LAUNCH(linear_kernel, dim3(waves4((long)B * Out)), dim3(256), 0, s, x, W, bias, y, B, In, Out, lrelu);
}
static void launch_normstyle(const float* x, float* y, int B, int n, hipStream_t s) {
    ARTALK_LAUNCH(normstyle_kernel, dim3(B), dim3(64), 0, s, x, y, n);
}
static void launch_demod(const float* sm, long ld, const float* wsq, float* d, int B, int Cin, int Cout, hipStream_t s) {
    ARTALK_LAUNCH(demod_kernel, dim3(waves4((long)B * Cout)), dim3(256), 0, s, sm, ld, wsq, d, B, Cin, Cout);
}
static void launch_add(const float* a, const float* b, float* out, long n, hipStream_t s) {
    ARTALK_LAUNCH(add_kernel, dim3(blocks256(n)), dim3(256), 0, s, a, b, out, n);
}
static void launch_to_nhwc(const float* x, float* out, int B, int C, long HW, hipStream_t s) {
    ARTALK_LAUNCH(nchw_to_nhwc_kernel, dim3(blocks256((long)B * C * HW)), dim3(256), 0, s, x, out, B, C, HW);
}
static void launch_to_nchw(const float* x, float* out, int B, int C, long HW, int sigmoid, hipStream_t s) {
    ARTALK_LAUNCH(nhwc_to_nchw_kernel, dim3(blocks256((long)B * C * HW)), dim3(256), 0, s, x, out, B, C, HW, sigmoid);
}

}  // namespace artalk

using namespace artalk;

// ------------------------------------------------------------------ the module -------------------------------------------------------
namespace {

struct SuConv { const float* w = nullptr; const float* b = nullptr; int cin = 0, cout = 0, k = 0; const void* wp = nullptr; };      // wp: packed for the bf16 modes
struct SuMod { SuConv c; const float* wsq = nullptr; const float* nw = nullptr; int mod_off = 0; };      // nw, wsq: style convs only

}  // namespace

struct artalk_styleunet {
    int device = 0, in_dim = 0, out_dim = 0, S = 0, L = 0, num_layers = 0;
    bool finalized = false, timing = false;
    int precision = CONV_PRECISION_F32;      // of the convolutions (artalk_styleunet_set_precision)
    int slab_max = 1, slab = 1;
    int64_t frame_floats = 0;
    WeightStore store;                       // the manifest, and every uploaded tensor
    std::vector<DevBuf<uint16_t>> packed;    // bf16 hi / lo planes of every conv weight: empty until a bf16 mode is first selected
    DevBuf<float> ws;
    // device weights
    SuConv first, final_conv;
    std::vector<SuConv> dn1, dn2, dnsk, up1, up2, upsk, cs0, cs2, ch0, ch2;
    const float *lin_w = nullptr, *lin_b = nullptr, *mlp_w[8] = {}, *mlp_b[8] = {}, *mod_w = nullptr, *mod_b = nullptr, *const_in = nullptr;
    int mod_total = 0;
    SuMod sc1, rgb1;
    std::vector<SuMod> sconv, rgb;
    std::vector<const float*> noise_buf;
    // timing of the conv kernel (tools/styleunet_bench.py)
    CallTimer timer;                         // the call, and a pair of events per conv launch
    std::vector<int32_t> ev_geom;           // per timed launch: frames, H, Cin, Cout, k
    std::vector<double> launch_ms;           // per timed launch of the last call
    std::string err;
};

static thread_local std::string g_su_error;

namespace {

int su_fail(artalk_styleunet* u, int rc, const std::string& msg) { u->err = msg; return rc; }

int su_ch(int size) { return size <= 32 ? 256 : 8192 / size; }      // 64: 128, 128: 64, 256: 32, 512: 16, 1024: 8

void su_add(artalk_styleunet* u, const std::string& name, std::vector<int64_t> shape) { u->store.declare(name, std::move(shape)); }

void su_manifest(artalk_styleunet* u) {
    const int L = u->L, S = u->S, F = 512;
    auto conv = [&](const std::string& n, int cin, int cout, int k, bool bias = true) {
        su_add(u, n + ".weight", {cout, cin, k, k});
        if (bias) su_add(u, n + ".bias", {cout});
    };
    auto resblock = [&](const std::string& n, int cin, int cout) {
        conv(n + ".conv1", cin, cin, 3); conv(n + ".conv2", cin, cout, 3); conv(n + ".skip", cin, cout, 1, false);
    };
    auto modconv = [&](const std::string& n, int cin, int cout, int k) {
        su_add(u, n + ".weight", {1, cout, cin, k, k});
        su_add(u, n + ".modulation.weight", {cin, F});
        su_add(u, n + ".modulation.bias", {cin});
    };
    auto styleconv = [&](const std::string& n, int cin, int cout) {
        su_add(u, n + ".weight", {1});
        su_add(u, n + ".bias", {1, cout, 1, 1});
        modconv(n + ".modulated_conv", cin, cout, 3);
    };
    auto torgb = [&](const std::string& n, int cin) {
        su_add(u, n + ".bias", {1, u->out_dim, 1, 1});
        modconv(n + ".modulated_conv", cin, u->out_dim, 1);
    };
    conv("conv_body_first", u->in_dim, su_ch(S), 1);
    int c = su_ch(S);
    for (int j = 0, i = L; i > 2; --i, ++j) { resblock("conv_body_down." + std::to_string(j), c, su_ch(1 << (i - 1))); c = su_ch(1 << (i - 1)); }
    conv("final_conv", c, 256, 3);
    c = 256;
    for (int j = 0, i = 3; i <= L; ++i, ++j) { resblock("conv_body_up." + std::to_string(j), c, su_ch(1 << i)); c = su_ch(1 << i); }
    for (int j = 0, i = 3; i <= L; ++i, ++j) conv("toRGB." + std::to_string(j), su_ch(1 << i), 3, 1);      // dead in the forward pass
    su_add(u, "final_linear.weight", {F, 4096});
    su_add(u, "final_linear.bias", {F});
    const std::string d = "stylegan_decoder.";
    for (int j = 0; j < 8; ++j) {
        su_add(u, d + "style_mlp." + std::to_string(2 * j + 1) + ".weight", {F, F});
        su_add(u, d + "style_mlp." + std::to_string(2 * j + 1) + ".bias", {F});
    }
    su_add(u, d + "constant_input.weight", {1, 512, 4, 4});
    styleconv(d + "style_conv1", 512, 512);
    torgb(d + "to_rgb1", 512);
    c = 512;
    for (int j = 0, i = 3; i <= L; ++i, ++j) {
        const int co = 2 * su_ch(1 << i);
        styleconv(d + "style_convs." + std::to_string(2 * j), c, co);
        styleconv(d + "style_convs." + std::to_string(2 * j + 1), co, co);
        c = co;
    }
    for (int j = 0, i = 3; i <= L; ++i, ++j) torgb(d + "to_rgbs." + std::to_string(j), 2 * su_ch(1 << i));
    for (int l = 0; l < u->num_layers; ++l) { const int r = 1 << ((l + 5) / 2); su_add(u, d + "noises.noise" + std::to_string(l), {1, 1, r, r}); }
    for (const char* which : {"condition_scale.", "condition_shift."})
        for (int j = 0, i = 3; i <= L; ++i, ++j) {
            const int cc = su_ch(1 << i);
            conv(which + std::to_string(j) + ".0", cc, cc, 3);
            conv(which + std::to_string(j) + ".2", cc, 2 * cc, 3);
        }
}

// One pass over the module: with dry = true it only sizes the workspace (floats per frame); otherwise it enqueues the n frames at x.
struct SuRun {
    artalk_styleunet* u; int n; hipStream_t s; bool dry;
    int64_t off = 0, peak = 0;      // a stack: what a block needs only inside itself is released at its end (one stream: reuse is ordered)
    float* alloc(int64_t per_frame) {
        per_frame = (per_frame + 3) & ~(int64_t)3;
        float* p = dry ? nullptr : u->ws.get() + off;      // off counts floats: of one frame (dry) or of the n frames of this slab
        off += per_frame * (dry ? 1 : n);
        if (off > peak) peak = off;
        return p;
    }
    void conv(const SuConv& c, const float* x, long x_bstride, float* out, int H, int lrelu, const float* res = nullptr,
              const SuMod* m = nullptr, const float* smod = nullptr, const float* dmod = nullptr, const float* noise = nullptr,
              long noise_bstride = 0, const float* sft_scale = nullptr, const float* sft_shift = nullptr) {
        if (dry) return;
        ConvArgs a{};
        a.x = x; a.x_bstride = x_bstride; a.w = c.w; a.out = out; a.B = n; a.H = H; a.W = H; a.Cin = c.cin; a.Cout = c.cout; a.k = c.k;
        a.in_scale = smod; a.in_scale_ld = u->mod_total; a.out_scale = dmod; a.gain = (m && m->nw) ? 1.41421356237309504880f : 1.f;
        a.noise = noise; a.noise_bstride = noise_bstride; a.noise_w = m ? m->nw : nullptr;
        a.bias = c.b; a.lrelu = lrelu; a.sft_scale = sft_scale; a.sft_shift = sft_shift; a.res = res;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (u->timer.pair(&e0, &e1))
            for (int v : {n, H, c.cin, c.cout, c.k}) u->ev_geom.push_back(v);
        if (u->precision != CONV_PRECISION_F32) launch_conv_bf16(a, c.wp, u->precision, s, e0, e1);
        else launch_conv(a, s, e0, e1);
    }
    void resample(const float* x, float* out, int H, int C, int up) {
        if (dry) return;
        const long total = (long)n * (up ? 4L * H * H : (long)(H / 2) * (H / 2)) * C;
        ARTALK_LAUNCH(resample2_kernel, dim3(blocks256(total)), dim3(256), 0, s, x, out, n, H, H, C, up);
    }
    void linear(const float* x, const float* W, const float* b, float* y, int In, int Out, int lrelu) {
        if (dry) return;
        launch_linear(x, W, b, y, n, In, Out, lrelu, s);
    }

    // noise: per layer the pointer of this slab's first frame and the frame stride
    void run(const float* x, const float* const* noise, const int64_t* nstride, int activation, float* out_dev) {
        const int S = u->S, L = u->L;
        const long SS = (long)S * S;
        float* xin = alloc(SS * u->in_dim);
        if (!dry) launch_to_nhwc(x, xin, n, u->in_dim, SS, s);
        float* feat = alloc(SS * u->first.cout);
        conv(u->first, xin, SS * u->in_dim, feat, S, 1);
        auto resblock = [&](const SuConv& c1, const SuConv& c2, const SuConv& sk, const float* in, int H, int up) -> float* {
            const int OH = up ? 2 * H : H / 2;
            const long hw = (long)H * H, ohw = (long)OH * OH;
            float* o = alloc(ohw * c2.cout);
            const int64_t mark = off;
            float* t1 = alloc(hw * c1.cout);
            conv(c1, in, hw * c1.cin, t1, H, 1);
            float* t2 = alloc(ohw * c1.cout);
            resample(t1, t2, H, c1.cout, up);
            float* xs = alloc(ohw * c1.cin);
            resample(in, xs, H, c1.cin, up);
            float* skp = alloc(ohw * sk.cout);
            conv(sk, xs, ohw * sk.cin, skp, OH, 0);
            conv(c2, t2, ohw * c2.cin, o, OH, 1, skp);
            off = mark;
            return o;
        };
        std::vector<float*> skips(L - 2);
        int cur = S;
        for (int i = 0; i < L - 2; ++i) {
            feat = resblock(u->dn1[i], u->dn2[i], u->dnsk[i], feat, cur, 0);
            cur /= 2;
            skips[L - 3 - i] = feat;
        }
        float* f4 = alloc(16 * 256);
        conv(u->final_conv, feat, 16L * u->final_conv.cin, f4, 4, 1);
        float* code = alloc(512);
        linear(f4, u->lin_w, u->lin_b, code, 4096, 512, 0);
        std::vector<float*> conds(2 * (L - 2));
        feat = f4;
        for (int i = 0; i < L - 2; ++i) {
            const long hw = (long)cur * cur;
            const int c = u->up1[i].cin;
            float* sum = alloc(hw * c);      // (stays: the block's output is stacked above it)
            if (!dry) launch_add(feat, skips[i], sum, (long)n * hw * c, s);
            feat = resblock(u->up1[i], u->up2[i], u->upsk[i], sum, cur, 1);
            cur *= 2;
            const long ohw = (long)cur * cur;
            const int cc = u->up2[i].cout;
            for (int w = 0; w < 2; ++w) {
                const SuConv& c0 = w ? u->ch0[i] : u->cs0[i];
                const SuConv& c2 = w ? u->ch2[i] : u->cs2[i];
                float* o = alloc(ohw * 2 * cc);
                const int64_t mark = off;
                float* t = alloc(ohw * cc);
                conv(c0, feat, ohw * cc, t, cur, 1);
                conv(c2, t, ohw * cc, o, cur, 0);
                off = mark;
                conds[2 * i + w] = o;
            }
        }
        // ---- style path ----
        float* lat = alloc(512);
        if (!dry) launch_normstyle(code, lat, n, 512, s);
        for (int j = 0; j < 8; ++j) {
            float* nx = alloc(512);
            linear(lat, u->mlp_w[j], u->mlp_b[j], nx, 512, 512, 1);
            lat = nx;
        }
        float* smod = alloc(u->mod_total);
        linear(lat, u->mod_w, u->mod_b, smod, 512, u->mod_total, 0);
        auto styleconv = [&](const SuMod& m, const float* in, long in_bstride, float* out, int H, int layer, const float* sc, const float* sh) {
            float* d = alloc(m.c.cout);
            if (!dry) launch_demod(smod + m.mod_off, (long)u->mod_total, m.wsq, d, n, m.c.cin, m.c.cout, s);
            conv(m.c, in, in_bstride, out, H, 1, nullptr, &m, dry ? nullptr : smod + m.mod_off, d, dry ? nullptr : noise[layer],
                 dry ? 0 : (long)nstride[layer], sc, sh);
        };
        float* o = alloc(16 * 512);
        styleconv(u->sc1, u->const_in, 0, o, 4, 0, nullptr, nullptr);
        float* skip = alloc(16 * u->out_dim);
        conv(u->rgb1.c, o, 16L * 512, skip, 4, 0, nullptr, &u->rgb1, dry ? nullptr : smod + u->rgb1.mod_off);
        cur = 4;
        for (int j = 0; j < L - 2; ++j) {
            const SuMod &m1 = u->sconv[2 * j], &m2 = u->sconv[2 * j + 1], &mr = u->rgb[j];
            const long ohw = 4L * cur * cur;
            float* o2 = alloc(ohw * m2.c.cout);
            float* sk2 = alloc(ohw * u->out_dim);
            const int64_t mark = off;
            float* up = alloc(ohw * m1.c.cin);
            resample(o, up, cur, m1.c.cin, 1);
            float* o1 = alloc(ohw * m1.c.cout);
            styleconv(m1, up, ohw * m1.c.cin, o1, 2 * cur, 1 + 2 * j, conds[2 * j], conds[2 * j + 1]);
            styleconv(m2, o1, ohw * m2.c.cin, o2, 2 * cur, 2 + 2 * j, nullptr, nullptr);
            float* su = alloc(ohw * u->out_dim);
            resample(skip, su, cur, u->out_dim, 1);
            conv(mr.c, o2, ohw * mr.c.cin, sk2, 2 * cur, 0, su, &mr, dry ? nullptr : smod + mr.mod_off);
            off = mark;
            o = o2; skip = sk2; cur *= 2;
        }
        if (!dry) launch_to_nchw(skip, out_dev, n, u->out_dim, SS, activation, s);
    }
};

// Packs every conv weight for the bf16 modes (once per module; the null stream, and waits for it).
bool su_pack_bf16(artalk_styleunet* u) {
    if (!u->packed.empty()) return true;
    std::vector<SuConv*> all = {&u->first, &u->final_conv, &u->sc1.c, &u->rgb1.c};
    for (auto* v : {&u->dn1, &u->dn2, &u->dnsk, &u->up1, &u->up2, &u->upsk, &u->cs0, &u->cs2, &u->ch0, &u->ch2})
        for (SuConv& c : *v) all.push_back(&c);
    for (auto* v : {&u->sconv, &u->rgb})
        for (SuMod& m : *v) all.push_back(&m.c);
    bool ok = true;
    for (SuConv* c : all) {
        u->packed.emplace_back();
        if (!u->packed.back().alloc(conv_packed_elems(c->cin, c->cout, c->k))) { ok = false; break; }
        c->wp = u->packed.back().get();
        launch_conv_pack(c->w, u->packed.back().get(), c->cin, c->cout, c->k, nullptr);
    }
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) ok = false;
    if (!ok) u->packed.clear();
    return ok;
}

}  // namespace

// the per-layer noise arguments of artalk_styleunet_forward and artalk_gaga_render (ptrs == NULL: the module's own noise)
int artalk::su_check_noise(int num_layers, const float* const* ptrs, const int64_t* strides, std::string* err) {
    if (!ptrs) return ARTALK_OK;
    if (!strides) { *err = "noise_batch_strides must not be NULL when noise_ptrs is given"; return ARTALK_EINVAL; }
    for (int l = 0; l < num_layers; ++l) {
        const int64_t r = 1 << ((l + 5) / 2);
        if (!ptrs[l]) { *err = "noise_ptrs[" + std::to_string(l) + "] is NULL"; return ARTALK_EINVAL; }
        if (strides[l] != 0 && strides[l] < r * r) {
            *err = "noise_batch_strides[" + std::to_string(l) + "] must be 0 or at least " + std::to_string(r * r);
            return ARTALK_EINVAL;
        }
    }
    return ARTALK_OK;
}

extern "C" {

const char* artalk_styleunet_last_error(const artalk_styleunet* u) { return u ? u->err.c_str() : g_su_error.c_str(); }

void artalk_styleunet_destroy(artalk_styleunet* u) {
    if (!u) return;
    if (u->store.on_device() || !u->timer.empty()) {     // (else nothing was ever taken from the device)
        (void)hipSetDevice(u->device);
        (void)hipDeviceSynchronize();
    }
    delete u;
}

int artalk_styleunet_create(int device_id, int in_dim, int out_dim, int out_size, artalk_styleunet** out) {
    if (!out) { g_su_error = "out is NULL"; return ARTALK_EINVAL; }
    if (device_id < 0) { g_su_error = "device_id must not be negative"; return ARTALK_EINVAL; }
    if (in_dim < 1 || in_dim > 4096) { g_su_error = "in_dim must be in 1..4096"; return ARTALK_EINVAL; }
    if (out_dim < 1 || out_dim > 4096) { g_su_error = "out_dim must be in 1..4096"; return ARTALK_EINVAL; }
    if (out_size < 8 || out_size > 1024 || (out_size & (out_size - 1))) { g_su_error = "out_size must be a power of two in 8..1024"; return ARTALK_EINVAL; }
    artalk_styleunet* u = new artalk_styleunet();
    u->device = device_id; u->in_dim = in_dim; u->out_dim = out_dim; u->S = out_size;
    for (u->L = 0; (1 << u->L) < out_size; ++u->L) {}
    u->num_layers = (u->L - 2) * 2 + 1;
    su_manifest(u);
    // modulation rows of every modulated conv, in launch order, are one Linear: the latent is the same for all of them
    u->mod_total = 0;
    SuRun dry{u, 1, nullptr, true};
    // (the dry run reads channel counts only: fill them from the manifest)
    auto shape_conv = [&](const std::string& n, SuConv& c) {
        const auto& sh = u->store.shape(n + ".weight");
        const size_t o = sh.size() == 5 ? 1 : 0;
        c.cout = (int)sh[o]; c.cin = (int)sh[o + 1]; c.k = (int)sh[o + 2];
    };
    const int nb = u->L - 2;
    u->dn1.resize(nb); u->dn2.resize(nb); u->dnsk.resize(nb); u->up1.resize(nb); u->up2.resize(nb); u->upsk.resize(nb);
    u->cs0.resize(nb); u->cs2.resize(nb); u->ch0.resize(nb); u->ch2.resize(nb); u->sconv.resize(2 * nb); u->rgb.resize(nb);
    shape_conv("conv_body_first", u->first);
    shape_conv("final_conv", u->final_conv);
    const std::string d = "stylegan_decoder.";
    auto shape_mod = [&](const std::string& n, SuMod& m) {
        shape_conv(n + ".modulated_conv", m.c);
        m.mod_off = u->mod_total;
        u->mod_total += (m.c.cin + 3) & ~3;      // 16-byte aligned rows for the conv's vector loads
    };
    shape_mod(d + "style_conv1", u->sc1);
    shape_mod(d + "to_rgb1", u->rgb1);
    for (int j = 0; j < nb; ++j) {
        const std::string js = std::to_string(j);
        shape_conv("conv_body_down." + js + ".conv1", u->dn1[j]); shape_conv("conv_body_down." + js + ".conv2", u->dn2[j]);
        shape_conv("conv_body_down." + js + ".skip", u->dnsk[j]);
        shape_conv("conv_body_up." + js + ".conv1", u->up1[j]); shape_conv("conv_body_up." + js + ".conv2", u->up2[j]);
        shape_conv("conv_body_up." + js + ".skip", u->upsk[j]);
        shape_conv("condition_scale." + js + ".0", u->cs0[j]); shape_conv("condition_scale." + js + ".2", u->cs2[j]);
        shape_conv("condition_shift." + js + ".0", u->ch0[j]); shape_conv("condition_shift." + js + ".2", u->ch2[j]);
        shape_mod(d + "style_convs." + std::to_string(2 * j), u->sconv[2 * j]);
        shape_mod(d + "style_convs." + std::to_string(2 * j + 1), u->sconv[2 * j + 1]);
        shape_mod(d + "to_rgbs." + js, u->rgb[j]);
    }
    dry.run(nullptr, nullptr, nullptr, 0, nullptr);
    u->frame_floats = dry.peak;
    const int64_t budget = 4ll << 30;      // 4 GiB of activations, skips and conditions
    const int64_t slab = budget / (u->frame_floats * 4);
    u->slab_max = (int)(slab < 1 ? 1 : slab > 64 ? 64 : slab);
    u->slab = u->slab_max;
    *out = u;
    return ARTALK_OK;
}

int artalk_styleunet_set_tensor(artalk_styleunet* u, const char* key, const void* host_ptr, int ndim, const int64_t* shape) {
    if (!u) { g_su_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (!key || !host_ptr || !shape) return su_fail(u, ARTALK_EINVAL, "key, host_ptr and shape must not be NULL");
    if (u->finalized) return su_fail(u, ARTALK_ESTATE, "weights are final after artalk_styleunet_finalize (packed copies exist); create a new handle");
    return u->store.set(key, host_ptr, ndim, shape, &u->err);
}

int artalk_styleunet_finalize(artalk_styleunet* u) {
    if (!u) { g_su_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (u->finalized) return su_fail(u, ARTALK_ESTATE, "artalk_styleunet_finalize was already called");
    if (u->store.missing(&u->err)) return ARTALK_EMISSING;
    if (hipSetDevice(u->device) != hipSuccess) return su_fail(u, ARTALK_EHIP, "hipSetDevice failed");
    WeightStore& st = u->store;
    auto pack = [&](const std::string& n, SuConv& c, bool bias) {
        c.w = st.upload(pack_conv_weight(st.host(n + ".weight"), c.cout, c.cin, c.cin, c.k));
        c.b = bias ? st.upload(n + ".bias") : nullptr;
    };
    std::vector<float> modw((size_t)u->mod_total * 512, 0.f), modb((size_t)u->mod_total, 0.f);
    auto pack_mod = [&](const std::string& n, SuMod& m, bool style) {
        pack(n + ".modulated_conv", m.c, false);
        m.c.b = st.upload(n + ".bias");
        const std::vector<float>& mw = st.host(n + ".modulated_conv.modulation.weight");
        const std::vector<float>& mb = st.host(n + ".modulated_conv.modulation.bias");
        std::memcpy(&modw[(size_t)m.mod_off * 512], mw.data(), mw.size() * sizeof(float));
        std::memcpy(&modb[m.mod_off], mb.data(), mb.size() * sizeof(float));
        if (style) {
            m.nw = st.upload(n + ".weight");
            const std::vector<float>& w = st.host(n + ".modulated_conv.weight");
            const int kk = m.c.k * m.c.k;
            std::vector<float> sq((size_t)m.c.cout * m.c.cin);
            for (size_t e = 0; e < sq.size(); ++e) {
                float acc = 0.f;
                for (int q = 0; q < kk; ++q) acc += w[e * kk + q] * w[e * kk + q];
                sq[e] = acc;
            }
            m.wsq = st.upload(sq);
        }
    };
    const int nb = u->L - 2;
    const std::string d = "stylegan_decoder.";
    pack("conv_body_first", u->first, true);
    pack("final_conv", u->final_conv, true);
    for (int j = 0; j < nb; ++j) {
        const std::string js = std::to_string(j);
        pack("conv_body_down." + js + ".conv1", u->dn1[j], true); pack("conv_body_down." + js + ".conv2", u->dn2[j], true);
        pack("conv_body_down." + js + ".skip", u->dnsk[j], false);
        pack("conv_body_up." + js + ".conv1", u->up1[j], true); pack("conv_body_up." + js + ".conv2", u->up2[j], true);
        pack("conv_body_up." + js + ".skip", u->upsk[j], false);
        pack("condition_scale." + js + ".0", u->cs0[j], true); pack("condition_scale." + js + ".2", u->cs2[j], true);
        pack("condition_shift." + js + ".0", u->ch0[j], true); pack("condition_shift." + js + ".2", u->ch2[j], true);
        pack_mod(d + "style_convs." + std::to_string(2 * j), u->sconv[2 * j], true);
        pack_mod(d + "style_convs." + std::to_string(2 * j + 1), u->sconv[2 * j + 1], true);
        pack_mod(d + "to_rgbs." + js, u->rgb[j], false);
    }
    pack_mod(d + "style_conv1", u->sc1, true);
    pack_mod(d + "to_rgb1", u->rgb1, false);
    u->mod_w = st.upload(modw);
    u->mod_b = st.upload(modb);
    {   // final_linear reads the 4 x 4 x 256 feature channels-last: column c 16 + p of the reference becomes p 256 + c
        const std::vector<float>& w = st.host("final_linear.weight");
        std::vector<float> t(w.size());
        for (int o = 0; o < 512; ++o)
            for (int c = 0; c < 256; ++c)
                for (int p = 0; p < 16; ++p) t[(size_t)o * 4096 + p * 256 + c] = w[(size_t)o * 4096 + c * 16 + p];
        u->lin_w = st.upload(t);
        u->lin_b = st.upload("final_linear.bias");
    }
    for (int j = 0; j < 8; ++j) {
        u->mlp_w[j] = st.upload(d + "style_mlp." + std::to_string(2 * j + 1) + ".weight");
        u->mlp_b[j] = st.upload(d + "style_mlp." + std::to_string(2 * j + 1) + ".bias");
    }
    {   // constant input [1][512][4][4] -> [4][4][512]
        const std::vector<float>& w = st.host(d + "constant_input.weight");
        std::vector<float> t(w.size());
        for (int c = 0; c < 512; ++c)
            for (int p = 0; p < 16; ++p) t[(size_t)p * 512 + c] = w[(size_t)c * 16 + p];
        u->const_in = st.upload(t);
    }
    u->noise_buf.resize(u->num_layers);
    for (int l = 0; l < u->num_layers; ++l) u->noise_buf[l] = st.upload(d + "noises.noise" + std::to_string(l));
    if (st.ok() && !u->ws.alloc((size_t)u->frame_floats * u->slab_max)) {
        return su_fail(u, ARTALK_EHIP, "hipMalloc of the workspace failed (" + std::to_string(u->frame_floats * u->slab_max * 4) + " bytes)");
    }
    if (!st.ok() || hipDeviceSynchronize() != hipSuccess) return su_fail(u, ARTALK_EHIP, "uploading the weights failed");
    st.release_host();
    if (u->precision != CONV_PRECISION_F32 && !su_pack_bf16(u)) return su_fail(u, ARTALK_EHIP, "packing the conv weights for the bf16 modes failed");
    u->finalized = true;
    return ARTALK_OK;
}

int artalk_styleunet_set_precision(artalk_styleunet* u, int mode) {
    if (!u) { g_su_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (mode != CONV_PRECISION_F32 && mode != CONV_PRECISION_BF16X3 && mode != CONV_PRECISION_BF16)
        return su_fail(u, ARTALK_EINVAL, "precision must be 0 (f32), 1 (bf16x3) or 2 (bf16)");
    if (mode != CONV_PRECISION_F32 && u->finalized) {      // (before finalize the mode is only remembered)
        if (hipSetDevice(u->device) != hipSuccess) return su_fail(u, ARTALK_EHIP, "hipSetDevice failed");
        if (!su_pack_bf16(u)) return su_fail(u, ARTALK_EHIP, "packing the conv weights for the bf16 modes failed");
    }
    u->precision = mode;
    return ARTALK_OK;
}

int artalk_styleunet_get_precision(const artalk_styleunet* u) {
    if (!u) { g_su_error = "handle is NULL"; return ARTALK_EINVAL; }
    return u->precision;
}

int artalk_styleunet_set_slab(artalk_styleunet* u, int frames) {
    if (!u) { g_su_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (frames < 0 || frames > u->slab_max)
        return su_fail(u, ARTALK_EINVAL, "slab must be in 0.." + std::to_string(u->slab_max) + " frames (0: the default)");
    u->slab = frames == 0 ? u->slab_max : frames;
    return u->slab;
}

int artalk_styleunet_dims(const artalk_styleunet* u, int* in_dim, int* out_dim, int* out_size, int* finalized, int* slab) {
    if (!u) { g_su_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (in_dim) *in_dim = u->in_dim;
    if (out_dim) *out_dim = u->out_dim;
    if (out_size) *out_size = u->S;
    if (finalized) *finalized = u->finalized ? 1 : 0;
    if (slab) *slab = u->slab;
    return u->device;
}

int artalk_styleunet_set_timing(artalk_styleunet* u, int enable) {
    if (!u) { g_su_error = "handle is NULL"; return ARTALK_EINVAL; }
    u->timing = enable != 0;
    return ARTALK_OK;
}

int artalk_styleunet_get_timing(const artalk_styleunet* u, double* conv_ms, double* total_ms) {
    if (!u) { g_su_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (conv_ms) *conv_ms = u->timer.pairs_ms();
    if (total_ms) *total_ms = u->timer.total_ms();
    return ARTALK_OK;
}

int artalk_styleunet_get_launch_timing(const artalk_styleunet* u, double* launch_ms, int32_t* geometry, int n) {
    if (!u) { g_su_error = "handle is NULL"; return ARTALK_EINVAL; }
    const int have = (int)u->launch_ms.size();
    for (int i = 0; i < have && i < n; ++i) {
        if (launch_ms) launch_ms[i] = u->launch_ms[i];
        if (geometry) for (int e = 0; e < 5; ++e) geometry[5 * i + e] = u->ev_geom[5 * (size_t)i + e];
    }
    return have;
}

int artalk_styleunet_forward(artalk_styleunet* u, const float* x_dev, int B, const float* const* noise_ptrs_or_null,
                             const int64_t* noise_batch_strides, int activation, float* out_dev, void* stream) {
    if (!u) { g_su_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (!u->finalized) return su_fail(u, ARTALK_ESTATE, "artalk_styleunet_forward before artalk_styleunet_finalize");
    if (B < 0) return su_fail(u, ARTALK_EINVAL, "B must not be negative");
    if (!x_dev || !out_dev) return su_fail(u, ARTALK_EINVAL, "x and out must not be NULL");
    const int rc = su_check_noise(u->num_layers, noise_ptrs_or_null, noise_batch_strides, &u->err);
    if (rc != ARTALK_OK) return rc;
    if (B == 0) return ARTALK_OK;
    (void)hipSetDevice(u->device);
    hipStream_t s = (hipStream_t)stream;
    const long SS = (long)u->S * u->S;
    std::vector<const float*> np(u->num_layers);
    std::vector<int64_t> ns(u->num_layers);
    if (u->timing) u->ev_geom.clear();
    if (!u->timer.begin(s, u->timing)) return su_fail(u, ARTALK_EHIP, "hipEventCreate failed");
    for (int b0 = 0; b0 < B; b0 += u->slab) {
        const int n = B - b0 < u->slab ? B - b0 : u->slab;
        for (int l = 0; l < u->num_layers; ++l) {
            ns[l] = noise_ptrs_or_null ? noise_batch_strides[l] : 0;
            np[l] = (noise_ptrs_or_null ? noise_ptrs_or_null[l] : u->noise_buf[l]) + (long)b0 * ns[l];
        }
        SuRun run{u, n, s, false};
        run.run(x_dev + (long)b0 * u->in_dim * SS, np.data(), ns.data(), activation, out_dev + (long)b0 * u->out_dim * SS);
    }
    if (hipGetLastError() != hipSuccess) return su_fail(u, ARTALK_EHIP, "kernel launch failed");
    if (!u->timer.end()) return su_fail(u, ARTALK_EHIP, "the call failed on the device");
    if (u->timing) u->launch_ms = u->timer.pair_ms();
    return ARTALK_OK;
}

// what artalk_op_conv2d_ex and artalk_op_conv2d_plan refuse in the arguments they share
static bool conv_op_shape_ok(const void* x, int64_t x_bstride, const void* w, int B, int H, int W, int Cin, int Cout, int k, int precision) {
    if (!x || !w) return false;
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (k != 1 && k != 3)) return false;
    if ((int64_t)B * H * W > (int64_t)1 << 30 || (int64_t)H * W > INT_MAX) return false;
    if (x_bstride != 0 && x_bstride < (int64_t)H * W * Cin) return false;
    return precision == CONV_PRECISION_F32 || precision == CONV_PRECISION_BF16X3 || precision == CONV_PRECISION_BF16;
}

int artalk_op_conv2d_plan(uint64_t x_addr, int64_t x_bstride, uint64_t w_addr, uint64_t in_scale_addr, int B, int H, int W, int Cin, int Cout,
                          int k, int precision, int32_t* out, int n) {
    const void *x = (const void*)(uintptr_t)x_addr, *w = (const void*)(uintptr_t)w_addr;
    if (!conv_op_shape_ok(x, x_bstride, w, B, H, W, Cin, Cout, k, precision) || n < 0 || (n > 0 && !out)) return ARTALK_EINVAL;
    ConvArgs a{};
    a.x = (const float*)x; a.x_bstride = x_bstride; a.w = (const float*)w; a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.k = k;
    a.in_scale = (const float*)(uintptr_t)in_scale_addr; a.in_scale_ld = Cin;
    const ConvPlan p = plan_conv(a, precision);
    const int32_t v[] = {p.nt, p.va, p.vb, p.np, (int32_t)p.gx, (int32_t)p.gy, p.nsteps, p.cinp, p.kp};
    const int count = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < count; ++i) out[i] = v[i];
    return count;
}

int artalk_op_conv2d_ex(const float* x, int64_t x_bstride, const float* w, float* out, int B, int H, int W, int Cin, int Cout, int k,
                        const float* in_scale, const float* out_scale, float gain, const float* noise, int64_t noise_bstride,
                        const float* noise_weight, const float* bias, int lrelu, const float* sft_scale, const float* sft_shift,
                        const float* residual, int precision, void* stream) {
    if (!out || !conv_op_shape_ok(x, x_bstride, w, B, H, W, Cin, Cout, k, precision)) return ARTALK_EINVAL;
    if (noise && (!noise_weight || (noise_bstride != 0 && noise_bstride < (int64_t)H * W))) return ARTALK_EINVAL;
    if ((sft_scale == nullptr) != (sft_shift == nullptr)) return ARTALK_EINVAL;
    ConvArgs a{};
    a.x = x; a.x_bstride = x_bstride; a.w = w; a.out = out; a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.k = k;
    a.in_scale = in_scale; a.in_scale_ld = Cin; a.out_scale = out_scale; a.gain = gain; a.noise = noise; a.noise_bstride = noise_bstride; a.noise_w = noise_weight;
    a.bias = bias; a.lrelu = lrelu; a.sft_scale = sft_scale; a.sft_shift = sft_shift; a.res = residual;
    hipStream_t s = (hipStream_t)stream;
    if (precision == CONV_PRECISION_F32) {
        launch_conv(a, s);
        return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
    }
    // the packed weight lives for this call only: pack and conv run on the caller's stream, and the call waits for them before it frees
    DevBuf<uint16_t> packed;
    if (!packed.alloc(conv_packed_elems(Cin, Cout, k))) return ARTALK_EHIP;
    launch_conv_pack(w, packed.get(), Cin, Cout, k, s);
    launch_conv_bf16(a, packed.get(), precision, s);
    const bool ok = hipGetLastError() == hipSuccess;
    return hipStreamSynchronize(s) == hipSuccess && ok ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_conv2d(const float* x, int64_t x_bstride, const float* w, float* out, int B, int H, int W, int Cin, int Cout, int k,
                     const float* in_scale, const float* out_scale, float gain, const float* noise, int64_t noise_bstride,
                     const float* noise_weight, const float* bias, int lrelu, const float* sft_scale, const float* sft_shift,
                     const float* residual, void* stream) {
    return artalk_op_conv2d_ex(x, x_bstride, w, out, B, H, W, Cin, Cout, k, in_scale, out_scale, gain, noise, noise_bstride, noise_weight, bias,
                               lrelu, sft_scale, sft_shift, residual, CONV_PRECISION_F32, stream);
}

int artalk_op_resample2(const float* x, float* out, int B, int H, int W, int C, int up, void* stream) {
    if (!x || !out || B < 1 || H < 1 || W < 1 || C < 1) return ARTALK_EINVAL;
    if (!up && ((H | W) & 1)) return ARTALK_EINVAL;
    const long total = (long)B * (up ? 4L * H * W : (long)(H / 2) * (W / 2)) * C;
    ARTALK_LAUNCH(resample2_kernel, dim3(blocks256(total)), dim3(256), 0, (hipStream_t)stream, x, out, B, H, W, C, up);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// The style path and layout kernels alone, through the launchers SuRun uses (tests/test_styleunet_glue_gpu.py).  Beyond what the header
// names they refuse a size whose grid would not fit a launch.
static inline bool su_grid_ok(int64_t blocks) { return blocks <= INT_MAX; }

int artalk_op_su_linear(const float* x, const float* W, const float* bias_or_null, float* y, int B, int In, int Out, int lrelu, void* stream) {
    if (!x || !W || !y || B < 1 || In < 1 || Out < 1 || !su_grid_ok(((int64_t)B * Out + 3) / 4)) return ARTALK_EINVAL;
    launch_linear(x, W, bias_or_null, y, B, In, Out, lrelu, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_su_normstyle(const float* x, float* y, int B, int n, void* stream) {
    if (!x || !y || B < 1 || n < 1) return ARTALK_EINVAL;
    launch_normstyle(x, y, B, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_su_demod(const float* s, int64_t ld, const float* wsq, float* d, int B, int Cin, int Cout, void* stream) {
    if (!s || !wsq || !d || B < 1 || Cin < 1 || Cout < 1 || ld < Cin || !su_grid_ok(((int64_t)B * Cout + 3) / 4)) return ARTALK_EINVAL;
    launch_demod(s, (long)ld, wsq, d, B, Cin, Cout, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_su_add(const float* a, const float* b, float* out, int64_t n, void* stream) {
    if (!a || !b || !out || n < 1 || !su_grid_ok((n + 255) / 256)) return ARTALK_EINVAL;
    launch_add(a, b, out, (long)n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// B C HW as a product of three positive values that fits a launch (no overflow on the way)
static bool su_layout_ok(const void* x, const void* out, int B, int C, int64_t HW) {
    if (!x || !out || B < 1 || C < 1 || HW < 1) return false;
    const int64_t cap = (int64_t)INT_MAX * 256;
    return HW <= cap / B / C;
}

int artalk_op_su_to_nhwc(const float* x, float* out, int B, int C, int64_t HW, void* stream) {
    if (!su_layout_ok(x, out, B, C, HW)) return ARTALK_EINVAL;
    launch_to_nhwc(x, out, B, C, (long)HW, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_su_to_nchw(const float* x, float* out, int B, int C, int64_t HW, int sigmoid, void* stream) {
    if (!su_layout_ok(x, out, B, C, HW)) return ARTALK_EINVAL;
    launch_to_nchw(x, out, B, C, (long)HW, sigmoid, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

}  // extern "C"
