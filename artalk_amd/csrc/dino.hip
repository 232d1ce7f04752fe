// DINOBase of the GAGAvatar head's identity side, forward only, exact fp32, one image per call ("DINO features"): a
// stand-in for app/GAGAvatar/modules/dino_base.py - the ImageNet normalisation, the DINOv2 ViT (patch 14, LayerScale, no register
// tokens, pos_embed used as it is), the last four blocks' normed patch tokens, and the DPT-style head that fuses them into the feature
// plane [output_dim][8 g][8 g].  The second output is the normed FIRST PATCH token of the last block (what the reference's
// image_features[-1][:, 0] is once get_intermediate_layers has stripped the class token).
//
// The arithmetic runs on kernels the library already has:
//   launch_gemm (fp32 MFMA)    patch embedding (K = 588 zero-padded to 608), q|k|v, proj and fc2 with gate = LayerScale and residual, fc1
//                              with GELU(erf), the 1 x 1 projections, the k = s transposed convolutions, the stride-2 3 x 3 conv (split-K)
//   launch_layernorm           widths 128 / 512 / 768 / 1024; another width takes dino_layernorm_kernel below
//   launch_attention           fp32, read straight out of the fused q|k|v rows
//   launch_conv                every stride-1 conv of the head, with bias / ReLU / residual in its epilogue
// Around them the data movements below, all bandwidth-bound and small: one thread per output value or per 4 channels, no LDS, no atomics.
// A call enqueues on the caller's stream and never waits (unless timing is on).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "artalk_hip.h"
#include "common.h"
#include "device_mem.h"
#include "styleunet_conv.h"
#include "weight_store.h"

namespace artalk {

constexpr int DN_PATCH = 14, DN_PK = 3 * DN_PATCH * DN_PATCH, DN_PKP = 608;      // patch GEMM: K = 588, padded to a multiple of 32
constexpr int DN_HID = 256;                                                       // hidden width of the head
constexpr int DN_PROJ[4] = {256, 512, 1024, 1024};
constexpr int DN_SPLITK = 8;                                                      // the stride-2 conv's K = 9 * 1024
constexpr float DN_EPS = 1e-6f;

__host__ __device__ inline int dn_pad8(int c) { return (c + 7) & ~7; }
static inline unsigned dn_blocks(long n) { return (unsigned)((n + 255) / 256); }

struct DnNorm { float mean[3], std[3]; int on; };

// ---- antialiased bilinear resize (torch's F.interpolate(mode = "bilinear", align_corners = False, antialias = True)) ----
// The triangle filter of torch's _upsample_bilinear2d_aa: scale = in / out, support = max(scale, 1), centre = scale (i + 0.5), taps
// [max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), in)), weight max(0, 1 - |(j + 0.5 - centre) / max(scale, 1)|),
// normalised to sum 1.  Enlarging, it is plain bilinear.  The weights are worked out in double and rounded once; rows are summed
// horizontally first, then vertically, in float.
__device__ __forceinline__ void dn_aa_range(int i, int in, int out, int* lo, int* n, double* centre, double* invscale, double* total) {
    const double scale = (double)in / (double)out;
    const double support = scale >= 1.0 ? scale : 1.0;
    *invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
    *centre = scale * ((double)i + 0.5);
    int a = (int)(*centre - support + 0.5); if (a < 0) a = 0;
    int b = (int)(*centre + support + 0.5); if (b > in) b = in;
    *lo = a; *n = b - a;
    double t = 0.0;
    for (int j = 0; j < b - a; ++j) { const double w = 1.0 - fabs(((double)(j + a) - *centre + 0.5) * *invscale); t += w > 0.0 ? w : 0.0; }
    *total = t;
}
__device__ __forceinline__ float dn_aa_weight(int j, double centre, double invscale, double total) {
    const double w = 1.0 - fabs(((double)j - centre + 0.5) * invscale);
    return (float)((w > 0.0 ? w : 0.0) / total);
}
// x [C][Hi][Wi] -> out: value (c, oy, ox) at out[c * cs + (oy * Wo + ox) * ps] (NCHW: cs = Ho Wo, ps = 1; channels-last: cs = 1,
// ps = C).  nrm.on: (v - mean[c]) / std[c] is applied to the result (torchvision's Normalize).
__global__ __launch_bounds__(256) void dino_resize_aa_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int Hi, int Wi, int Ho, int Wo,
                                                             long cs, long ps, const DnNorm nrm) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)C * Ho * Wo) return;
    const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho), c = (int)(i / ((long)Wo * Ho));
    int x0, nx, y0, ny;
    double cx, ix, tx, cy, iy, ty;
    dn_aa_range(ox, Wi, Wo, &x0, &nx, &cx, &ix, &tx);
    dn_aa_range(oy, Hi, Ho, &y0, &ny, &cy, &iy, &ty);
    const float* xc = x + (long)c * Hi * Wi;
    float acc = 0.f;
    for (int jy = 0; jy < ny; ++jy) {
        const float* row = xc + (long)(y0 + jy) * Wi + x0;
        float h = 0.f;
        for (int jx = 0; jx < nx; ++jx) h += dn_aa_weight(x0 + jx, cx, ix, tx) * row[jx];
        acc += dn_aa_weight(y0 + jy, cy, iy, ty) * h;
    }
    if (nrm.on) acc = (acc - nrm.mean[c]) / nrm.std[c];
    out[(long)c * cs + ((long)oy * Wo + ox) * ps] = acc;
}

// out = (x - mean[c]) / std[c] over [3][n]
__global__ __launch_bounds__(256) void dino_normalize_kernel(const float* __restrict__ x, float* __restrict__ out, long n, const DnNorm nrm) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * n) return;
    const int c = (int)(i / n);
    out[i] = (x[i] - nrm.mean[c]) / nrm.std[c];
}

// img [3][14 g][14 g] -> col [g g][608]: row (py, px), column c 196 + ky 14 + kx (the flattening of the conv weight), zeros from 588 on
__global__ __launch_bounds__(256) void dino_im2col_kernel(const float* __restrict__ img, float* __restrict__ col, int g) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g * g * DN_PKP) return;
    const int k = (int)(i % DN_PKP);
    const int p = (int)(i / DN_PKP), py = p / g, px = p - py * g;
    float v = 0.f;
    if (k < DN_PK) {
        const int c = k / (DN_PATCH * DN_PATCH), r = k - c * DN_PATCH * DN_PATCH, ky = r / DN_PATCH, kx = r - ky * DN_PATCH;
        const long S = (long)DN_PATCH * g;
        v = img[((long)c * S + py * DN_PATCH + ky) * S + px * DN_PATCH + kx];
    }
    col[i] = v;
}

// X[t] = (t == 0 ? cls : patch[t - 1]) + pos[t], T rows of D (D % 4 == 0, 16-byte aligned rows)
__global__ __launch_bounds__(256) void dino_tokens_kernel(const float* __restrict__ patch, const float* __restrict__ cls, const float* __restrict__ pos,
                                                          float* __restrict__ X, int T, int D) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= (long)T * D) return;
    const int t = (int)(i / D), d = (int)(i - (long)t * D);
    const f32x4 a = *reinterpret_cast<const f32x4*>(t ? patch + (long)(t - 1) * D + d : cls + d);
    const f32x4 b = *reinterpret_cast<const f32x4*>(pos + i);
    *reinterpret_cast<f32x4*>(X + i) = a + b;
}

// LayerNorm with affine for a width launch_layernorm has no kernel for: one wavefront per row, the row read three times (it is in L1)
__global__ __launch_bounds__(256) void dino_layernorm_kernel(const float* __restrict__ X, float* __restrict__ Y, const float* __restrict__ w,
                                                             const float* __restrict__ b, int M, int D, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* x = X + (long)row * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += x[c];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) { const float d = x[c] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
    float* y = Y + (long)row * D;
    for (int c = lane; c < D; c += 64) y[c] = (x[c] - mean) * rstd * w[c] + b[c];
}

// tap [1 + G][D] -> out [G][D]: the class token stripped.  (The object reads the rows in place; this is the stand-alone form.)
__global__ __launch_bounds__(256) void dino_strip_kernel(const float* __restrict__ tap, float* __restrict__ out, long n, int D) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    *reinterpret_cast<f32x4*>(out + i) = *reinterpret_cast<const f32x4*>(tap + D + i);
}

// The k = s transposed conv from its GEMM: r [g g][s s Co] with column (dy s + dx) Co + co -> out [s g][s g][Co], + bias (Co % 4 == 0)
__global__ __launch_bounds__(256) void dino_shuffle_kernel(const float* __restrict__ r, const float* __restrict__ bias, float* __restrict__ out, int g, int s,
                                                           int Co) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    const int W = s * g;
    if (i >= (long)W * W * Co) return;
    const int co = (int)(i % Co);
    const long p = i / Co;
    const int ox = (int)(p % W), oy = (int)(p / W);
    const int y = oy / s, dy = oy - y * s, x = ox / s, dx = ox - x * s;
    const f32x4 v = *reinterpret_cast<const f32x4*>(r + ((long)y * g + x) * ((long)s * s * Co) + (long)(dy * s + dx) * Co + co);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + co);
    *reinterpret_cast<f32x4*>(out + i) = v + bv;
}

// x [g][g][C] -> col [Ho Ho][9 C], Ho = (g - 1) / 2 + 1: column (ky 3 + kx) C + c holds x[2 oy + ky - 1][2 ox + kx - 1][c], zero outside
__global__ __launch_bounds__(256) void dino_gather_s2_kernel(const float* __restrict__ x, float* __restrict__ col, int g, int C) {
    const int Ho = (g - 1) / 2 + 1;
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= (long)Ho * Ho * 9 * C) return;
    const int c = (int)(i % C);
    long p = i / C;
    const int tap = (int)(p % 9); p /= 9;
    const int ox = (int)(p % Ho), oy = (int)(p / Ho);
    const int yy = 2 * oy + tap / 3 - 1, xx = 2 * ox + tap % 3 - 1;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (yy >= 0 && yy < g && xx >= 0 && xx < g) v = *reinterpret_cast<const f32x4*>(x + ((long)yy * g + xx) * C + c);
    *reinterpret_cast<f32x4*>(col + i) = v;
}

// img [n][3], feat [n][C] -> out [n][W], W = dn_pad8(3 + C): the image, then the features, then zeros
__global__ __launch_bounds__(256) void dino_concat_kernel(const float* __restrict__ img, const float* __restrict__ feat, float* __restrict__ out, long n, int C,
                                                          int W) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * W) return;
    const int c = (int)(i % W);
    const long p = i / W;
    out[i] = c < 3 ? img[p * 3 + c] : c < 3 + C ? feat[p * C + c - 3] : 0.f;
}

// x [Hi][Wi][C] -> out [Ho][Wo][C], bilinear with align_corners = True: source = i (in - 1) / (out - 1) (double, the fraction rounded
// once), out = l0y (l0x a + l1x b) + l1y (l0x c + l1x d) in torch's order.  C % 4 == 0.
__global__ __launch_bounds__(256) void dino_resize_ac_kernel(const float* __restrict__ x, float* __restrict__ out, int Hi, int Wi, int Ho, int Wo, int C) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= (long)Ho * Wo * C) return;
    const int c = (int)(i % C);
    const long p = i / C;
    const int ox = (int)(p % Wo), oy = (int)(p / Wo);
    const double sy = Ho > 1 ? (double)(Hi - 1) / (double)(Ho - 1) * oy : 0.0, sx = Wo > 1 ? (double)(Wi - 1) / (double)(Wo - 1) * ox : 0.0;
    int y0 = (int)sy, x0 = (int)sx;
    if (y0 > Hi - 1) y0 = Hi - 1;
    if (x0 > Wi - 1) x0 = Wi - 1;
    const int y1 = y0 < Hi - 1 ? y0 + 1 : y0, x1 = x0 < Wi - 1 ? x0 + 1 : x0;
    const float ly1 = (float)(sy - y0), lx1 = (float)(sx - x0), ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + ((long)y0 * Wi + x0) * C + c), b = *reinterpret_cast<const f32x4*>(x + ((long)y0 * Wi + x1) * C + c);
    const f32x4 d = *reinterpret_cast<const f32x4*>(x + ((long)y1 * Wi + x0) * C + c), e = *reinterpret_cast<const f32x4*>(x + ((long)y1 * Wi + x1) * C + c);
    *reinterpret_cast<f32x4*>(out + i) = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * d + lx1 * e);
}

// sum = a + b (b null: a), relu = max(sum, 0); sum_out may be null, relu_out may be a or b.  n % 4 == 0.
__global__ __launch_bounds__(256) void dino_add_relu_kernel(const float* a, const float* b, float* sum_out, float* relu_out, long n) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    f32x4 v = *reinterpret_cast<const f32x4*>(a + i);
    if (b) v += *reinterpret_cast<const f32x4*>(b + i);
    if (sum_out) *reinterpret_cast<f32x4*>(sum_out + i) = v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
    *reinterpret_cast<f32x4*>(relu_out + i) = v;
}

// x [n][C] -> out [C][n] through a 32 x 32 LDS tile (both sides contiguous); block (0, 0) also copies tok [D] -> f1 [D] (tok null: no)
__global__ __launch_bounds__(256) void dino_output_kernel(const float* __restrict__ x, float* __restrict__ out, long n, int C, const float* __restrict__ tok,
                                                          float* __restrict__ f1, int D) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long p0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    for (int j = ty; j < 32; j += 8) {
        const long p = p0 + j;
        const int c = c0 + tx;
        tile[j][tx] = (p < n && c < C) ? x[p * C + c] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j;
        const long p = p0 + tx;
        if (p < n && c < C) out[(long)c * n + p] = tile[tx][j];
    }
    if (tok && blockIdx.x == 0 && blockIdx.y == 0)
        for (int d = threadIdx.x; d < D; d += 256) f1[d] = tok[d];
}

static DnNorm dn_norm(bool on) {
    DnNorm n{};
    const float m[3] = {0.485f, 0.456f, 0.406f}, s[3] = {0.229f, 0.224f, 0.225f};
    for (int c = 0; c < 3; ++c) { n.mean[c] = m[c]; n.std[c] = s[c]; }
    n.on = on ? 1 : 0;
    return n;
}

static void dn_resize_aa(const float* x, float* out, int C, int Hi, int Wi, int Ho, int Wo, bool channels_last, bool normalize, hipStream_t s) {
    const long cs = channels_last ? 1 : (long)Ho * Wo, ps = channels_last ? C : 1;
    ARTALK_LAUNCH(dino_resize_aa_kernel, dim3(dn_blocks((long)C * Ho * Wo)), dim3(256), 0, s, x, out, C, Hi, Wi, Ho, Wo, cs, ps, dn_norm(normalize));
}
static bool dn_ln_native(int D) { return D == 128 || D == 512 || D == 768 || D == 1024; }
static void dn_layernorm(const float* X, float* Y, const float* w, const float* b, int M, int D, hipStream_t s) {
    if (dn_ln_native(D)) {
        LnArgs a;
        a.X = X; a.ldx = D; a.Y = Y; a.ldy = D; a.w = w; a.b = b; a.M = M; a.D = D; a.eps = DN_EPS;
        launch_layernorm(a, s);
    } else {
        ARTALK_LAUNCH(dino_layernorm_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, X, Y, w, b, M, D, DN_EPS);
    }
}

}  // namespace artalk

using namespace artalk;

namespace {

struct DnLin { const float* w = nullptr; const float* b = nullptr; };
struct DnBlock { const float *n1w, *n1b, *n2w, *n2b, *ls1, *ls2; DnLin qkv, proj, fc1, fc2; };
struct DnConv { const float* w = nullptr; const float* b = nullptr; int cin = 0, cinp = 0, cout = 0, k = 1; };
struct DnFuse { DnConv u1c1, u1c2, u2c1, u2c2, out; };

enum { DN_ST_GEMM = 0, DN_ST_ATTN = 1, DN_ST_CONV = 2, DN_ST_REST = 3, DN_STAGES = 4 };

}  // namespace

struct artalk_dino {
    int device = 0, D = 0, depth = 0, heads = 0, HD = 0, g = 0, od = 0;
    bool finalized = false, timing = false;
    WeightStore store;
    DevBuf<float> ws, stage;
    int64_t ws_floats = 0;
    const float *cls = nullptr, *pos = nullptr, *normw = nullptr, *normb = nullptr;
    DnLin patch;
    std::vector<DnBlock> blocks;
    DnLin projects[4], up[2], down;       // up: the two transposed convs (w as [s s Co][Ci]); down: the stride-2 conv (w as [Co][9 Ci])
    DnConv rn[4], outc;
    DnFuse fuse[4];
    StageTimer timer;
    CallTimer call;      // total_ms only: the stages are the StageTimer's
    double stage_ms[DN_STAGES] = {0, 0, 0, 0};
    std::string err;
};

static thread_local std::string g_dn_error;

namespace {

int dn_fail(artalk_dino* d, int rc, const std::string& msg) { d->err = msg; return rc; }

void dn_slot(artalk_dino* d, const std::string& name, std::vector<int64_t> shape, bool optional = false) { d->store.declare(name, std::move(shape), optional); }
void dn_wb(artalk_dino* d, const std::string& name, std::vector<int64_t> wshape, bool bias = true) {
    const int64_t cout = wshape[0];
    dn_slot(d, name + ".weight", std::move(wshape));
    if (bias) dn_slot(d, name + ".bias", {cout});
}

// keys in the order of the reference module's state_dict()
void dn_manifest(artalk_dino* d) {
    const int64_t D = d->D, G = (int64_t)d->g * d->g, H = DN_HID;
    const std::string m = "dino_model.";
    dn_slot(d, m + "cls_token", {1, 1, D});
    dn_slot(d, m + "pos_embed", {1, 1 + G, D});
    dn_slot(d, m + "mask_token", {1, D}, true);
    dn_wb(d, m + "patch_embed.proj", {D, 3, DN_PATCH, DN_PATCH});
    for (int i = 0; i < d->depth; ++i) {
        const std::string b = m + "blocks." + std::to_string(i) + ".";
        dn_slot(d, b + "norm1.weight", {D}); dn_slot(d, b + "norm1.bias", {D});
        dn_wb(d, b + "attn.qkv", {3 * D, D});
        dn_wb(d, b + "attn.proj", {D, D});
        dn_slot(d, b + "ls1.gamma", {D});
        dn_slot(d, b + "norm2.weight", {D}); dn_slot(d, b + "norm2.bias", {D});
        dn_wb(d, b + "mlp.fc1", {4 * D, D});
        dn_wb(d, b + "mlp.fc2", {D, 4 * D});
        dn_slot(d, b + "ls2.gamma", {D});
    }
    dn_slot(d, m + "norm.weight", {D}); dn_slot(d, m + "norm.bias", {D});
    for (int i = 0; i < 4; ++i) dn_wb(d, "projects." + std::to_string(i), {DN_PROJ[i], D, 1, 1});
    dn_wb(d, "resize_layers.0", {DN_PROJ[0], DN_PROJ[0], 4, 4});
    dn_wb(d, "resize_layers.1", {DN_PROJ[1], DN_PROJ[1], 2, 2});
    dn_wb(d, "resize_layers.3", {DN_PROJ[3], DN_PROJ[3], 3, 3});
    for (int i = 0; i < 4; ++i) dn_wb(d, "layer_rn." + std::to_string(i), {H, DN_PROJ[i] + 3, 3, 3}, false);
    for (int i = 0; i < 4; ++i) {
        const std::string r = "refinenet." + std::to_string(i) + ".";
        dn_wb(d, r + "out_conv", {H, H, 1, 1});
        for (int u = 1; u <= 2; ++u)
            for (int c = 1; c <= 2; ++c) dn_wb(d, r + "resConfUnit" + std::to_string(u) + ".conv" + std::to_string(c), {H, H, 3, 3});
    }
    dn_wb(d, "output_conv", {d->od, H, 3, 3});
}

inline int dn_h3(int g) { return (g - 1) / 2 + 1; }

// The workspace, in floats, every block 16-byte aligned.
struct DnWs : WsLayout {
    int64_t img, col, patch, X, Y, qkv, O, hid, tap[4], proj, gemm, part, feat, imgr, cat, rn[4], A, B, C, out;
    explicit DnWs(const artalk_dino* d) {
        const int64_t g = d->g, G = g * g, T = G + 1, D = d->D, S = DN_PATCH * g, P = 8 * g, h3 = dn_h3(d->g);
        const int64_t hw[4] = {16 * G, 4 * G, G, h3 * h3};
        img = take(3 * S * S); col = take(G * DN_PKP); patch = take(G * D);
        X = take(T * D); Y = take(T * D); qkv = take(T * 3 * D); O = take(T * D); hid = take(T * 4 * D);
        for (int i = 0; i < 4; ++i) tap[i] = take(T * D);
        proj = take(G * 1024);
        int64_t gm = G * 16 * DN_PROJ[0];
        if (G * 4 * DN_PROJ[1] > gm) gm = G * 4 * DN_PROJ[1];
        if (hw[3] * 9 * DN_PROJ[3] > gm) gm = hw[3] * 9 * DN_PROJ[3];
        gemm = take(gm);
        part = take((int64_t)DN_SPLITK * hw[3] * DN_PROJ[3]);
        int64_t fm = 0, cm = 0;
        for (int i = 0; i < 4; ++i) {
            if (hw[i] * DN_PROJ[i] > fm) fm = hw[i] * DN_PROJ[i];
            if (hw[i] * dn_pad8(DN_PROJ[i] + 3) > cm) cm = hw[i] * dn_pad8(DN_PROJ[i] + 3);
        }
        feat = take(fm); imgr = take(hw[0] * 3); cat = take(cm);
        for (int i = 0; i < 4; ++i) rn[i] = take(hw[i] * DN_HID);
        A = take(P * P * DN_HID); B = take(P * P * DN_HID); C = take(P * P * DN_HID);
        out = take(P * P * d->od);
    }
};

struct DnRun {
    artalk_dino* d; hipStream_t s;
    void mark(int stage) { d->timer.mark(stage); }
    void gemm(const float* A, long lda, const DnLin& l, float* C, int M, int N, int K, int act = ACT_NONE, const float* gate = nullptr, const float* R = nullptr,
              bool bias = true) {
        GemmArgs a;
        a.A = A; a.lda = lda; a.W = l.w; a.ldw = K; a.bias = bias ? l.b : nullptr; a.C = C; a.ldc = N; a.M = M; a.N = N; a.K = K; a.act = act; a.exact = 1;
        a.ksum_blocks = 1;      // fc2 sums over K = 4 dim: one chain that long is outside the head's allowance ("DINO features")
        if (gate) { a.gate = gate; a.ldg = 0; }
        if (R) { a.R = R; a.ldr = N; }
        launch_gemm(a, s);
    }
    void conv(const DnConv& l, const float* x, float* out, int H, int relu, const float* res) {
        ConvArgs a{};
        a.x = x; a.x_bstride = (long)H * H * l.cinp; a.w = l.w; a.out = out; a.B = 1; a.H = H; a.W = H; a.Cin = l.cinp; a.Cout = l.cout; a.k = l.k;
        a.gain = 1.f; a.bias = l.b; a.relu = relu; a.res = res;
        launch_conv(a, s);
    }
    void relu(const float* a, const float* b, float* sum, float* out, long n) {
        ARTALK_LAUNCH(dino_add_relu_kernel, dim3(dn_blocks(n / 4)), dim3(256), 0, s, a, b, sum, out, n);
    }
    // ResidualConvUnit: conv2(relu(conv1(relu(x)))) + x with relu(x) already in r; t is scratch
    void rcu(const DnConv& c1, const DnConv& c2, const float* x, const float* r, float* t, float* out, int H) {
        conv(c1, r, t, H, 1, nullptr);
        conv(c2, t, out, H, 0, x);
    }
    void run(const float* image, float* f0, float* f1) {
        const DnWs w(d);
        float* base = d->ws.get();
        const int g = d->g, G = g * g, T = G + 1, D = d->D, S = DN_PATCH * g, P = 8 * g;
        const int hs[5] = {4 * g, 2 * g, g, dn_h3(g), 0};
        mark(-1);
        // ---- backbone ----
        ARTALK_LAUNCH(dino_normalize_kernel, dim3(dn_blocks(3L * S * S)), dim3(256), 0, s, image, base + w.img, (long)S * S, dn_norm(true));
        ARTALK_LAUNCH(dino_im2col_kernel, dim3(dn_blocks((long)G * DN_PKP)), dim3(256), 0, s, base + w.img, base + w.col, g);
        mark(DN_ST_REST);
        gemm(base + w.col, DN_PKP, d->patch, base + w.patch, G, D, DN_PKP);
        mark(DN_ST_GEMM);
        ARTALK_LAUNCH(dino_tokens_kernel, dim3(dn_blocks((long)T * D / 4)), dim3(256), 0, s, base + w.patch, d->cls, d->pos, base + w.X, T, D);
        float *X = base + w.X, *Y = base + w.Y;
        for (int i = 0; i < d->depth; ++i) {
            const DnBlock& b = d->blocks[i];
            dn_layernorm(X, Y, b.n1w, b.n1b, T, D, s);
            mark(DN_ST_REST);
            gemm(Y, D, b.qkv, base + w.qkv, T, 3 * D, D);
            mark(DN_ST_GEMM);
            AttnArgs a;
            a.Q = base + w.qkv; a.K = base + w.qkv + D; a.V = base + w.qkv + 2 * D; a.ldq = a.ldk = a.ldv = 3L * D;
            a.O = base + w.O; a.ldo = D; a.B = 1; a.H = d->heads; a.HD = d->HD; a.Lq = T; a.Lk = T; a.scale = 1.0f / sqrtf((float)d->HD);
            launch_attention(a, s);
            mark(DN_ST_ATTN);
            gemm(base + w.O, D, b.proj, X, T, D, D, ACT_NONE, b.ls1, X);
            mark(DN_ST_GEMM);
            dn_layernorm(X, Y, b.n2w, b.n2b, T, D, s);
            mark(DN_ST_REST);
            gemm(Y, D, b.fc1, base + w.hid, T, 4 * D, D, ACT_GELU_ERF);
            gemm(base + w.hid, 4L * D, b.fc2, X, T, D, 4 * D, ACT_NONE, b.ls2, X);
            mark(DN_ST_GEMM);
            const int t = i - (d->depth - 4);
            if (t >= 0) dn_layernorm(X, base + w.tap[t], d->normw, d->normb, T, D, s);
        }
        mark(DN_ST_REST);
        // ---- head: the four levels ----
        for (int i = 0; i < 4; ++i) {
            const int Ci = DN_PROJ[i], H = hs[i];
            const float* tap = base + w.tap[i] + D;      // the class token stripped: [g][g][D] in place
            float* feat = base + w.feat;
            if (i == 2) {
                gemm(tap, D, d->projects[i], feat, G, Ci, D);
                mark(DN_ST_GEMM);
            } else {
                gemm(tap, D, d->projects[i], base + w.proj, G, Ci, D);
                if (i < 2) {
                    const int sc = i == 0 ? 4 : 2;
                    gemm(base + w.proj, Ci, d->up[i], base + w.gemm, G, sc * sc * Ci, Ci, ACT_NONE, nullptr, nullptr, false);
                    mark(DN_ST_GEMM);
                    ARTALK_LAUNCH(dino_shuffle_kernel, dim3(dn_blocks((long)H * H * Ci / 4)), dim3(256), 0, s, base + w.gemm, d->up[i].b, feat, g, sc, Ci);
                    mark(DN_ST_REST);
                } else {
                    mark(DN_ST_GEMM);
                    ARTALK_LAUNCH(dino_gather_s2_kernel, dim3(dn_blocks((long)H * H * 9 * Ci / 4)), dim3(256), 0, s, base + w.proj, base + w.gemm, g, Ci);
                    mark(DN_ST_REST);
                    GemmArgs a;      // K = 9216: split over DN_SPLITK workgroups whose partial sums add in a fixed order
                    a.A = base + w.gemm; a.lda = 9L * Ci; a.W = d->down.w; a.ldw = 9L * Ci; a.bias = d->down.b; a.C = feat; a.ldc = Ci;
                    a.M = H * H; a.N = Ci; a.K = 9 * Ci; a.exact = 1; a.splitk = DN_SPLITK; a.partial = base + w.part;
                    launch_gemm(a, s);
                    launch_splitk_reduce(a, s);
                    mark(DN_ST_GEMM);
                }
            }
            dn_resize_aa(base + w.img, base + w.imgr, 3, S, S, H, H, true, false, s);
            const int W = dn_pad8(Ci + 3);
            ARTALK_LAUNCH(dino_concat_kernel, dim3(dn_blocks((long)H * H * W)), dim3(256), 0, s, base + w.imgr, feat, base + w.cat, (long)H * H, Ci, W);
            mark(DN_ST_REST);
            conv(d->rn[i], base + w.cat, base + w.rn[i], H, 0, nullptr);
            mark(DN_ST_CONV);
        }
        // ---- head: the four fusion blocks, coarse to fine ----
        float *A = base + w.A, *B = base + w.B, *C = base + w.C;
        for (int j = 0; j < 4; ++j) {
            const int l = 3 - j, H = hs[l], Hn = j < 3 ? hs[l - 1] : 2 * H;
            const long n = (long)H * H * DN_HID;
            const DnFuse& f = d->fuse[j];
            const float* rn = base + w.rn[l];
            const float* x = rn;      // what resConfUnit2 takes
            if (j == 0) {
                relu(rn, nullptr, nullptr, A, n);
                mark(DN_ST_REST);
                rcu(f.u2c1, f.u2c2, x, A, B, A, H);
            } else {
                relu(rn, nullptr, nullptr, A, n);
                mark(DN_ST_REST);
                rcu(f.u1c1, f.u1c2, rn, A, B, A, H);      // A = resConfUnit1(rn)
                mark(DN_ST_CONV);
                relu(C, A, B, A, n);                      // B = path + A, A = relu(B)
                mark(DN_ST_REST);
                rcu(f.u2c1, f.u2c2, B, A, C, A, H);
            }
            mark(DN_ST_CONV);
            ARTALK_LAUNCH(dino_resize_ac_kernel, dim3(dn_blocks((long)Hn * Hn * DN_HID / 4)), dim3(256), 0, s, A, B, H, H, Hn, Hn, DN_HID);
            mark(DN_ST_REST);
            conv(f.out, B, C, Hn, 0, nullptr);
            mark(DN_ST_CONV);
        }
        conv(d->outc, C, base + w.out, P, 0, nullptr);
        mark(DN_ST_CONV);
        const long PP = (long)P * P;
        ARTALK_LAUNCH(dino_output_kernel, dim3((unsigned)((PP + 31) / 32), (unsigned)((d->od + 31) / 32)), dim3(256), 0, s, base + w.out, f0, PP, d->od,
                      base + w.tap[3] + D, f1, D);
        mark(DN_ST_REST);
    }
};

}  // namespace

extern "C" {

const char* artalk_dino_last_error(const artalk_dino* d) { return d ? d->err.c_str() : g_dn_error.c_str(); }

void artalk_dino_destroy(artalk_dino* d) {
    if (!d) return;
    if (d->store.on_device() || d->stage.capacity()) {      // (else nothing was ever taken from the device)
        (void)hipSetDevice(d->device);
        (void)hipDeviceSynchronize();
    }
    delete d;
}

int artalk_dino_create(int device_id, int vit_dim, int depth, int heads, int grid, int output_dim, artalk_dino** out) {
    if (!out) { g_dn_error = "out is NULL"; return ARTALK_EINVAL; }
    *out = nullptr;
    if (device_id < 0) { g_dn_error = "device_id must not be negative"; return ARTALK_EINVAL; }
    if (vit_dim < 32 || vit_dim > 4096 || vit_dim % 32) { g_dn_error = "vit_dim must be a multiple of 32 in 32..4096"; return ARTALK_EINVAL; }
    if (depth < 4 || depth > 64) { g_dn_error = "depth must be in 4..64 (the head taps the last four blocks)"; return ARTALK_EINVAL; }
    if (heads < 1 || vit_dim % heads || (vit_dim / heads != 64 && vit_dim / heads != 32)) {
        g_dn_error = "the head width vit_dim / heads must be 64 or 32";
        return ARTALK_EINVAL;
    }
    if (grid < 2 || grid > 64) { g_dn_error = "grid must be in 2..64 patches a side"; return ARTALK_EINVAL; }
    if (output_dim < 1 || output_dim > 1024) { g_dn_error = "output_dim must be in 1..1024"; return ARTALK_EINVAL; }
    artalk_dino* d = new artalk_dino();
    d->device = device_id; d->D = vit_dim; d->depth = depth; d->heads = heads; d->HD = vit_dim / heads; d->g = grid; d->od = output_dim;
    dn_manifest(d);
    d->ws_floats = DnWs(d).off;
    *out = d;
    return ARTALK_OK;
}

int artalk_dino_set_tensor(artalk_dino* d, const char* key, const void* host_ptr, int ndim, const int64_t* shape) {
    if (!d) { g_dn_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (!key || !host_ptr || !shape) return dn_fail(d, ARTALK_EINVAL, "key, host_ptr and shape must not be NULL");
    if (d->finalized) return dn_fail(d, ARTALK_ESTATE, "weights are final after artalk_dino_finalize; create a new handle");
    const int rc = d->store.set(key, host_ptr, ndim, shape, &d->err);
    if (rc == ARTALK_EINVAL && std::string(key) == "dino_model.pos_embed" && ndim == 3)      // a wrong shape: say which grid it is for
        d->err = "size mismatch for dino_model.pos_embed: it holds " + std::to_string(shape[1]) + " positions, a grid of " + std::to_string(d->g) + " x " +
                 std::to_string(d->g) + " takes " + std::to_string(d->g * d->g + 1) + " (position embeddings are not interpolated)";
    return rc;
}

int artalk_dino_finalize(artalk_dino* d) {
    if (!d) { g_dn_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (d->finalized) return dn_fail(d, ARTALK_ESTATE, "artalk_dino_finalize was already called");
    if (d->store.missing(&d->err)) return ARTALK_EMISSING;
    if (hipSetDevice(d->device) != hipSuccess) return dn_fail(d, ARTALK_EHIP, "hipSetDevice failed");
    WeightStore& st = d->store;
    auto lin = [&](const std::string& n) { DnLin l; l.w = st.upload(n + ".weight"); l.b = st.upload(n + ".bias"); return l; };
    // the concat's image channels come first in the reference too: its input channels keep their rows
    auto conv = [&](const std::string& n, int cin, int cout, int k, bool bias) {
        DnConv l; l.cin = cin; l.cinp = dn_pad8(cin); l.cout = cout; l.k = k;
        l.w = st.upload(pack_conv_weight(st.host(n + ".weight"), cout, cin, l.cinp, k));
        l.b = bias ? st.upload(n + ".bias") : nullptr;
        return l;
    };
    const int D = d->D;
    const std::string m = "dino_model.";
    d->cls = st.upload(m + "cls_token");
    d->pos = st.upload(m + "pos_embed");
    {      // [D][588] -> [D][608]
        const std::vector<float>& w = st.host(m + "patch_embed.proj.weight");
        std::vector<float> t((size_t)D * DN_PKP, 0.f);
        for (int o = 0; o < D; ++o)
            for (int k = 0; k < DN_PK; ++k) t[(size_t)o * DN_PKP + k] = w[(size_t)o * DN_PK + k];
        d->patch.w = st.upload(t);
        d->patch.b = st.upload(m + "patch_embed.proj.bias");
    }
    d->blocks.resize(d->depth);
    for (int i = 0; i < d->depth; ++i) {
        const std::string b = m + "blocks." + std::to_string(i) + ".";
        DnBlock& k = d->blocks[i];
        k.n1w = st.upload(b + "norm1.weight"); k.n1b = st.upload(b + "norm1.bias"); k.n2w = st.upload(b + "norm2.weight"); k.n2b = st.upload(b + "norm2.bias");
        k.ls1 = st.upload(b + "ls1.gamma"); k.ls2 = st.upload(b + "ls2.gamma");
        k.qkv = lin(b + "attn.qkv"); k.proj = lin(b + "attn.proj"); k.fc1 = lin(b + "mlp.fc1"); k.fc2 = lin(b + "mlp.fc2");
    }
    d->normw = st.upload(m + "norm.weight"); d->normb = st.upload(m + "norm.bias");
    for (int i = 0; i < 4; ++i) d->projects[i] = lin("projects." + std::to_string(i));      // [Ci][D][1][1] is [Ci][D]
    for (int i = 0; i < 2; ++i) {      // ConvTranspose2d weight [Ci][Co][s][s] -> [(dy s + dx) Co + co][ci]
        const int C = DN_PROJ[i], sc = i == 0 ? 4 : 2, ss = sc * sc;
        const std::vector<float>& w = st.host("resize_layers." + std::to_string(i) + ".weight");
        std::vector<float> t((size_t)ss * C * C);
        for (int ci = 0; ci < C; ++ci)
            for (int co = 0; co < C; ++co)
                for (int q = 0; q < ss; ++q) t[((size_t)q * C + co) * C + ci] = w[((size_t)ci * C + co) * ss + q];
        d->up[i].w = st.upload(t);
        d->up[i].b = st.upload("resize_layers." + std::to_string(i) + ".bias");
    }
    {      // Conv2d weight [Co][Ci][3][3] -> [co][(ky 3 + kx) Ci + ci]
        const int C = DN_PROJ[3];
        const std::vector<float>& w = st.host("resize_layers.3.weight");
        std::vector<float> t((size_t)C * 9 * C);
        for (int co = 0; co < C; ++co)
            for (int ci = 0; ci < C; ++ci)
                for (int q = 0; q < 9; ++q) t[((size_t)co * 9 + q) * C + ci] = w[((size_t)co * C + ci) * 9 + q];
        d->down.w = st.upload(t);
        d->down.b = st.upload("resize_layers.3.bias");
    }
    for (int i = 0; i < 4; ++i) d->rn[i] = conv("layer_rn." + std::to_string(i), DN_PROJ[i] + 3, DN_HID, 3, false);
    for (int i = 0; i < 4; ++i) {
        const std::string r = "refinenet." + std::to_string(i) + ".";
        DnFuse& f = d->fuse[i];
        f.out = conv(r + "out_conv", DN_HID, DN_HID, 1, true);
        if (i > 0) {      // refinenet.0.resConfUnit1 is in the dict and never runs
            f.u1c1 = conv(r + "resConfUnit1.conv1", DN_HID, DN_HID, 3, true);
            f.u1c2 = conv(r + "resConfUnit1.conv2", DN_HID, DN_HID, 3, true);
        }
        f.u2c1 = conv(r + "resConfUnit2.conv1", DN_HID, DN_HID, 3, true);
        f.u2c2 = conv(r + "resConfUnit2.conv2", DN_HID, DN_HID, 3, true);
    }
    d->outc = conv("output_conv", DN_HID, d->od, 3, true);
    if (st.ok() && !d->ws.alloc((size_t)d->ws_floats))
        return dn_fail(d, ARTALK_EHIP, "hipMalloc of the workspace failed (" + std::to_string(d->ws_floats * 4) + " bytes)");
    if (!st.ok() || hipDeviceSynchronize() != hipSuccess) return dn_fail(d, ARTALK_EHIP, "uploading the weights failed");
    st.release_host();
    d->finalized = true;
    return ARTALK_OK;
}

int artalk_dino_dims(const artalk_dino* d, int* vit_dim, int* depth, int* heads, int* grid, int* output_dim, int* finalized) {
    if (!d) { g_dn_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (vit_dim) *vit_dim = d->D;
    if (depth) *depth = d->depth;
    if (heads) *heads = d->heads;
    if (grid) *grid = d->g;
    if (output_dim) *output_dim = d->od;
    if (finalized) *finalized = d->finalized ? 1 : 0;
    return d->device;
}

int artalk_dino_set_timing(artalk_dino* d, int enable) {
    if (!d) { g_dn_error = "handle is NULL"; return ARTALK_EINVAL; }
    d->timing = enable != 0;
    return ARTALK_OK;
}

int artalk_dino_get_timing(const artalk_dino* d, double* stage_ms, double* total_ms) {
    if (!d) { g_dn_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (stage_ms) for (int i = 0; i < DN_STAGES; ++i) stage_ms[i] = d->stage_ms[i];
    if (total_ms) *total_ms = d->call.total_ms();
    return ARTALK_OK;
}

int artalk_dino_prepare_image(artalk_dino* d, const float* image, int height, int width, float* out_dev, void* stream) {
    if (!d) { g_dn_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (!image || !out_dev) return dn_fail(d, ARTALK_EINVAL, "image and out must not be NULL");
    if (height < 1 || width < 1 || height > 16384 || width > 16384) return dn_fail(d, ARTALK_EINVAL, "height and width must be in 1..16384");
    if (hipSetDevice(d->device) != hipSuccess) return dn_fail(d, ARTALK_EHIP, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)3 * height * width;
    if (!d->stage.grow(n, 0, 1, s)) return dn_fail(d, ARTALK_EHIP, "hipMalloc of the image staging block failed");
    hipPointerAttribute_t at{};
    const bool on_device = hipPointerGetAttributes(&at, image) == hipSuccess && at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();      // (plain host memory may be reported as an error: it is none)
    // a host image has been read when the call returns: the caller may free it at once
    if (hipMemcpyAsync(d->stage.get(), image, n * sizeof(float), hipMemcpyDefault, s) != hipSuccess || (!on_device && hipStreamSynchronize(s) != hipSuccess)) {
        (void)hipGetLastError();
        return dn_fail(d, ARTALK_EHIP, "copying the image failed");
    }
    const int S = DN_PATCH * d->g;
    dn_resize_aa(d->stage.get(), out_dev, 3, height, width, S, S, false, false, s);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : dn_fail(d, ARTALK_EHIP, "kernel launch failed");
}

int artalk_dino_forward(artalk_dino* d, const float* image_dev, int height, int width, float* feature0_dev, float* feature1_dev, void* stream) {
    if (!d) { g_dn_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (!image_dev || !feature0_dev || !feature1_dev) return dn_fail(d, ARTALK_EINVAL, "image, feature0 and feature1 must not be NULL");
    const int S = DN_PATCH * d->g;
    if (height != width) return dn_fail(d, ARTALK_EINVAL, "the image must be square, got " + std::to_string(height) + " x " + std::to_string(width));
    if (height != S)
        return dn_fail(d, ARTALK_EINVAL, "the image must be " + std::to_string(S) + " x " + std::to_string(S) + " (14 x grid; position embeddings are not interpolated), got " +
                                             std::to_string(height) + " x " + std::to_string(width));
    if (!d->finalized) return dn_fail(d, ARTALK_ESTATE, "artalk_dino_forward before artalk_dino_finalize");
    (void)hipSetDevice(d->device);
    hipStream_t s = (hipStream_t)stream;
    if (!d->call.begin(s, d->timing)) return dn_fail(d, ARTALK_EHIP, "hipEventCreate failed");
    d->timer.start(s, d->timing);
    DnRun run{d, s};
    run.run(image_dev, feature0_dev, feature1_dev);
    if (hipGetLastError() != hipSuccess) return dn_fail(d, ARTALK_EHIP, "kernel launch failed");
    if (!d->call.end()) return dn_fail(d, ARTALK_EHIP, "the call failed on the device");
    if (d->timing) {
        for (double& v : d->stage_ms) v = 0;
        d->timer.finish(d->stage_ms, DN_STAGES);
    }
    return ARTALK_OK;
}

int artalk_dino_read(artalk_dino* d, const char* what, float* out_dev, int64_t n, void* stream) {
    if (!d) { g_dn_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (!d->finalized) return dn_fail(d, ARTALK_ESTATE, "artalk_dino_read before artalk_dino_finalize");
    if (!what || !out_dev) return dn_fail(d, ARTALK_EINVAL, "what and out must not be NULL");
    const std::string k = what;
    const DnWs w(d);
    const int64_t G = (int64_t)d->g * d->g, h3 = dn_h3(d->g);
    const int64_t hw[4] = {16 * G, 4 * G, G, h3 * h3};
    int64_t off = -1, len = 0;
    if (k.size() == 4 && k.compare(0, 3, "tap") == 0 && k[3] >= '0' && k[3] <= '3') { off = w.tap[k[3] - '0'] + d->D; len = G * d->D; }
    if (k.size() == 3 && k.compare(0, 2, "rn") == 0 && k[2] >= '0' && k[2] <= '3') { off = w.rn[k[2] - '0']; len = hw[k[2] - '0'] * DN_HID; }
    if (off < 0) return dn_fail(d, ARTALK_EINVAL, "what must be tap0..tap3 or rn0..rn3");
    if (n != len) return dn_fail(d, ARTALK_EINVAL, k + " holds " + std::to_string(len) + " floats");
    (void)hipSetDevice(d->device);
    if (hipMemcpyAsync(out_dev, d->ws.get() + off, (size_t)len * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return dn_fail(d, ARTALK_EHIP, "the copy failed");
    }
    return ARTALK_OK;
}

// ---- single kernels ----
#define DN_DONE() return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP
static inline bool dn_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int artalk_op_dino_resize_aa(const float* x, float* out, int C, int Hi, int Wi, int Ho, int Wo, int channels_last, int normalize, void* stream) {
    if (!x || !out || C < 1 || C > 4096 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || Hi > 16384 || Wi > 16384 || Ho > 16384 || Wo > 16384) return ARTALK_EINVAL;
    if (normalize && C != 3) return ARTALK_EINVAL;
    dn_resize_aa(x, out, C, Hi, Wi, Ho, Wo, channels_last != 0, normalize != 0, (hipStream_t)stream);
    DN_DONE();
}

int artalk_op_dino_normalize(const float* x, float* out, int64_t n, void* stream) {
    if (!x || !out || n < 1 || n > ((int64_t)1 << 28)) return ARTALK_EINVAL;
    ARTALK_LAUNCH(dino_normalize_kernel, dim3(dn_blocks(3 * n)), dim3(256), 0, (hipStream_t)stream, x, out, (long)n, dn_norm(true));
    DN_DONE();
}

int artalk_op_dino_im2col(const float* img, float* col, int grid, void* stream) {
    if (!img || !col || grid < 1 || grid > 64) return ARTALK_EINVAL;
    ARTALK_LAUNCH(dino_im2col_kernel, dim3(dn_blocks((long)grid * grid * DN_PKP)), dim3(256), 0, (hipStream_t)stream, img, col, grid);
    DN_DONE();
}

int artalk_op_dino_tokens(const float* patch, const float* cls, const float* pos, float* X, int T, int D, void* stream) {
    if (!patch || !cls || !pos || !X || T < 2 || T > 65536 || D < 4 || D > 4096 || D % 4) return ARTALK_EINVAL;
    if (!dn_al16(patch) || !dn_al16(cls) || !dn_al16(pos) || !dn_al16(X)) return ARTALK_EINVAL;
    ARTALK_LAUNCH(dino_tokens_kernel, dim3(dn_blocks((long)T * D / 4)), dim3(256), 0, (hipStream_t)stream, patch, cls, pos, X, T, D);
    DN_DONE();
}

int artalk_op_dino_layernorm(const float* X, float* Y, const float* w, const float* b, int M, int D, void* stream) {
    if (!X || !Y || !w || !b || M < 1 || D < 4 || D > 4096 || D % 4) return ARTALK_EINVAL;
    if (!dn_al16(X) || !dn_al16(Y) || !dn_al16(w) || !dn_al16(b)) return ARTALK_EINVAL;
    dn_layernorm(X, Y, w, b, M, D, (hipStream_t)stream);
    DN_DONE();
}

int artalk_op_dino_strip(const float* tap, float* out, int G, int D, void* stream) {
    if (!tap || !out || G < 1 || G > 65536 || D < 4 || D > 4096 || D % 4 || !dn_al16(tap) || !dn_al16(out)) return ARTALK_EINVAL;
    ARTALK_LAUNCH(dino_strip_kernel, dim3(dn_blocks((long)G * D / 4)), dim3(256), 0, (hipStream_t)stream, tap, out, (long)G * D, D);
    DN_DONE();
}

int artalk_op_dino_shuffle(const float* r, const float* bias, float* out, int grid, int s, int Co, void* stream) {
    if (!r || !bias || !out || grid < 1 || grid > 64 || s < 1 || s > 8 || Co < 4 || Co > 4096 || Co % 4) return ARTALK_EINVAL;
    if (!dn_al16(r) || !dn_al16(bias) || !dn_al16(out)) return ARTALK_EINVAL;
    ARTALK_LAUNCH(dino_shuffle_kernel, dim3(dn_blocks((long)s * grid * s * grid * Co / 4)), dim3(256), 0, (hipStream_t)stream, r, bias, out, grid, s, Co);
    DN_DONE();
}

int artalk_op_dino_gather_s2(const float* x, float* col, int grid, int C, void* stream) {
    if (!x || !col || grid < 1 || grid > 64 || C < 4 || C > 4096 || C % 4 || !dn_al16(x) || !dn_al16(col)) return ARTALK_EINVAL;
    const int Ho = (grid - 1) / 2 + 1;
    ARTALK_LAUNCH(dino_gather_s2_kernel, dim3(dn_blocks((long)Ho * Ho * 9 * C / 4)), dim3(256), 0, (hipStream_t)stream, x, col, grid, C);
    DN_DONE();
}

int artalk_op_dino_concat(const float* img, const float* feat, float* out, int64_t n, int C, void* stream) {
    if (!img || !feat || !out || n < 1 || n > ((int64_t)1 << 24) || C < 1 || C > 4096) return ARTALK_EINVAL;
    const int W = dn_pad8(C + 3);
    ARTALK_LAUNCH(dino_concat_kernel, dim3(dn_blocks(n * W)), dim3(256), 0, (hipStream_t)stream, img, feat, out, (long)n, C, W);
    DN_DONE();
}

int artalk_op_dino_resize_ac(const float* x, float* out, int Hi, int Wi, int Ho, int Wo, int C, void* stream) {
    if (!x || !out || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || Hi > 4096 || Wi > 4096 || Ho > 4096 || Wo > 4096 || C < 4 || C > 4096 || C % 4) return ARTALK_EINVAL;
    if (!dn_al16(x) || !dn_al16(out)) return ARTALK_EINVAL;
    ARTALK_LAUNCH(dino_resize_ac_kernel, dim3(dn_blocks((long)Ho * Wo * C / 4)), dim3(256), 0, (hipStream_t)stream, x, out, Hi, Wi, Ho, Wo, C);
    DN_DONE();
}

int artalk_op_dino_add_relu(const float* a, const float* b, float* sum_out, float* relu_out, int64_t n, void* stream) {
    if (!a || !relu_out || n < 4 || n % 4 || n > ((int64_t)1 << 32)) return ARTALK_EINVAL;
    if (!dn_al16(a) || !dn_al16(b) || !dn_al16(sum_out) || !dn_al16(relu_out)) return ARTALK_EINVAL;
    ARTALK_LAUNCH(dino_add_relu_kernel, dim3(dn_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, a, b, sum_out, relu_out, (long)n);
    DN_DONE();
}

int artalk_op_dino_output(const float* x, float* out, int64_t n, int C, const float* tok, float* f1, int D, void* stream) {
    if (!x || !out || n < 1 || n > ((int64_t)1 << 26) || C < 1 || C > 4096) return ARTALK_EINVAL;
    if (tok && (!f1 || D < 1 || D > 4096)) return ARTALK_EINVAL;
    ARTALK_LAUNCH(dino_output_kernel, dim3((unsigned)((n + 31) / 32), (unsigned)((C + 31) / 32)), dim3(256), 0, (hipStream_t)stream, x, out, (long)n, C, tok, f1, D);
    DN_DONE();
}

}  // extern "C"
