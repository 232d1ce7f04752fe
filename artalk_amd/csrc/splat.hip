// Gaussian splat rasteriser, forward only, 32 feature channels: a stand-in for the CUDA extension diff_gaussian_rasterization_32d that
// the reference's GAGAvatar head imports (app/GAGAvatar/utils_renderer.py:6) and calls under torch.no_grad (models.py:63).  The
// definition these kernels implement is written out in DESIGN.md ("Gaussian splat rasteriser"); tests/splat_ref.py restates it in
// numpy.  Parity with the CUDA extension itself is unpinned: neither its source nor a build of it is at hand.
//   splat_preprocess_kernel<true>   per (frame, Gaussian), all frames of the call: radius -> radii, tiles touched -> one 64-bit sum per frame
//   splat_preprocess_kernel<false>  per Gaussian of one frame: centre, conic + opacity, depth, tile rectangle, tiles touched
//   (exclusive scan of the tiles touched: hipCUB)
//   splat_emit_kernel               per Gaussian: its (tile << 32 | bits of depth, index) pairs, rows of the rectangle in order
//   (stable radix sort of the pairs on 32 + bits(tiles) key bits: hipCUB; a frame without pairs skips it)
//   splat_ranges_kernel             per pair: where each tile's run starts and ends
//   splat_blend_kernel              one workgroup of 256 threads per 16 x 16 tile: the tile's Gaussians pass through LDS in batches of
//                                   256 (geometry and the 32 colours), every thread keeps T and 32 sums in registers and walks the batch
//                                   front to back; the workgroup leaves when all its pixels have stopped
// artalk_splat_render_sets: an attribute may also lie in a pool of sets, and every frame names its set: the address of frame t's
// attribute is base + set[t] * set stride + t * frame stride.  The count pass, which covers all frames in one launch, reads set[t] from
// a device copy; the per-frame launches get bases the host has moved to the frame's set.  artalk_splat_render is the call without sets.
// Both preprocess forms run the same inlined function with floating-point contraction off, so the count the host sizes the pair buffers
// from is the count the second pass emits; the emit kernel checks every index against the capacity all the same.
// The number of pairs depends on the data.  artalk_splat_render therefore WAITS ONCE on its stream, after the counting pass, to read its
// frames' pair counts and grow its buffers (the CUDA extension does the same through its resize callbacks): this object is not bound by
// artalk_model's no-synchronisation rule.  Growing a buffer frees the old one, which waits for the device as well; a second call of the
// same shape allocates nothing.
#include "common.h"
#include "device_mem.h"
#include "../../include/artalk_hip.h"

#include <hipcub/hipcub.hpp>

#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace artalk {

constexpr int kSplatCh = 32;           // NUM_CHANNELS of the extension's 32d build
constexpr int kSplatTile = 16;         // tile edge in pixels
constexpr int kSplatBatch = 256;       // Gaussians staged per trip through LDS (one per thread)

struct SplatCam { float V[16], P[16]; };      // row-major, row-vector convention: (p, 1) . V
struct SplatAttrs {
    const float *means, *colors, *opac, *scales, *rots;
    long s_means, s_colors, s_opac, s_scales, s_rots;      // elements between two frames; 0: one set for every frame
    const int* sets;                                       // device [T]: the set of every frame, or null (every frame: set 0)
    long p_means, p_colors, p_opac, p_scales, p_rots;      // elements between two sets
};
struct SplatView {
    int N, H, W, gx, gy;               // gx x gy tiles
    float tanx, tany, fx, fy, mod;
};
struct SplatGeom {
    float x, y, depth;
    float4 conic_op;
    int radius, x0, x1, y0, y1;
};

// truncation towards zero, then the clamp, in float: equal to clamp(int(v), 0, hi) for every v an int can hold, and defined beyond
// (a NaN gives 0, +-inf a bound)
__device__ __forceinline__ int splat_tile_bound(float v, int hi) { return (int)fminf(fmaxf(truncf(v), 0.0f), (float)hi); }

// One Gaussian of one frame.  false: culled (radius 0, no tiles).
__device__ __forceinline__ bool splat_project(const SplatAttrs& a, const SplatView& v, const SplatCam& cam, int t, int i, SplatGeom& g) {
#pragma clang fp contract(off)
    const long set = a.sets ? (long)a.sets[t] : 0;
    const float* p = a.means + set * a.p_means + (long)t * a.s_means + (long)i * 3;
    const float px = p[0], py = p[1], pz = p[2];
    const float* V = cam.V;
    const float* P = cam.P;
    const float tx0 = px * V[0] + py * V[4] + pz * V[8] + V[12];
    const float ty0 = px * V[1] + py * V[5] + pz * V[9] + V[13];
    const float tz = px * V[2] + py * V[6] + pz * V[10] + V[14];
    if (!(tz > 0.2f)) return false;
    const float hx = px * P[0] + py * P[4] + pz * P[8] + P[12];
    const float hy = px * P[1] + py * P[5] + pz * P[9] + P[13];
    const float hw = px * P[3] + py * P[7] + pz * P[11] + P[15];
    const float wq = hw + 1e-7f;
    const float qx = hx / wq, qy = hy / wq;

    const float* sc = a.scales + set * a.p_scales + (long)t * a.s_scales + (long)i * 3;
    const float* rq = a.rots + set * a.p_rots + (long)t * a.s_rots + (long)i * 4;
    const float s0 = v.mod * sc[0], s1 = v.mod * sc[1], s2 = v.mod * sc[2];
    const float v0 = s0 * s0, v1 = s1 * s1, v2 = s2 * s2;
    const float r = rq[0], x = rq[1], y = rq[2], z = rq[3];
    const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
    const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
    const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
    // Sigma = R diag(v) R^T (symmetric)
    const float S00 = R00 * R00 * v0 + R01 * R01 * v1 + R02 * R02 * v2;
    const float S01 = R00 * R10 * v0 + R01 * R11 * v1 + R02 * R12 * v2;
    const float S02 = R00 * R20 * v0 + R01 * R21 * v1 + R02 * R22 * v2;
    const float S11 = R10 * R10 * v0 + R11 * R11 * v1 + R12 * R12 * v2;
    const float S12 = R10 * R20 * v0 + R11 * R21 * v1 + R12 * R22 * v2;
    const float S22 = R20 * R20 * v0 + R21 * R21 * v1 + R22 * R22 * v2;

    const float limx = 1.3f * v.tanx, limy = 1.3f * v.tany;
    const float tx = fminf(limx, fmaxf(-limx, tx0 / tz)) * tz;
    const float ty = fminf(limy, fmaxf(-limy, ty0 / tz)) * tz;
    const float J00 = v.fx / tz, J02 = -(v.fx * tx) / (tz * tz);
    const float J11 = v.fy / tz, J12 = -(v.fy * ty) / (tz * tz);
    // A = J . V[:3,:3]^T: A[r][j] = sum_i J[r][i] V[j][i]
    const float A00 = J00 * V[0] + J02 * V[2], A01 = J00 * V[4] + J02 * V[6], A02 = J00 * V[8] + J02 * V[10];
    const float A10 = J11 * V[1] + J12 * V[2], A11 = J11 * V[5] + J12 * V[6], A12 = J11 * V[9] + J12 * V[10];
    // B = A Sigma (2 x 3), cov = B A^T
    const float B00 = A00 * S00 + A01 * S01 + A02 * S02, B01 = A00 * S01 + A01 * S11 + A02 * S12, B02 = A00 * S02 + A01 * S12 + A02 * S22;
    const float B10 = A10 * S00 + A11 * S01 + A12 * S02, B11 = A10 * S01 + A11 * S11 + A12 * S12, B12 = A10 * S02 + A11 * S12 + A12 * S22;
    const float ca = B00 * A00 + B01 * A01 + B02 * A02 + 0.3f;
    const float cb = B00 * A10 + B01 * A11 + B02 * A12;
    const float cc = B10 * A10 + B11 * A11 + B12 * A12 + 0.3f;
    const float det = ca * cc - cb * cb;
    if (det == 0.0f) return false;
    const float mid = 0.5f * (ca + cc);
    const float lam = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
    const float rad = ceilf(3.0f * sqrtf(lam));
    if (!(rad < 1.0e9f)) return false;      // a radius no int holds (or a NaN): not drawn
    const float cx = ((qx + 1.0f) * (float)v.W - 1.0f) * 0.5f;
    const float cy = ((qy + 1.0f) * (float)v.H - 1.0f) * 0.5f;
    g.x0 = splat_tile_bound((cx - rad) / 16.0f, v.gx);
    g.x1 = splat_tile_bound((cx + rad + 15.0f) / 16.0f, v.gx);
    g.y0 = splat_tile_bound((cy - rad) / 16.0f, v.gy);
    g.y1 = splat_tile_bound((cy + rad + 15.0f) / 16.0f, v.gy);
    if (g.x1 <= g.x0 || g.y1 <= g.y0) return false;
    g.x = cx; g.y = cy; g.depth = tz;
    g.conic_op = make_float4(cc / det, -cb / det, ca / det, a.opac[set * a.p_opac + (long)t * a.s_opac + i]);
    g.radius = (int)rad;
    return true;
}

// COUNT: grid (ceil(N / 256), frames), frame t0 + blockIdx.y; radii [T][N] and counts [T] are the call's.
// else:  grid (ceil(N / 256)), frame t0; the geometry arrays are one frame's.
template <bool COUNT>
__global__ __launch_bounds__(256) void splat_preprocess_kernel(SplatAttrs a, SplatView v, const SplatCam* __restrict__ cams, int cam_stride,
                                                               int t0, int* __restrict__ radii, unsigned long long* __restrict__ counts,
                                                               float2* __restrict__ xy, float4* __restrict__ conic_op,
                                                               float* __restrict__ depth, uint4* __restrict__ rect,
                                                               unsigned int* __restrict__ touched) {
    __shared__ unsigned int s_sum;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int t = t0 + blockIdx.y;
    if (COUNT) {
        if (threadIdx.x == 0) s_sum = 0;
        __syncthreads();
    }
    unsigned int n = 0;
    if (i < v.N) {
        SplatGeom g;
        const bool ok = splat_project(a, v, cams[(long)t * cam_stride], t, i, g);
        if (ok) n = (unsigned int)(g.x1 - g.x0) * (unsigned int)(g.y1 - g.y0);      // at most 256 x 256
        if (COUNT) {
            radii[(long)t * v.N + i] = ok ? g.radius : 0;
        } else {
            touched[i] = n;
            if (ok) {
                xy[i] = make_float2(g.x, g.y);
                conic_op[i] = g.conic_op;
                depth[i] = g.depth;
                rect[i] = make_uint4(g.x0, g.x1, g.y0, g.y1);
            }
        }
    }
    if (COUNT) {
        if (n) atomicAdd(&s_sum, n);      // integers: the sum does not depend on the order (256 x 65 536 fits)
        __syncthreads();
        if (threadIdx.x == 0 && s_sum) atomicAdd(counts + t, (unsigned long long)s_sum);
    }
}

// grid (ceil(N / 256)): keys / vals hold `cap` pairs; nothing is written at or beyond it, whatever the offsets say
__global__ __launch_bounds__(256) void splat_emit_kernel(int N, int gx, const uint4* __restrict__ rect, const unsigned int* __restrict__ touched,
                                                         const unsigned int* __restrict__ offsets, const float* __restrict__ depth,
                                                         unsigned long long* __restrict__ keys, unsigned int* __restrict__ vals,
                                                         unsigned int cap) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N || touched[i] == 0) return;
    const uint4 rc = rect[i];
    const unsigned long long d = __float_as_uint(depth[i]);      // depth > 0.2: its bits order like its value
    unsigned int off = offsets[i];
    for (unsigned int y = rc.z; y < rc.w; ++y)
        for (unsigned int x = rc.x; x < rc.y; ++x, ++off)
            if (off < cap) {
                keys[off] = ((unsigned long long)(y * gx + x) << 32) | d;
                vals[off] = (unsigned int)i;
            }
}

// grid (ceil(P / 256)); ranges [tiles] zeroed before
__global__ __launch_bounds__(256) void splat_ranges_kernel(unsigned int P, const unsigned long long* __restrict__ keys, uint2* __restrict__ ranges,
                                                           unsigned int tiles) {
    const unsigned int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    const unsigned int tile = (unsigned int)(keys[idx] >> 32);
    if (tile >= tiles) return;
    if (idx == 0) {
        ranges[tile].x = 0;
    } else {
        const unsigned int prev = (unsigned int)(keys[idx - 1] >> 32);
        if (prev != tile) {
            if (prev < tiles) ranges[prev].y = idx;
            ranges[tile].x = idx;
        }
    }
    if (idx == P - 1) ranges[tile].y = P;
}

// grid (gx, gy), 256 threads = the tile's 16 x 16 pixels.  colors: the frame's [N][32]; out: the frame's [32][H][W].
// LDS: 256 x (8 + 16 + 128) B = 38 KiB, so four workgroups fit a CU's 160 KiB.  In the walk every lane of a wave reads the same LDS
// address (a broadcast, no bank conflict); the staging writes are consecutive dwords / 16-byte slots per lane.
__global__ __launch_bounds__(256) void splat_blend_kernel(SplatView v, const uint2* __restrict__ ranges, const unsigned int* __restrict__ vals,
                                                          const float2* __restrict__ xy, const float4* __restrict__ conic_op,
                                                          const float* __restrict__ colors, int colors_vec, const float* __restrict__ bg,
                                                          float* __restrict__ out) {
    __shared__ float4 s_con[kSplatBatch];
    __shared__ float2 s_xy[kSplatBatch];
    __shared__ unsigned int s_id[kSplatBatch];
    __shared__ float4 s_col[kSplatBatch * (kSplatCh / 4)];
    const int tid = threadIdx.x;
    const int px = blockIdx.x * kSplatTile + (tid & 15), py = blockIdx.y * kSplatTile + (tid >> 4);
    const bool inside = px < v.W && py < v.H;      // an edge tile's pixels beyond the image take part in the staging only
    const float pxf = (float)px, pyf = (float)py;
    const uint2 range = ranges[blockIdx.y * v.gx + blockIdx.x];
    bool done = !inside;
    float T = 1.0f;
    float C[kSplatCh];
#pragma unroll
    for (int ch = 0; ch < kSplatCh; ++ch) C[ch] = 0.0f;
    for (unsigned int base = range.x; base < range.y; base += kSplatBatch) {
        // (the barrier in the count also keeps the previous batch's readers ahead of the writes below)
        if (__syncthreads_count(done ? 1 : 0) == 256) break;
        const int n = (int)min((unsigned int)kSplatBatch, range.y - base);
        if (tid < n) {
            const unsigned int id = min(vals[base + tid], (unsigned int)(v.N - 1));      // (in range by construction; no read beyond the arrays if not)
            s_id[tid] = id;
            s_xy[tid] = xy[id];
            s_con[tid] = conic_op[id];
        }
        __syncthreads();
        if (colors_vec) {      // 8 lanes fetch one Gaussian's 128 bytes, 32 Gaussians per trip
            const int part = tid & 7;
#pragma unroll
            for (int k = 0; k < kSplatBatch / 32; ++k) {
                const int j = k * 32 + (tid >> 3);
                if (j < n) s_col[j * 8 + part] = reinterpret_cast<const float4*>(colors)[(long)s_id[j] * 8 + part];
            }
        } else {               // a colour pointer that is not 16-byte aligned: dword loads, 8 Gaussians per trip
            float* sc = reinterpret_cast<float*>(s_col);
            const int ch = tid & 31;
            for (int j = tid >> 5; j < n; j += 8) sc[j * kSplatCh + ch] = colors[(long)s_id[j] * kSplatCh + ch];
        }
        __syncthreads();
        for (int j = 0; !done && j < n; ++j) {
            float w, Tn;
            {
#pragma clang fp contract(off)
                const float2 c = s_xy[j];
                const float4 con = s_con[j];
                const float dx = c.x - pxf, dy = c.y - pyf;
                const float power = -0.5f * (con.x * dx * dx + con.z * dy * dy) - con.y * dx * dy;
                if (power > 0.0f) continue;
                const float alpha = fminf(0.99f, con.w * expf(power));
                if (alpha < 1.0f / 255.0f) continue;
                Tn = T * (1.0f - alpha);
                if (Tn < 0.0001f) { done = true; continue; }
                w = alpha * T;
            }
#pragma unroll
            for (int q = 0; q < kSplatCh / 4; ++q) {
                const float4 col = s_col[j * 8 + q];
                C[4 * q] = fmaf(col.x, w, C[4 * q]);
                C[4 * q + 1] = fmaf(col.y, w, C[4 * q + 1]);
                C[4 * q + 2] = fmaf(col.z, w, C[4 * q + 2]);
                C[4 * q + 3] = fmaf(col.w, w, C[4 * q + 3]);
            }
            T = Tn;
        }
    }
    if (inside) {
        const long HW = (long)v.H * v.W;
        float* o = out + (long)py * v.W + px;
#pragma unroll
        for (int ch = 0; ch < kSplatCh; ++ch) o[ch * HW] = bg ? fmaf(T, bg[ch], C[ch]) : C[ch];
    }
}

}  // namespace artalk

using namespace artalk;

namespace {

enum { kStageCount, kStagePreprocess, kStageScanEmit, kStageSort, kStageRanges, kStageBlend, kSplatStages };

}  // namespace

struct artalk_splat {
    int device = 0;
    DevBuf<SplatCam> cams;
    DevBuf<int> sets;          // render_sets: the set of every frame of the call
    DevBuf<unsigned long long> counts, keys_in, keys_out;
    DevBuf<float2> xy; DevBuf<float4> conic; DevBuf<float> depth; DevBuf<uint4> rect;      // per Gaussian of the frame in work
    DevBuf<unsigned int> touched, offsets, vals_in, vals_out;
    DevBuf<uint2> ranges;
    DevBuf<char> scan_tmp, sort_tmp;
    PinnedBuf<char> host;      // cameras (and set indices) going up, pair counts coming down
    bool timing = false, used = false;
    double stage_ms[kSplatStages] = {0, 0, 0, 0, 0, 0};
    long long last_pairs = 0;
    int last_frames = 0;
    std::string err;
};

static thread_local std::string g_splat_error;

// room for n elements and a quarter more (pair counts change from call to call); earlier calls on the stream may still read the old block
template <typename T>
static bool splat_grow(artalk_splat* s, DevBuf<T>& b, size_t n, hipStream_t st) {
    if (b.grow(n, 1, 4, st)) return true;
    s->err = "hipMalloc of " + std::to_string(DevBuf<T>::grown_bytes(n, 1, 4)) + " bytes failed";
    return false;
}

static int splat_bits(unsigned int tiles) {      // bits that hold every tile index below `tiles`
    int b = 0;
    while (b < 32 && (1ull << b) < tiles) ++b;
    return b;
}

extern "C" {

const char* artalk_splat_last_error(const artalk_splat* s) { return s ? s->err.c_str() : g_splat_error.c_str(); }

void artalk_splat_destroy(artalk_splat* s) {
    if (!s) return;
    if (s->used) {      // (never used: the buffers are empty and the device stays untouched)
        (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();
    }
    delete s;
}

int artalk_splat_create(int device_id, artalk_splat** out) {
    if (!out) { g_splat_error = "out is NULL"; return ARTALK_EINVAL; }
    *out = nullptr;
    if (device_id < 0) { g_splat_error = "device_id must not be negative"; return ARTALK_EINVAL; }
    artalk_splat* s = new artalk_splat();      // the device is first touched by a render call that passes its checks
    s->device = device_id;
    *out = s;
    return ARTALK_OK;
}

int artalk_splat_set_timing(artalk_splat* s, int enable) {
    if (!s) { g_splat_error = "rasteriser is NULL"; return ARTALK_EINVAL; }
    s->timing = enable != 0;
    return ARTALK_OK;
}

int artalk_splat_get_timing(const artalk_splat* s, double* stage_ms, int n, long long* pairs, int* frames) {
    if (!s) { g_splat_error = "rasteriser is NULL"; return ARTALK_EINVAL; }
    if (stage_ms) for (int i = 0; i < n && i < kSplatStages; ++i) stage_ms[i] = s->stage_ms[i];
    if (pairs) *pairs = s->last_pairs;
    if (frames) *frames = s->last_frames;
    return kSplatStages;
}

int artalk_splat_render_sets(artalk_splat* s, int N, int T, int H, int W, const float* means_dev, int64_t means_stride, const float* colors_dev,
                             int64_t colors_stride, const float* opacities_dev, int64_t opacities_stride, const float* scales_dev,
                             int64_t scales_stride, const float* rotations_dev, int64_t rotations_stride, const float* view_host,
                             const float* proj_host, int n_cams, float tanfovx, float tanfovy, float scale_modifier,
                             const float* bg_dev_or_null, float* out_dev, int32_t* radii_dev, const int32_t* set_of_frame_host, int n_sets,
                             int64_t means_set_stride, int64_t colors_set_stride, int64_t opacities_set_stride, int64_t scales_set_stride,
                             int64_t rotations_set_stride, void* stream) {
    if (!s) { g_splat_error = "rasteriser is NULL"; return ARTALK_EINVAL; }
    if (N < 0) { s->err = "N must not be negative"; return ARTALK_EINVAL; }
    if (T < 0) { s->err = "T must not be negative"; return ARTALK_EINVAL; }
    if (H < 1 || H > 4096) { s->err = "H must be in 1..4096"; return ARTALK_EINVAL; }
    if (W < 1 || W > 4096) { s->err = "W must be in 1..4096"; return ARTALK_EINVAL; }
    if (!(tanfovx > 0.f) || !(tanfovy > 0.f)) { s->err = "tanfovx and tanfovy must be positive"; return ARTALK_EINVAL; }
    if (n_cams != 1 && n_cams != T) { s->err = "n_cams must be 1 or T"; return ARTALK_EINVAL; }
    if (!out_dev) { s->err = "out is NULL"; return ARTALK_EINVAL; }
    if (N > 0 && !radii_dev) { s->err = "radii is NULL"; return ARTALK_EINVAL; }
    if (N > 0 && (!means_dev || !colors_dev || !opacities_dev || !scales_dev || !rotations_dev)) {
        s->err = "means, colors, opacities, scales and rotations must not be NULL";
        return ARTALK_EINVAL;
    }
    if (N > 0 && (!view_host || !proj_host)) { s->err = "viewmatrix and projmatrix must not be NULL"; return ARTALK_EINVAL; }
    if (means_stride < 0 || colors_stride < 0 || opacities_stride < 0 || scales_stride < 0 || rotations_stride < 0) {
        s->err = "a frame stride must not be negative";
        return ARTALK_EINVAL;
    }
    const int32_t* sets = T > 0 ? set_of_frame_host : nullptr;
    if (sets) {
        if (means_set_stride < 0 || colors_set_stride < 0 || opacities_set_stride < 0 || scales_set_stride < 0 || rotations_set_stride < 0) {
            s->err = "a set stride must not be negative";
            return ARTALK_EINVAL;
        }
        for (int t = 0; t < T; ++t)
            if (sets[t] < 0 || sets[t] >= n_sets) {
                s->err = "frame " + std::to_string(t) + " names set " + std::to_string(sets[t]) + ", outside [0, " + std::to_string(n_sets) + ")";
                return ARTALK_EINVAL;
            }
    }
    if (T == 0) return ARTALK_OK;
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); s->err = "hipSetDevice failed"; return ARTALK_EHIP; }
    hipStream_t st = (hipStream_t)stream;
    s->used = true;

    SplatView v;
    v.N = N; v.H = H; v.W = W;
    v.gx = (W + kSplatTile - 1) / kSplatTile; v.gy = (H + kSplatTile - 1) / kSplatTile;
    v.tanx = tanfovx; v.tany = tanfovy;
    v.fx = (float)W / (2.0f * tanfovx); v.fy = (float)H / (2.0f * tanfovy);
    v.mod = scale_modifier;
    const unsigned int tiles = (unsigned int)v.gx * v.gy;
    const long HW = (long)H * W;
    const int nblk = (N + 255) / 256;
    SplatAttrs a{means_dev, colors_dev, opacities_dev, scales_dev, rotations_dev,
                 (long)means_stride, (long)colors_stride, (long)opacities_stride, (long)scales_stride, (long)rotations_stride,
                 nullptr, 0, 0, 0, 0, 0};
    if (sets) { a.p_means = (long)means_set_stride; a.p_colors = (long)colors_set_stride; a.p_opac = (long)opacities_set_stride;
                a.p_scales = (long)scales_set_stride; a.p_rots = (long)rotations_set_stride; }

    StageTimer timer;
    timer.start(st, s->timing);
    for (double& m : s->stage_ms) m = 0;
    s->last_pairs = 0; s->last_frames = T;

    if (!splat_grow(s, s->ranges, tiles, st)) return ARTALK_EHIP;
    const unsigned long long* counts_host = nullptr;
    if (N > 0) {
        const size_t cam_bytes = (size_t)n_cams * sizeof(SplatCam), cnt_bytes = (size_t)T * sizeof(unsigned long long);
        const size_t set_bytes = sets ? (size_t)T * sizeof(int) : 0;      // behind the cameras, which are 128 bytes each
        if (!s->host.grow(cam_bytes + cnt_bytes + set_bytes, 0, 1, st)) { s->err = "hipHostMalloc failed"; return ARTALK_EHIP; }
        size_t scan_bytes = 0;
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const unsigned int*)nullptr, (unsigned int*)nullptr, N, st);
        if (!splat_grow(s, s->cams, n_cams, st) || !splat_grow(s, s->counts, T, st) || !splat_grow(s, s->xy, N, st) ||
            !splat_grow(s, s->conic, N, st) || !splat_grow(s, s->depth, N, st) || !splat_grow(s, s->rect, N, st) ||
            !splat_grow(s, s->touched, N, st) || !splat_grow(s, s->offsets, N, st) || !splat_grow(s, s->scan_tmp, scan_bytes ? scan_bytes : 16, st) ||
            (sets && !splat_grow(s, s->sets, T, st)))
            return ARTALK_EHIP;
        // the pinned block is free here: every earlier call waited on its stream after its upload, and its download ended that wait
        SplatCam* hc = (SplatCam*)(s->host.get() + cnt_bytes);
        for (int c = 0; c < n_cams; ++c) {
            std::memcpy(hc[c].V, view_host + (size_t)c * 16, sizeof(float) * 16);
            std::memcpy(hc[c].P, proj_host + (size_t)c * 16, sizeof(float) * 16);
        }
        if (sets) std::memcpy(s->host.get() + cnt_bytes + cam_bytes, sets, set_bytes);
        if (hipMemcpyAsync(s->cams.get(), hc, cam_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
            (sets && hipMemcpyAsync(s->sets.get(), s->host.get() + cnt_bytes + cam_bytes, set_bytes, hipMemcpyHostToDevice, st) != hipSuccess) ||
            hipMemsetAsync(s->counts.get(), 0, cnt_bytes, st) != hipSuccess) {
            (void)hipGetLastError();
            s->err = "camera upload failed";
            return ARTALK_EHIP;
        }
        timer.mark(-1);
        SplatAttrs ac = a;
        ac.sets = sets ? s->sets.get() : nullptr;
        for (int t0 = 0; t0 < T; t0 += 32768) {      // (grid.y is a 16-bit quantity)
            const int n = T - t0 < 32768 ? T - t0 : 32768;
            ARTALK_LAUNCH(splat_preprocess_kernel<true>, dim3(nblk, n), dim3(256), 0, st, ac, v, (const SplatCam*)s->cams.get(), n_cams == 1 ? 0 : 1,
                          t0, radii_dev, s->counts.get(), (float2*)nullptr, (float4*)nullptr, (float*)nullptr, (uint4*)nullptr,
                          (unsigned int*)nullptr);
        }
        timer.mark(kStageCount);
        // the one wait of the call: the pair counts size the key buffers
        if (hipMemcpyAsync(s->host.get(), s->counts.get(), cnt_bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            s->err = std::string("counting pass failed: ") + hipGetErrorString(hipGetLastError());
            return ARTALK_EHIP;
        }
        counts_host = (const unsigned long long*)s->host.get();
        unsigned long long maxp = 0;
        for (int t = 0; t < T; ++t) {
            if (counts_host[t] > maxp) maxp = counts_host[t];
            s->last_pairs += (long long)counts_host[t];
        }
        if (maxp > (unsigned long long)INT_MAX) {
            s->err = "a frame has " + std::to_string(maxp) + " (tile, Gaussian) pairs; at most 2^31 - 1 are supported";
            return ARTALK_ECAPACITY;
        }
        if (maxp > 0) {
            size_t sort_bytes = 0;
            (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                     (const unsigned int*)nullptr, (unsigned int*)nullptr, (int)maxp, 0,
                                                     32 + splat_bits(tiles), st);
            if (!splat_grow(s, s->keys_in, maxp, st) || !splat_grow(s, s->keys_out, maxp, st) || !splat_grow(s, s->vals_in, maxp, st) ||
                !splat_grow(s, s->vals_out, maxp, st) || !splat_grow(s, s->sort_tmp, sort_bytes ? sort_bytes : 16, st))
                return ARTALK_EHIP;
        }
    }

    bool ok = true;
    for (int t = 0; t < T && ok; ++t) {
        const unsigned int P = counts_host ? (unsigned int)counts_host[t] : 0u;
        timer.mark(-1);
        const long set = sets ? (long)sets[t] : 0;
        if (N > 0) {
            SplatAttrs at = a;      // the frame's set: bases moved on the host
            at.means += set * a.p_means; at.opac += set * a.p_opac; at.scales += set * a.p_scales; at.rots += set * a.p_rots;
            ARTALK_LAUNCH(splat_preprocess_kernel<false>, dim3(nblk), dim3(256), 0, st, at, v, (const SplatCam*)s->cams.get(), n_cams == 1 ? 0 : 1, t,
                          (int*)nullptr, (unsigned long long*)nullptr, s->xy.get(), s->conic.get(), s->depth.get(), s->rect.get(), s->touched.get());
            timer.mark(kStagePreprocess);
        }
        ok = ok && hipMemsetAsync(s->ranges.get(), 0, (size_t)tiles * sizeof(uint2), st) == hipSuccess;
        if (P > 0) {
            size_t scan_bytes = s->scan_tmp.capacity(), sort_bytes = s->sort_tmp.capacity();
            ok = ok && hipcub::DeviceScan::ExclusiveSum(s->scan_tmp.get(), scan_bytes, (const unsigned int*)s->touched.get(), s->offsets.get(),
                                                        N, st) == hipSuccess;
            ARTALK_LAUNCH(splat_emit_kernel, dim3(nblk), dim3(256), 0, st, N, v.gx, (const uint4*)s->rect.get(), (const unsigned int*)s->touched.get(),
                          (const unsigned int*)s->offsets.get(), (const float*)s->depth.get(), s->keys_in.get(), s->vals_in.get(), P);
            timer.mark(kStageScanEmit);
            ok = ok && hipcub::DeviceRadixSort::SortPairs(s->sort_tmp.get(), sort_bytes, (const unsigned long long*)s->keys_in.get(),
                                                          s->keys_out.get(), (const unsigned int*)s->vals_in.get(), s->vals_out.get(), (int)P, 0, 32 + splat_bits(tiles), st) == hipSuccess;
            timer.mark(kStageSort);
            ARTALK_LAUNCH(splat_ranges_kernel, dim3((P + 255) / 256), dim3(256), 0, st, P, (const unsigned long long*)s->keys_out.get(), s->ranges.get(), tiles);
            timer.mark(kStageRanges);
        }
        const float* col_t = colors_dev ? colors_dev + set * a.p_colors + (long)t * colors_stride : nullptr;
        const int vec = (((unsigned long long)col_t) & 15) == 0 ? 1 : 0;
        ARTALK_LAUNCH(splat_blend_kernel, dim3(v.gx, v.gy), dim3(256), 0, st, v, (const uint2*)s->ranges.get(), (const unsigned int*)s->vals_out.get(),
                      (const float2*)s->xy.get(), (const float4*)s->conic.get(), col_t, vec, bg_dev_or_null, out_dev + (long)t * kSplatCh * HW);
        timer.mark(kStageBlend);
    }
    timer.finish(s->stage_ms, kSplatStages);
    if (!ok || hipGetLastError() != hipSuccess) { s->err = "a launch failed"; return ARTALK_EHIP; }
    return ARTALK_OK;
}

int artalk_splat_render(artalk_splat* s, int N, int T, int H, int W, const float* means_dev, int64_t means_stride, const float* colors_dev,
                        int64_t colors_stride, const float* opacities_dev, int64_t opacities_stride, const float* scales_dev,
                        int64_t scales_stride, const float* rotations_dev, int64_t rotations_stride, const float* view_host,
                        const float* proj_host, int n_cams, float tanfovx, float tanfovy, float scale_modifier, const float* bg_dev_or_null,
                        float* out_dev, int32_t* radii_dev, void* stream) {
    return artalk_splat_render_sets(s, N, T, H, W, means_dev, means_stride, colors_dev, colors_stride, opacities_dev, opacities_stride, scales_dev,
                                    scales_stride, rotations_dev, rotations_stride, view_host, proj_host, n_cams, tanfovx, tanfovy,
                                    scale_modifier, bg_dev_or_null, out_dev, radii_dev, nullptr, 0, 0, 0, 0, 0, 0, stream);
}

}  // extern "C"
