// Frames out ("Frames out"): fp32 planar frames [F][3][H][W] in [0, 1] -> what a video encoder takes, 8 bits a sample.
//
//   frames_rgb24_kernel     out [F][H][W][3]: q(r), q(g), q(b) interleaved (PyAV's "rgb24")
//   frames_yuv420p_kernel   out [F]{ Y [H][W], U [H/2][W/2], V [H/2][W/2] }: BT.601 limited range in integers from the quantised r, g, b,
//                           chroma from the rounded mean of each 2 x 2 block (an I420 frame: PyAV's "yuv420p", a Y4M file's C420)
//
// q(v) = (uint8)(clamp(v, 0, 1) * 255.0f): the reference's (x * 255.0).astype(np.uint8), truncation, on a clamped value (NaN -> 0).
// Each kernel has a plain form and a fused form (kFinish) that first applies gaga_finish_kernel's clamp and watermark blend (gaga.hip) in
// the same expression order with contraction off, so that finish followed by the plain form and the fused form agree bit for bit.
//
// A lane owns four neighbouring pixels (rgb24: of the frame taken as one row of H W pixels; yuv420p: of two rows, a 4 x 2 block).  It
// reads each run of four fp32 with one 16-byte load and writes three dwords of rgb24, or one dword of Y per row and two bytes of U and of
// V, where the ADDRESSES allow it: frame sizes need not be multiples of four bytes (3 x 5 rgb24: 45, 2 x 2 yuv420p: 6), so later
// frames of a batch, and views that start off a 16-byte boundary, take the scalar path, which gives the same bytes.  All element indices
// are 64-bit.  No atomics, no reductions: bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "artalk_hip.h"
#include "common.h"
#include "kernels.h"

namespace artalk {

namespace {

// gaga_finish_kernel's value of element (c, pix) of an S x S frame: clamp(0, 1), then the watermark blend on the bottom-right h x w patch
__device__ __forceinline__ float finish_value(float v, const float* __restrict__ wm, int h, int w, int S, int c, long pix) {
#pragma clang fp contract(off)
    v = fminf(fmaxf(v, 0.f), 1.f);
    if (wm) {
        const int y = (int)(pix / S) - (S - h), x = (int)(pix % S) - (S - w);
        if (y >= 0 && x >= 0) {
            const float a = wm[(3L * h + y) * w + x] * 0.8f;
            v = v * (1.f - a) + wm[((long)c * h + y) * w + x] * a;
        }
    }
    return v;
}

__device__ __forceinline__ int quant8(float v) {
#pragma clang fp contract(off)
    const float c = fminf(fmaxf(v, 0.f), 1.f);      // NaN -> 0
    const float p = c * 255.0f;
    return (int)p;                                   // truncation, 0 .. 255
}

// four fp32 from p (n of them real): one 16-byte load when p allows it
__device__ __forceinline__ void load4(const float* __restrict__ p, int n, float v[4]) {
    if (n == 4 && ((uintptr_t)p & 15) == 0) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = i < n ? p[i] : 0.f;
    }
}

// src [F][3][P] (P = H W pixels), out [F][P][3].  One lane per group of four pixels of a frame; the last group of a frame may be short.
template <bool kFinish>
__global__ __launch_bounds__(256) void frames_rgb24_kernel(const float* __restrict__ src, uint8_t* __restrict__ out, long F, int H, int W,
                                                           const float* __restrict__ wm, int h, int w) {
    const long P = (long)H * W, G = (P + 3) / 4;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= F * G) return;
    const long f = idx / G, p0 = (idx - f * G) * 4;
    const int n = P - p0 < 4 ? (int)(P - p0) : 4;
    const float* s = src + f * 3 * P + p0;
    uint8_t* o = out + (f * P + p0) * 3;
    int q[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v[4];
        load4(s + (long)c * P, n, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) q[c][i] = quant8(kFinish ? finish_value(v[i], wm, h, w, W, c, p0 + i) : v[i]);
    }
    if (n == 4 && ((uintptr_t)o & 3) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);      // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3, little endian
        o4[0] = (uint32_t)q[0][0] | (uint32_t)q[1][0] << 8 | (uint32_t)q[2][0] << 16 | (uint32_t)q[0][1] << 24;
        o4[1] = (uint32_t)q[1][1] | (uint32_t)q[2][1] << 8 | (uint32_t)q[0][2] << 16 | (uint32_t)q[1][2] << 24;
        o4[2] = (uint32_t)q[2][2] | (uint32_t)q[0][3] << 8 | (uint32_t)q[1][3] << 16 | (uint32_t)q[2][3] << 24;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n) { o[i * 3] = (uint8_t)q[0][i]; o[i * 3 + 1] = (uint8_t)q[1][i]; o[i * 3 + 2] = (uint8_t)q[2][i]; }
    }
}

// src [F][3][H][W], H and W even; out [F]{Y [H][W], U [H/2][W/2], V [H/2][W/2]}.  One lane per 4 x 2 block (2 x 2 at the right edge when
// W % 4 == 2).  >> on a negative int is an arithmetic shift.
template <bool kFinish>
__global__ __launch_bounds__(256) void frames_yuv420p_kernel(const float* __restrict__ src, uint8_t* __restrict__ out, long F, int H, int W,
                                                             const float* __restrict__ wm, int h, int w) {
    const long P = (long)H * W, GX = (W + 3) / 4, GY = H / 2, G = GX * GY;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= F * G) return;
    const long f = idx / G, g = idx - f * G;
    const int gy = (int)(g / GX), x0 = (int)(g - (long)gy * GX) * 4, y0 = gy * 2;
    const int n = W - x0 < 4 ? W - x0 : 4;      // 4 or 2
    uint8_t* frame = out + f * (P + P / 2);
    int q[2][3][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const long pix = (long)(y0 + r) * W + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[4];
            load4(src + (f * 3 + c) * P + pix, n, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) q[r][c][i] = quant8(kFinish ? finish_value(v[i], wm, h, w, W, c, pix + i) : v[i]);
        }
        int y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = ((66 * q[r][0][i] + 129 * q[r][1][i] + 25 * q[r][2][i] + 128) >> 8) + 16;
        uint8_t* oy = frame + pix;
        if (n == 4 && ((uintptr_t)oy & 3) == 0) {
            *reinterpret_cast<uint32_t*>(oy) = (uint32_t)y[0] | (uint32_t)y[1] << 8 | (uint32_t)y[2] << 16 | (uint32_t)y[3] << 24;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) oy[i] = (uint8_t)y[i];
        }
    }
    int u[2], v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = (q[0][c][2 * j] + q[0][c][2 * j + 1] + q[1][c][2 * j] + q[1][c][2 * j + 1] + 2) >> 2;
        u[j] = ((-38 * m[0] - 74 * m[1] + 112 * m[2] + 128) >> 8) + 128;
        v[j] = ((112 * m[0] - 94 * m[1] - 18 * m[2] + 128) >> 8) + 128;
    }
    uint8_t* ou = frame + P + (long)gy * (W / 2) + x0 / 2;
    uint8_t* ov = ou + P / 4;
    if (n == 4 && ((uintptr_t)ou & 1) == 0) *reinterpret_cast<uint16_t*>(ou) = (uint16_t)(u[0] | u[1] << 8);
    else { ou[0] = (uint8_t)u[0]; if (n == 4) ou[1] = (uint8_t)u[1]; }
    if (n == 4 && ((uintptr_t)ov & 1) == 0) *reinterpret_cast<uint16_t*>(ov) = (uint16_t)(v[0] | v[1] << 8);
    else { ov[0] = (uint8_t)v[0]; if (n == 4) ov[1] = (uint8_t)v[1]; }
}

template <bool kFinish>
void launch_pack(const float* src, long F, int H, int W, int format, uint8_t* out, const float* wm, int h, int w, hipStream_t s) {
    if (F <= 0) return;
    const long P = (long)H * W;
    const long groups = F * (format == ARTALK_FRAMES_RGB24 ? (P + 3) / 4 : (long)((W + 3) / 4) * (H / 2));
    const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
    if (format == ARTALK_FRAMES_RGB24) ARTALK_LAUNCH(frames_rgb24_kernel<kFinish>, grid, block, 0, s, src, out, F, H, W, wm, h, w);
    else ARTALK_LAUNCH(frames_yuv420p_kernel<kFinish>, grid, block, 0, s, src, out, F, H, W, wm, h, w);
}

}  // namespace

int64_t frames_bytes(int format, int H, int W) {
    if (H < 1 || W < 1 || H > kFramesMaxSide || W > kFramesMaxSide) return ARTALK_EINVAL;
    if (format == ARTALK_FRAMES_RGB24) return (int64_t)H * W * 3;
    if (format == ARTALK_FRAMES_YUV420P) return (H % 2 || W % 2) ? (int64_t)ARTALK_EINVAL : (int64_t)H * W * 3 / 2;
    return ARTALK_EINVAL;
}

int frames_check(int format, int F, int H, int W, bool have_src, bool have_out, std::string* err) {
    if (format != ARTALK_FRAMES_RGB24 && format != ARTALK_FRAMES_YUV420P) {
        *err = "unknown frame format " + std::to_string(format) + " (ARTALK_FRAMES_RGB24 = 1, ARTALK_FRAMES_YUV420P = 2)";
        return ARTALK_EINVAL;
    }
    if (H < 1 || W < 1 || H > kFramesMaxSide || W > kFramesMaxSide) {
        *err = "H and W must be in 1.." + std::to_string(kFramesMaxSide) + " (got " + std::to_string(H) + " x " + std::to_string(W) + ")";
        return ARTALK_EINVAL;
    }
    if (format == ARTALK_FRAMES_YUV420P && (H % 2 || W % 2)) {
        *err = "yuv420p needs an even H and W (got " + std::to_string(H) + " x " + std::to_string(W) + ")";
        return ARTALK_EINVAL;
    }
    if (F < 0) { *err = "F must not be negative"; return ARTALK_EINVAL; }
    if (F > 0 && (!have_src || !have_out)) { *err = "src and out must not be NULL"; return ARTALK_EINVAL; }
    // one lane per four pixels, 256 lanes a block: the grid's x must fit 31 bits
    if (((int64_t)F * (((int64_t)H * W + 3) / 4) + 255) / 256 > 0x7fffffffll) { *err = "F x H x W is too large for one launch"; return ARTALK_EINVAL; }
    return ARTALK_OK;
}

void launch_frames_pack(const float* src, long F, int H, int W, int format, uint8_t* out, hipStream_t s) {
    launch_pack<false>(src, F, H, W, format, out, nullptr, 0, 0, s);
}

void launch_frames_finish_pack(const float* img, const float* wm, int h, int w, int S, long F, int format, uint8_t* out, hipStream_t s) {
    launch_pack<true>(img, F, S, S, format, out, wm, wm ? h : 0, wm ? w : 0, s);
}

}  // namespace artalk

using namespace artalk;

static thread_local std::string g_frames_error;

extern "C" {

const char* artalk_frames_last_error(void) { return g_frames_error.c_str(); }

int64_t artalk_frames_bytes(int format, int H, int W) { return frames_bytes(format, H, W); }

int artalk_frames_pack(const float* src_dev, int F, int H, int W, int format, uint8_t* out_dev, void* stream) {
    const int rc = frames_check(format, F, H, W, src_dev != nullptr, out_dev != nullptr, &g_frames_error);
    if (rc != ARTALK_OK) return rc;
    if (F == 0) return ARTALK_OK;
    launch_frames_pack(src_dev, F, H, W, format, out_dev, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) { g_frames_error = "a launch failed"; return ARTALK_EHIP; }
    return ARTALK_OK;
}

int artalk_op_frames_check(int format, int F, int H, int W, int have_src, int have_out, char* msg, int msg_cap) {
    std::string err;
    const int rc = frames_check(format, F, H, W, have_src != 0, have_out != 0, &err);
    if (msg && msg_cap > 0) { std::strncpy(msg, err.c_str(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
    return rc;
}

int artalk_op_gaga_finish_pack(const float* img_dev, int F, int S, const float* rgba_dev_or_null, int h, int w, int format, uint8_t* out_dev,
                               void* stream) {
    if (F < 1 || S > 4096) return ARTALK_EINVAL;
    if (frames_check(format, F, S, S, img_dev != nullptr, out_dev != nullptr, &g_frames_error) != ARTALK_OK) return ARTALK_EINVAL;
    if (rgba_dev_or_null && (h < 1 || w < 1 || h > S || w > S)) return ARTALK_EINVAL;
    launch_frames_finish_pack(img_dev, rgba_dev_or_null, h, w, S, F, format, out_dev, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

}  // extern "C"
