// Gaussian generators of the GAGAvatar head's identity side, forward only, exact fp32 ("Gaussian generators"): a
// stand-in for LinearGSGenerator, the two ConvGSGenerators, build_points_planes, the direction encoding and the assembly of _gs_params
// (app/GAGAvatar/models.py:65-87, 141-233, 236-252).  The two DINO features of one avatar come in, the avatar's N = V + 2 P^2
// Gaussians go out, in the arrays artalk_gaga_set_avatar takes.
//
// Every matrix product is one launch of the StyleUNet's exact-fp32 implicit-GEMM conv (styleunet.hip, launch_conv) with bias and,
// between layers, the plain ReLU of ConvArgs: the local generators' three 3 x 3 layers and their 1 x 1 layer at B = 1, H = W = P, every
// Linear of the global generator as a k = 1 conv at H = V, W = 1.  Around them:
//
//   gs_local_input_kernel    NCHW f_feature0 ++ direnc -> channels-last [P P][C + 27, padded to a multiple of 8] (once, read by both
//                            local generators)
//   gs_global_input_kernel   rows head_base[v] ++ f_feature1
//   gs_concat_dir_kernel     the V feature rows ++ direnc, padded likewise
//   gs_local_attr_kernel     the per-pixel activations of a local generator, the plane point of the pixel and xyz
//   gs_global_attr_kernel    the four column norms over V (one workgroup's work, fixed order), then the global generator's activations
//
// What depends on the avatar's transform (plane geometry, direction encoding) is worked out on the host in double and handed to the
// kernels by value, so a call enqueues on the caller's stream and never waits.  No atomics, nothing split over workgroups.
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

constexpr int GS_DIR = 27;          // sin and cos of 3 x 4 harmonics, then the direction itself
constexpr int GS_OUT = 41;          // colour 32 + opacity 1 + scale 3 + rotation 4 + position 1
constexpr int GS_HEAD = 128;        // hidden width of the global generator's attribute heads
constexpr float GS_SCALE = 0.05f, GS_EPS = 1e-12f;

struct GsDir { float v[GS_DIR]; };
// The planes of one avatar: origin = -R t, dir = R (0, 0, 1), dist = |origin . dir| (host, double, from the float32 matrix).
struct GsPlane { double origin[3], R[9], dist; float dir[3]; int P; };

// torch.linspace(1, -1, P, dtype = float32)[i]
__host__ __device__ inline float gs_linspace(int i, int P) {
    const float step = -2.0f / (float)(P - 1);
    return i < P / 2 ? 1.0f + step * (float)i : -1.0f - step * (float)(P - 1 - i);
}
// component c of plane_points[y P + x] = origin + dist R (u_x / 12, u_y / 12, 1): double, rounded once
__host__ __device__ inline float gs_plane_point(const GsPlane& pl, int x, int y, int c) {
    const double ux = (double)gs_linspace(x, pl.P) / 12.0, uy = (double)gs_linspace(y, pl.P) / 12.0;
    return (float)(pl.origin[c] + pl.dist * (pl.R[3 * c] * ux + pl.R[3 * c + 1] * uy + pl.R[3 * c + 2]));
}

// A concatenation with direnc is stored with its width padded to a multiple of 8 by zero channels (and the layer that reads it gets zero
// weight rows there), so that the conv takes its vector loads: at Cin = 283 the element-wise loads ran the first 3 x 3 layer at 47 TF/s
// against 76 TF/s for the two behind it.  The conv zero-fills a K chunk beyond Cin anyway and 16-wide chunks start where they did, so
// the padding changes no bit.
__host__ __device__ inline int gs_pad8(int c) { return (c + 7) & ~7; }

__device__ __forceinline__ float gs_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// f0 [C][PP], d -> out [PP][W], W = gs_pad8(C + 27): channels c < C from f0, then direnc, then zeros.  One workgroup moves a tile of
// 32 pixels x 32 channels through LDS, so that the reads (along the pixels) and the writes (along the channels) are both contiguous.
__global__ __launch_bounds__(256) void gs_local_input_kernel(const float* __restrict__ f0, const GsDir d, float* __restrict__ out, int C, int W, long PP) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long p0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j;
        const long p = p0 + tx;
        float v = 0.f;
        if (p < PP) {
            if (c < C) v = f0[(long)c * PP + p];
            else if (c < C + GS_DIR) v = d.v[c - C];
        }
        tile[j][tx] = v;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const long p = p0 + j;
        const int c = c0 + tx;
        if (p < PP && c < W) out[p * W + c] = tile[tx][j];
    }
}

// head_base [V][Dh], f1 [Dg] -> out [V][Dh + Dg]
__global__ __launch_bounds__(256) void gs_global_input_kernel(const float* __restrict__ head_base, const float* __restrict__ f1,
                                                              float* __restrict__ out, int V, int Dh, int Dg) {
    const int W = Dh + Dg;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)V * W) return;
    const int c = (int)(i % W);
    const long v = i / W;
    out[i] = c < Dh ? head_base[v * Dh + c] : f1[c - Dh];
}

// feat [V][H], d -> out [V][W], W = gs_pad8(H + 27): the features, then direnc, then zeros
__global__ __launch_bounds__(256) void gs_concat_dir_kernel(const float* __restrict__ feat, const GsDir d, float* __restrict__ out, int V, int H, int W) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)V * W) return;
    const int c = (int)(i % W);
    const long v = i / W;
    out[i] = c < H ? feat[v * H + c] : c < H + GS_DIR ? d.v[c - H] : 0.f;
}

// o [P P][41] -> the P P rows that start at the five output pointers; one thread per pixel.  The sigmoid of the colours follows the
// reference's colors[..., :3] on an NCHW tensor: all 32 channels of the pixels in columns x < 3, no channel elsewhere.
__global__ __launch_bounds__(256) void gs_local_attr_kernel(const float* __restrict__ o, const GsPlane pl, float sign, float* __restrict__ xyz,
                                                            float* __restrict__ colors, float* __restrict__ opacities,
                                                            float* __restrict__ scales, float* __restrict__ rotations) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)pl.P * pl.P) return;
    const int y = (int)(p / pl.P), x = (int)(p - (long)y * pl.P);
    const float* r = o + p * GS_OUT;
    const bool sg = x < 3;
    for (int c = 0; c < 32; ++c) { const float v = r[c]; colors[p * 32 + c] = sg ? gs_sigmoid(v) : v; }
    opacities[p] = gs_sigmoid(r[32]);
    for (int c = 0; c < 3; ++c) scales[p * 3 + c] = gs_sigmoid(r[33 + c]) * GS_SCALE;
    const float q0 = r[36], q1 = r[37], q2 = r[38], q3 = r[39];
    const float nrm = fmaxf(sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3), GS_EPS);
    rotations[p * 4] = q0 / nrm; rotations[p * 4 + 1] = q1 / nrm; rotations[p * 4 + 2] = q2 / nrm; rotations[p * 4 + 3] = q3 / nrm;
    const float pos = sign * gs_sigmoid(r[40]);
    for (int c = 0; c < 3; ++c) xyz[p * 3 + c] = gs_plane_point(pl, x, y, c) + pos * pl.dir[c];
}

// col [V][32], op [V], sc [V][3], rot [V][4] -> rows 0 .. V - 1 of the outputs.  The reference's F.normalize runs over dim 1 of a
// (1, V, 4) tensor: component c is divided by max(|column c over all V rows|, 1e-12).  The four norms are one workgroup's work - wave c
// sums column c, lane l the rows l, l + 64, ... in order, then a butterfly - and every workgroup of the grid repeats it (80 KB of reads
// at V = 5023) before it takes its share of the rows: the same order everywhere, hence the same bits, and no second launch.
__global__ __launch_bounds__(256) void gs_global_attr_kernel(const float* __restrict__ col, const float* __restrict__ op, const float* __restrict__ sc,
                                                             const float* __restrict__ rot, int V, float* __restrict__ xyz,
                                                             float* __restrict__ colors, float* __restrict__ opacities,
                                                             float* __restrict__ scales, float* __restrict__ rotations) {
    __shared__ float nrm[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float s = 0.f;
    for (int v = lane; v < V; v += 64) { const float q = rot[(long)v * 4 + wave]; s += q * q; }
    s = wave_sum(s);
    if (lane == 0) nrm[wave] = fmaxf(sqrtf(s), GS_EPS);
    __syncthreads();
    const long first = (long)blockIdx.x * 256 + t, step = (long)gridDim.x * 256;
    for (long i = first; i < (long)V * 32; i += step) { const float v = col[i]; colors[i] = (i & 31) < 3 ? gs_sigmoid(v) : v; }
    for (long i = first; i < (long)V * 4; i += step) rotations[i] = rot[i] / nrm[i & 3];
    for (long i = first; i < (long)V * 3; i += step) { scales[i] = gs_sigmoid(sc[i]) * GS_SCALE; xyz[i] = 0.f; }
    for (long i = first; i < V; i += step) opacities[i] = gs_sigmoid(op[i]);
}
static inline unsigned gs_global_attr_blocks(int V) { const int b = (V + 63) / 64; return (unsigned)(b > 128 ? 128 : b); }

static inline unsigned gs_blocks(long n) { return (unsigned)((n + 255) / 256); }

// the transform's part of a call: false for a matrix that is not finite
static bool gs_planes_setup(const float* T, int P, GsPlane* pl, GsDir* d) {
    double t[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) pl->R[3 * i + j] = (double)T[4 * i + j];
        t[i] = (double)T[4 * i + 3];
    }
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(T[i])) return false;
    double dot = 0.0;
    for (int i = 0; i < 3; ++i) {
        pl->origin[i] = -(pl->R[3 * i] * t[0] + pl->R[3 * i + 1] * t[1] + pl->R[3 * i + 2] * t[2]);
        pl->dir[i] = T[4 * i + 2];      // R (0, 0, 1): exact
        dot += pl->origin[i] * (double)pl->dir[i];
    }
    pl->dist = std::fabs(dot);
    pl->P = P;
    // HarmonicEmbedding(4), omega_0 = 1, logspace, append_input: sin(e) ++ cos(e) ++ dir with e = (dir_x 1, 2, 4, 8, dir_y 1, ...)
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 4; ++k) {
            const double e = (double)pl->dir[c] * (double)(1 << k);
            d->v[4 * c + k] = (float)std::sin(e);
            d->v[12 + 4 * c + k] = (float)std::cos(e);
        }
    for (int c = 0; c < 3; ++c) d->v[24 + c] = pl->dir[c];
    return true;
}

}  // namespace artalk

using namespace artalk;

namespace {

struct GsLayer { std::string name; const float* w = nullptr; const float* b = nullptr; int cin = 0, cinp = 0, cout = 0, k = 1; };      // cinp: cin as stored

}  // namespace

struct artalk_gsgen {
    int device = 0, V = 0, Dh = 0, Dg = 0, C = 0, P = 0, Hl = 0, Hc = 0;
    bool finalized = false, timing = false;
    WeightStore store;
    DevBuf<float> ws;
    int64_t ws_floats = 0;
    const float* head_base = nullptr;
    GsLayer feat[4], head[4][2], local[2][4];
    CallTimer timer;      // the call, and a pair of events per conv launch
    std::string err;
};

static thread_local std::string g_gs_error;

namespace {

const char* const kHeads[4] = {"color", "opacity", "scale", "rotation"};
const int kHeadOut[4] = {32, 1, 3, 4};

int gs_fail(artalk_gsgen* g, int rc, const std::string& msg) { g->err = msg; return rc; }

// k = 0: a Linear, whose weight is [cout][cin] in the state dict and runs as a 1 x 1 conv
void gs_add(artalk_gsgen* g, GsLayer& l, const std::string& name, int cin, int cout, int k) {
    l.name = name; l.cin = cin; l.cinp = cin; l.cout = cout; l.k = k ? k : 1;
    if (k == 0) g->store.declare(name + ".weight", {cout, cin});
    else g->store.declare(name + ".weight", {cout, cin, k, k});
    g->store.declare(name + ".bias", {cout});
}

// keys in the order of the reference module's state_dict()
void gs_manifest(artalk_gsgen* g) {
    g->store.declare("head_base", {g->V, g->Dh});
    const std::string gg = "gs_generator_g.";
    for (int i = 0; i < 4; ++i) gs_add(g, g->feat[i], gg + "feature_layers." + std::to_string(2 * i), i ? g->Hl : g->Dh + g->Dg, g->Hl, 0);
    for (int h = 0; h < 4; ++h) {
        gs_add(g, g->head[h][0], gg + kHeads[h] + "_layers.0", g->Hl + GS_DIR, GS_HEAD, 0);
        g->head[h][0].cinp = gs_pad8(g->Hl + GS_DIR);
        gs_add(g, g->head[h][1], gg + kHeads[h] + "_layers.2", GS_HEAD, kHeadOut[h], 0);
    }
    for (int l = 0; l < 2; ++l) {
        const std::string n = "gs_generator_l" + std::to_string(l) + ".gaussian_conv.";
        gs_add(g, g->local[l][0], n + "0", g->C + GS_DIR, g->Hc, 3);
        g->local[l][0].cinp = gs_pad8(g->C + GS_DIR);
        gs_add(g, g->local[l][1], n + "2", g->Hc, g->Hc, 3);
        gs_add(g, g->local[l][2], n + "4", g->Hc, g->Hc, 3);
        gs_add(g, g->local[l][3], n + "6", g->Hc, GS_OUT, 1);
    }
}

// The workspace, in floats, every block 16-byte aligned (the conv's vector loads).
struct GsWs : WsLayout {
    int64_t xin, a, b, o, gin, ga, gb, gcat, gh, hout[4];
    explicit GsWs(const artalk_gsgen* g) {
        const int64_t PP = (int64_t)g->P * g->P, V = g->V;
        xin = take(PP * gs_pad8(g->C + GS_DIR)); a = take(PP * g->Hc); b = take(PP * g->Hc); o = take(PP * GS_OUT);
        gin = take(V * (g->Dh + g->Dg)); ga = take(V * g->Hl); gb = take(V * g->Hl); gcat = take(V * gs_pad8(g->Hl + GS_DIR)); gh = take(V * GS_HEAD);
        for (int h = 0; h < 4; ++h) hout[h] = take(V * kHeadOut[h]);
    }
};

struct GsRun {
    artalk_gsgen* g; hipStream_t s;
    void conv(const GsLayer& l, const float* x, float* out, int H, int W, int relu) {
        ConvArgs a{};
        a.x = x; a.x_bstride = (long)H * W * l.cinp; a.w = l.w; a.out = out; a.B = 1; a.H = H; a.W = W; a.Cin = l.cinp; a.Cout = l.cout; a.k = l.k;
        a.gain = 1.f; a.bias = l.b; a.relu = relu;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        g->timer.pair(&e0, &e1);
        launch_conv(a, s, e0, e1);
    }
    void run(const float* f0, const float* f1, const GsPlane& pl, const GsDir& d, float* xyz, float* colors, float* opacities, float* scales,
             float* rotations) {
        const GsWs w(g);
        float* base = g->ws.get();
        const int P = g->P, V = g->V;
        const long PP = (long)P * P;
        // ---- local generators: rows V + l P P ..
        const int Wl = gs_pad8(g->C + GS_DIR), Wg = gs_pad8(g->Hl + GS_DIR);
        ARTALK_LAUNCH(gs_local_input_kernel, dim3((unsigned)((PP + 31) / 32), (unsigned)((Wl + 31) / 32)), dim3(256), 0, s, f0, d, base + w.xin, g->C, Wl, PP);
        for (int l = 0; l < 2; ++l) {
            conv(g->local[l][0], base + w.xin, base + w.a, P, P, 1);
            conv(g->local[l][1], base + w.a, base + w.b, P, P, 1);
            conv(g->local[l][2], base + w.b, base + w.a, P, P, 1);
            conv(g->local[l][3], base + w.a, base + w.o, P, P, 0);
            const long r0 = V + l * PP;
            ARTALK_LAUNCH(gs_local_attr_kernel, dim3(gs_blocks(PP)), dim3(256), 0, s, base + w.o, pl, l ? -1.f : 1.f, xyz + r0 * 3, colors + r0 * 32,
                          opacities + r0, scales + r0 * 3, rotations + r0 * 4);
        }
        // ---- global generator: rows 0 .. V - 1
        ARTALK_LAUNCH(gs_global_input_kernel, dim3(gs_blocks((long)V * (g->Dh + g->Dg))), dim3(256), 0, s, g->head_base, f1, base + w.gin, V, g->Dh,
                      g->Dg);
        conv(g->feat[0], base + w.gin, base + w.ga, V, 1, 1);
        conv(g->feat[1], base + w.ga, base + w.gb, V, 1, 1);
        conv(g->feat[2], base + w.gb, base + w.ga, V, 1, 1);
        conv(g->feat[3], base + w.ga, base + w.gb, V, 1, 0);
        ARTALK_LAUNCH(gs_concat_dir_kernel, dim3(gs_blocks((long)V * Wg)), dim3(256), 0, s, base + w.gb, d, base + w.gcat, V, g->Hl, Wg);
        for (int h = 0; h < 4; ++h) {
            conv(g->head[h][0], base + w.gcat, base + w.gh, V, 1, 1);
            conv(g->head[h][1], base + w.gh, base + w.hout[h], V, 1, 0);
        }
        ARTALK_LAUNCH(gs_global_attr_kernel, dim3(gs_global_attr_blocks(V)), dim3(256), 0, s, base + w.hout[0], base + w.hout[1], base + w.hout[2], base + w.hout[3], V, xyz,
                      colors, opacities, scales, rotations);
    }
};

}  // namespace

extern "C" {

const char* artalk_gsgen_last_error(const artalk_gsgen* g) { return g ? g->err.c_str() : g_gs_error.c_str(); }

void artalk_gsgen_destroy(artalk_gsgen* g) {
    if (!g) return;
    if (g->store.on_device() || !g->timer.empty()) {      // (else nothing was ever taken from the device)
        (void)hipSetDevice(g->device);
        (void)hipDeviceSynchronize();
    }
    delete g;
}

int artalk_gsgen_create(int device_id, int V, int Dh, int Dg, int C, int P, artalk_gsgen** out) {
    if (!out) { g_gs_error = "out is NULL"; return ARTALK_EINVAL; }
    if (device_id < 0) { g_gs_error = "device_id must not be negative"; return ARTALK_EINVAL; }
    if (V < 1 || V > (1 << 22)) { g_gs_error = "V must be in 1..4194304"; return ARTALK_EINVAL; }
    if (Dh < 1 || Dh > 16384 || Dg < 1 || Dg > 16384) { g_gs_error = "Dh and Dg must be in 1..16384"; return ARTALK_EINVAL; }
    if ((Dh + Dg) % 4 != 0) { g_gs_error = "Dh + Dg must be a multiple of 4 (the hidden width is a quarter of it)"; return ARTALK_EINVAL; }
    if (C < 2 || C > 4096 || (C & 1)) { g_gs_error = "C must be even and in 2..4096 (the hidden width is half of it)"; return ARTALK_EINVAL; }
    if (P < 3 || P > 4096) { g_gs_error = "P must be in 3..4096"; return ARTALK_EINVAL; }
    artalk_gsgen* g = new artalk_gsgen();
    g->device = device_id; g->V = V; g->Dh = Dh; g->Dg = Dg; g->C = C; g->P = P; g->Hl = (Dh + Dg) / 4; g->Hc = C / 2;
    gs_manifest(g);
    g->ws_floats = GsWs(g).off;
    *out = g;
    return ARTALK_OK;
}

int artalk_gsgen_set_tensor(artalk_gsgen* g, const char* key, const void* host_ptr, int ndim, const int64_t* shape) {
    if (!g) { g_gs_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (!key || !host_ptr || !shape) return gs_fail(g, ARTALK_EINVAL, "key, host_ptr and shape must not be NULL");
    if (g->finalized) return gs_fail(g, ARTALK_ESTATE, "weights are final after artalk_gsgen_finalize; create a new handle");
    return g->store.set(key, host_ptr, ndim, shape, &g->err);
}

int artalk_gsgen_finalize(artalk_gsgen* g) {
    if (!g) { g_gs_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (g->finalized) return gs_fail(g, ARTALK_ESTATE, "artalk_gsgen_finalize was already called");
    if (g->store.missing(&g->err)) return ARTALK_EMISSING;
    if (hipSetDevice(g->device) != hipSuccess) return gs_fail(g, ARTALK_EHIP, "hipSetDevice failed");
    WeightStore& st = g->store;
    auto pack = [&](GsLayer& l) {
        l.w = st.upload(pack_conv_weight(st.host(l.name + ".weight"), l.cout, l.cin, l.cinp, l.k));
        l.b = st.upload(l.name + ".bias");
    };
    g->head_base = st.upload("head_base");
    for (GsLayer& l : g->feat) pack(l);
    for (auto& h : g->head) for (GsLayer& l : h) pack(l);
    for (auto& lg : g->local) for (GsLayer& l : lg) pack(l);
    if (st.ok() && !g->ws.alloc((size_t)g->ws_floats))
        return gs_fail(g, ARTALK_EHIP, "hipMalloc of the workspace failed (" + std::to_string(g->ws_floats * 4) + " bytes)");
    if (!st.ok() || hipDeviceSynchronize() != hipSuccess) return gs_fail(g, ARTALK_EHIP, "uploading the weights failed");
    st.release_host();
    g->finalized = true;
    return ARTALK_OK;
}

int artalk_gsgen_dims(const artalk_gsgen* g, int* V, int* Dh, int* Dg, int* C, int* P, int* finalized) {
    if (!g) { g_gs_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (V) *V = g->V;
    if (Dh) *Dh = g->Dh;
    if (Dg) *Dg = g->Dg;
    if (C) *C = g->C;
    if (P) *P = g->P;
    if (finalized) *finalized = g->finalized ? 1 : 0;
    return g->device;
}

int artalk_gsgen_set_timing(artalk_gsgen* g, int enable) {
    if (!g) { g_gs_error = "handle is NULL"; return ARTALK_EINVAL; }
    g->timing = enable != 0;
    return ARTALK_OK;
}

int artalk_gsgen_get_timing(const artalk_gsgen* g, double* conv_ms, double* total_ms) {
    if (!g) { g_gs_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (conv_ms) *conv_ms = g->timer.pairs_ms();
    if (total_ms) *total_ms = g->timer.total_ms();
    return ARTALK_OK;
}

int artalk_gsgen_planes(const float* transform_3x4_host, int P, float* points_out, float* dir_out, float* direnc_out) {
    if (!transform_3x4_host) { g_gs_error = "transform must not be NULL"; return ARTALK_EINVAL; }
    if (P < 3 || P > 4096) { g_gs_error = "P must be in 3..4096"; return ARTALK_EINVAL; }
    GsPlane pl; GsDir d;
    if (!gs_planes_setup(transform_3x4_host, P, &pl, &d)) { g_gs_error = "transform holds a value that is not finite"; return ARTALK_EINVAL; }
    if (points_out)
        for (int y = 0; y < P; ++y)
            for (int x = 0; x < P; ++x)
                for (int c = 0; c < 3; ++c) points_out[((size_t)y * P + x) * 3 + c] = gs_plane_point(pl, x, y, c);
    if (dir_out) for (int c = 0; c < 3; ++c) dir_out[c] = pl.dir[c];
    if (direnc_out) for (int c = 0; c < GS_DIR; ++c) direnc_out[c] = d.v[c];
    return ARTALK_OK;
}

int artalk_gsgen_generate(artalk_gsgen* g, const float* feature0_dev, const float* feature1_dev, const float* transform_3x4_host, float* xyz_dev,
                          float* colors_dev, float* opacities_dev, float* scales_dev, float* rotations_dev, void* stream) {
    if (!g) { g_gs_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (!g->finalized) return gs_fail(g, ARTALK_ESTATE, "artalk_gsgen_generate before artalk_gsgen_finalize");
    if (!feature0_dev || !feature1_dev) return gs_fail(g, ARTALK_EINVAL, "feature0 and feature1 must not be NULL");
    if (!transform_3x4_host) return gs_fail(g, ARTALK_EINVAL, "transform must not be NULL");
    if (!xyz_dev || !colors_dev || !opacities_dev || !scales_dev || !rotations_dev)
        return gs_fail(g, ARTALK_EINVAL, "xyz, colors, opacities, scales and rotations must not be NULL");
    GsPlane pl; GsDir d;
    if (!gs_planes_setup(transform_3x4_host, g->P, &pl, &d)) return gs_fail(g, ARTALK_EINVAL, "transform holds a value that is not finite");
    (void)hipSetDevice(g->device);
    hipStream_t s = (hipStream_t)stream;
    if (!g->timer.begin(s, g->timing)) return gs_fail(g, ARTALK_EHIP, "hipEventCreate failed");
    GsRun run{g, s};
    run.run(feature0_dev, feature1_dev, pl, d, xyz_dev, colors_dev, opacities_dev, scales_dev, rotations_dev);
    if (hipGetLastError() != hipSuccess) return gs_fail(g, ARTALK_EHIP, "kernel launch failed");
    if (!g->timer.end()) return gs_fail(g, ARTALK_EHIP, "the call failed on the device");
    return ARTALK_OK;
}

// ---- single kernels ----
int artalk_op_conv2d_relu(const float* x, int64_t x_bstride, const float* w, float* out, int B, int H, int W, int Cin, int Cout, int k,
                          const float* bias, int relu, void* stream) {
    if (!x || !w || !out) return ARTALK_EINVAL;
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (k != 1 && k != 3)) return ARTALK_EINVAL;
    if ((int64_t)B * H * W > (int64_t)1 << 30 || (int64_t)H * W > INT_MAX) return ARTALK_EINVAL;
    if (x_bstride != 0 && x_bstride < (int64_t)H * W * Cin) return ARTALK_EINVAL;
    ConvArgs a{};
    a.x = x; a.x_bstride = x_bstride; a.w = w; a.out = out; a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.k = k;
    a.in_scale_ld = Cin; a.gain = 1.f; a.bias = bias; a.relu = relu != 0;
    launch_conv(a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gs_local_input(const float* feature0_dev, const float* direnc_host, float* out_dev, int C, int P, void* stream) {
    if (!feature0_dev || !direnc_host || !out_dev || C < 1 || C > 4096 || P < 1 || P > 4096) return ARTALK_EINVAL;
    GsDir d;
    for (int c = 0; c < GS_DIR; ++c) d.v[c] = direnc_host[c];
    const long PP = (long)P * P;
    const int W = gs_pad8(C + GS_DIR);
    ARTALK_LAUNCH(gs_local_input_kernel, dim3((unsigned)((PP + 31) / 32), (unsigned)((W + 31) / 32)), dim3(256), 0, (hipStream_t)stream, feature0_dev, d,
                  out_dev, C, W, PP);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gs_global_input(const float* head_base_dev, const float* feature1_dev, float* out_dev, int V, int Dh, int Dg, void* stream) {
    if (!head_base_dev || !feature1_dev || !out_dev || V < 1 || V > (1 << 22) || Dh < 1 || Dh > 16384 || Dg < 1 || Dg > 16384) return ARTALK_EINVAL;
    ARTALK_LAUNCH(gs_global_input_kernel, dim3(gs_blocks((long)V * (Dh + Dg))), dim3(256), 0, (hipStream_t)stream, head_base_dev, feature1_dev, out_dev,
                  V, Dh, Dg);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gs_concat_dir(const float* feat_dev, const float* direnc_host, float* out_dev, int V, int H, void* stream) {
    if (!feat_dev || !direnc_host || !out_dev || V < 1 || V > (1 << 22) || H < 1 || H > 16384) return ARTALK_EINVAL;
    GsDir d;
    for (int c = 0; c < GS_DIR; ++c) d.v[c] = direnc_host[c];
    const int W = gs_pad8(H + GS_DIR);
    ARTALK_LAUNCH(gs_concat_dir_kernel, dim3(gs_blocks((long)V * W)), dim3(256), 0, (hipStream_t)stream, feat_dev, d, out_dev, V, H, W);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gs_local_attr(const float* conv_out_dev, const float* transform_3x4_host, int P, int sign, int64_t row0, float* xyz_dev,
                            float* colors_dev, float* opacities_dev, float* scales_dev, float* rotations_dev, void* stream) {
    if (!conv_out_dev || !transform_3x4_host || !xyz_dev || !colors_dev || !opacities_dev || !scales_dev || !rotations_dev) return ARTALK_EINVAL;
    if (P < 3 || P > 4096 || (sign != 1 && sign != -1) || row0 < 0 || row0 > ((int64_t)1 << 32)) return ARTALK_EINVAL;
    GsPlane pl; GsDir d;
    if (!gs_planes_setup(transform_3x4_host, P, &pl, &d)) return ARTALK_EINVAL;
    ARTALK_LAUNCH(gs_local_attr_kernel, dim3(gs_blocks((long)P * P)), dim3(256), 0, (hipStream_t)stream, conv_out_dev, pl, (float)sign,
                  xyz_dev + row0 * 3, colors_dev + row0 * 32, opacities_dev + row0, scales_dev + row0 * 3, rotations_dev + row0 * 4);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gs_global_attr(const float* colors_in_dev, const float* opacities_in_dev, const float* scales_in_dev, const float* rotations_in_dev,
                             int V, float* xyz_dev, float* colors_dev, float* opacities_dev, float* scales_dev, float* rotations_dev, void* stream) {
    if (!colors_in_dev || !opacities_in_dev || !scales_in_dev || !rotations_in_dev) return ARTALK_EINVAL;
    if (!xyz_dev || !colors_dev || !opacities_dev || !scales_dev || !rotations_dev || V < 1 || V > (1 << 22)) return ARTALK_EINVAL;
    ARTALK_LAUNCH(gs_global_attr_kernel, dim3(gs_global_attr_blocks(V)), dim3(256), 0, (hipStream_t)stream, colors_in_dev, opacities_in_dev, scales_in_dev,
                  rotations_in_dev, V, xyz_dev, colors_dev, opacities_dev, scales_dev, rotations_dev);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

}  // extern "C"
