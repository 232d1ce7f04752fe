// The per-frame path of the GAGAvatar head ("GAGAvatar head"): motion codes -> RGB frames.  A stand-in for
// GAGAvatar.build_forward_batch + forward_expression (reference app/GAGAvatar/models.py:63-138) on top of the three pieces that exist
// already: FLAME skinning (flame.hip), the 32-channel splat rasteriser (splat.hip) and the StyleUNet upsampler (styleunet.hip).
//
//   gaga_flame_inputs_kernel   motion rows -> the betas and full_pose arrays artalk_flame_verts takes           (models.py:114-119)
//   gaga_forehead_kernel       EMA over frames of K listed vertices; its state outlives the call               (models.py:120-125)
//   gaga_means_kernel          per-frame Gaussian centres: V skinned vertices, then the avatar's static points (models.py:90)
//   gaga_finish_kernel         clamp(0, 1) and the watermark blend, in place                                   (models.py:95, 131-138)
//   gaga_gather_codes_kernel   the head-rotation codes of the listed rows, packed for the one copy to the host (stream calls only)
//   (frames.hip)               the same clamp and blend fused with the packing into 8-bit frames, for artalk_gaga_render_u8
//   artalk_gaga_cameras        host only: head-rotation codes -> the view / projection matrices the rasteriser reads (models.py:127)
// One path serves the classic call and live streams ("Live streams through the head"), where avatars stay resident
// in a pool of slots, every stream has an EMA state of its own and every frame names its motion row, its stream and its slot.  The first
// three kernels take those names as lists, and a null list means identity, as SplatAttrs::sets does in splat.hip: frame t reads motion
// row t and slot 0, and the forehead launch is one entry over frames 0 .. n-1 on row 0 of the state it is given.  That is the classic
// call: its avatar is a set of one slot, its state a pool of one row, and it builds and uploads no list.
//
// All fp32 and element-wise (no reductions, no atomics): bit-identical from run to run.  The EMA and the blend use torch's rounding
// order - every product and sum rounded on its own, never contracted to an FMA - so they equal the torch statements bit for bit.
// hipcc contracts a * b + c by default and HIP's __fmul_rn / __fadd_rn are plain operators that contract like any other, so the two
// kernels switch contraction off for their bodies (#pragma clang fp contract(off)).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "artalk_hip.h"
#include "common.h"
#include "device_mem.h"
#include "kernels.h"

namespace artalk {

constexpr int kGagaMotion = 106;      // a motion row: 100 expression, 3 head rotation, 3 jaw
constexpr int kGagaCh = 32;           // channels of the splat image
constexpr int kForeheadDefault = 68;
// the vertices the reference smooths (models.py:326-331): 68 distinct FLAME vertex ids, the largest 3913
static const int32_t kForeheadIdx[kForeheadDefault] = {
    2168, 2165, 3068, 2199, 2196, 3720, 2091, 2088, 3524, 625,  628,  3871, 705,  708,  2030, 667,  670,
    3708, 3706, 3729, 3721, 3773, 3789, 3735, 3732, 3786, 3876, 3878, 3913, 3899, 3872, 3874, 3864, 3865,
    3158, 3157, 336,  335,  3153, 3705, 2177, 2176, 3540, 671,  672,  3863, 2134, 16,   17,   2138, 2139,
    2567, 2566, 337,  338,  3154, 3712, 2178, 2179, 3495, 674,  673,  3868, 2135, 27,   18,   1429, 1430};

// one thread per (frame, column) of betas ++ full_pose: betas = shapecode ++ m[0:100]; full_pose = (0 x 6 | m[103:106] | 0 x 6).
// Frame t reads motion row rows[t] (null: t) and the shapecode of slot slots[t] (null: 0) of shape [slots][NS]
__global__ void gaga_flame_inputs_kernel(const float* __restrict__ motion, long stride, const int64_t* __restrict__ rows,
                                         const int32_t* __restrict__ slots, const float* __restrict__ shape, int NS,
                                         float* __restrict__ betas, float* __restrict__ pose, int T) {
    const int NB = NS + 100, W = NB + 15;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)T * W) return;
    const int t = (int)(idx / W), c = (int)(idx - (long)t * W);
    const float* m = motion + (rows ? (long)rows[t] : (long)t) * stride;
    if (c < NB) {
        betas[(long)t * NB + c] = c < NS ? shape[(slots ? (long)slots[t] : 0L) * NS + c] : m[c - NS];
    } else {
        const int p = c - NB;
        pose[(long)t * 15 + p] = (p >= 6 && p < 9) ? m[103 + (p - 6)] : 0.f;
    }
}

// Workgroup e serves one entry: its state and flag are row pool_row[e] of state_pool [rows][K][3] / flag_pool [rows] (flag != 0: the
// state is set), its frames are frames[off[e] .. off[e + 1]) - indices into verts [..][V][3], each at most once, walked in this order.
// With the three lists null the launch has one entry: row 0, frames 0 .. n-1.  Thread i owns coordinate i % 3 of listed vertex i / 3:
// unset state: state = cur (that frame is left as it is); otherwise state = 0.98 state + 0.02 cur, written back into the vertex.  State
// and flag are read at the start and written at the end; an entry without frames keeps both.  No two workgroups share a row or a frame,
// so nothing crosses a workgroup.  An entry's loads do not depend on the recurrence, only its stores do: they are issued eight frames
// ahead (a frame is listed once, so no store reaches a later load).
constexpr int kForeheadAhead = 8;
// one entry's walk over its n frames, the j-th of them frame_of(j) of verts: the one statement of the recurrence
template <typename FrameOf>
__device__ __forceinline__ void gaga_forehead_walk(float* __restrict__ verts, const int32_t* __restrict__ index, int K, int V, int n,
                                                   float* __restrict__ state, bool was_set, FrameOf frame_of) {
#pragma clang fp contract(off)
    const long per = (long)V * 3;
    for (int i = threadIdx.x; i < K * 3; i += blockDim.x) {
        const int k = i / 3, c = i - k * 3;
        float* p = verts + (long)index[k] * 3 + c;
        float s = state[i];
        bool set = was_set;
        for (int j0 = 0; j0 < n; j0 += kForeheadAhead) {
            float cur[kForeheadAhead];
            long at[kForeheadAhead];
#pragma unroll
            for (int u = 0; u < kForeheadAhead; ++u) {      // past the end: the last frame once more, loaded and not used - no branch before a load
                at[u] = (long)frame_of(min(j0 + u, n - 1)) * per;
                cur[u] = p[at[u]];
            }
#pragma unroll
            for (int u = 0; u < kForeheadAhead; ++u) {
                if (j0 + u >= n) break;
                if (!set) { s = cur[u]; set = true; }
                else { s = 0.98f * s + 0.02f * cur[u]; p[at[u]] = s; }
            }
        }
        state[i] = s;
    }
}
__global__ __launch_bounds__(256) void gaga_forehead_kernel(float* __restrict__ verts, const int32_t* __restrict__ index, int K, int V, int n_frames,
                                                            const int32_t* __restrict__ pool_row, const int32_t* __restrict__ off,
                                                            const int32_t* __restrict__ frames, float* __restrict__ state_pool,
                                                            int* __restrict__ flag_pool) {
    const int e = blockIdx.x;
    const int begin = off ? off[e] : 0, n = off ? off[e + 1] - begin : n_frames;
    if (n <= 0) return;      // (the whole workgroup)
    const long row = pool_row ? pool_row[e] : 0;
    const bool was_set = flag_pool[row] != 0;
    __syncthreads();      // every thread has read the flag before thread 0 writes it
    float* state = state_pool + row * K * 3;
    // the null test stays out of the walk: a select per frame would put a branch before every load and undo the load-ahead
    if (frames) {
        const int32_t* fr = frames + begin;
        gaga_forehead_walk(verts, index, K, V, n, state, was_set, [fr](int j) { return fr[j]; });
    } else {
        gaga_forehead_walk(verts, index, K, V, n, state, was_set, [](int j) { return j; });
    }
    if (threadIdx.x == 0 && K > 0) flag_pool[row] = 1;
}

// means [F][N][3]: rows 0 .. V-1 from the frame's vertices, rows V .. N-1 from slot slots[f] (null: 0) of xyz [slots][N][3]
__global__ void gaga_means_kernel(const float* __restrict__ verts, const float* __restrict__ xyz, const int32_t* __restrict__ slots,
                                  float* __restrict__ means, int F, int V, int N) {
    const long per = (long)N * 3, e = (long)blockIdx.x * blockDim.x + threadIdx.x;      // grid: x over a frame's elements, y over frames
    if (e >= per) return;
    for (int f = blockIdx.y; f < F; f += gridDim.y)
        means[f * per + e] = e < (long)V * 3 ? verts[(long)f * V * 3 + e] : xyz[(slots ? (long)slots[f] : 0L) * per + e];
}

// in place on img [F][3][S][S]: clamp(0, 1); on the bottom-right h x w patch a = alpha * 0.8, p = p * (1 - a) + rgb * a.
// wm [4][h][w] (r, g, b, alpha) or null
__global__ void gaga_finish_kernel(float* __restrict__ img, const float* __restrict__ wm, int h, int w, int S, int F) {
#pragma clang fp contract(off)
    const long SS = (long)S * S, idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)F * 3 * SS) return;
    float v = fminf(fmaxf(img[idx], 0.f), 1.f);
    if (wm) {
        const long pix = idx % SS;
        const int c = (int)((idx / SS) % 3);
        const int y = (int)(pix / S) - (S - h), x = (int)(pix % S) - (S - w);
        if (y >= 0 && x >= 0) {
            const float a = wm[(3L * h + y) * w + x] * 0.8f;
            v = v * (1.f - a) + wm[((long)c * h + y) * w + x] * a;
        }
    }
    img[idx] = v;
}

// codes [T][3] = motion[rows[t]][100:103]
__global__ void gaga_gather_codes_kernel(const float* __restrict__ motion, long stride, const int64_t* __restrict__ rows, float* __restrict__ codes,
                                         int T) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * 3) return;
    const int t = idx / 3;
    codes[idx] = motion[(long)rows[t] * stride + 100 + (idx - t * 3)];
}

static inline unsigned gaga_blocks(long n) { return (unsigned)((n + 255) / 256); }

static void launch_gaga_flame_inputs(const float* motion, long stride, const int64_t* rows, const int32_t* slots, const float* shape, int NS,
                                     float* betas, float* pose, int T, hipStream_t s) {
    ARTALK_LAUNCH(gaga_flame_inputs_kernel, dim3(gaga_blocks((long)T * (NS + 115))), dim3(256), 0, s, motion, stride, rows, slots, shape, NS, betas,
                  pose, T);
}
// `entries` workgroups over the CSR (pool_row, off, frames); all three null: one entry, n_frames frames in order on row 0
static void launch_gaga_forehead(float* verts, const int32_t* index, int K, int V, int entries, int n_frames, const int32_t* pool_row,
                                 const int32_t* off, const int32_t* frames, float* state_pool, int* flag_pool, hipStream_t s) {
    ARTALK_LAUNCH(gaga_forehead_kernel, dim3(entries), dim3(256), 0, s, verts, index, K, V, n_frames, pool_row, off, frames, state_pool, flag_pool);
}
static void launch_gaga_means(const float* verts, const float* xyz, const int32_t* slots, float* means, int F, int V, int N, hipStream_t s) {
    ARTALK_LAUNCH(gaga_means_kernel, dim3(gaga_blocks((long)N * 3), F < 65535 ? F : 65535), dim3(256), 0, s, verts, xyz, slots, means, F, V, N);
}
static void launch_gaga_finish(float* img, const float* wm, int h, int w, int S, int F, hipStream_t s) {
    ARTALK_LAUNCH(gaga_finish_kernel, dim3(gaga_blocks((long)F * 3 * S * S)), dim3(256), 0, s, img, wm, h, w, S, F);
}

// ---- the host checks every entry point applies before the device is touched (artalk_op_gaga_check exposes them to the CPU tests)
static int check_avatar(int V, int N, std::string* err) {
    if (N < V) { *err = "N (" + std::to_string(N) + ") must be at least V (" + std::to_string(V) + "): the first V Gaussians ride on the vertices"; return ARTALK_EINVAL; }
    return ARTALK_OK;
}
static int check_forehead(int V, const int32_t* index, int K, std::string* err) {
    if (K < 0) { *err = "K must not be negative"; return ARTALK_EINVAL; }
    if (K > 0 && !index) { *err = "idx is NULL"; return ARTALK_EINVAL; }
    std::vector<char> seen((size_t)(V > 0 ? V : 0), 0);
    for (int k = 0; k < K; ++k) {
        if (index[k] < 0 || index[k] >= V) { *err = "forehead index " + std::to_string(index[k]) + " is outside [0, V = " + std::to_string(V) + ")"; return ARTALK_EINVAL; }
        if (seen[index[k]]) { *err = "forehead index " + std::to_string(index[k]) + " is listed twice"; return ARTALK_EINVAL; }
        seen[index[k]] = 1;
    }
    return ARTALK_OK;
}
static int check_watermark(int S, int h, int w, std::string* err) {
    if (h < 1 || w < 1 || h > S || w > S) {
        *err = "a watermark of " + std::to_string(h) + " x " + std::to_string(w) + " does not fit the " + std::to_string(S) + " x " + std::to_string(S) + " image";
        return ARTALK_EINVAL;
    }
    return ARTALK_OK;
}
static int check_render(int T, int64_t motion_stride, bool have_avatar, bool finalized, std::string* err) {
    if (T < 0) { *err = "T must not be negative"; return ARTALK_EINVAL; }
    if (motion_stride < kGagaMotion) { *err = "motion_stride must be at least 106"; return ARTALK_EINVAL; }
    if (!have_avatar) { *err = "no avatar set: call artalk_gaga_set_avatar first"; return ARTALK_EINVAL; }
    if (!finalized) { *err = "the upsampler is not finalized (artalk_styleunet_finalize)"; return ARTALK_ESTATE; }
    return ARTALK_OK;
}

// the frame lists of artalk_gaga_render_streams against the streams (open[id] != 0: open) and the slots (filled[slot] != 0: occupied)
static int check_frames(int T, const int64_t* row, const int32_t* stream, const int32_t* slot, const uint8_t* open, int n_ids,
                        const uint8_t* filled, int n_slots, std::string* err) {
    if (T < 0) { *err = "T must not be negative"; return ARTALK_EINVAL; }
    if (!row || !stream || !slot) { *err = "frame_row, frame_stream and frame_slot must not be NULL"; return ARTALK_EINVAL; }
    for (int t = 0; t < T; ++t) {
        const std::string f = "frame " + std::to_string(t);
        if (row[t] < 0) { *err = f + ": motion row " + std::to_string(row[t]) + " is negative"; return ARTALK_EINVAL; }
        if (stream[t] < 0 || stream[t] >= n_ids) { *err = f + ": stream " + std::to_string(stream[t]) + " was never opened"; return ARTALK_EINVAL; }
        if (!open || !open[stream[t]]) { *err = f + ": stream " + std::to_string(stream[t]) + " is closed"; return ARTALK_EINVAL; }
        if (slot[t] < 0 || slot[t] >= n_slots) {
            *err = f + ": slot " + std::to_string(slot[t]) + " is outside the pool's [0, " + std::to_string(n_slots) + ")";
            return ARTALK_EINVAL;
        }
        if (!filled || !filled[slot[t]]) { *err = f + ": slot " + std::to_string(slot[t]) + " is empty (artalk_gaga_pool_set)"; return ARTALK_EINVAL; }
    }
    return ARTALK_OK;
}
static int check_pool(int V, int slots, int N, std::string* err) {
    if (slots < 1 || slots > 4096) { *err = "slots must be in 1..4096"; return ARTALK_EINVAL; }
    return check_avatar(V, N, err);
}

}  // namespace artalk

using namespace artalk;

namespace {
enum { kGagaInputsFlame, kGagaForeheadMeans, kGagaSplat, kGagaUpsampler, kGagaFinish, kGagaStages };

// An avatar set: `slots` avatars of N Gaussians each, one device slab per attribute ([slots][N][..], shape [slots][NB - 100]).  Which
// slots hold an avatar, and their [R | t], stay on the host, where the cameras are built.
struct GagaSet {
    int slots = 0, N = 0;
    DevBuf<float> xyz, colors, opac, scales, rots, shape;
    std::vector<uint8_t> filled;       // [slots]
    std::vector<float> transform;      // [slots][12]
    bool has(int slot) const { return slot >= 0 && slot < slots && filled[(size_t)slot]; }
    void drop() {
        slots = N = 0;
        filled.clear(); transform.clear();
        for (DevBuf<float>* b : {&xyz, &colors, &opac, &scales, &rots, &shape}) b->reset();
    }
};

// A state pool of the forehead EMA: state [rows][K][3] and flag [rows] (!= 0: the row's state is set)
struct GagaStates {
    int rows = 0;
    DevBuf<float> state;
    DevBuf<int> flag;
    void drop() { rows = 0; state.reset(); flag.reset(); }
};
}  // namespace

struct artalk_gaga {
    int device = 0, V = 0, NB = 0, S = 0, num_layers = 0;
    artalk_flame* flame = nullptr;
    artalk_splat* splat = nullptr;
    artalk_styleunet* unet = nullptr;
    // the classic call's avatar (artalk_gaga_set_avatar), a set of one slot, and the resident avatars (artalk_gaga_pool_*)
    GagaSet avatar, pool;
    // forehead EMA: the listed vertices; the classic call's state, a pool of one row, and the streams', one row per open stream.  The
    // two are separate objects: a classic call never touches a stream's row, nor a stream call the classic row
    int K = 0;
    DevBuf<int32_t> index;
    GagaStates classic, streams;
    // live streams: stream_open[id] / stream_row[id] for every id ever handed out (ids are not reused, rows are)
    std::vector<uint8_t> stream_open;
    std::vector<int32_t> stream_row;
    int streams_open = 0;
    // the frame lists of one artalk_gaga_render_streams call, on their way to the device
    PinnedBuf<char> plan_host;
    DevBuf<char> plan_dev;
    DevBuf<float> codes_dev;     // [frames][3]
    // watermark
    DevBuf<float> wm;
    int wm_h = 0, wm_w = 0;
    // scratch of one slab
    int slab_req = 0, cap_frames = 0, cap_N = 0;
    DevBuf<float> betas, pose, verts, means, img;
    DevBuf<int32_t> radii;
    PinnedBuf<float> codes_host;      // [frames][3]
    // 8-bit frames out (artalk_gaga_render_u8): the upsampler's fp32 slab, the stream of the copies to the host and its two events
    int cap_rgb = 0;
    DevBuf<float> rgb;
    Stream copy_stream;
    Event packed, copied;
    bool timing = false;
    double stage_ms[kGagaStages] = {0, 0, 0, 0, 0};
    std::string err;
};

static thread_local std::string g_gaga_error;

namespace {

int gaga_fail(artalk_gaga* g, int rc, const std::string& msg) { g->err = msg; return rc; }

// frames whose means, radii, splat image and vertices fit 512 MiB, at most 64 and at most the upsampler's slab in force
int gaga_default_slab(const artalk_gaga* g, int N) {
    const int64_t per = (int64_t)N * 16 + (int64_t)kGagaCh * g->S * g->S * 4 + (int64_t)g->V * 12 + (int64_t)g->NB * 4 + 60;
    int64_t n = (512ll << 20) / per;
    return (int)(n < 1 ? 1 : n > 64 ? 64 : n);
}

// the slab for avatars of N Gaussians: the classic avatar's for artalk_gaga_set_slab and the classic call, the pool's for a stream call
int gaga_slab(const artalk_gaga* g, int N) {
    int unet_slab = 1;
    (void)artalk_styleunet_dims(g->unet, nullptr, nullptr, nullptr, nullptr, &unet_slab);
    const int want = g->slab_req > 0 ? g->slab_req : gaga_default_slab(g, N);
    return want < unet_slab ? want : unet_slab;
}
int gaga_classic_N(const artalk_gaga* g) { return g->avatar.has(0) ? g->avatar.N : g->V; }

// the frame lists of artalk_gaga_render_streams, host arrays of T entries each
struct GagaFrames { const int64_t* row; const int32_t* stream; const int32_t* slot; };

// Where a call's frames come from.  A classic call: its one-slot set, its one-row state and every list null - frame t is motion row t on
// slot 0, a slab's forehead launch one entry over its frames in order.  A stream call: the pool, the streams' states and the lists as the
// kernels read them, one block on the device (gaga_upload_plan): rows [T] int64, slots [T], and the forehead kernel's CSR over every
// (slab, stream present in it) pair in slab order - ent_row [E] (the stream's row of the state pool), off [E + 1] into frames [T], whose
// values count from the start of their slab.  Slab k launches entries slab_ent[k] .. slab_ent[k + 1]; off[slab_ent[k + 1]] closes it.
struct GagaSource {
    const GagaSet* set;
    const GagaStates* states;
    const char* splat_call;                    // the rasteriser entry point an error names
    long motion_step;                          // floats the motion base moves per frame of the call: the row stride, or 0 under a row list
    const int32_t* slot_host = nullptr;        // [T]
    const int64_t* rows = nullptr;
    const int32_t *slots = nullptr, *ent_row = nullptr, *off = nullptr, *frames = nullptr;
    std::vector<int> slab_ent;
    // slab k's forehead entries: their number, *first the first of them
    int entries(int k, int* first) const {
        *first = slab_ent.empty() ? 0 : slab_ent[(size_t)k];
        return slab_ent.empty() ? 1 : slab_ent[(size_t)k + 1] - *first;
    }
};
// list + i, a null list staying null
template <typename T>
const T* gaga_from(const T* list, long i) { return list ? list + i : nullptr; }

bool gaga_upload_plan(artalk_gaga* g, const GagaFrames& fr, int T, int slab, GagaSource* plan, hipStream_t s) {
    const size_t t = (size_t)T, bytes = t * 8 + (4 * t + 1) * 4;
    if (!g->plan_host.grow(bytes, 0, 1, s) || !g->plan_dev.grow(bytes, 1, 4, s)) return false;
    // the pinned block is free here: every earlier call, on whichever stream, waited on that stream after this upload - for the rotation
    // codes, or on its way out when something failed in between
    char* h = g->plan_host.get();
    int64_t* rows = (int64_t*)h;
    int32_t* slots = (int32_t*)(h + t * 8);
    int32_t *ent_row = slots + t, *off = ent_row + t, *frames = off + t + 1;
    std::memcpy(rows, fr.row, t * 8);
    std::memcpy(slots, fr.slot, t * 4);
    int E = 0;
    plan->slab_ent.clear();
    std::vector<int32_t> ids;                  // the streams of the slab, by first appearance
    std::vector<std::vector<int32_t>> lists;
    for (int f0 = 0; f0 < T; f0 += slab) {
        const int n = T - f0 < slab ? T - f0 : slab;
        plan->slab_ent.push_back(E);
        ids.clear(); lists.clear();
        for (int j = 0; j < n; ++j) {
            size_t e = 0;
            while (e < ids.size() && ids[e] != fr.stream[f0 + j]) ++e;
            if (e == ids.size()) { ids.push_back(fr.stream[f0 + j]); lists.emplace_back(); }
            lists[e].push_back(j);
        }
        int at = f0;
        for (size_t e = 0; e < ids.size(); ++e, ++E) {
            ent_row[E] = g->stream_row[ids[e]];
            off[E] = at;
            for (int32_t j : lists[e]) frames[at++] = j;
        }
    }
    off[E] = T;
    plan->slab_ent.push_back(E);
    if (hipMemcpyAsync(g->plan_dev.get(), h, bytes, hipMemcpyHostToDevice, s) != hipSuccess) { (void)hipGetLastError(); return false; }
    const char* d = g->plan_dev.get();
    plan->rows = (const int64_t*)d;
    plan->slots = (const int32_t*)(d + t * 8);
    plan->ent_row = plan->slots + t; plan->off = plan->ent_row + t; plan->frames = plan->off + t + 1;
    return true;
}

// ---- avatar sets
// a takes `slots` empty slots for avatars of N Gaussians; what it held is gone.  The device is current.  false (a is empty): no memory
bool gaga_set_reserve(artalk_gaga* g, GagaSet& a, int slots, int N) {
    (void)hipDeviceSynchronize();     // an earlier call may still read the set that is replaced
    a.drop();
    const size_t n = (size_t)slots * N;
    if (!a.xyz.alloc(n * 3) || !a.colors.alloc(n * kGagaCh) || !a.opac.alloc(n) || !a.scales.alloc(n * 3) || !a.rots.alloc(n * 4) ||
        !a.shape.alloc((size_t)slots * (g->NB - 100))) {
        a.drop();
        return false;
    }
    a.slots = slots; a.N = N;
    a.filled.assign((size_t)slots, 0);
    a.transform.assign((size_t)slots * 12, 0.f);
    return true;
}

// Uploads an avatar into slot `slot` of a.  After the checks every caller shares, admit() applies the caller's own rule - the pool
// refuses a slot outside it and another N, the classic set is reserved anew for another N - and leaves a ready to take the avatar.
template <typename Admit>
int gaga_set_fill(artalk_gaga* g, GagaSet& a, int slot, int N, const float* xyz, const float* colors, const float* opacities, const float* scales,
                  const float* rotations, const float* shapecode, const float* transform_3x4, Admit admit) {
    if (!xyz || !colors || !opacities || !scales || !rotations || !transform_3x4 || (g->NB > 100 && !shapecode))
        return gaga_fail(g, ARTALK_EINVAL, "xyz, colors, opacities, scales, rotations, shapecode and transform must not be NULL");
    int rc = check_avatar(g->V, N, &g->err);
    if (rc == ARTALK_OK) rc = admit();
    if (rc != ARTALK_OK) return rc;
    if (hipSetDevice(g->device) != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "hipSetDevice failed");
    if (a.filled[(size_t)slot]) (void)hipDeviceSynchronize();      // an earlier call may still read the avatar that is replaced
    a.filled[(size_t)slot] = 0;
    const size_t n = (size_t)N, at = (size_t)slot * n, NS = (size_t)(g->NB - 100);
    const auto up = [](float* dst, const float* src, size_t count) {
        return count == 0 || hipMemcpy(dst, src, count * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(a.xyz.get() + at * 3, xyz, n * 3) || !up(a.colors.get() + at * kGagaCh, colors, n * kGagaCh) || !up(a.opac.get() + at, opacities, n) ||
        !up(a.scales.get() + at * 3, scales, n * 3) || !up(a.rots.get() + at * 4, rotations, n * 4) || !up(a.shape.get() + (size_t)slot * NS, shapecode, NS)) {
        (void)hipGetLastError();
        return gaga_fail(g, ARTALK_EHIP, "uploading the avatar failed");
    }
    (void)hipDeviceSynchronize();      // the slot is whole before any call reads it
    std::memcpy(a.transform.data() + (size_t)slot * 12, transform_3x4, 12 * sizeof(float));
    a.filled[(size_t)slot] = 1;
    return ARTALK_OK;
}

// ---- state pools
// unsets row `row` of p.  The device is idle; it is idle again afterwards
int gaga_zero_row(artalk_gaga* g, GagaStates& p, int row) {
    const size_t w = (size_t)(g->K ? g->K : 1) * 3;
    if (hipMemset(p.flag.get() + row, 0, sizeof(int)) != hipSuccess || hipMemset(p.state.get() + (size_t)row * w, 0, w * sizeof(float)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        return gaga_fail(g, ARTALK_EHIP, "hipMemset failed");
    }
    return ARTALK_OK;
}

}  // namespace

extern "C" {

const char* artalk_gaga_last_error(const artalk_gaga* g) { return g ? g->err.c_str() : g_gaga_error.c_str(); }

void artalk_gaga_destroy(artalk_gaga* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();
    delete g;
}

int artalk_gaga_cameras(const float* rot_host, int64_t rot_stride, int T, const float* transform_3x4_host, float* view_out, float* proj_out,
                        float* cam_out_or_null) {
    if (!rot_host || !transform_3x4_host || !view_out || !proj_out) { g_gaga_error = "rot, transform, view and proj must not be NULL"; return ARTALK_EINVAL; }
    if (T < 0) { g_gaga_error = "T must not be negative"; return ARTALK_EINVAL; }
    if (rot_stride < 3) { g_gaga_error = "rot_stride must be at least 3"; return ARTALK_EINVAL; }
    // the projection of artalk_amd.splat.build_camera_matrices with focal 12, z_near 0.01, z_far 100, transposed for row vectors
    const double focal = 12.0, zn = 0.01, zf = 100.0;
    const double p00 = 1.0 / std::tan(std::atan(1.0 / focal)), p22 = zf / (zf - zn), p32 = -(zf * zn) / (zf - zn);
    for (int t = 0; t < T; ++t) {
        const float* r = rot_host + (size_t)t * rot_stride;
        const double w[3] = {-(double)r[0], (double)r[1], -(double)r[2]};
        const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
        // R = I + A [w]x + B [w]x^2, A = sin(th) / th, B = (1 - cos(th)) / th^2 = 2 sin^2(th / 2) / th^2 (no cancellation near 0)
        const double sh = std::sin(0.5 * th);
        const double A = th > 0.0 ? std::sin(th) / th : 1.0, B = th > 0.0 ? 2.0 * sh * sh / th2 : 0.5;
        const double Kx[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
        double R[9];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const double kk = Kx[a * 3] * Kx[b] + Kx[a * 3 + 1] * Kx[3 + b] + Kx[a * 3 + 2] * Kx[6 + b];
                R[a * 3 + b] = (a == b ? 1.0 : 0.0) + A * Kx[a * 3 + b] + B * kk;
            }
        // the frame's [M | t]: M = diag(-1, 1, -1) . R^T; the translation stays the avatar's own
        double cam[12];
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) cam[a * 4 + b] = (a == 1 ? 1.0 : -1.0) * R[b * 3 + a];
            cam[a * 4 + 3] = (double)transform_3x4_host[a * 4 + 3];
        }
        if (cam_out_or_null) for (int e = 0; e < 12; ++e) cam_out_or_null[(size_t)t * 12 + e] = (float)cam[e];
        double view[16];
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) view[a * 4 + b] = cam[a * 4 + b];
            view[a * 4 + 3] = 0.0;
            view[12 + a] = cam[a * 4 + 3];
        }
        view[15] = 1.0;
        for (int a = 0; a < 4; ++a) { view[a * 4] = -view[a * 4]; view[a * 4 + 1] = -view[a * 4 + 1]; }
        float* vo = view_out + (size_t)t * 16;
        float* po = proj_out + (size_t)t * 16;
        for (int a = 0; a < 4; ++a) {
            for (int b = 0; b < 4; ++b) vo[a * 4 + b] = (float)view[a * 4 + b];
            po[a * 4] = (float)(view[a * 4] * p00);
            po[a * 4 + 1] = (float)(view[a * 4 + 1] * p00);
            po[a * 4 + 2] = (float)(view[a * 4 + 2] * p22 + view[a * 4 + 3] * p32);
            po[a * 4 + 3] = (float)view[a * 4 + 2];
        }
    }
    return ARTALK_OK;
}

int artalk_gaga_create(int device_id, artalk_flame* flame, artalk_splat* splat, artalk_styleunet* unet, int V, int NB, int S, artalk_gaga** out) {
    if (!out) { g_gaga_error = "out is NULL"; return ARTALK_EINVAL; }
    *out = nullptr;
    if (device_id < 0) { g_gaga_error = "device_id must not be negative"; return ARTALK_EINVAL; }
    if (!flame || !splat || !unet) { g_gaga_error = "flame, splat and unet must not be NULL"; return ARTALK_EINVAL; }
    if (V < 1 || NB < 100 || S < 1) { g_gaga_error = "V and S must be positive and NB at least 100"; return ARTALK_EINVAL; }
    int fV = 0, fNB = 0, in_dim = 0, out_dim = 0, uS = 0;
    const int fdev = artalk_flame_dims(flame, &fV, &fNB, nullptr);
    const int udev = artalk_styleunet_dims(unet, &in_dim, &out_dim, &uS, nullptr, nullptr);
    if (fV != V || fNB != NB) {
        g_gaga_error = "the FLAME model has V = " + std::to_string(fV) + ", NB = " + std::to_string(fNB) + ", not " + std::to_string(V) + ", " + std::to_string(NB);
        return ARTALK_EINVAL;
    }
    if (uS != S || in_dim != kGagaCh || out_dim != 3) {
        g_gaga_error = "the upsampler must map 32 channels to 3 at " + std::to_string(S) + " x " + std::to_string(S) + " (it maps " +
                       std::to_string(in_dim) + " to " + std::to_string(out_dim) + " at " + std::to_string(uS) + ")";
        return ARTALK_EINVAL;
    }
    if (fdev != device_id || udev != device_id) { g_gaga_error = "the FLAME model and the upsampler must live on device " + std::to_string(device_id); return ARTALK_EINVAL; }
    artalk_gaga* g = new artalk_gaga();
    g->device = device_id; g->V = V; g->NB = NB; g->S = S;
    g->flame = flame; g->splat = splat; g->unet = unet;
    for (g->num_layers = 0; (1 << g->num_layers) < S; ++g->num_layers) {}
    g->num_layers = (g->num_layers - 2) * 2 + 1;
    *out = g;
    if (V > 3913) {
        const int rc = artalk_gaga_set_forehead(g, kForeheadIdx, kForeheadDefault);
        if (rc != ARTALK_OK) { g_gaga_error = g->err; artalk_gaga_destroy(g); *out = nullptr; return rc; }
    }
    return ARTALK_OK;
}

int artalk_gaga_set_avatar(artalk_gaga* g, int N, const float* xyz, const float* colors, const float* opacities, const float* scales,
                           const float* rotations, const float* shapecode, const float* transform_3x4) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    return gaga_set_fill(g, g->avatar, 0, N, xyz, colors, opacities, scales, rotations, shapecode, transform_3x4, [&] {
        if (N == g->avatar.N) return ARTALK_OK;      // the one slot takes another N from call to call: it is reserved anew
        if (hipSetDevice(g->device) != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "hipSetDevice failed");
        return gaga_set_reserve(g, g->avatar, 1, N) ? ARTALK_OK : gaga_fail(g, ARTALK_EHIP, "uploading the avatar failed");
    });
}

int artalk_gaga_reset_state(artalk_gaga* g) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (g->classic.rows == 0) return ARTALK_OK;      // no indices: there is no state
    if (hipSetDevice(g->device) != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "hipSetDevice failed");
    (void)hipDeviceSynchronize();
    return gaga_zero_row(g, g->classic, 0);
}

int artalk_gaga_set_forehead(artalk_gaga* g, const int32_t* idx, int K) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    const int rc = check_forehead(g->V, idx, K, &g->err);
    if (rc != ARTALK_OK) return rc;
    if (g->streams_open > 0 && K != g->K)
        return gaga_fail(g, ARTALK_ESTATE, "K = " + std::to_string(K) + " differs from the " + std::to_string(g->K) + " vertices the " +
                                           std::to_string(g->streams_open) + " open streams keep a state for: close them first");
    if (hipSetDevice(g->device) != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "hipSetDevice failed");
    (void)hipDeviceSynchronize();
    if (K != g->K) g->streams.drop();      // (no stream is open) rows of another width
    g->index.reset(); g->classic.drop(); g->K = 0;
    if (K == 0) return ARTALK_OK;
    if (!g->index.alloc((size_t)K) || !g->classic.flag.alloc(1) || !g->classic.state.alloc((size_t)K * 3)) {
        g->index.reset(); g->classic.drop();
        return gaga_fail(g, ARTALK_EHIP, "hipMalloc failed");
    }
    g->K = K; g->classic.rows = 1;
    if (hipMemcpy(g->index.get(), idx, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
        return gaga_fail(g, ARTALK_EHIP, "uploading the indices failed");
    return artalk_gaga_reset_state(g);
}

int artalk_gaga_set_watermark(artalk_gaga* g, const float* rgba_host, int h, int w) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (rgba_host) {
        const int rc = check_watermark(g->S, h, w, &g->err);
        if (rc != ARTALK_OK) return rc;
    }
    if (!rgba_host && !g->wm.get()) return ARTALK_OK;
    if (hipSetDevice(g->device) != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "hipSetDevice failed");
    (void)hipDeviceSynchronize();
    g->wm.reset();
    g->wm_h = g->wm_w = 0;
    if (!rgba_host) return ARTALK_OK;
    if (!g->wm.upload(rgba_host, (size_t)4 * h * w)) return gaga_fail(g, ARTALK_EHIP, "uploading the watermark failed");
    g->wm_h = h; g->wm_w = w;
    return ARTALK_OK;
}

int artalk_gaga_set_slab(artalk_gaga* g, int frames) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (frames < 0 || frames > 64) return gaga_fail(g, ARTALK_EINVAL, "slab must be in 0..64 frames (0: the default)");
    g->slab_req = frames;
    return gaga_slab(g, gaga_classic_N(g));
}

int artalk_gaga_streams_slab(const artalk_gaga* g) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    return gaga_slab(g, g->pool.slots > 0 ? g->pool.N : gaga_classic_N(g));
}

int artalk_gaga_set_timing(artalk_gaga* g, int enable) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    g->timing = enable != 0;
    return ARTALK_OK;
}

int artalk_gaga_get_timing(const artalk_gaga* g, double* stage_ms, int n) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (stage_ms) for (int i = 0; i < n && i < kGagaStages; ++i) stage_ms[i] = g->stage_ms[i];
    return kGagaStages;
}

// The loop of artalk_gaga_render, artalk_gaga_render_u8 and (fr != null) artalk_gaga_render_streams.  format == 0: fp32 frames into
// out_dev, finished in place.  Otherwise the upsampler writes each slab into g->rgb and the fused finish-and-pack kernel writes its 8-bit
// frames into out_u8 (and, with out_host, a copy on g->copy_stream follows each slab's pack kernel).  With fr, frame t takes motion row
// fr->row[t], the resident avatar of slot fr->slot[t] and the EMA state of stream fr->stream[t]; without, row t, the classic avatar and
// the classic state.  The slab loop is one code for both (GagaSource).
static int gaga_render_any(artalk_gaga* g, const float* motion_dev, int64_t motion_stride, int T, const float* const* noise_ptrs_or_null,
                           const int64_t* noise_batch_strides, int activation, float* out_dev, int format, uint8_t* out_u8, uint8_t* out_host,
                           void* stream, const char* name, const GagaFrames* fr = nullptr) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (!motion_dev || (format ? !out_u8 : !out_dev)) return gaga_fail(g, ARTALK_EINVAL, "motion and out must not be NULL");
    int finalized = 0;
    (void)artalk_styleunet_dims(g->unet, nullptr, nullptr, nullptr, &finalized, nullptr);
    if (fr) {
        const int rcs = check_frames(T, fr->row, fr->stream, fr->slot, g->stream_open.data(), (int)g->stream_open.size(), g->pool.filled.data(),
                                     g->pool.slots, &g->err);
        if (rcs != ARTALK_OK) return rcs;
    }
    const int rc = check_render(T, motion_stride, fr || g->avatar.has(0), finalized != 0, &g->err);
    if (rc != ARTALK_OK) return rc;
    const int rcn = su_check_noise(g->num_layers, noise_ptrs_or_null, noise_batch_strides, &g->err);
    if (rcn != ARTALK_OK) return rcn;
    if (format) {
        const int rcf = frames_check(format, T, g->S, g->S, true, true, &g->err);
        if (rcf != ARTALK_OK) return rcf;
    }
    if (T == 0) return ARTALK_OK;
    if (hipSetDevice(g->device) != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    if (format) {      // the call waits on its stream and orders a second stream against it: not inside a capture
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); return gaga_fail(g, ARTALK_EHIP, "hipStreamIsCapturing failed"); }
        if (cap != hipStreamCaptureStatusNone) return gaga_fail(g, ARTALK_EINVAL, std::string(name) + " waits on its stream: it cannot run during stream capture");
    }
    // where the call's frames come from, said once: from here on the function reads src, not fr
    GagaSource src{fr ? &g->pool : &g->avatar, fr ? &g->streams : &g->classic, fr ? "artalk_splat_render_sets" : "artalk_splat_render",
                   fr ? 0 : (long)motion_stride, fr ? fr->slot : nullptr};
    const GagaSet& set = *src.set;
    const int V = g->V, N = set.N, S = g->S, NB = g->NB;
    const long SS = (long)S * S;
    const int slab = gaga_slab(g, N);
    const int frames = T < slab ? T : slab;
    if (frames > g->cap_frames || N > g->cap_N) {
        (void)hipDeviceSynchronize();
        g->cap_frames = g->cap_N = 0; g->radii.reset();
        for (DevBuf<float>* b : {&g->betas, &g->pose, &g->verts, &g->means, &g->img}) b->reset();
        const size_t f = (size_t)frames;      // exact sizes: a slab is as large as it gets
        if (!g->betas.alloc(f * NB) || !g->pose.alloc(f * 15) || !g->verts.alloc(f * V * 3) || !g->means.alloc(f * N * 3) ||
            !g->img.alloc(f * kGagaCh * SS) || !g->radii.alloc(f * N))
            return gaga_fail(g, ARTALK_EHIP, "hipMalloc of the scratch for " + std::to_string(frames) + " frames failed");
        g->cap_frames = frames; g->cap_N = N;
    }
    const int64_t fbytes = format ? frames_bytes(format, S, S) : 0;
    if (format && frames > g->cap_rgb) {
        (void)hipDeviceSynchronize();
        g->cap_rgb = 0; g->rgb.reset();
        if (!g->rgb.alloc((size_t)frames * 3 * SS)) return gaga_fail(g, ARTALK_EHIP, "hipMalloc of the fp32 slab for " + std::to_string(frames) + " frames failed");
        g->cap_rgb = frames;
    }
    if (out_host && (!g->copy_stream.create() || !g->packed.create() || !g->copied.create()))
        return gaga_fail(g, ARTALK_EHIP, "creating the copy stream or its events failed");
    if (!g->codes_host.grow((size_t)T * 3, 0, 1, s)) return gaga_fail(g, ARTALK_EHIP, "hipHostMalloc failed");
    // The two differences between the call kinds.  Only a stream call uploads its lists and gathers the head-rotation codes of its
    // scattered rows into one block; the classic call copies columns 100:103 of its rows as they lie.
    hipError_t codes;
    if (fr) {
        if (!g->codes_dev.grow((size_t)T * 3, 1, 4, s)) return gaga_fail(g, ARTALK_EHIP, "hipMalloc of the rotation codes failed");
        if (!gaga_upload_plan(g, *fr, T, slab, &src, s)) {      // (nothing is in flight: the upload is the function's last step)
            return gaga_fail(g, ARTALK_EHIP, "uploading the frame lists failed");
        }
        ARTALK_LAUNCH(gaga_gather_codes_kernel, dim3(gaga_blocks((long)T * 3)), dim3(256), 0, s, motion_dev, (long)motion_stride, src.rows,
                      g->codes_dev.get(), T);
        codes = hipMemcpyAsync(g->codes_host.get(), g->codes_dev.get(), (size_t)T * 3 * sizeof(float), hipMemcpyDeviceToHost, s);
    } else {
        codes = hipMemcpy2DAsync(g->codes_host.get(), 3 * sizeof(float), motion_dev + 100, (size_t)motion_stride * sizeof(float), 3 * sizeof(float),
                                 (size_t)T, hipMemcpyDeviceToHost, s);
    }
    // the first wait of the call: the head-rotation codes become the cameras, which the rasteriser reads on the host
    if (codes != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        (void)hipGetLastError();
        if (fr) (void)hipStreamSynchronize(s);      // the frame lists may still be on their way up from the pinned block
        return gaga_fail(g, ARTALK_EHIP, "reading the rotation codes failed");
    }
    std::vector<float> view((size_t)T * 16), proj((size_t)T * 16);
    for (int t = 0; t < T; ++t)      // every frame under its slot's [R | t]
        (void)artalk_gaga_cameras(g->codes_host.get() + (size_t)t * 3, 3, 1, set.transform.data() + (size_t)(src.slot_host ? src.slot_host[t] : 0) * 12,
                                  view.data() + (size_t)t * 16, proj.data() + (size_t)t * 16, nullptr);

    StageTimer timer;
    timer.start(s, g->timing);
    for (double& m : g->stage_ms) m = 0;
    std::vector<const float*> np(g->num_layers);
    const float tanfov = (float)(1.0 / 12.0);
    for (int f0 = 0; f0 < T; f0 += slab) {
        const int n = T - f0 < slab ? T - f0 : slab;
        timer.mark(-1);      // (what lies between two slabs counts to no stage)
        launch_gaga_flame_inputs(motion_dev + f0 * src.motion_step, (long)motion_stride, gaga_from(src.rows, f0), gaga_from(src.slots, f0),
                                 set.shape.get(), NB - 100, g->betas.get(), g->pose.get(), n, s);
        if (artalk_flame_verts(g->flame, g->betas.get(), g->pose.get(), n, g->verts.get(), s) != ARTALK_OK)
            return gaga_fail(g, ARTALK_EHIP, std::string("artalk_flame_verts failed: ") + artalk_flame_last_error(g->flame));
        timer.mark(kGagaInputsFlame);
        int e0 = 0;
        const int entries = src.entries(f0 / slab, &e0);
        if (g->K > 0) launch_gaga_forehead(g->verts.get(), g->index.get(), g->K, V, entries, n, gaga_from(src.ent_row, e0), gaga_from(src.off, e0),
                                           src.frames, src.states->state.get(), src.states->flag.get(), s);
        launch_gaga_means(g->verts.get(), set.xyz.get(), gaga_from(src.slots, f0), g->means.get(), n, V, N, s);
        timer.mark(kGagaForeheadMeans);
        // (without a slot list the rasteriser reads set 0 and none of the set strides: the call is artalk_splat_render)
        int rc2 = artalk_splat_render_sets(g->splat, N, n, S, S, g->means.get(), (int64_t)N * 3, set.colors.get(), 0, set.opac.get(), 0,
                                           set.scales.get(), 0, set.rots.get(), 0, view.data() + (size_t)f0 * 16, proj.data() + (size_t)f0 * 16, n,
                                           tanfov, tanfov, 1.0f, nullptr, g->img.get(), g->radii.get(), gaga_from(src.slot_host, f0), set.slots, 0,
                                           (int64_t)N * kGagaCh, N, (int64_t)N * 3, (int64_t)N * 4, s);
        if (rc2 != ARTALK_OK) return gaga_fail(g, rc2, std::string(src.splat_call) + " failed: " + artalk_splat_last_error(g->splat));
        timer.mark(kGagaSplat);
        if (noise_ptrs_or_null) for (int l = 0; l < g->num_layers; ++l) np[l] = noise_ptrs_or_null[l] + (long)f0 * noise_batch_strides[l];
        float* out = format ? g->rgb.get() : out_dev + (long)f0 * 3 * SS;
        rc2 = artalk_styleunet_forward(g->unet, g->img.get(), n, noise_ptrs_or_null ? np.data() : nullptr, noise_batch_strides, activation, out, s);
        if (rc2 != ARTALK_OK) return gaga_fail(g, rc2, std::string("artalk_styleunet_forward failed: ") + artalk_styleunet_last_error(g->unet));
        timer.mark(kGagaUpsampler);
        if (!format) {
            launch_gaga_finish(out, g->wm.get(), g->wm_h, g->wm_w, S, n, s);
        } else {
            uint8_t* o8 = out_u8 + (int64_t)f0 * fbytes;
            launch_frames_finish_pack(out, g->wm.get(), g->wm_h, g->wm_w, S, n, format, o8, s);
            if (out_host) {      // out_u8 holds the whole clip: nothing this copy reads is written again
                if (hipEventRecord(g->packed.get(), s) != hipSuccess || hipStreamWaitEvent(g->copy_stream.get(), g->packed.get(), 0) != hipSuccess ||
                    hipMemcpyAsync(out_host + (int64_t)f0 * fbytes, o8, (size_t)((int64_t)n * fbytes), hipMemcpyDeviceToHost, g->copy_stream.get()) != hipSuccess) {
                    (void)hipGetLastError();
                    return gaga_fail(g, ARTALK_EHIP, "copying a slab's frames to the host failed");
                }
            }
        }
        timer.mark(kGagaFinish);
    }
    if (out_host) {      // a synchronisation of the caller's stream covers the host buffer
        if (hipEventRecord(g->copied.get(), g->copy_stream.get()) != hipSuccess || hipStreamWaitEvent(s, g->copied.get(), 0) != hipSuccess) {
            (void)hipGetLastError();
            return gaga_fail(g, ARTALK_EHIP, "ordering the caller's stream behind the last copy failed");
        }
    }
    timer.finish(g->stage_ms, kGagaStages);
    if (hipGetLastError() != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "a launch failed");
    return ARTALK_OK;
}

int artalk_gaga_render(artalk_gaga* g, const float* motion_dev, int64_t motion_stride, int T, const float* const* noise_ptrs_or_null,
                       const int64_t* noise_batch_strides, int activation, float* out_dev, void* stream) {
    return gaga_render_any(g, motion_dev, motion_stride, T, noise_ptrs_or_null, noise_batch_strides, activation, out_dev, 0, nullptr, nullptr, stream,
                           "artalk_gaga_render");
}

int artalk_gaga_render_u8(artalk_gaga* g, const float* motion_dev, int64_t motion_stride, int T, const float* const* noise_ptrs_or_null,
                          const int64_t* noise_batch_strides, int activation, int format, uint8_t* out_dev, uint8_t* out_host_or_null,
                          void* stream) {
    if (g && format != ARTALK_FRAMES_RGB24 && format != ARTALK_FRAMES_YUV420P) return gaga_fail(g, ARTALK_EINVAL, "unknown frame format " + std::to_string(format));
    const int rc = gaga_render_any(g, motion_dev, motion_stride, T, noise_ptrs_or_null, noise_batch_strides, activation, nullptr, format,
                                   out_dev, out_host_or_null, stream, "artalk_gaga_render_u8");
    // a call that failed between two slabs leaves no copy in flight: the caller may free both buffers
    if (rc != ARTALK_OK && g && out_host_or_null && g->copy_stream.get()) (void)hipStreamSynchronize(g->copy_stream.get());
    return rc;
}

// ---- resident avatars
int artalk_gaga_pool_reserve(artalk_gaga* g, int slots, int N) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    const int rc = check_pool(g->V, slots, N, &g->err);
    if (rc != ARTALK_OK) return rc;
    if (g->pool.slots > 0 && g->streams_open > 0)
        return gaga_fail(g, ARTALK_ESTATE, "the pool cannot be reserved again while " + std::to_string(g->streams_open) + " streams are open");
    if (hipSetDevice(g->device) != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "hipSetDevice failed");
    if (!gaga_set_reserve(g, g->pool, slots, N))
        return gaga_fail(g, ARTALK_EHIP, "hipMalloc of a pool of " + std::to_string(slots) + " avatars of " + std::to_string(N) + " Gaussians failed");
    return ARTALK_OK;
}

static int gaga_check_slot(artalk_gaga* g, int slot) {
    if (slot >= 0 && slot < g->pool.slots) return ARTALK_OK;
    return gaga_fail(g, ARTALK_EINVAL, "slot " + std::to_string(slot) + " is outside the pool's [0, " + std::to_string(g->pool.slots) + ")");
}

int artalk_gaga_pool_set(artalk_gaga* g, int slot, int N, const float* xyz, const float* colors, const float* opacities, const float* scales,
                         const float* rotations, const float* shapecode, const float* transform_3x4) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    return gaga_set_fill(g, g->pool, slot, N, xyz, colors, opacities, scales, rotations, shapecode, transform_3x4, [&] {
        const int rc = gaga_check_slot(g, slot);
        if (rc != ARTALK_OK || N == g->pool.N) return rc;
        return gaga_fail(g, ARTALK_EINVAL, "N (" + std::to_string(N) + ") is not the pool's " + std::to_string(g->pool.N) + ": resident avatars share N");
    });
}

int artalk_gaga_pool_clear(artalk_gaga* g, int slot) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    const int rc = gaga_check_slot(g, slot);
    if (rc != ARTALK_OK) return rc;
    if (!g->pool.filled[(size_t)slot]) return ARTALK_OK;
    if (hipSetDevice(g->device) != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "hipSetDevice failed");
    (void)hipDeviceSynchronize();
    g->pool.filled[(size_t)slot] = 0;
    return ARTALK_OK;
}

// ---- per-stream forehead state
static int gaga_check_stream(artalk_gaga* g, int id) {
    if (id < 0 || id >= (int)g->stream_open.size()) return gaga_fail(g, ARTALK_EINVAL, "stream " + std::to_string(id) + " was never opened");
    if (!g->stream_open[(size_t)id]) return gaga_fail(g, ARTALK_EINVAL, "stream " + std::to_string(id) + " is closed");
    return ARTALK_OK;
}

int artalk_gaga_stream_open(artalk_gaga* g, int* id) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (!id) return gaga_fail(g, ARTALK_EINVAL, "id is NULL");
    *id = -1;
    if (hipSetDevice(g->device) != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "hipSetDevice failed");
    (void)hipDeviceSynchronize();      // a closed stream's last call may still write the row that is handed out again
    GagaStates& p = g->streams;
    std::vector<char> taken((size_t)p.rows, 0);
    for (size_t i = 0; i < g->stream_open.size(); ++i)
        if (g->stream_open[i]) taken[(size_t)g->stream_row[i]] = 1;
    int row = 0;
    while (row < p.rows && taken[(size_t)row]) ++row;
    if (row == p.rows) {      // grow, keeping the open streams' rows
        const int cap = p.rows ? 2 * p.rows : 8;
        const size_t w = (size_t)(g->K ? g->K : 1) * 3;
        DevBuf<float> st;
        DevBuf<int> fl;
        if (!st.alloc_zero((size_t)cap * w) || !fl.alloc_zero((size_t)cap)) return gaga_fail(g, ARTALK_EHIP, "hipMalloc of the stream states failed");
        if (p.rows > 0 && (hipMemcpy(st.get(), p.state.get(), (size_t)p.rows * w * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess ||
                           hipMemcpy(fl.get(), p.flag.get(), (size_t)p.rows * sizeof(int), hipMemcpyDeviceToDevice) != hipSuccess)) {
            (void)hipGetLastError();
            return gaga_fail(g, ARTALK_EHIP, "copying the stream states failed");
        }
        (void)hipDeviceSynchronize();
        p.state = std::move(st); p.flag = std::move(fl);
        p.rows = cap;
    }
    const int rc = gaga_zero_row(g, p, row);
    if (rc != ARTALK_OK) return rc;
    g->stream_open.push_back(1);
    g->stream_row.push_back(row);
    ++g->streams_open;
    *id = (int)g->stream_open.size() - 1;
    return ARTALK_OK;
}

int artalk_gaga_stream_close(artalk_gaga* g, int id) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    const int rc = gaga_check_stream(g, id);
    if (rc != ARTALK_OK) return rc;
    g->stream_open[(size_t)id] = 0;      // the row is cleared when it is handed out again, after a wait for the device
    --g->streams_open;
    return ARTALK_OK;
}

int artalk_gaga_stream_reset(artalk_gaga* g, int id) {
    if (!g) { g_gaga_error = "handle is NULL"; return ARTALK_EINVAL; }
    const int rc = gaga_check_stream(g, id);
    if (rc != ARTALK_OK) return rc;
    if (hipSetDevice(g->device) != hipSuccess) return gaga_fail(g, ARTALK_EHIP, "hipSetDevice failed");
    (void)hipDeviceSynchronize();
    return gaga_zero_row(g, g->streams, g->stream_row[(size_t)id]);
}

int artalk_gaga_render_streams(artalk_gaga* g, const float* motion_dev, int64_t motion_stride, int T, const int64_t* frame_row_host,
                               const int32_t* frame_stream_host, const int32_t* frame_slot_host, const float* const* noise_ptrs_or_null,
                               const int64_t* noise_batch_strides, int activation, int format, float* out_dev, uint8_t* out_u8,
                               uint8_t* out_host_or_null, void* stream) {
    if (g && format != 0 && format != ARTALK_FRAMES_RGB24 && format != ARTALK_FRAMES_YUV420P)
        return gaga_fail(g, ARTALK_EINVAL, "unknown frame format " + std::to_string(format));
    if (g && format == 0 && out_host_or_null) return gaga_fail(g, ARTALK_EINVAL, "out_host needs an 8-bit format");
    const GagaFrames fr{frame_row_host, frame_stream_host, frame_slot_host};
    const int rc = gaga_render_any(g, motion_dev, motion_stride, T, noise_ptrs_or_null, noise_batch_strides, activation, out_dev, format, out_u8,
                                   out_host_or_null, stream, "artalk_gaga_render_streams", &fr);
    if (rc != ARTALK_OK && g && out_host_or_null && g->copy_stream.get()) (void)hipStreamSynchronize(g->copy_stream.get());
    return rc;
}

// ---- single launches and the host checks, for the tests
int artalk_op_gaga_flame_inputs(const float* motion_dev, int64_t motion_stride, const float* shapecode_dev, int NB, int T, float* betas_dev,
                                float* pose_dev, void* stream) {
    if (!motion_dev || !betas_dev || !pose_dev || T < 1 || NB < 100 || motion_stride < kGagaMotion || (NB > 100 && !shapecode_dev)) return ARTALK_EINVAL;
    launch_gaga_flame_inputs(motion_dev, (long)motion_stride, nullptr, nullptr, shapecode_dev, NB - 100, betas_dev, pose_dev, T, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gaga_forehead(float* verts_dev, const int32_t* idx_dev, int K, int T, int V, float* state_dev, int* flag_dev, void* stream) {
    if (!verts_dev || !state_dev || !flag_dev || K < 0 || T < 0 || V < 1 || K > V || (K > 0 && !idx_dev)) return ARTALK_EINVAL;
    if (K == 0 || T == 0) return ARTALK_OK;
    launch_gaga_forehead(verts_dev, idx_dev, K, V, 1, T, nullptr, nullptr, nullptr, state_dev, flag_dev, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gaga_means(const float* verts_dev, const float* xyz_dev, float* means_dev, int F, int V, int N, void* stream) {
    if (!verts_dev || !xyz_dev || !means_dev || F < 1 || V < 1 || N < V) return ARTALK_EINVAL;
    launch_gaga_means(verts_dev, xyz_dev, nullptr, means_dev, F, V, N, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gaga_flame_inputs_sets(const float* motion_dev, int64_t motion_stride, const int64_t* frame_row_dev, const int32_t* frame_slot_dev,
                                     const float* shapecode_pool_dev, int NB, int T, float* betas_dev, float* pose_dev, void* stream) {
    if (!motion_dev || !frame_row_dev || !frame_slot_dev || !betas_dev || !pose_dev || T < 1 || NB < 100 || motion_stride < kGagaMotion ||
        (NB > 100 && !shapecode_pool_dev))
        return ARTALK_EINVAL;
    launch_gaga_flame_inputs(motion_dev, (long)motion_stride, frame_row_dev, frame_slot_dev, shapecode_pool_dev, NB - 100, betas_dev, pose_dev, T,
                             (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gaga_forehead_streams(float* verts_dev, const int32_t* idx_dev, int K, int V, int n_streams, const int32_t* pool_row_dev,
                                    const int32_t* offsets_dev, const int32_t* frames_dev, float* state_pool_dev, int* flag_pool_dev, void* stream) {
    if (!verts_dev || !state_pool_dev || !flag_pool_dev || K < 0 || n_streams < 0 || V < 1 || K > V || (K > 0 && !idx_dev)) return ARTALK_EINVAL;
    if (n_streams > 0 && (!pool_row_dev || !offsets_dev || !frames_dev)) return ARTALK_EINVAL;
    if (K == 0 || n_streams == 0) return ARTALK_OK;
    launch_gaga_forehead(verts_dev, idx_dev, K, V, n_streams, 0, pool_row_dev, offsets_dev, frames_dev, state_pool_dev, flag_pool_dev,
                         (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gaga_means_sets(const float* verts_dev, const float* xyz_pool_dev, const int32_t* frame_slot_dev, float* means_dev, int F, int V,
                              int N, void* stream) {
    if (!verts_dev || !xyz_pool_dev || !frame_slot_dev || !means_dev || F < 1 || V < 1 || N < V) return ARTALK_EINVAL;
    launch_gaga_means(verts_dev, xyz_pool_dev, frame_slot_dev, means_dev, F, V, N, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gaga_streams_check(int V, int pool_slots, int pool_N, int T, int64_t motion_stride, const int64_t* frame_row_host,
                                 const int32_t* frame_stream_host, const int32_t* frame_slot_host, const uint8_t* stream_open_host, int n_stream_ids,
                                 const uint8_t* slot_filled_host, int unet_finalized, int format, int S, char* msg, int msg_cap) {
    std::string err;
    int rc = check_pool(V, pool_slots, pool_N, &err);
    if (rc == ARTALK_OK) rc = check_frames(T, frame_row_host, frame_stream_host, frame_slot_host, stream_open_host, n_stream_ids, slot_filled_host, pool_slots, &err);
    if (rc == ARTALK_OK) rc = check_render(T, motion_stride, true, unet_finalized != 0, &err);
    if (rc == ARTALK_OK && format != 0) rc = frames_check(format, T, S, S, true, true, &err);
    if (msg && msg_cap > 0) { std::strncpy(msg, err.c_str(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
    return rc;
}

int artalk_op_gaga_finish(float* img_dev, int F, int S, const float* rgba_dev_or_null, int h, int w, void* stream) {
    if (!img_dev || F < 1 || S < 1 || S > 4096) return ARTALK_EINVAL;
    if (rgba_dev_or_null && (h < 1 || w < 1 || h > S || w > S)) return ARTALK_EINVAL;
    launch_gaga_finish(img_dev, rgba_dev_or_null, rgba_dev_or_null ? h : 0, rgba_dev_or_null ? w : 0, S, F, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gaga_check(int V, int S, int N, const int32_t* idx_host, int K, int wm_h, int wm_w, int T, int64_t motion_stride, int have_avatar,
                         int unet_finalized, char* msg, int msg_cap) {
    std::string err;
    int rc = check_avatar(V, N, &err);
    if (rc == ARTALK_OK) rc = check_forehead(V, idx_host, K, &err);
    if (rc == ARTALK_OK && (wm_h != 0 || wm_w != 0)) rc = check_watermark(S, wm_h, wm_w, &err);
    if (rc == ARTALK_OK) rc = check_render(T, motion_stride, have_avatar != 0, unet_finalized != 0, &err);
    if (msg && msg_cap > 0) { std::strncpy(msg, err.c_str(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
    return rc;
}

}  // extern "C"
