// FLAME linear blend skinning: the first consumer of the 106-d codes (reference app/flame_model/FLAME.py:117-142 ->
// app/flame_model/lbs.py:142-233), SURVEY.md section 8f rank 3.  106-d motion + 300-d shape -> 5023 x 3 vertices per frame.
//   v_shaped = v_template + shapedirs . betas                 (lbs.py:185, blend_shapes :262)  -> fp32 MFMA GEMM, K = 400
//   J        = J_regressor . v_shaped                          (lbs.py:189, vertices2joints :241) -> flame_joints_kernel
//   R_j      = rodrigues(pose_j); pose_feature = R_1.. - I     (lbs.py:195-198, batch_rodrigues :266) -> flame_pose_kernel
//   v_posed  = v_shaped + pose_feature . posedirs              (lbs.py:200-212)                  -> fp32 MFMA GEMM, K = 36
//   A_j      = rigid transform chain relative to the rest pose (lbs.py:214, batch_rigid_transform :313)
//   verts    = (sum_j w_vj A_j) [v_posed, 1]                   (lbs.py:216-231)                  -> flame_skin_kernel
// The C ABI of the vertex path (artalk_flame_*) follows the kernels.
#include "common.h"
#include "device_mem.h"
#include "../../include/artalk_hip.h"

namespace artalk {

constexpr int FJ = 5;   // joints of FLAME: global, neck, jaw, left eye, right eye

// one thread per (frame, joint): axis-angle -> rotation matrix; joints >= 1 also emit R - I into the pose-feature row
__global__ void flame_pose_kernel(const float* __restrict__ pose /*[T][FJ*3]*/, float* __restrict__ rot /*[T][FJ][9]*/,
                                  float* __restrict__ feat /*[T][ldf]*/, int T, int ldf) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * FJ) return;
    const int t = idx / FJ, j = idx % FJ;
    const float* p = pose + (long)t * FJ * 3 + j * 3;
    const float x = p[0], y = p[1], z = p[2];
    const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);          // torch.norm(rot_vecs + 1e-8)
    const float rx = x / angle, ry = y / angle, rz = z / angle;
    const float s = sinf(angle), c = cosf(angle);
    const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
    float KK[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) KK[a * 3 + b] = K[a * 3] * K[b] + K[a * 3 + 1] * K[3 + b] + K[a * 3 + 2] * K[6 + b];
    float R[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = ((e % 4 == 0) ? 1.f : 0.f) + s * K[e] + (1.f - c) * KK[e];
#pragma unroll
    for (int e = 0; e < 9; ++e) rot[((long)t * FJ + j) * 9 + e] = R[e];
    if (j >= 1)
#pragma unroll
        for (int e = 0; e < 9; ++e) feat[(long)t * ldf + (j - 1) * 9 + e] = R[e] - ((e % 4 == 0) ? 1.f : 0.f);
}

// one workgroup per frame: J[t][j][k] = sum_v Jreg[j][v] * v_shaped[t][v][k]
__global__ __launch_bounds__(256) void flame_joints_kernel(const float* __restrict__ vs /*[T][V*3]*/, const float* __restrict__ jreg /*[FJ][V]*/,
                                                           float* __restrict__ J /*[T][FJ][3]*/, int V) {
    __shared__ float red[4][FJ * 3];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float acc[FJ * 3];
#pragma unroll
    for (int e = 0; e < FJ * 3; ++e) acc[e] = 0.f;
    const float* v = vs + (long)t * V * 3;
    for (int i = tid; i < V; i += 256) {
        const float x = v[i * 3], y = v[i * 3 + 1], z = v[i * 3 + 2];
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
            const float w = jreg[(long)j * V + i];
            acc[j * 3] = fmaf(w, x, acc[j * 3]); acc[j * 3 + 1] = fmaf(w, y, acc[j * 3 + 1]); acc[j * 3 + 2] = fmaf(w, z, acc[j * 3 + 2]);
        }
    }
#pragma unroll
    for (int e = 0; e < FJ * 3; ++e) {
        const float s = wave_sum(acc[e]);
        if (lane == 0) red[wv][e] = s;
    }
    __syncthreads();
    if (tid < FJ * 3) J[(long)t * FJ * 3 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// grid (ceil(V/256), T): rigid transform chain per frame (recomputed per block: 5 joints), then skin 256 vertices
__global__ __launch_bounds__(256) void flame_skin_kernel(const float* __restrict__ vposed /*[T][V*3]*/, const float* __restrict__ rot,
                                                         const float* __restrict__ J, const int* __restrict__ parents,
                                                         const float* __restrict__ weights /*[V][FJ]*/, float* __restrict__ out,
                                                         int V, float scale) {
    __shared__ float A[FJ][12];      // rows 0..2 of the relative transforms, row-major 3x4
    const int t = blockIdx.y;
    if (threadIdx.x == 0) {
        float G[FJ][12];
        const float* R = rot + (long)t * FJ * 9;
        const float* Jt = J + (long)t * FJ * 3;
        for (int j = 0; j < FJ; ++j) {
            const int par = parents[j];
            float rel[3];
            for (int k = 0; k < 3; ++k) rel[k] = (j == 0) ? Jt[k] : Jt[j * 3 + k] - Jt[par * 3 + k];
            float Tm[12];
            for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) Tm[a * 4 + b] = R[j * 9 + a * 3 + b]; Tm[a * 4 + 3] = rel[a]; }
            if (j == 0) {
                for (int e = 0; e < 12; ++e) G[0][e] = Tm[e];
            } else {   // G_j = G_parent * T_j   (bottom rows are [0 0 0 1])
                for (int a = 0; a < 3; ++a) {
                    for (int b = 0; b < 4; ++b) {
                        float s = 0.f;
                        for (int k = 0; k < 3; ++k) s += G[par][a * 4 + k] * Tm[k * 4 + b];
                        if (b == 3) s += G[par][a * 4 + 3];
                        G[j][a * 4 + b] = s;
                    }
                }
            }
        }
        for (int j = 0; j < FJ; ++j)       // A_j = G_j with translation G_j.t - G_j.R * J_j  (lbs.py:371-372)
            for (int a = 0; a < 3; ++a) {
                float s = 0.f;
                for (int k = 0; k < 3; ++k) { A[j][a * 4 + k] = G[j][a * 4 + k]; s += G[j][a * 4 + k] * Jt[j * 3 + k]; }
                A[j][a * 4 + 3] = G[j][a * 4 + 3] - s;
            }
    }
    __syncthreads();
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    float Tm[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) Tm[e] = 0.f;
#pragma unroll
    for (int j = 0; j < FJ; ++j) {
        const float w = weights[(long)v * FJ + j];
#pragma unroll
        for (int e = 0; e < 12; ++e) Tm[e] = fmaf(w, A[j][e], Tm[e]);
    }
    const float* p = vposed + ((long)t * V + v) * 3;
    const float x = p[0], y = p[1], z = p[2];
    float* o = out + ((long)t * V + v) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = (Tm[a * 4] * x + Tm[a * 4 + 1] * y + Tm[a * 4 + 2] * z + Tm[a * 4 + 3]) * scale;
}

void launch_flame_pose(const float* pose, float* rot, float* feat, int T, int ldf, hipStream_t s) {
    ARTALK_LAUNCH(flame_pose_kernel, dim3((T * FJ + 127) / 128), dim3(128), 0, s, pose, rot, feat, T, ldf);
}
void launch_flame_joints(const float* vs, const float* jreg, float* J, int T, int V, hipStream_t s) {
    ARTALK_LAUNCH(flame_joints_kernel, dim3(T), dim3(256), 0, s, vs, jreg, J, V);
}
void launch_flame_skin(const float* vposed, const float* rot, const float* J, const int* parents, const float* weights, float* out,
                       int T, int V, float scale, hipStream_t s) {
    ARTALK_LAUNCH(flame_skin_kernel, dim3((V + 255) / 256, T), dim3(256), 0, s, vposed, rot, J, parents, weights, out, V, scale);
}

}  // namespace artalk

using namespace artalk;

// ---------------------------------------------------------------------------------- FLAME vertices
struct artalk_flame {
    int device = 0, V = 0, NB = 0, NBp = 0, P = 0, Pp = 0, cap = 0;
    float scale = 1.f;
    DevBuf<float> v_template, shapedirs, posedirs, jreg, weights;
    DevBuf<int> parents;
    DevBuf<float> betas, feat, rot, J, vshaped, vposed;      // scratch of `cap` frames
    std::string err;
};

static thread_local std::string g_flame_error;

extern "C" {

const char* artalk_flame_last_error(const artalk_flame* f) { return f ? f->err.c_str() : g_flame_error.c_str(); }

void artalk_flame_destroy(artalk_flame* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    (void)hipDeviceSynchronize();
    delete f;
}

// Host arrays in the layouts of the reference's FLAMEModel buffers (app/flame_model/FLAME.py:36-45):
// v_template [V][3], shapedirs [V][3][NB], posedirs_t [V*3][P] (= the reference buffer transposed), J_regressor [5][V],
// parents [5] (parents[0] = -1), lbs_weights [V][5].
int artalk_flame_create(int device_id, int V, int NB, int P, const float* v_template, const float* shapedirs, const float* posedirs_t,
                        const float* J_regressor, const int32_t* parents, const float* lbs_weights, float scale, artalk_flame** out) {
    if (!out || !v_template || !shapedirs || !posedirs_t || !J_regressor || !parents || !lbs_weights || V <= 0 || NB <= 0 || P != 36) {
        g_flame_error = "bad argument (FLAME has 5 joints: posedirs must have 36 rows)";
        return ARTALK_EINVAL;
    }
    if (parents[0] != -1) { g_flame_error = "parents[0] must be -1"; return ARTALK_EINVAL; }
    for (int j = 1; j < 5; ++j) if (parents[j] < 0 || parents[j] >= j) { g_flame_error = "parents must form a tree in topological order"; return ARTALK_EINVAL; }
    if (hipSetDevice(device_id) != hipSuccess) { g_flame_error = "hipSetDevice failed"; return ARTALK_EHIP; }
    artalk_flame* f = new artalk_flame();
    f->device = device_id; f->V = V; f->NB = NB; f->P = P; f->scale = scale;
    f->NBp = (NB + 31) / 32 * 32; f->Pp = 64;
    auto up = [&](DevBuf<float>& d, const float* h, int64_t rows, int64_t cols, int64_t cols_pad) {      // pad columns stay zero
        if (!d.alloc_zero(rows * cols_pad)) return false;
        if (cols == cols_pad) { (void)hipMemcpy(d.get(), h, rows * cols * 4, hipMemcpyHostToDevice); }
        else (void)hipMemcpy2D(d.get(), cols_pad * 4, h, cols * 4, cols * 4, rows, hipMemcpyHostToDevice);
        return true;
    };
    if (!up(f->v_template, v_template, 1, (int64_t)V * 3, (int64_t)V * 3) ||
        !up(f->shapedirs, shapedirs, (int64_t)V * 3, NB, f->NBp) ||       // GEMM weight [N = 3V][K = NB padded]
        !up(f->posedirs, posedirs_t, (int64_t)V * 3, P, f->Pp) || !up(f->jreg, J_regressor, 5, V, V) || !up(f->weights, lbs_weights, V, 5, 5) ||
        !f->parents.alloc_zero(5)) {
        g_flame_error = "hipMalloc failed"; artalk_flame_destroy(f); return ARTALK_EHIP;
    }
    (void)hipMemcpy(f->parents.get(), parents, 5 * sizeof(int), hipMemcpyHostToDevice);
    if (hipDeviceSynchronize() != hipSuccess) { g_flame_error = "upload failed"; artalk_flame_destroy(f); return ARTALK_EHIP; }
    *out = f;
    return ARTALK_OK;
}

int artalk_flame_dims(const artalk_flame* f, int* V, int* NB, float* scale) {
    if (!f) { g_flame_error = "handle is NULL"; return ARTALK_EINVAL; }
    if (V) *V = f->V;
    if (NB) *NB = f->NB;
    if (scale) *scale = f->scale;
    return f->device;
}

// betas_dev [T][NB] (shape ++ expression), full_pose_dev [T][15] (global, neck, jaw, eye_l, eye_r axis-angles: FLAME.py:131-136)
// -> out_dev [T][V][3] = vertices * scale
int artalk_flame_verts(artalk_flame* f, const float* betas_dev, const float* full_pose_dev, int T, float* out_dev, void* stream) {
    if (!f || !betas_dev || !full_pose_dev || !out_dev || T <= 0) return ARTALK_EINVAL;
    (void)hipSetDevice(f->device);
    hipStream_t s = (hipStream_t)stream;
    if (T > f->cap) {
        (void)hipDeviceSynchronize();
        f->cap = 0;
        for (DevBuf<float>* b : {&f->betas, &f->feat, &f->rot, &f->J, &f->vshaped, &f->vposed}) b->reset();
        const int64_t N = (int64_t)f->V * 3;
        if (!f->betas.alloc_zero((int64_t)T * f->NBp) || !f->feat.alloc_zero((int64_t)T * f->Pp) || !f->rot.alloc_zero((int64_t)T * 45) ||
            !f->J.alloc_zero((int64_t)T * 15) || !f->vshaped.alloc_zero(T * N) || !f->vposed.alloc_zero(T * N)) {
            f->err = "hipMalloc failed"; return ARTALK_EHIP;
        }
        (void)hipDeviceSynchronize();   // zero fills run on the null stream
        f->cap = T;
    }
    const int N = f->V * 3;
    float *betas = f->betas.get(), *feat = f->feat.get(), *rot = f->rot.get(), *J = f->J.get(), *vshaped = f->vshaped.get(), *vposed = f->vposed.get();
    // betas into the K-padded GEMM operand (pad columns stay zero from allocation)
    if (hipMemcpy2DAsync(betas, (size_t)f->NBp * 4, betas_dev, (size_t)f->NB * 4, (size_t)f->NB * 4, T, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        f->err = "copy failed"; return ARTALK_EHIP;
    }
    GemmArgs g;     // v_shaped = v_template + betas . shapedirs^T      (exact fp32 MFMA)
    g.A = betas; g.lda = f->NBp; g.W = f->shapedirs.get(); g.ldw = f->NBp; g.C = vshaped; g.ldc = N; g.R = f->v_template.get(); g.ldr = 0;
    g.M = T; g.N = N; g.K = f->NBp;
    launch_gemm(g, s);
    launch_flame_joints(vshaped, f->jreg.get(), J, T, f->V, s);
    launch_flame_pose(full_pose_dev, rot, feat, T, f->Pp, s);
    GemmArgs p;     // v_posed = v_shaped + pose_feature . posedirs
    p.A = feat; p.lda = f->Pp; p.W = f->posedirs.get(); p.ldw = f->Pp; p.C = vposed; p.ldc = N; p.R = vshaped; p.ldr = N;
    p.M = T; p.N = N; p.K = f->Pp;
    launch_gemm(p, s);
    launch_flame_skin(vposed, rot, J, f->parents.get(), f->weights.get(), out_dev, T, f->V, f->scale, s);
    if (hipGetLastError() != hipSuccess) { f->err = "kernel launch failed"; return ARTALK_EHIP; }
    return ARTALK_OK;
}

}  // extern "C"
