// Single-kernel entry points of the C ABI (artalk_op_*): what the kernel-level tests and the tuning tools call.  None of them touches
// an artalk_model; from model.h they take the model's constants, the session table and the smoother's host checks (calls.hip).
#include "model.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstring>
#include <set>
#include <string>
#include <vector>

using namespace artalk;

extern "C" {

// ---------------------------------------------------------------------------------- single-kernel entry points
int artalk_op_gemm(const float* A, int64_t lda, const float* W, const float* bias, const float* gate, const float* R, float* C,
                   int M, int N, int K, int act, void* stream) {
    if (!A || !W || !C || K % 32 != 0 || M < 0 || N <= 0) return ARTALK_EINVAL;
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.bias = bias; g.C = C; g.ldc = N; g.gate = gate; g.ldg = N; g.R = R; g.ldr = N;
    g.M = M; g.N = N; g.K = K; g.act = act;
    launch_gemm(g, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// artalk_op_gemm with GemmArgs::ksum_blocks on: the kernels the DINO object launches (K summed in blocks of 256)
int artalk_op_gemm_blocked(const float* A, int64_t lda, const float* W, const float* bias, const float* gate, const float* R, float* C,
                           int M, int N, int K, int act, void* stream) {
    if (!A || !W || !C || K % 32 != 0 || M < 0 || N <= 0) return ARTALK_EINVAL;
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.bias = bias; g.C = C; g.ldc = N; g.gate = gate; g.ldg = N; g.R = R; g.ldr = N;
    g.M = M; g.N = N; g.K = K; g.act = act; g.ksum_blocks = 1;
    launch_gemm(g, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_gemm_ex(const float* A, int64_t lda, const float* W, const float* bias, float* C, int M, int N, int K, int act,
                      int force_cfg, void* stream) {
    if (!A || !W || !C || K % 32 != 0 || M < 0 || N <= 0 || force_cfg < -1 || force_cfg == 0 || force_cfg > 4) return ARTALK_EINVAL;
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.bias = bias; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = act;
    g.force_cfg = force_cfg;
    launch_gemm(g, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// out_dev: blocks*256 floats of scratch; *flops receives the FLOPs of the launch (time it with events on `stream`)
int artalk_op_mfma_f32_peak(float* out_dev, int blocks, int iters, int nacc, double* flops, void* stream) {
    if (!out_dev || !flops || blocks <= 0 || iters <= 0) return ARTALK_EINVAL;
    *flops = launch_mfma_f32_peak(out_dev, blocks, iters, nacc, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// f16x3 split GEMM on fp32 inputs (W is packed into a temporary): same contract as artalk_op_gemm_ex; cfg 0: 128x128, 1: 64x64, -1: heuristic
static bool op_exp_ok(int e) { return e >= -8 && e <= kActExp; }      // what artalk_set_site_scales accepts

int artalk_op_gemm_f16s(const float* A, int64_t lda, const float* W, const float* bias, float* C, int M, int N, int K, int act,
                        int force_cfg, void* stream) {
    return artalk_op_gemm_f16s_ex(A, lda, W, bias, C, M, N, K, act, force_cfg, kActExp, nullptr, stream);
}
// the same with the site exponent of A (split while staging, or packed with it under force_cfg | 0x100) and the model status word
int artalk_op_gemm_f16s_ex(const float* A, int64_t lda, const float* W, const float* bias, float* C, int M, int N, int K, int act,
                           int force_cfg, int a_exp, int* status_dev, void* stream) {
    if (!A || !W || !C || K % 32 != 0 || M <= 32 || N <= 0 || !op_exp_ok(a_exp)) return ARTALK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    DevBuf<unsigned int> wp, ap;
    if (!wp.alloc((size_t)N * K)) return ARTALK_EHIP;
    launch_pack_split(W, wp.get(), (long)N * K, true, s);
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = W; g.Wp = wp.get(); g.ldw = K; g.bias = bias; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = act;
    g.force_cfg = force_cfg & 0xff;
    g.a_exp = a_exp; g.status = status_dev;
    if (force_cfg >= 0 && (force_cfg & 0x100)) {   // tuning: pre-packed A (what a fused producer would hand over)
        if (!ap.alloc((size_t)M * lda)) return ARTALK_EHIP;
        launch_pack_split(A, ap.get(), (long)M * lda, false, s, status_dev, a_exp);
        g.A = reinterpret_cast<const float*>(ap.get()); g.a_packed = 1;
    }
    run_gemm(g, plan_gemm(g, GemmPolicy{1, true}, nullptr), nullptr, s);
    (void)hipStreamSynchronize(s);      // (the temporaries go when the function returns)
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// bf16 GEMM on fp32 inputs (W is converted into a temporary bf16 copy); C[m, n] = R + gate * act(bf16(A) bf16(W)^T + bias), ldc = ldg =
// ldr = N; A and W 16-byte aligned.  force_cfg: -1 = the engine's own tile choice, else bits 0-7 = tile of gemm_bf16_kernel (0: 64x64, 1: 128x128, 2: 32x128, 0xff: own
// choice), bits 8-15 = split-K factor (slabs in a temporary, finished by the split-K reduce pass), bits 16-23 = grid.z batch (A, W,
// bias, R and C of batch z follow each other: strides M*lda, N*K, N, M*N, M*N), bit 24 = amode 1 (grouped positional-conv window:
// pc_cin = 64, taps = K / 64, pad = taps / 2, rows of T = bits 25-30 frames each; the batch stride of A is then 64 columns).
int artalk_op_gemm_bf16(const float* A, int64_t lda, const float* W, const float* bias, const float* gate, const float* R, float* C,
                        int M, int N, int K, int act, int force_cfg, void* stream) {
    if (!A || !W || !C || K % 32 != 0 || M < 0 || N <= 0 || lda <= 0 || lda % 4 != 0) return ARTALK_EINVAL;
    if (((uintptr_t)A | (uintptr_t)W) & 15) return ARTALK_EINVAL;     // both are read with 16-byte vector loads (every batch's too: K % 32 == 0)
    const int cfg = force_cfg < 0 ? 0xff : force_cfg & 0xff;
    const int S = force_cfg < 0 ? 1 : std::max(1, (force_cfg >> 8) & 0xff);
    const int nb = force_cfg < 0 ? 1 : std::max(1, (force_cfg >> 16) & 0xff);
    const int am = force_cfg < 0 ? 0 : (force_cfg >> 24) & 1;
    const int T = force_cfg < 0 ? 0 : (force_cfg >> 25) & 63;
    if ((cfg > 2 && cfg != 0xff) || S > 16 || (am && (T <= 0 || M % T != 0 || K % 64 != 0 || nb * 64 > lda))) return ARTALK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    DevBuf<uint16_t> wb;
    DevBuf<float> part;
    if (!wb.alloc((size_t)nb * N * K)) return ARTALK_EHIP;
    if (S > 1 && !part.alloc((size_t)S * nb * M * N)) return ARTALK_EHIP;
    launch_pack_bf16(W, wb.get(), (long)nb * N * K, s);
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = W; g.Wb = wb.get(); g.ldw = K; g.bias = bias; g.C = C; g.ldc = N; g.gate = gate; g.ldg = N; g.R = R; g.ldr = N;
    g.M = M; g.N = N; g.K = K; g.act = act; g.force_cfg = cfg == 0xff ? -1 : cfg;
    g.batch = nb; g.sA = am ? 64 : (long)M * lda; g.sW = (long)N * K; g.sBias = bias ? N : 0; g.sC = (long)M * N; g.sR = R ? (long)M * N : 0;
    if (am) { g.amode = 1; g.pc_T = T; g.pc_tstride = T; g.pc_pad = K / 64 / 2; g.pc_cin = 64; }
    if (S > 1) {
        if (nb > 1 || am) return ARTALK_EINVAL;     // (split-K is a batch-1 plain-window form)
        g.splitk = S; g.partial = part.get();
    }
    run_gemm(g, plan_gemm(g, GemmPolicy{2}, nullptr), nullptr, s);
    (void)hipStreamSynchronize(s);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// split-K scratch of the tuning entry point below (never used by the model path): the current buffer and the ones it outgrew
// (never destroyed: at process exit the runtime may be gone before a static destructor runs; artalk_op_release_scratch frees them)
static DevBuf<float>& g_op_scratch = *new DevBuf<float>;
static std::vector<DevBuf<float>>& g_op_retired = *new std::vector<DevBuf<float>>;
// Frees every scratch buffer of artalk_op_gemm_f16s_packed (current and retired).  The caller guarantees that no captured graph
// that replays such a launch is used afterwards (tools/* destroy their graphs first; pytest calls it at session end).
int artalk_op_release_scratch(void) {
    if (hipDeviceSynchronize() != hipSuccess) return ARTALK_EHIP;
    g_op_retired.clear();
    g_op_scratch.reset();
    return ARTALK_OK;
}
// building blocks for tuning the split GEMM without allocation noise: pack once, then launch on packed operands
int artalk_op_pack_split(const float* in, void* out_u32, int64_t n, int is_weight, void* stream) {
    return artalk_op_pack_split_ex(in, out_u32, n, is_weight, kActExp, nullptr, stream);
}
int artalk_op_pack_split_ex(const float* in, void* out_u32, int64_t n, int is_weight, int p8_exp, int* status_dev, void* stream) {
    if (!in || !out_u32 || n <= 0 || !op_exp_ok(p8_exp)) return ARTALK_EINVAL;
    launch_pack_split(in, (unsigned int*)out_u32, n, is_weight != 0, (hipStream_t)stream, status_dev, p8_exp);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_gemm_f16s_packed(const void* A, int a_packed, int64_t lda, const void* Wp, const float* bias, float* C, int M, int N,
                               int K, int act, int force_cfg, void* stream) {
    return artalk_op_gemm_f16s_packed_ex(A, a_packed, lda, Wp, bias, C, M, N, K, act, force_cfg, kActExp, kActExp, nullptr, nullptr, stream);
}
int artalk_op_gemm_f16s_packed_ex(const void* A, int a_packed, int64_t lda, const void* Wp, const float* bias, float* C, int M, int N,
                                  int K, int act, int force_cfg, int a_exp, int c_exp, void* c2_u32, int* status_dev, void* stream) {
    if (!A || !Wp || !C || K % 32 != 0 || M <= 0 || N <= 0 || (M <= 32 && (force_cfg & 0xff) < 20)) return ARTALK_EINVAL;
    if (!op_exp_ok(a_exp) || !op_exp_ok(c_exp)) return ARTALK_EINVAL;
    if (c2_u32 && (force_cfg < 2 || ((act >> 8) & 1) || N % 8 != 0)) return ARTALK_EINVAL;      // the second copy: LDS-DMA kernels, fp32 C
    if (force_cfg >= 2 && 32 * ((force_cfg >> 8) & 0xff) > K) return ARTALK_EINVAL;      // a split factor that leaves a workgroup no K step
    GemmArgs g;
    g.a_exp = a_exp; g.c_exp = c_exp; g.status = status_dev; g.c2 = (float*)c2_u32;
    g.A = (const float*)A; g.a_packed = a_packed; g.lda = lda; g.W = nullptr; g.Wp = (const unsigned int*)Wp; g.ldw = K; g.bias = bias;
    g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = act & 0xff; g.force_cfg = force_cfg;
    g.c_p8 = (act >> 8) & 1;      // tuning: bit 8 of `act` = result in the P8 split format (same pitch)
    if ((act >> 9) & 1) { g.R = C; g.ldr = N; }      // tuning: bit 9 = residual read from C (in place, as the encoder's out-projection / FFN-out run)
    if (force_cfg >= 2) {   // LDS-DMA kernels (both operands in P8): include/artalk_hip.h lists the configurations
        int cfg = force_cfg & 0xff;
        const int S = (force_cfg >> 8) & 0xff;
        // retired configurations stay valid and run what replaced them (same accumulation order, same bits): 13 (the non-persistent
        // 256x256 kernel) the plan, 29 (the 5-stage mid-grid ring) and 33 (the 128x128 ping-pong form) the mid-grid kernel, 30 (the
        // one-barrier ping-pong form) the two-barrier one
        if (cfg == 13) cfg = 99;
        else if (cfg == 29 || cfg == 33) cfg = 28;
        else if (cfg == 30) cfg = 31;
        const int cls = gemm_p8_class(cfg);
        if (!a_packed || (cls == P8_NONE && cfg != 99)) return ARTALK_EINVAL;
        g.force_cfg = cfg == 99 ? -1 : cfg;      // 99: the planner's own choice (without split-K)
        if (cls == P8_SMALL) {     // bits 8-15: split-K factor (slabs in a temporary)
            g.w_nt = (force_cfg >> 16) & 1;      // tuning: bit 16 = non-temporal weight pieces
            if (S > 1) {
                const size_t need = (size_t)S * M * N;      // floats
                if (need > g_op_scratch.capacity()) {
                    // a smaller scratch is NOT freed here: graphs captured from earlier calls (tools/gemm_f16s_bench.py replays one per
                    // variant) still write to it - freeing it turned their replay into a memory fault.  It is RETIRED instead and freed by
                    // artalk_op_release_scratch(), which the owner of those graphs calls once they are gone.  At least 64 MB, so that it rarely grows.
                    DevBuf<float> fresh;
                    if (!fresh.alloc(std::max(need, (size_t)16 << 20))) return ARTALK_EHIP;
                    if (g_op_scratch.get()) g_op_retired.push_back(std::move(g_op_scratch));
                    g_op_scratch = std::move(fresh);
                }
                g.splitk = S; g.partial = g_op_scratch.get();
            }
        }
    }
    const GemmPlan plan = plan_gemm(g, GemmPolicy{1, force_cfg < 2}, nullptr);
    if (force_cfg >= 2 && plan.path != GEMM_P8) return ARTALK_EINVAL;      // (a P8 row pitch the LDS-DMA kernels cannot read)
    run_gemm(g, plan, nullptr, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// A HIP stream restricted to a set of compute units (hipExtStreamCreateWithCUMask): bit i of the mask = CU (i / 8) of XCD (i % 8) on
// MI355X (tools/cu_mask_probe.hip), so the low / high 128 bits are the two halves of every XCD.  The stream a model restricted with
// artalk_set_cu_mask is driven on.
int artalk_op_create_masked_stream(const uint32_t* mask, int n_words, void** out_stream) {
    if (!mask || !out_stream || n_words <= 0) return ARTALK_EINVAL;
    hipStream_t s = nullptr;
    if (hipExtStreamCreateWithCUMask(&s, (uint32_t)n_words, mask) != hipSuccess) return ARTALK_EHIP;
    *out_stream = s;
    return ARTALK_OK;
}
int artalk_op_destroy_stream(void* stream) { return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? ARTALK_OK : ARTALK_EHIP; }

int artalk_op_gemm_p8_plan(int M, int N, int K, int residual) {
    GemmArgs g;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N; g.a_packed = 1;
    g.Wp = reinterpret_cast<const unsigned int*>(16);      // only its presence and alignment are looked at (so are R's)
    if (residual) { g.R = reinterpret_cast<const float*>(16); g.ldr = N; }
    plan_gemm(g, GemmPolicy{1}, nullptr);
    return g.force_cfg;
}

int artalk_op_layernorm(const float* X, float* Y, const float* w, const float* b, const float* scale, const float* shift, int M,
                        int D, float eps, int act, void* stream) {
    return artalk_op_layernorm_ex(X, Y, w, b, scale, shift, M, D, eps, act, kActExp, 0, 0, nullptr, stream);
}
int artalk_op_layernorm_ex(const float* X, float* Y, const float* w, const float* b, const float* scale, const float* shift, int M,
                           int D, float eps, int act, int p8_exp, int junk_period, int junk_from, int* status_dev, void* stream) {
    if (!X || !Y || (D != 128 && D != 512 && D != 768 && D != 1024) || !op_exp_ok(p8_exp)) return ARTALK_EINVAL;
    if (junk_period < 0 || junk_from < 0 || (junk_period > 0 && junk_from > junk_period)) return ARTALK_EINVAL;
    if ((act & 0x100) && D == 128) return ARTALK_EINVAL;      // the 128-wide kernel (style encoder: fp32 A sites) has no P8 store
    LnArgs a;
    a.p8_exp = p8_exp; a.junk_period = junk_period; a.junk_from = junk_from; a.status = (act & 0x100) ? status_dev : nullptr;
    a.X = X; a.ldx = D; a.Y = Y; a.ldy = D; a.w = w; a.b = b; a.scale = scale; a.shift = shift; a.ldm = D; a.M = M; a.D = D;
    a.eps = eps; a.act = act & 0xff; a.out_p8 = (act & 0x100) ? 1 : 0;   // act | 0x100: write Y in the P8 split format
    launch_layernorm(a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_attention(const float* Q, const float* K, const float* V, float* O, int B, int H, int HD, int Lq, int Lk, float scale,
                        int l2norm, const float* qscale, int split, void* stream) {
    return artalk_op_attention_ex(Q, K, V, O, B, H, HD, Lq, Lk, scale, l2norm, qscale, split, kActExp, kActExp, 0, nullptr, stream);
}
int artalk_op_attention_ex(const float* Q, const float* K, const float* V, float* O, int B, int H, int HD, int Lq, int Lk, float scale,
                           int l2norm, const float* qscale, int split, int qkv_exp, int o_exp, int out_p8, int* status_dev, void* stream) {
    if (!Q || !K || !V || !O || (HD != 64 && HD != 32) || ((l2norm & 1) && !qscale)) return ARTALK_EINVAL;
    if (!op_exp_ok(qkv_exp) || !op_exp_ok(o_exp)) return ARTALK_EINVAL;
    AttnArgs a;
    a.qkv_exp = qkv_exp; a.o_exp = o_exp; a.out_p8 = out_p8 ? 1 : 0; a.status = out_p8 ? status_dev : nullptr;
    a.split16 = (l2norm >> 1) & 1;      // l2norm | 2: the fp16 operand-split kernel of f16x3 mode
    a.qkv_p8 = (l2norm >> 2) & 1;       // l2norm | 4 (with | 2, without L2 norm): Q, K, V are given in the P8 split format
    l2norm &= 1;
    const long D = (long)H * HD;
    a.Q = Q; a.K = K; a.V = V; a.O = O; a.ldq = a.ldk = a.ldv = a.ldo = D;
    a.q_bstride = a.o_bstride = (long)Lq * D; a.k_bstride = a.v_bstride = (long)Lk * D;
    a.B = B; a.H = H; a.HD = HD; a.Lq = Lq; a.Lk = Lk; a.scale = scale; a.l2norm = l2norm; a.qscale = qscale;
    a.split_q = split; a.split_k = split;
    launch_attention(a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// ---- the launchers in the forms the AR / VAE / style bodies use them (include/artalk_hip.h).  Everything is checked on the host first:
// a launch is made only when every row, column group and batch it addresses lies inside the sizes the caller states.
static bool op_map_ok(const int32_t* m) { return m[0] > 0 && m[1] >= 0 && m[2] >= 0; }
// the largest row a map sends rows 0 .. M-1 to (the last row of the last batch, or of the one before it when the last is short)
static int64_t op_map_last(const int32_t* m, int M) {
    if (m[0] == INT_MAX) return (int64_t)M - 1;
    const int64_t rpb = m[0], bs = m[1], off = m[2], qb = (M - 1) / rpb, rem = (M - 1) % rpb;
    int64_t last = qb * bs + off + rem;
    if (qb > 0) last = std::max(last, (qb - 1) * bs + off + rpb - 1);
    return last;
}
static bool op_al(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }
// rows 0 .. last of pitch ld, `width` elements each, inside `elems` (all in 4-byte elements)
static bool op_fits(int64_t last, int64_t ld, int64_t width, int64_t elems) {
    return last >= 0 && ld >= 0 && width > 0 && last <= INT_MAX && last * ld + width <= elems;
}
// two buffers of na / nb 4-byte elements share a byte
static bool op_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}
// distance in elements between the scale and shift rows of one modulation table (-1: not a whole number of elements)
static int64_t op_mod_gap(const float* scale, const float* shift) {
    const uintptr_t a = (uintptr_t)scale, b = (uintptr_t)shift, d = a < b ? b - a : a - b;
    return d % 4 == 0 ? (int64_t)(d / 4) : -1;
}
// artalk_op_rows_dry_run: the three entry points below return ARTALK_OK where they would touch the device
static thread_local bool g_rows_dry_run = false;
int artalk_op_rows_dry_run(int enable) { g_rows_dry_run = enable != 0; return ARTALK_OK; }

#define ROWS_FIELD(f) (int64_t)offsetof(artalk_op_gemm_rows_args, f)
int artalk_op_gemm_rows_layout(int64_t* out, int n) {
    static const int64_t lay[] = {
        (int64_t)sizeof(artalk_op_gemm_rows_args),
        ROWS_FIELD(mode), ROWS_FIELD(M), ROWS_FIELD(N), ROWS_FIELD(K), ROWS_FIELD(act), ROWS_FIELD(A), ROWS_FIELD(lda), ROWS_FIELD(a_elems),
        ROWS_FIELD(a_exp), ROWS_FIELD(W), ROWS_FIELD(ldw), ROWS_FIELD(w_elems), ROWS_FIELD(bias), ROWS_FIELD(bias_elems), ROWS_FIELD(C),
        ROWS_FIELD(ldc), ROWS_FIELD(c_elems), ROWS_FIELD(cmap), ROWS_FIELD(gate), ROWS_FIELD(ldg), ROWS_FIELD(gate_elems), ROWS_FIELD(gmap),
        ROWS_FIELD(R), ROWS_FIELD(ldr), ROWS_FIELD(r_elems), ROWS_FIELD(c_p8), ROWS_FIELD(c_exp), ROWS_FIELD(force_cfg), ROWS_FIELD(splitk),
        ROWS_FIELD(ngrp), ROWS_FIELD(grpW), ROWS_FIELD(grpB), ROWS_FIELD(grpC), ROWS_FIELD(status_dev), ROWS_FIELD(ln_Y), ROWS_FIELD(ln_ldy),
        ROWS_FIELD(ln_y_elems), ROWS_FIELD(ln_scale), ROWS_FIELD(ln_shift), ROWS_FIELD(ln_ldm), ROWS_FIELD(ln_mod_elems), ROWS_FIELD(ln_mmap),
        ROWS_FIELD(ln_eps), ROWS_FIELD(ln_out_p8), ROWS_FIELD(ln_p8_exp), ROWS_FIELD(used_cfg), ROWS_FIELD(used_splitk), ROWS_FIELD(fused_ln),
        ROWS_FIELD(cus)};
    const int total = (int)(sizeof(lay) / sizeof(lay[0]));
    if (!out || n < total) return ARTALK_EINVAL;
    for (int i = 0; i < total; ++i) out[i] = lay[i];
    return total;
}
#undef ROWS_FIELD

int artalk_op_gemm_rows(const artalk_op_gemm_rows_args* a, void* stream) {
    if (!a || !a->A || !a->W || !a->C || a->mode < 0 || a->mode > 2) return ARTALK_EINVAL;
    const int M = a->M, N = a->N, K = a->K;
    if (M <= 0 || N <= 0 || K <= 0 || K % 32 != 0 || a->act < 0 || a->act > 3) return ARTALK_EINVAL;
    if (!op_exp_ok(a->a_exp) || !op_exp_ok(a->c_exp) || !op_exp_ok(a->ln_p8_exp)) return ARTALK_EINVAL;
    if (!op_map_ok(a->cmap) || !op_map_ok(a->gmap) || !op_map_ok(a->ln_mmap)) return ARTALK_EINVAL;
    if (a->lda <= 0 || a->ldw < K || a->ldc <= 0) return ARTALK_EINVAL;
    const bool p8 = a->mode == 1, ident_c = a->cmap[0] == INT_MAX;
    if (a->c_p8 && (!p8 || N % 8 != 0 || a->ldc % 8 != 0)) return ARTALK_EINVAL;
    // alignment: A and W rows are read as 16-byte vectors (P8 rows as 32-byte groups); the f16x3 kernels take the 16-byte epilogue only
    const int ka = p8 ? 8 : 4, kw = a->mode == 0 ? 4 : 8;
    if (!op_al(a->A, 16) || !op_al(a->W, 16) || a->lda % ka != 0 || a->ldw % kw != 0) return ARTALK_EINVAL;
    if (p8) {
        if (!op_al(a->C, 16) || !op_al(a->bias, 16) || !op_al(a->gate, 16) || !op_al(a->R, 16) || N % 4 != 0 || a->ldc % 4 != 0) return ARTALK_EINVAL;
        if ((a->R && a->ldr % 4 != 0) || (a->gate && a->ldg % 4 != 0)) return ARTALK_EINVAL;
    }
    // tile configuration and split
    const int cfg = (a->force_cfg == -1 || a->force_cfg == 99) ? -1 : a->force_cfg;
    if (cfg != -1 && !(a->mode == 0 ? (cfg >= 1 && cfg <= 4) : a->mode == 2 ? (cfg >= 0 && cfg <= 2) : gemm_p8_class(cfg) != P8_NONE))
        return ARTALK_EINVAL;
    if (a->splitk < 0 || a->splitk > 16 || (a->splitk > 1 && 32 * a->splitk > K)) return ARTALK_EINVAL;
    if (a->cus < 0 || (a->cus != 0 && !p8)) return ARTALK_EINVAL;      // a CU partition sizes the grid of the persistent f16x3 kernels only
    // column groups
    const int G = a->ngrp ? N / a->ngrp : 1;
    if (a->ngrp) {
        if (!p8 || a->ngrp < 0 || a->ngrp % 128 != 0 || N % a->ngrp != 0 || a->grpW < 0 || a->grpB < 0 || a->grpC < 0 || a->grpW % 8 != 0 ||
            a->grpB % 4 != 0 || a->grpC % 4 != 0 || a->gate || a->R || a->ln_Y || a->splitk > 1 || (cfg != -1 && gemm_p8_class(cfg) != P8_GROUPS))
            return ARTALK_EINVAL;
    }
    const int64_t gw = a->ngrp ? a->ngrp : N;      // columns one group (or the whole launch) touches from its base
    // sizes: A, W, bias, C, R, gate
    if (!op_fits(M - 1, a->lda, K, a->a_elems)) return ARTALK_EINVAL;
    const int64_t w_last = (int64_t)(G - 1) * a->grpW + (gw - 1) * a->ldw + K;      // elements of W the launch reads (and the copy holds)
    if (w_last > a->w_elems) return ARTALK_EINVAL;
    if (a->bias && (int64_t)(G - 1) * a->grpB + gw > a->bias_elems) return ARTALK_EINVAL;
    const int64_t c_last = op_map_last(a->cmap, M);
    if (!ident_c && M > a->cmap[0] && a->cmap[1] < a->cmap[0]) return ARTALK_EINVAL;      // result rows of two batches would collide
    if (a->ldc < gw || !op_fits(c_last, a->ldc, (int64_t)(G - 1) * a->grpC + gw, a->c_elems)) return ARTALK_EINVAL;
    if (a->R && (a->ldr < N || !op_fits(c_last, a->ldr, N, a->r_elems))) return ARTALK_EINVAL;
    // a residual in place is read and written by the same lane; any other overlap of R and C would race between rows
    if (a->R && !((const void*)a->R == (const void*)a->C && a->ldr == a->ldc) &&
        op_overlap(a->R, c_last * a->ldr + N, a->C, c_last * a->ldc + N))
        return ARTALK_EINVAL;
    if (a->gate && (a->ldg < N || !op_fits(op_map_last(a->gmap, M), a->ldg, N, a->gate_elems))) return ARTALK_EINVAL;
    // the LayerNorm that follows
    LnArgs ln;
    if (a->ln_Y) {
        if (N != kE || a->c_p8 || !a->ln_scale || !a->ln_shift || a->ln_ldm < kE || a->ln_ldy < kE || a->ln_ldm % 4 != 0 || a->ln_ldy % 4 != 0 ||
            a->ldc % 4 != 0 || !op_al(a->C, 16) || !op_al(a->ln_Y, 16) || !op_al(a->ln_scale, 16) || !op_al(a->ln_shift, 16))
            return ARTALK_EINVAL;
        if (a->ln_out_p8 && a->ln_ldy % 8 != 0) return ARTALK_EINVAL;
        if (!op_fits(M - 1, a->ln_ldy, kE, a->ln_y_elems)) return ARTALK_EINVAL;
        const int64_t gap = op_mod_gap(a->ln_scale, a->ln_shift);
        if (gap < 0 || !op_fits(op_map_last(a->ln_mmap, M), a->ln_ldm, gap + kE, a->ln_mod_elems)) return ARTALK_EINVAL;
        if (op_overlap(a->ln_Y, (int64_t)(M - 1) * a->ln_ldy + kE, a->C, c_last * a->ldc + N)) return ARTALK_EINVAL;
        ln.X = (const float*)a->C; ln.ldx = a->ldc; ln.Y = (float*)a->ln_Y; ln.ldy = a->ln_ldy; ln.scale = a->ln_scale; ln.shift = a->ln_shift;
        ln.ldm = a->ln_ldm; ln.mmap = RowMap{a->ln_mmap[0], a->ln_mmap[1], a->ln_mmap[2]}; ln.M = M; ln.D = kE; ln.eps = a->ln_eps;
        ln.out_p8 = a->ln_out_p8 ? 1 : 0; ln.p8_exp = a->ln_p8_exp; ln.status = a->ln_out_p8 ? a->status_dev : nullptr;
    }
    GemmArgs g;
    g.A = (const float*)a->A; g.lda = a->lda; g.a_packed = p8 ? 1 : 0; g.a_exp = a->a_exp; g.W = a->W; g.ldw = a->ldw; g.bias = a->bias;
    g.C = (float*)a->C; g.ldc = a->ldc; g.cmap = RowMap{a->cmap[0], a->cmap[1], a->cmap[2]}; g.c_p8 = a->c_p8 ? 1 : 0; g.c_exp = a->c_exp;
    g.gate = a->gate; g.ldg = a->ldg; g.gmap = RowMap{a->gmap[0], a->gmap[1], a->gmap[2]}; g.R = a->R; g.ldr = a->ldr;
    g.M = M; g.N = N; g.K = K; g.act = a->act; g.force_cfg = cfg; g.status = a->status_dev;
    g.ngrp = a->ngrp; g.grpW = a->grpW; g.grpB = a->grpB; g.grpC = a->grpC; g.cus = a->cus;
    // a forced split is kept; with splitk 0 and no forced configuration the f16x3 planner may split on its own (the other families'
    // small-grid rule stays off).  The planner looks at the presence of Wp and the alignment of the slabs only: both are made below.
    g.splitk = a->splitk > 1 ? a->splitk : 1;
    if (p8) g.Wp = reinterpret_cast<const unsigned int*>(16);
    const GemmPolicy pol{a->mode, false, reinterpret_cast<float*>(16), p8 && a->splitk == 0 && cfg == -1 ? (int64_t)8 * M * N : 0};
    const GemmPlan plan = plan_gemm(g, pol, a->ln_Y ? &ln : nullptr);
    if (a->ngrp && gemm_p8_class(plan.cfg) != P8_GROUPS) return ARTALK_EINVAL;
    if (p8 && a->splitk > 1 && gemm_p8_class(plan.cfg) != P8_SMALL) return ARTALK_EINVAL;
    if (a->ln_Y && !plan.fused_ln && !ident_c) return ARTALK_EINVAL;      // launch_layernorm reads x as dense rows
    if (a->used_cfg) *a->used_cfg = plan.cfg;
    if (a->used_splitk) *a->used_splitk = g.splitk;
    if (a->fused_ln) *a->fused_ln = plan.fused_ln ? 1 : 0;
    if (g_rows_dry_run) return ARTALK_OK;
    // ---- the device from here on
    hipStream_t s = (hipStream_t)stream;
    DevBuf<unsigned char> wcopy;      // the weights packed (4 bytes each) or in bf16 (2 bytes each)
    DevBuf<float> part;
    if (a->mode != 0 && !wcopy.alloc((size_t)w_last * (p8 ? 4 : 2))) return ARTALK_EHIP;
    if (g.splitk > 1 && !part.alloc((size_t)g.splitk * M * N)) return ARTALK_EHIP;
    g.partial = part.get();
    if (p8) { launch_pack_split(a->W, (unsigned int*)wcopy.get(), w_last, true, s); g.Wp = (const unsigned int*)wcopy.get(); }
    if (a->mode == 2) { launch_pack_bf16(a->W, wcopy.get(), w_last, s); g.Wb = wcopy.get(); }
    run_gemm(g, plan, &ln, s);
    if (a->ln_Y && !plan.fused_ln) launch_layernorm(ln, s);
    const hipError_t e1 = hipStreamSynchronize(s);
    return (e1 == hipSuccess && hipGetLastError() == hipSuccess) ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_layernorm_rows(const float* X, float* Y, const float* w, const float* b, const float* scale, const float* shift, int M,
                             int D, float eps, int act, int p8_exp, int junk_period, int junk_from, int* status_dev, int64_t ldx,
                             int64_t ldy, int64_t ldm, const int32_t* mmap, int64_t x_elems, int64_t y_elems, int64_t mod_elems,
                             void* stream) {
    if (!X || !Y || !mmap || M <= 0 || (D != 128 && D != 512 && D != 768 && D != 1024) || !op_exp_ok(p8_exp)) return ARTALK_EINVAL;
    if (junk_period < 0 || junk_from < 0 || (junk_period > 0 && junk_from > junk_period)) return ARTALK_EINVAL;
    if ((act & 0x100) && D == 128) return ARTALK_EINVAL;      // the 128-wide kernel has no P8 store
    if ((w == nullptr) != (b == nullptr) || (scale == nullptr) != (shift == nullptr) || !op_map_ok(mmap)) return ARTALK_EINVAL;
    const int vb = D == 128 ? 8 : 16, ve = vb / 4;      // bytes / elements of one access of the kernel (float2 at D = 128, 16 bytes otherwise)
    if (!op_al(X, vb) || !op_al(Y, vb) || !op_al(w, vb) || !op_al(b, vb) || !op_al(scale, vb) || !op_al(shift, vb)) return ARTALK_EINVAL;
    if (ldx < D || ldy < D || ldx % ve != 0 || ldy % ve != 0 || ((act & 0x100) && ldy % 8 != 0)) return ARTALK_EINVAL;
    if (!op_fits(M - 1, ldx, D, x_elems) || !op_fits(M - 1, ldy, D, y_elems)) return ARTALK_EINVAL;
    if (scale) {
        if (ldm < D || ldm % ve != 0) return ARTALK_EINVAL;
        const int64_t gap = op_mod_gap(scale, shift);
        if (gap < 0 || !op_fits(op_map_last(mmap, M), ldm, gap + D, mod_elems)) return ARTALK_EINVAL;
    }
    // in place only row on row (a wave reads its row before it writes it); any other overlap of X and Y would race between rows
    if (!((const void*)X == (const void*)Y && ldx == ldy) && op_overlap(X, (int64_t)(M - 1) * ldx + D, Y, (int64_t)(M - 1) * ldy + D))
        return ARTALK_EINVAL;
    if (g_rows_dry_run) return ARTALK_OK;
    LnArgs a;
    a.p8_exp = p8_exp; a.junk_period = junk_period; a.junk_from = junk_from; a.status = (act & 0x100) ? status_dev : nullptr;
    a.X = X; a.ldx = ldx; a.Y = Y; a.ldy = ldy; a.w = w; a.b = b; a.scale = scale; a.shift = shift; a.ldm = ldm;
    a.mmap = RowMap{mmap[0], mmap[1], mmap[2]}; a.M = M; a.D = D;
    a.eps = eps; a.act = act & 0xff; a.out_p8 = (act & 0x100) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    launch_layernorm(a, s);
    const hipError_t e1 = hipStreamSynchronize(s);
    return (e1 == hipSuccess && hipGetLastError() == hipSuccess) ? ARTALK_OK : ARTALK_EHIP;
}

static_assert(ATTN_F32_64 == ARTALK_ATTN_F32_64 && ATTN_F32_32 == ARTALK_ATTN_F32_32 && ATTN_SHORT == ARTALK_ATTN_SHORT && ATTN_F16 == ARTALK_ATTN_F16 &&
              ATTN_F16_P8 == ARTALK_ATTN_F16_P8 && ATTN_F16_WIDE == ARTALK_ATTN_F16_WIDE && ATTN_F16_PP == ARTALK_ATTN_F16_PP &&
              ATTN_F16_WIDE_AR == ARTALK_ATTN_F16_WIDE_AR && ATTN_F16_WIDE_AR_P8 == ARTALK_ATTN_F16_WIDE_AR_P8, "include/artalk_hip.h");
// the shape, flag and partition checks artalk_op_attention_rows_cus and artalk_op_attention_plan share
static bool op_attn_shape_ok(int B, int H, int HD, int Lq, int Lk, int l2norm, int split, int out_p8, int cus) {
    if ((HD != 64 && HD != 32) || B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0 || split < 0 || l2norm < 0 || l2norm > 7 || cus < 0) return false;
    const int split16 = (l2norm >> 1) & 1, qkv_p8 = (l2norm >> 2) & 1;
    if ((split16 || qkv_p8 || out_p8) && HD != 64) return false;      // the f16 kernels and the P8 rows are 64-wide heads
    return !(qkv_p8 && (!split16 || (l2norm & 1)));
}
int artalk_op_attention_plan(int B, int H, int HD, int Lq, int Lk, int l2norm, int split, int cus, int n_cu) {
    if (!op_attn_shape_ok(B, H, HD, Lq, Lk, l2norm, split, 0, cus) || n_cu <= 0) return ARTALK_EINVAL;
    AttnArgs a;
    a.B = B; a.H = H; a.HD = HD; a.Lq = Lq; a.Lk = Lk; a.l2norm = l2norm & 1; a.split16 = (l2norm >> 1) & 1; a.qkv_p8 = (l2norm >> 2) & 1;
    a.split_q = split; a.split_k = split; a.cus = cus;
    return (int)plan_attention(a, n_cu);
}
int artalk_op_attention_rows(const float* Q, const float* K, const float* V, float* O, int B, int H, int HD, int Lq, int Lk,
                             float scale, int l2norm, const float* qscale, int split, int qkv_exp, int o_exp, int out_p8,
                             int* status_dev, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bstride, int64_t k_bstride,
                             int64_t v_bstride, int64_t o_bstride, int64_t q_elems, int64_t k_elems, int64_t v_elems, int64_t o_elems,
                             void* stream) {
    return artalk_op_attention_rows_cus(Q, K, V, O, B, H, HD, Lq, Lk, scale, l2norm, qscale, split, qkv_exp, o_exp, out_p8, status_dev, ldq, ldk,
                                        ldv, ldo, q_bstride, k_bstride, v_bstride, o_bstride, q_elems, k_elems, v_elems, o_elems, 0, nullptr,
                                        stream);
}
int artalk_op_attention_rows_cus(const float* Q, const float* K, const float* V, float* O, int B, int H, int HD, int Lq, int Lk,
                                 float scale, int l2norm, const float* qscale, int split, int qkv_exp, int o_exp, int out_p8,
                                 int* status_dev, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bstride, int64_t k_bstride,
                                 int64_t v_bstride, int64_t o_bstride, int64_t q_elems, int64_t k_elems, int64_t v_elems, int64_t o_elems,
                                 int cus, int* used_kernel, void* stream) {
    if (!Q || !K || !V || !O || (HD != 64 && HD != 32) || ((l2norm & 1) && !qscale)) return ARTALK_EINVAL;
    if (!op_exp_ok(qkv_exp) || !op_exp_ok(o_exp)) return ARTALK_EINVAL;
    if (!op_attn_shape_ok(B, H, HD, Lq, Lk, l2norm, split, out_p8, cus)) return ARTALK_EINVAL;
    const int split16 = (l2norm >> 1) & 1, qkv_p8 = (l2norm >> 2) & 1;
    const int64_t D = (int64_t)H * HD;
    // rows are read and written as 16-byte vectors, P8 rows as 32-byte groups
    const int kin = qkv_p8 ? 8 : 4, kout = out_p8 ? 8 : 4;
    if (!op_al(Q, 4 * kin) || !op_al(K, 4 * kin) || !op_al(V, 4 * kin) || !op_al(O, 4 * kout)) return ARTALK_EINVAL;
    if (ldq % kin != 0 || ldk % kin != 0 || ldv % kin != 0 || ldo % kout != 0 || q_bstride % kin != 0 || k_bstride % kin != 0 ||
        v_bstride % kin != 0 || o_bstride % kout != 0)
        return ARTALK_EINVAL;
    if (ldq < D || ldk < D || ldv < D || ldo < D || q_bstride < 0 || k_bstride < 0 || v_bstride < 0) return ARTALK_EINVAL;
    if (B > 1 && o_bstride < (int64_t)(Lq - 1) * ldo + D) return ARTALK_EINVAL;      // output batches would overlap
    auto fits = [&](int64_t bstride, int64_t ld, int L, int64_t elems) {
        return (int64_t)(B - 1) * bstride + (int64_t)(L - 1) * ld + D <= elems;
    };
    if (!fits(q_bstride, ldq, Lq, q_elems) || !fits(k_bstride, ldk, Lk, k_elems) || !fits(v_bstride, ldv, Lk, v_elems) ||
        !fits(o_bstride, ldo, Lq, o_elems))
        return ARTALK_EINVAL;
    AttnArgs a;
    a.qkv_exp = qkv_exp; a.o_exp = o_exp; a.out_p8 = out_p8 ? 1 : 0; a.status = out_p8 ? status_dev : nullptr;
    a.split16 = split16; a.qkv_p8 = qkv_p8;
    a.Q = Q; a.K = K; a.V = V; a.O = O; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.q_bstride = q_bstride; a.k_bstride = k_bstride; a.v_bstride = v_bstride; a.o_bstride = o_bstride;
    a.B = B; a.H = H; a.HD = HD; a.Lq = Lq; a.Lk = Lk; a.scale = scale; a.l2norm = l2norm & 1; a.qscale = qscale;
    a.split_q = split; a.split_k = split; a.cus = cus;
    if (g_rows_dry_run) {
        if (used_kernel) *used_kernel = (int)plan_attention(a, 0);
        return ARTALK_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    const AttnKernel ran = launch_attention(a, s);
    if (used_kernel) *used_kernel = (int)ran;
    const hipError_t e1 = hipStreamSynchronize(s);
    return (e1 == hipSuccess && hipGetLastError() == hipSuccess) ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_w2v_front(const float* audio, int C, int n, const float* w, const float* bias, const float* lnw, const float* lnb,
                        float* xnorm_out, float* Y, void* stream) {
    return artalk_op_w2v_front_ex(audio, C, n, w, bias, lnw, lnb, xnorm_out, Y, 0, kActExp, nullptr, stream);
}
int artalk_op_w2v_front_ex(const float* audio, int C, int n, const float* w, const float* bias, const float* lnw, const float* lnb,
                           float* xnorm_out, float* Y, int out_p8, int p8_exp, int* status_dev, void* stream) {
    if (!audio || !xnorm_out || !Y || C <= 0 || n < 10 || !op_exp_ok(p8_exp)) return ARTALK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    std::vector<long> off(C);
    for (int i = 0; i < C; ++i) off[i] = (long)i * n;
    DevBuf<long> doff;
    if (!doff.alloc(C)) return ARTALK_EHIP;
    (void)hipMemcpy(doff.get(), off.data(), C * sizeof(long), hipMemcpyHostToDevice);
    const int T = (n - 10) / 5 + 1;
    launch_audio_normalize(audio, doff.get(), xnorm_out, C, n, s);
    launch_conv0(xnorm_out, n, w, bias, lnw, lnb, Y, C, T, T, s, out_p8 ? 1 : 0, out_p8 ? status_dev : nullptr, p8_exp);
    (void)hipStreamSynchronize(s);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_resample_mean(const float* x, int nch, int n, const float* taps, int orig, int nw, int width, float* out, int n_out,
                            void* stream) {
    if (!x || !taps || !out || nch <= 0 || n <= 0 || orig <= 0 || nw <= 0 || width < 0 || n_out < 0) return ARTALK_EINVAL;
    // the kernel's loop index is an int that advances by up to 2^20 per trip, and outputs past ceil(n * nw / orig) hear no input
    if (n_out > 2147483647 - (1 << 20) || (long long)n_out > ((long long)n * nw + orig - 1) / orig) return ARTALK_EINVAL;
    if (n_out == 0) return ARTALK_OK;
    launch_resample_mean(x, nch, n, taps, orig, nw, width, out, n_out, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_pool_silu(const float* X, int C, int T, int D, float* Y, void* stream) {
    return artalk_op_pool_silu_ex(X, C, T, D, Y, 0, kActExp, nullptr, stream);
}
int artalk_op_pool_silu_ex(const float* X, int C, int T, int D, float* Y, int out_p8, int p8_exp, int* status_dev, void* stream) {
    if (!X || !Y || D % 4 != 0 || (out_p8 && D % 8 != 0) || !op_exp_ok(p8_exp)) return ARTALK_EINVAL;
    static const int pn[5] = {1, 5, 25, 50, 100};
    launch_pool_silu(X, T, T, Y, C, pn, 5, D, (hipStream_t)stream, out_p8 ? 1 : 0, out_p8 ? status_dev : nullptr, p8_exp);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// wav2vec2 positional convolution of f16x3 mode (launch_posconv_p8): X [n_chunks * Ts][1024] fp32 rows (frames t < T of a chunk are read),
// Wp [1024][128 * 64] packed weights (k = tap * 64 + input channel of the group), C = R + act(conv + bias), rows t < Ts of every chunk
int artalk_op_posconv_p8_ex(const float* X, const void* Wp, const float* bias, const float* R, float* C, int n_chunks, int T, int Ts,
                            int act, int a_exp, int* status_dev, void* stream) {
    if (!X || !Wp || !C || n_chunks <= 0 || T <= 0 || T > Ts || Ts > 256 || act < 0 || act > 3 || !op_exp_ok(a_exp)) return ARTALK_EINVAL;
    if (((uintptr_t)X | (uintptr_t)Wp | (uintptr_t)C | (uintptr_t)bias | (uintptr_t)R) & 15) return ARTALK_EINVAL;
    GemmArgs g;
    g.A = X; g.lda = 1024; g.Wp = (const unsigned int*)Wp; g.ldw = 128 * 64; g.bias = bias; g.C = C; g.ldc = 1024; g.R = R; g.ldr = 1024;
    g.M = n_chunks * Ts; g.N = 1024; g.K = 128 * 64; g.act = act; g.a_exp = a_exp; g.status = status_dev;
    launch_posconv_p8(g, n_chunks, T, Ts, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// ---- the wav2vec2 stage's kernels in the chunk-strided forms run_wav2vec launches them (include/artalk_hip.h): checked on the host
// like the *_rows entry points above, dry run included
int artalk_op_w2v_front_rows(const float* audio, int64_t audio_elems, const int64_t* chunk_off, int C, int n, const float* w,
                             const float* bias, const float* lnw, const float* lnb, float* xnorm_out, float* Y, int64_t row_stride,
                             int64_t y_elems, int out_p8, int p8_exp, int* status_dev, void* stream) {
    if (!audio || !chunk_off || !w || !bias || !lnw || !lnb || !xnorm_out || !Y || C <= 0 || n < 10 || !op_exp_ok(p8_exp)) return ARTALK_EINVAL;
    const int T = (n - 10) / 5 + 1;
    if (row_stride < T || row_stride > INT_MAX) return ARTALK_EINVAL;
    if (!op_al(Y, out_p8 ? 32 : 16)) return ARTALK_EINVAL;      // rows are stored as 16-byte vectors, P8 rows as 32-byte groups
    for (int i = 0; i < C; ++i)
        if (chunk_off[i] < 0 || chunk_off[i] > audio_elems - n) return ARTALK_EINVAL;
    if (!op_fits((int64_t)(C - 1) * row_stride + T - 1, 512, 512, y_elems)) return ARTALK_EINVAL;
    if (g_rows_dry_run) return ARTALK_OK;
    hipStream_t s = (hipStream_t)stream;
    std::vector<long> off(chunk_off, chunk_off + C);
    DevBuf<long> doff;
    if (!doff.upload(off.data(), C)) return ARTALK_EHIP;
    launch_audio_normalize(audio, doff.get(), xnorm_out, C, n, s);
    launch_conv0(xnorm_out, n, w, bias, lnw, lnb, Y, C, T, (int)row_stride, s, out_p8 ? 1 : 0, out_p8 ? status_dev : nullptr, p8_exp);
    const hipError_t e1 = hipStreamSynchronize(s);
    return (e1 == hipSuccess && hipGetLastError() == hipSuccess) ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_pool_silu_rows(const float* X, int C, int T, int D, float* Y, int out_p8, int p8_exp, int* status_dev, int64_t x_tstride,
                             int64_t x_elems, int64_t y_elems, void* stream) {
    if (!X || !Y || C <= 0 || T < 1 || D <= 0 || D % 4 != 0 || (out_p8 && D % 8 != 0) || !op_exp_ok(p8_exp)) return ARTALK_EINVAL;
    if (x_tstride < T || x_tstride > INT_MAX) return ARTALK_EINVAL;
    if (!op_al(X, 16) || !op_al(Y, out_p8 ? 32 : 16)) return ARTALK_EINVAL;
    if (!op_fits((int64_t)(C - 1) * x_tstride + T - 1, D, D, x_elems) || !op_fits((int64_t)C * kNTok - 1, D, D, y_elems)) return ARTALK_EINVAL;
    if (g_rows_dry_run) return ARTALK_OK;
    static const int pn[5] = {1, 5, 25, 50, 100};
    hipStream_t s = (hipStream_t)stream;
    launch_pool_silu(X, (int)x_tstride, T, Y, C, pn, 5, D, s, out_p8 ? 1 : 0, out_p8 ? status_dev : nullptr, p8_exp);
    const hipError_t e1 = hipStreamSynchronize(s);
    return (e1 == hipSuccess && hipGetLastError() == hipSuccess) ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_posconv_rows(int mode, const float* X, int64_t x_elems, const float* W, const float* bias, const float* R, float* C,
                           int64_t c_elems, int n_chunks, int T, int Ts, int groups, int cg, int taps, int act, int a_exp, int force_cfg,
                           int* status_dev, void* stream) {
    if (mode < 0 || mode > 2 || !X || !W || !C || (R && R != C)) return ARTALK_EINVAL;
    if (n_chunks <= 0 || T < 1 || T > Ts || groups <= 0 || cg <= 0 || taps <= 0 || act < 0 || act > 3 || !op_exp_ok(a_exp)) return ARTALK_EINVAL;
    if (cg % 4 != 0 || ((int64_t)cg * taps) % 32 != 0 || (int64_t)cg * taps > INT_MAX || (int64_t)groups * cg > INT_MAX) return ARTALK_EINVAL;
    if (mode == 1 ? (groups != 16 || cg != 64 || taps != 128 || Ts > 256 || force_cfg != -1)
                  : (force_cfg != -1 && (mode == 0 ? (force_cfg < 1 || force_cfg > 4) : (force_cfg < 0 || force_cfg > 2))))
        return ARTALK_EINVAL;
    // X and W rows are read as 16-byte vectors in every mode; the f16x3 kernel takes the 16-byte epilogue only
    if (!op_al(X, 16) || !op_al(W, 16)) return ARTALK_EINVAL;
    if (mode == 1 && (!op_al(C, 16) || !op_al(bias, 16))) return ARTALK_EINVAL;
    const int64_t H = (int64_t)groups * cg, M = (int64_t)n_chunks * Ts, K = (int64_t)cg * taps;
    if (M > INT_MAX) return ARTALK_EINVAL;
    // frames t < T of every chunk are read, rows t < Ts of every chunk are written
    if (!op_fits((int64_t)(n_chunks - 1) * Ts + T - 1, H, H, x_elems) || !op_fits(M - 1, H, H, c_elems)) return ARTALK_EINVAL;
    if (op_overlap(X, (int64_t)(n_chunks - 1) * Ts * H + (int64_t)T * H, C, M * H)) return ARTALK_EINVAL;      // a row of X is read by many rows of C
    if (g_rows_dry_run) return ARTALK_OK;
    hipStream_t s = (hipStream_t)stream;
    DevBuf<unsigned char> wcopy;      // the weights packed (4 bytes each) or in bf16 (2 bytes each)
    if (mode != 0 && !wcopy.alloc((size_t)(H * K) * (mode == 1 ? 4 : 2))) return ARTALK_EHIP;
    GemmArgs g;
    g.A = X; g.lda = H; g.W = W; g.ldw = K; g.bias = bias; g.C = C; g.ldc = H; g.R = R; g.ldr = H;
    g.M = (int)M; g.act = act; g.a_exp = a_exp; g.K = (int)K;
    if (mode == 1) {
        launch_pack_split(W, (unsigned int*)wcopy.get(), H * K, true, s);
        g.N = (int)H; g.Wp = (const unsigned int*)wcopy.get(); g.status = status_dev;
        launch_posconv_p8(g, n_chunks, T, Ts, s);
    } else {
        // the grouped GEMM over grid.z of run_wav2vec (amode 1)
        g.amode = 1; g.pc_T = T; g.pc_tstride = Ts; g.pc_pad = taps / 2; g.pc_cin = cg;
        g.N = cg; g.force_cfg = force_cfg;
        g.batch = groups; g.sA = cg; g.sW = (long)cg * K; g.sBias = bias ? cg : 0; g.sC = cg; g.sR = R ? cg : 0;
        if (mode == 2) { launch_pack_bf16(W, wcopy.get(), H * K, s); g.Wb = wcopy.get(); }
        run_gemm(g, plan_gemm(g, GemmPolicy{mode}, nullptr), nullptr, s);
    }
    const hipError_t e1 = hipStreamSynchronize(s);
    return (e1 == hipSuccess && hipGetLastError() == hipSuccess) ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_bsq_history(const float* enc_out, uint8_t* hist_bits, float* prev_fdec, float* msfeat, int B, void* stream) {
    return artalk_op_bsq_history_ex(enc_out, hist_bits, prev_fdec, msfeat, B, nullptr, stream);
}
int artalk_op_bsq_history_ex(const float* enc_out, uint8_t* hist_bits, float* prev_fdec, float* msfeat, int B, int* status_dev, void* stream) {
    if (!enc_out || !hist_bits || !prev_fdec || !msfeat || B <= 0) return ARTALK_EINVAL;
    if (init_ms_tables() != 0) return ARTALK_EHIP;
    launch_bsq_history(enc_out, hist_bits, prev_fdec, msfeat, B, (hipStream_t)stream, status_dev);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// ---- the glue kernels of ar_glue.hip, one launch each (tests/test_glue_ops_gpu.py); the sizes the kernels fix (768, 181, 100, 32, 106 ->
// 128, 50) are the model's
int artalk_op_ar_bits_next(const float* logits, uint8_t* bits, float* fhat, float* nextfeat, int B, int level, int* status_dev, void* stream) {
    if (!logits || !bits || B <= 0 || level < 0 || level > 4 || (level < 4 && (!fhat || !nextfeat))) return ARTALK_EINVAL;
    if (init_ms_tables() != 0) return ARTALK_EHIP;
    launch_ar_bits_next(logits, bits, fhat, nextfeat, B, level, (hipStream_t)stream, status_dev);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_vq_embed(const float* feat, int n, const float* We, const float* be, const float* pos, float* X, int xrows, int xoff,
                       const float* style_cond, const float* pos0, int B, void* stream) {
    if (!feat || !We || !be || !pos || !X || n <= 0 || B <= 0 || xoff < 0 || xrows < xoff + n) return ARTALK_EINVAL;
    if (style_cond && (!pos0 || xoff < 1)) return ARTALK_EINVAL;      // the style row is row 0 of each clip's block
    if (((uintptr_t)We) & 15) return ARTALK_EINVAL;                     // weight rows are read as float4
    launch_vq_embed(feat, n, We, be, pos, X, xrows, xoff, style_cond, pos0, B, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_ar_begin(const float* style_cond, const float* lvlpos, float* x0, float* fhat, int B, void* stream) {
    if (!style_cond || !lvlpos || !x0 || !fhat || B <= 0) return ARTALK_EINVAL;
    launch_ar_begin(style_cond, lvlpos, x0, fhat, B, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_dec_input(const float* prev_fdec, const float* fhat, const uint8_t* bits, const float* dpos, float* X, int B, void* stream) {
    if (!prev_fdec || !fhat || !bits || !dpos || !X || B <= 0) return ARTALK_EINVAL;
    if (init_ms_tables() != 0) return ARTALK_EHIP;
    launch_dec_input(prev_fdec, fhat, bits, dpos, X, B, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_dec_finish(const float* dec, const float* mean, const float* std_, const float* epos, float* out, int64_t out_bstride,
                         int chunk, float* E, int B, int* status_dev, void* stream) {
    if (!dec || !mean || !std_ || !epos || !out || !E || B <= 0 || chunk < 0) return ARTALK_EINVAL;
    if (out_bstride < ((int64_t)chunk + 1) * 100 * 106) return ARTALK_EINVAL;      // a clip's rows would run into the next clip's
    launch_dec_finish(dec, mean, std_, epos, out, (long)out_bstride, chunk, E, B, (hipStream_t)stream, status_dev);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_enc_input_zero(const float* mean, const float* std_, const float* epos, float* E, int B, void* stream) {
    if (!mean || !std_ || !epos || !E || B <= 0) return ARTALK_EINVAL;
    launch_enc_input_zero(mean, std_, epos, E, B, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_style_input(const float* motion, const float* mean, const float* std_, float* X, int B, void* stream) {
    if (!motion || !mean || !std_ || !X || B <= 0) return ARTALK_EINVAL;
    launch_style_input(motion, mean, std_, X, B, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_add_row(float* X, const float* v, int M, int D, void* stream) {
    if (!X || !v || M <= 0 || D <= 0) return ARTALK_EINVAL;
    launch_add_row(X, v, M, D, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_style_finish(const float* feat, const float* Ws, const float* bs, const float* null_cond, const uint8_t* has_style,
                           float* style_cond, int B, const float* cached, int64_t cached_stride, void* stream) {
    if (!feat || !Ws || !bs || !null_cond || !style_cond || B <= 0) return ARTALK_EINVAL;
    if (cached && cached_stride < 768) return ARTALK_EINVAL;
    launch_style_finish(feat, Ws, bs, null_cond, has_style, style_cond, B, (hipStream_t)stream, cached, (long)cached_stride);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_broadcast16(const void* src, void* dst, int64_t bytes, int B, void* stream) {
    if (!src || !dst || B <= 0 || bytes <= 0 || bytes % 16 != 0 || bytes / 16 > 0x7fffffff) return ARTALK_EINVAL;
    if (((uintptr_t)src | (uintptr_t)dst) & 15) return ARTALK_EINVAL;
    launch_broadcast16(src, dst, (long)bytes, B, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
static bool op_session_rows(float* style, float* prev_in, float* prev_fdec, int s16, int p16, int f16, SessionRows* w) {
    if (!style || !prev_in || !prev_fdec || s16 <= 0 || p16 <= 0 || f16 <= 0) return false;
    if (((uintptr_t)style | (uintptr_t)prev_in | (uintptr_t)prev_fdec) & 15) return false;
    if ((int64_t)s16 + p16 + f16 > 0x7fffffff) return false;
    w->style = reinterpret_cast<uint4*>(style); w->prev_in = reinterpret_cast<uint4*>(prev_in); w->prev_fdec = reinterpret_cast<uint4*>(prev_fdec);
    w->s16 = s16; w->p16 = p16; w->f16 = f16;
    return true;
}
int artalk_op_session_gather(const float* const* slots_dev, float* style, float* prev_in, float* prev_fdec, int s16, int p16, int f16, int n,
                             void* stream) {
    SessionRows w;
    if (!slots_dev || n <= 0 || !op_session_rows(style, prev_in, prev_fdec, s16, p16, f16, &w)) return ARTALK_EINVAL;
    launch_session_gather(slots_dev, w, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_savgol_stream(float* const* slots_dev, const float* raw, int64_t raw_stride, const int* seen, const int* n_frames,
                            const uint8_t* last, float* out, int64_t out_stride, int n, void* stream) {
    if (!slots_dev || !seen || !n_frames || !last || !out || n <= 0) return ARTALK_EINVAL;
    std::string err;
    bool need_raw = false;
    for (int i = 0; i < n; ++i) {
        const std::string who = "artalk_op_savgol_stream: row " + std::to_string(i);
        if (int rc = smooth_row_range(who, n_frames[i], last[i] != 0, &err)) return rc;
        if (int rc = smooth_row_length(who, seen[i], n_frames[i], last[i] != 0, &err)) return rc;
        need_raw |= n_frames[i] > 0;
    }
    if (int rc = smooth_stride_check("artalk_op_savgol_stream", raw != nullptr, need_raw, raw_stride, out_stride, kOpMotionDim, &err)) return rc;
    if (g_rows_dry_run) return ARTALK_OK;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int4> meta((size_t)n);
    for (int i = 0; i < n; ++i) meta[i] = make_int4(seen[i], n_frames[i], last[i] ? 1 : 0, 0);
    DevBuf<int4> dmeta;
    if (!dmeta.upload(meta.data(), (size_t)n)) return ARTALK_EHIP;
    launch_savgol_stream(slots_dev, dmeta.get(), (long)slot_carry_off(kOpCodeDim), raw, (long)raw_stride, out, (long)out_stride, n, kOpMotionDim, s);
    const hipError_t e1 = hipStreamSynchronize(s);
    return (e1 == hipSuccess && hipGetLastError() == hipSuccess) ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_session_smooth_check(const int64_t* open_ids, const int64_t* open_seen, const uint8_t* open_done, int n_open,
                                   const int64_t* ended_ids, int n_ended, const int64_t* ids, int n, int have_raw, int64_t raw_stride,
                                   const int* n_frames, const uint8_t* last, int64_t out_stride, int* first_out, int* count_out, char* msg,
                                   int msg_len) {
    if (n_open < 0 || n_ended < 0 || (n_open && (!open_ids || !open_seen || !open_done)) || (n_ended && !ended_ids) || !ids || n <= 0)
        return ARTALK_EINVAL;
    artalk_model::Sessions ss;
    for (int i = 0; i < n_open; ++i) {
        artalk_model::Sessions::Open o;
        o.slot = i; o.seen = open_seen[i]; o.smooth_done = open_done[i] != 0;
        ss.open.emplace(open_ids[i], o);
    }
    for (int i = 0; i < n_ended; ++i) ss.ended_by_scales.insert(ended_ids[i]);
    std::vector<artalk_model::Sessions::Open*> st;
    std::string err;
    const int rc = smooth_check(ss, ids, n, have_raw != 0, raw_stride, n_frames, last, out_stride, kOpMotionDim, &st, &err);
    if (msg && msg_len > 0) { std::strncpy(msg, err.c_str(), (size_t)msg_len - 1); msg[msg_len - 1] = 0; }
    for (int i = 0; rc == ARTALK_OK && first_out && count_out && i < n; ++i)
        smooth_span(st[i]->seen, n_frames ? n_frames[i] : 100, last && last[i], &first_out[i], &count_out[i]);
    return rc;
}
int artalk_op_session_scatter(float* const* slots_dev, const float* style, const float* prev_in, const float* prev_fdec, int s16, int p16,
                              int f16, int n, int with_style, void* stream) {
    SessionRows w;      // (the scatter kernel only reads the three buffers)
    if (!slots_dev || n <= 0 ||
        !op_session_rows(const_cast<float*>(style), const_cast<float*>(prev_in), const_cast<float*>(prev_fdec), s16, p16, f16, &w))
        return ARTALK_EINVAL;
    launch_session_scatter(slots_dev, w, n, with_style != 0, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}
int artalk_op_absmax(const float* buf, int rows, int cols, int64_t ld, int is_p8, int p8_exp, int junk_period, int junk_from,
                     unsigned int* slot_dev, void* stream) {
    if (!buf || !slot_dev || rows < 0 || cols <= 0 || cols % 8 != 0 || ld < cols || !op_exp_ok(p8_exp)) return ARTALK_EINVAL;
    if (junk_period < 0 || junk_from < 0 || (junk_period > 0 && junk_from > junk_period)) return ARTALK_EINVAL;
    launch_absmax(buf, rows, cols, (long)ld, is_p8 ? 1 : 0, slot_dev, (hipStream_t)stream, junk_period, junk_from, p8_exp);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

}  // extern "C"
