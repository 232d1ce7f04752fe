// The launch sequence of the audio->motion path on a model object (model.h): the stages, the clip groups of the AR/VAE body and
// their graphs, the chunk step that the batch, streaming and session calls (calls.hip) run.
//
// Execution plan (differs from the reference's loop order, app/models.py:92-114, same arithmetic per token):
//   1. style encoder for all clips                                   (app/models.py:67-73)
//   2. wav2vec2 for ALL 4-second chunks of ALL clips in one batched pass - chunk i of the audio does not depend on
//      the AR state (app/models.py:93), so M = chunks*200 rows per GEMM instead of 199
//   3. for each chunk index j (sequential: chunk j+1 needs the re-encoded motion of chunk j), all clips that
//      still have a chunk j batched:  AdaLN table for all 12 blocks + head in ONE GEMM (the conditioning is
//      layer-independent, app/transformer.py:32), K/V of the 181 history tokens once per layer, then the 5
//      scale steps with a per-layer KV cache (only the new level's tokens run), VAE decode,
//      re-encode + quantise to the next history.
#include "model.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace artalk;

namespace artalk {
thread_local KernelTimer* g_ktimer = nullptr;
bool ktimer_events(hipEvent_t* e0, hipEvent_t* e1) {
    KernelTimer* t = g_ktimer;
    if (!t) return false;
    while (t->pool.size() < t->used + 2) {
        Event e;
        if (!e.create()) return false;
        t->pool.push_back(std::move(e));
    }
    *e0 = t->pool[t->used].get(); *e1 = t->pool[t->used + 1].get();
    t->recs.emplace_back(t->bucket, t->used);
    t->used += 2;
    return true;
}
}  // namespace artalk

namespace {
// ------------------------------------------------------------------------------------------------ profiling
// records the next event of the pool on s; false: the event cannot be made, nothing is recorded and the caller skips its mark or pair
bool next_event(artalk_model* m, hipStream_t s, size_t* idx) {
    if (m->ev_used == m->ev_pool.size()) {
        Event e;
        if (!e.create()) return false;
        m->ev_pool.push_back(std::move(e));
    }
    *idx = m->ev_used++;
    (void)hipEventRecord(m->ev_pool[*idx].get(), s);
    return true;
}
void kbucket(artalk_model* m, int b) { m->ktimer.bucket = b; }
}  // namespace

namespace artalk {      // called from other files: declared in model.h
void stage_mark(artalk_model* m, hipStream_t s, int bucket) {
    if (!m->profiling || m->in_graph_body) return;
    size_t i;
    if (next_event(m, s, &i)) m->marks.emplace_back(bucket, i);
}
}  // namespace artalk

namespace {
// fuse_ln: the AdaLN-modulated LayerNorm that consumes this GEMM's (768-wide, residual-stream) result.  If the GEMM is split
// over K, its reduce pass also writes that LayerNorm's output (one launch instead of two) and gemm() returns true; otherwise
// the caller launches the LayerNorm itself.
// audit hook: records max |x| of a just-produced P8 buffer (or of the fp32 buffer that holds the same activation in f32 mode, or that a
// register-staged GEMM will split).  ex = the site's exponent (a SiteExps member of this model): what the buffer was written with, and
// what artalk_calibrate adjusts from the recorded maximum; the site's name is the one the site table gives that member.  Works in both
// precision modes: the calibration pass runs in exact-f32 mode, where nothing can overflow on the way to a later site.
void audit(artalk_model* m, const float* buf, int rows, int cols, long ld, bool is_p8, hipStream_t s, int* ex, int junk_period = 0,
           int junk_from = 0) {
    if (!m->audit || !m->audit_vals) return;
    auto st = m->site_of.find(ex);
    if (st == m->site_of.end()) { m->err = "internal: audited exponent is not in the site table"; m->sticky_error = true; return; }
    const std::string& name = m->sites[st->second].name;
    auto it = m->audit_index.find(name);
    int idx;
    if (it == m->audit_index.end()) {
        if ((int)m->audit_names.size() >= kAuditSlots) return;
        idx = (int)m->audit_names.size();
        m->audit_names.push_back(name);
        m->audit_exp.push_back(ex);
        m->audit_index.emplace(name, idx);
    } else idx = it->second;
    launch_absmax(buf, rows, cols & ~7, ld, is_p8 ? 1 : 0, m->audit_vals + idx, s, junk_period, junk_from, ex ? *ex : kActExp);
}

// plan_M > 0: the launch has fewer rows than the launch of plan_M rows whose rows it computes (the conv stack of run_wav2vec without the
// frames that hear zero padding alone): it is planned as that launch - kernel family, tile configuration, split-K factor - and the plan
// is pinned on the rows it runs, so that every row sees the summation order it would have seen there.
bool gemm(artalk_model* m, const GemmArgs& g0, hipStream_t s, const LnArgs* fuse_ln = nullptr, int plan_M = 0) {
    GemmArgs g = g0;
    const int run_M = g.M;
    if (plan_M > 0) g.M = plan_M;
    g.graph_tag = m->in_body ? 1 : 0;
    g.cus = m->n_cus;
    g.status = m->precision == 1 ? (m->view ? m->view->status : m->ws.status) : nullptr;     // P8 range guard at the producers
    if (m->precision == 1 && !g.exact) g.Wp = packed_of(m, g.W);
    if (m->precision == 2 && !g.exact) {
        g.Wb = bf16_of(m, g.W);
        if (!g.Wb || ((unsigned long long)g.Wb & 15) || (g.ldw & 7)) {
            m->err = "internal: bf16 GEMM without an aligned bf16 weight copy"; m->sticky_error = true; return false;
        }
        if (g.a_packed) { m->err = "internal: P8 activation handed to a bf16 GEMM"; m->sticky_error = true; return false; }
    }
    const Workspace& cw = m->view ? *m->view : m->ws;
    const GemmPolicy pol{m->precision, false, cw.splitk, cw.splitk_floats, m->splitk_tiles, m->splitk_target};
    GemmPlan plan = plan_gemm(g, pol, fuse_ln);
    if (plan_M > 0) {
        g.M = run_M;
        if (plan.path != GEMM_P8) g.force_cfg = plan.cfg;      // (the P8 plan has set it; the other launchers would choose again from M)
        else if (gemm_p8_class(plan.cfg) == P8_BIG) {
            // the big-tile kernel's two tile heights run the same K loop per row (bit-identical results: tests/test_p8_depth_gpu.py): the
            // height is chosen for the rows this launch has, where the cost model still sees a big-tile launch
            GemmArgs h = g;
            h.force_cfg = g0.force_cfg; h.splitk = g0.splitk; h.partial = g0.partial;
            const GemmPlan alt = plan_gemm(h, pol, fuse_ln);
            if (alt.path == GEMM_P8 && gemm_p8_class(alt.cfg) == P8_BIG && h.splitk == g.splitk) { g.force_cfg = alt.cfg; plan.cfg = alt.cfg; }
        }
    }
    if (g.a_packed && plan.path == GEMM_F32) { m->err = "internal: P8 activation handed to an fp32 GEMM"; m->sticky_error = true; return false; }
    size_t i0 = 0, i1 = 0;
    const bool timed = m->profiling && plan.dominant && !m->in_body && next_event(m, s, &i0);
    run_gemm(g, plan, fuse_ln, s);
    if (timed && next_event(m, s, &i1)) m->dom_events.emplace_back(i0, gemm_flops(g));      // (i1 == i0 + 1: artalk_get_profile)
    return plan.fused_ln;
}

// ---- intermediate taps (include/artalk_hip.h: artalk_set_tap) ----
// copies `rows` x `cols` fp32 values per clip (compact source [B][rows][cols]) to row `row0` of field `field` of the chunk's slots
void tap_copy(artalk_model* m, int field, int row0, const float* src, int rows, int cols, int B, hipStream_t s) {
    if (!m->tap || m->in_graph_body || m->tap_chunk >= m->tap_maxch || B > m->tap_B) return;
    float* dst = m->tap + ((long)m->tap_chunk * m->tap_B) * TAP_SLOT + field + (long)row0 * cols;
    (void)hipMemcpy2DAsync(dst, (size_t)TAP_SLOT * 4, src, (size_t)rows * cols * 4, (size_t)rows * cols * 4, B, hipMemcpyDeviceToDevice, s);
}

enum { LF_EXACT = 1, LF_A_P8 = 2, LF_C_P8 = 4 };   // linear() flags: decision-critical (fp32 path) / A is in P8 / write C in P8
// plain y = act(x W^T + b) [+ R]
void linear(artalk_model* m, const float* A, long lda, const float* W, const float* bias, float* C, long ldc, int M, int N, int K,
            int act, const float* R, hipStream_t s, int flags = 0, float* c2 = nullptr, int a_exp = kActExp, int c_exp = kActExp,
            int plan_M = 0) {
    GemmArgs g;
    g.c2 = c2; g.a_exp = a_exp; g.c_exp = c_exp;
    g.exact = flags & LF_EXACT; g.a_packed = (flags & LF_A_P8) ? 1 : 0; g.c_p8 = (flags & LF_C_P8) ? 1 : 0;
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.act = act;
    g.R = R; g.ldr = ldc;
    gemm(m, g, s, nullptr, plan_M);
}

void layernorm(const float* X, float* Y, const float* w, const float* b, int M, int D, float eps, int act, hipStream_t s, int out_p8 = 0,
               int* status = nullptr, int junk_period = 0, int junk_from = 0, int p8_exp = kActExp) {
    LnArgs a;
    a.out_p8 = out_p8; a.p8_exp = p8_exp; a.status = out_p8 ? status : nullptr; a.junk_period = junk_period; a.junk_from = junk_from;
    a.X = X; a.ldx = D; a.Y = Y; a.ldy = D; a.w = w; a.b = b; a.M = M; a.D = D; a.eps = eps; a.act = act;
    launch_layernorm(a, s);
}

}  // namespace

namespace artalk {      // called from other files: declared in model.h
// ------------------------------------------------------------------------------------------------ stages

// wav2vec2 on chunks [c0, c0+n) of the chunk list (app/modules/wav2vec.py:11-20); writes SiLU(pooled cond) rows c0*181..
void run_wav2vec(artalk_model* m, const float* audio, int c0, int n, float* out_w2v, hipStream_t s, const ConvPasses* tail) {
    const artalk_config& c = m->cfg;
    Workspace& w = m->ws;
    const int CD = c.w2v_conv_dim, Hs = c.w2v_hidden;
    // f16x3 mode: every activation whose only consumer is a GEMM is written by its producer directly in the P8 split
    // format (same bytes), so the big GEMMs can stage both operands with LDS-DMA (gemm_p8_2wgp_kernel / gemm_p8_big_kernel).
    const int p8 = m->precision == 1 ? 1 : 0;
    const int AP = p8 ? LF_A_P8 : 0;
    Range r_w2v("artalk.wav2vec2");
    roctxRangePushA("artalk.wav2vec2.conv_stack");      // K1-K3: normalise, conv0+LN+GELU, conv1-6 as GEMMs + LN + GELU
    kbucket(m, KB_CONV);
    // The samples of every chunk are normalised, zeros included (the statistics are the reference's); with passes, in pass order.
    launch_audio_normalize(audio, tail ? tail->perm : w.src_off + c0, w.xnorm, n, kSamplesPerChunk, s);
    SiteExps& ex = m->ex;
    // Pass p: its chunks compute T[i] frames of layer i at a row stride of S[i] per chunk, S[i-1] = 2 S[i] in every geometry.  The passes'
    // rows of a layer follow one another (pass p starts at row0 = sum of n[q] S_q[i] over q < p), so a pass's start doubles from layer to
    // layer as its stride does, and ONE GEMM per layer - output row r reads input rows 2r .. - covers all passes.  Without length
    // classes (tail = null): one pass of n whole chunks.
    ConvPasses one;
    one.np = 1; one.n[0] = n; one.cls[0] = 3;
    const ConvPasses& ps = tail ? *tail : one;
    auto geo_T = [&](int p) { const artalk_model::TailGeo& tg = m->tail_geo[ps.cls[p]]; return ps.cls[p] != 3 && tg.partial ? tg.T : m->conv_T; };
    auto geo_S = [&](int p) { const artalk_model::TailGeo& tg = m->tail_geo[ps.cls[p]]; return ps.cls[p] != 3 && tg.partial ? tg.S : m->conv_S; };
    auto row0 = [&](int p, int i) { long r = 0; for (int q = 0; q < p; ++q) r += (long)ps.n[q] * geo_S(q)[i]; return r; };
    float* src = w.convA; float* dst = w.convB;
    for (int p = 0; p < ps.np; ++p) {
        const int *T = geo_T(p), *S = geo_S(p);
        float* y = src + row0(p, 0) * CD;
        launch_conv0(w.xnorm + (long)ps.off[p] * kSamplesPerChunk, kSamplesPerChunk, m->conv0_w, m->conv_b[0], m->conv_lnw[0], m->conv_lnb[0], y, ps.n[p],
                     T[0], S[0], s, p8, w.status, ex.conv[0]);
        audit(m, y, ps.n[p] * S[0], CD, CD, p8, s, &ex.conv[0], S[0], T[0]);
    }
    for (int i = 1; i < c.w2v_n_conv; ++i) {
        // stride-2 conv as a GEMM: output row r reads input rows 2r..2r+k-1 (contiguous K = k*512 floats).  With passes it has fewer rows
        // than the launch over n whole chunks, and is planned as that launch (gemm(): plan_M): kernel family, tile configuration and
        // split over K decide a row's summation order, its place in the launch does not.
        const int M = (int)row0(ps.np, i), plan_M = M == n * m->conv_S[i] ? 0 : n * m->conv_S[i];
        linear(m, src, (long)c.w2v_conv_stride[i] * CD, m->conv_w[i], m->conv_b[i], dst, CD, M, CD, c.w2v_conv_kernel[i] * CD,
               ACT_NONE, nullptr, s, AP, nullptr, ex.conv[i - 1], kActExp, plan_M);
        // the last conv output feeds a LayerNorm (feature projection), not a GEMM: it stays fp32
        // rows t >= T[i] of every chunk are layout padding (computed from the padding rows below them): no range guard there.  One
        // launch takes two passes (LnArgs::junk_row2: each with its own padding rows).
        for (int p = 0; p < ps.np; p += 2) {
            const int *T = geo_T(p), *S = geo_S(p);
            float* y = dst + row0(p, i) * CD;
            const int Mp = ps.n[p] * S[i], Mq = p + 1 < ps.np ? ps.n[p + 1] * geo_S(p + 1)[i] : 0;
            LnArgs a;
            a.plan_M = plan_M;
            a.out_p8 = (p8 && i + 1 < c.w2v_n_conv) ? 1 : 0; a.p8_exp = ex.conv[i]; a.status = a.out_p8 ? w.status : nullptr;
            a.junk_period = S[i]; a.junk_from = T[i];
            if (Mq) { a.junk_row2 = Mp; a.junk_period2 = geo_S(p + 1)[i]; a.junk_from2 = geo_T(p + 1)[i]; }
            a.X = y; a.ldx = CD; a.Y = y; a.ldy = CD; a.w = m->conv_lnw[i]; a.b = m->conv_lnb[i]; a.M = Mp + Mq; a.D = CD; a.eps = 1e-5f; a.act = ACT_GELU_ERF;
            launch_layernorm(a, s);
            if (i + 1 < c.w2v_n_conv) {
                audit(m, y, Mp, CD, CD, p8, s, &ex.conv[i], S[i], T[i]);
                if (Mq) audit(m, y + (long)Mp * CD, Mq, CD, CD, p8, s, &ex.conv[i], a.junk_period2, a.junk_from2);
            }
        }
        std::swap(src, dst);
    }
    if (tail) {
        // the encoder's layout (Ts rows per chunk, the call's chunk order) into the other buffer: row t of a chunk is its computed row
        // min(t, tc), the rows past tc being copies of row tc (same inputs, same instruction sequence: the same bits)
        launch_conv_tail_gather(src, tail->tab, dst, n, m->Tw, m->Ts, CD, s);
        std::swap(src, dst);
    }
    stage_mark(m, s, PB_CONV);
    roctxRangePop();
    Range r_enc("artalk.wav2vec2.encoder");             // K4-K7: projection, pos-conv, 24 layers, final LN, pooling + SiLU
    kbucket(m, KB_ENC);
    const int M = n * m->Ts;
    // hidden states use a 200-row stride per chunk, 199 valid.  The padding row is never read by a valid row; the LayerNorms store
    // it as zeros (LnArgs::junk_period), and the attention output's padding row is never written (zero since allocation), so
    // everything computed in it stays finite and inside the P8 range without the GEMM epilogues having to know about it.
    const int JP = m->Ts, JF = m->Tw;
    // feature projection (hf:429-434)
    layernorm(src, dst, m->fp_lnw, m->fp_lnb, M, CD, c.w2v_ln_eps, ACT_NONE, s, p8, w.status, JP, JF, ex.fp_ln);
    audit(m, dst, M, CD, CD, p8, s, &ex.fp_ln, JP, JF);
    linear(m, dst, CD, m->fp_w, m->fp_b, w.h0, Hs, M, Hs, CD, ACT_NONE, nullptr, s, AP, nullptr, ex.fp_ln);
    // positional conv embedding (hf:360-368): h1 = h0 + gelu(groupconv(h0) + b)
    audit(m, w.h0, M, Hs, Hs, false, s, &ex.posconv_in, JP, JF);
    {
        const int cg = Hs / c.w2v_pos_groups;
        GemmArgs g;
        g.A = w.h0; g.lda = Hs; g.W = m->pos_w; g.ldw = (long)cg * c.w2v_pos_kernel; g.bias = m->pos_b; g.C = w.h1; g.ldc = Hs; g.R = w.h0; g.ldr = Hs;
        g.M = M; g.act = ACT_GELU_ERF; g.a_exp = ex.posconv_in;
        if (p8 && cg == 64 && c.w2v_pos_kernel == 128 && c.w2v_pos_groups == 16 && m->Ts <= 256) {
            // f16x3 mode: one workgroup per (chunk, group) with the chunk's input window resident in LDS (posconv_p8_kernel)
            g.N = Hs; g.K = cg * c.w2v_pos_kernel; g.Wp = packed_of(m, m->pos_w); g.status = w.status;
            launch_posconv_p8(g, n, m->Tw, m->Ts, s);
        } else {
            // grouped GEMM over grid.z whose A operand gathers the zero-padded window (amode 1)
            g.amode = 1; g.pc_T = m->Tw; g.pc_tstride = m->Ts; g.pc_pad = c.w2v_pos_kernel / 2; g.pc_cin = cg;
            g.N = cg; g.K = cg * c.w2v_pos_kernel;
            g.batch = c.w2v_pos_groups; g.sA = cg; g.sW = (long)cg * cg * c.w2v_pos_kernel; g.sBias = cg; g.sC = cg; g.sR = cg;
            gemm(m, g, s);
        }
    }
    float* h = w.h1;
    const int nh = c.w2v_heads, hd = Hs / nh;
    for (int i = 0; i < c.w2v_layers; ++i) {
        const W2VLayer& L = m->w2v[i];
        SiteExps::W2V& E = ex.w2v[i];
        layernorm(h, w.xln, L.ln1w, L.ln1b, M, Hs, c.w2v_ln_eps, ACT_NONE, s, p8, w.status, JP, JF, E.ln1);
        audit(m, w.xln, M, Hs, Hs, p8, s, &E.ln1, JP, JF);
        linear(m, w.xln, Hs, L.qkv_w, L.qkv_b, w.qkv, 3 * Hs, M, 3 * Hs, Hs, ACT_NONE, nullptr, s, AP | (p8 ? LF_C_P8 : 0), nullptr, E.ln1, E.qkv);   // q, k, v leave in P8
        AttnArgs a;
        a.qkv_p8 = p8; a.qkv_exp = E.qkv; a.o_exp = E.attn;
        a.Q = w.qkv; a.K = w.qkv + Hs; a.V = w.qkv + 2 * Hs;
        a.ldq = a.ldk = a.ldv = 3 * Hs; a.q_bstride = a.k_bstride = a.v_bstride = (long)m->Ts * 3 * Hs;
        a.O = w.att; a.ldo = Hs; a.o_bstride = (long)m->Ts * Hs;
        a.B = n; a.H = nh; a.HD = hd; a.Lq = m->Tw; a.Lk = m->Tw; a.scale = 1.0f / std::sqrt((float)hd);
        audit(m, w.qkv, M, 3 * Hs, 3 * Hs, p8, s, &E.qkv, JP, JF);
        a.out_p8 = p8; a.split16 = p8; a.status = p8 ? w.status : nullptr; a.cus = m->n_cus;
        launch_attention(a, s);
        audit(m, w.att, M, Hs, Hs, p8, s, &E.attn, JP, JF);
        linear(m, w.att, Hs, L.out_w, L.out_b, h, Hs, M, Hs, Hs, ACT_NONE, h, s, AP, nullptr, E.attn);
        layernorm(h, w.xln, L.ln2w, L.ln2b, M, Hs, c.w2v_ln_eps, ACT_NONE, s, p8, w.status, JP, JF, E.ln2);
        audit(m, w.xln, M, Hs, Hs, p8, s, &E.ln2, JP, JF);
        linear(m, w.xln, Hs, L.ff1_w, L.ff1_b, w.ffn, c.w2v_ffn, M, c.w2v_ffn, Hs, ACT_GELU_ERF, nullptr, s, AP | (p8 ? LF_C_P8 : 0), nullptr, E.ln2, E.ffn);
        audit(m, w.ffn, M, c.w2v_ffn, c.w2v_ffn, p8, s, &E.ffn, JP, JF);
        linear(m, w.ffn, c.w2v_ffn, L.ff2_w, L.ff2_b, h, Hs, M, Hs, c.w2v_ffn, ACT_NONE, h, s, AP, nullptr, E.ffn);
    }
    layernorm(h, w.xln, m->enc_lnw, m->enc_lnb, M, Hs, c.w2v_ln_eps, ACT_NONE, s);
    if (out_w2v)
        (void)hipMemcpy2DAsync(out_w2v + (long)c0 * m->Tw * Hs, (size_t)m->Tw * Hs * 4, w.xln, (size_t)m->Ts * Hs * 4,
                               (size_t)m->Tw * Hs * 4, n, hipMemcpyDeviceToDevice, s);
    launch_pool_silu(w.xln, m->Ts, m->Tw, w.silu_cond + (long)c0 * kNTok * kCond, n, m->pn, c.n_levels, kCond, s, p8, w.status, ex.silu_cond);
    audit(m, w.silu_cond + (long)c0 * kNTok * kCond, n * kNTok, kCond, kCond, p8, s, &ex.silu_cond);
    stage_mark(m, s, PB_ENC);
}

// style_motion rows: a (50,106) clip where the host flag is 1, a cached 768-float condition where it is 2 (artalk_style_encode);
// `encode` = some row has flag 1 (the host knows: has_style is a host array), otherwise the encoder stack is skipped altogether
void run_style(artalk_model* m, const float* style_motion, int B, hipStream_t s, bool encode) {
    const artalk_config& c = m->cfg;
    Workspace& w = m->ws;
    const int S = c.style_dim, L = c.style_len, M = B * L;
    Range r_style("artalk.style_encoder");
    kbucket(m, KB_STYLE);
    if (style_motion && encode) {
        launch_style_input(style_motion, m->st_mean, m->st_std, w.s_in, B, s);
        SiteExps& ex = m->ex;
        audit(m, w.s_in, M, 128, 128, false, s, &ex.style_in);
        linear(m, w.s_in, 128, m->st_proj_w, m->st_proj_b, w.s_h, S, M, S, 128, ACT_NONE, nullptr, s, 0, nullptr, ex.style_in);
        launch_add_row(w.s_h, m->st_pe, M, S, s);   // PositionalEncoding quirk: pe[:, seq_len] added to every token
        for (int i = 0; i < c.style_layers; ++i) {
            const StyleLayer& Ly = m->style[i];
            SiteExps::ST& E = ex.style[i];
            audit(m, w.s_h, M, S, S, false, s, &E.h);
            linear(m, w.s_h, S, Ly.in_w, Ly.in_b, w.s_qkv, 3 * S, M, 3 * S, S, ACT_NONE, nullptr, s, 0, nullptr, E.h);
            AttnArgs a;
            a.Q = w.s_qkv; a.K = w.s_qkv + S; a.V = w.s_qkv + 2 * S; a.ldq = a.ldk = a.ldv = 3 * S;
            a.q_bstride = a.k_bstride = a.v_bstride = (long)L * 3 * S;
            a.O = w.s_att; a.ldo = S; a.o_bstride = (long)L * S;
            a.B = B; a.H = c.style_heads; a.HD = S / c.style_heads; a.Lq = L; a.Lk = L;
            a.scale = 1.0f / std::sqrt((float)(S / c.style_heads));
            launch_attention(a, s);
            audit(m, w.s_att, M, S, S, false, s, &E.attn);
            linear(m, w.s_att, S, Ly.out_w, Ly.out_b, w.s_tmp, S, M, S, S, ACT_NONE, w.s_h, s, 0, nullptr, E.attn);
            layernorm(w.s_tmp, w.s_h, Ly.n1w, Ly.n1b, M, S, 1e-5f, ACT_NONE, s);
            audit(m, w.s_h, M, S, S, false, s, &E.h1);
            linear(m, w.s_h, S, Ly.l1_w, Ly.l1_b, w.s_ffn, c.style_ffn, M, c.style_ffn, S, ACT_GELU_ERF, nullptr, s, 0, nullptr, E.h1);
            audit(m, w.s_ffn, M, c.style_ffn, c.style_ffn, false, s, &E.ffn);
            linear(m, w.s_ffn, c.style_ffn, Ly.l2_w, Ly.l2_b, w.s_tmp, S, M, S, c.style_ffn, ACT_NONE, w.s_h, s, 0, nullptr, E.ffn);
            layernorm(w.s_tmp, w.s_h, Ly.n2w, Ly.n2b, M, S, 1e-5f, ACT_NONE, s);
        }
    }
    launch_style_finish(w.s_h, m->sc_w, m->sc_b, m->null_style, style_motion ? w.has_style : nullptr, w.style_cond, B, s,
                        style_motion, (long)L * c.motion_dim);
}

}  // namespace artalk

namespace {
// one VAE transformer stack (app/modules/bitwise_vae.py:149-157 / :183-191) on B sequences of T tokens, in place on ws.vh
void run_vae_stack(artalk_model* m, const VAESide& S, int B, int T, int split, hipStream_t s) {
    const artalk_config& c = m->cfg;
    Workspace& w = m->view ? *m->view : m->ws;
    const int H = c.vae_hidden, M = B * T, F = H * 3 / 2;
    const int p8 = m->precision == 1 ? 1 : 0;      // GEMM-only activations in the P8 split format (see run_chunk_body)
    const int AP = p8 ? LF_A_P8 : 0;
    const int sd = &S == &m->enc ? 0 : 1;
    for (int i = 0; i < c.vae_depth; ++i) {
        const VAELayer& L = S.layers[i];
        SiteExps::VAE& E = m->ex.vae[sd][i];
        layernorm(w.vh, w.vln, L.lnw, L.lnb, M, H, 1e-5f, ACT_NONE, s, p8, w.status, 0, 0, E.ln);
        audit(m, w.vln, M, H, H, p8, s, &E.ln);
        linear(m, w.vln, H, L.qkv_w, nullptr, w.vqkv, 3 * H, M, 3 * H, H, ACT_NONE, nullptr, s, AP | (p8 ? LF_C_P8 : 0), nullptr, E.ln, E.qkv);   // q, k, v leave in P8
        AttnArgs a;
        a.qkv_p8 = p8; a.qkv_exp = E.qkv; a.o_exp = E.attn;
        a.Q = w.vqkv; a.K = w.vqkv + H; a.V = w.vqkv + 2 * H; a.ldq = a.ldk = a.ldv = 3 * H;
        a.q_bstride = a.k_bstride = a.v_bstride = (long)T * 3 * H;
        a.O = w.vatt; a.ldo = H; a.o_bstride = (long)T * H;
        a.B = B; a.H = c.vae_heads; a.HD = H / c.vae_heads; a.Lq = T; a.Lk = T;
        a.scale = 1.0f / std::sqrt((float)H);      // hidden_dim**-0.5, NOT head_dim (bitwise_vae.py:198)
        audit(m, w.vqkv, M, 3 * H, 3 * H, p8, s, &E.qkv);
        a.split_q = split; a.split_k = split; a.out_p8 = p8; a.split16 = p8; a.status = p8 ? w.status : nullptr; a.cus = m->n_cus;
        launch_attention(a, s);
        audit(m, w.vatt, M, H, H, p8, s, &E.attn);
        // the MLP reads the residual stream itself (no LayerNorm in front of it, bitwise_vae.py:139-145).  In f16x3 mode the
        // out-projection writes it a second time in P8 (w.vln) so that the MLP GEMM can stage it by LDS-DMA (the register-staged
        // kernel on fp32 rows took 36 us at M = 6400, a split pass + the small-grid kernel 4 + 15, the second copy from the epilogue 15)
        linear(m, w.vatt, H, L.out_w, L.out_b, w.vh, H, M, H, H, ACT_NONE, w.vh, s, AP, p8 ? w.vln : nullptr, E.attn, E.resid);
        audit(m, p8 ? w.vln : w.vh, M, H, H, p8, s, &E.resid);
        linear(m, p8 ? w.vln : w.vh, H, L.m1_w, L.m1_b, w.vmlp, F, M, F, H, ACT_GELU_TANH, nullptr, s, p8 ? (LF_A_P8 | LF_C_P8) : 0, nullptr, E.resid, E.mlp);
        audit(m, w.vmlp, M, F, F, p8, s, &E.mlp);
        linear(m, w.vmlp, F, L.m2_w, L.m2_b, w.vh, H, M, H, F, ACT_NONE, w.vh, s, AP, nullptr, E.mlp);
    }
}

// motion (already in ws.enc_in as normalised + pos-embedded rows) -> history bits, decoder features, prev tokens
void run_reencode(artalk_model* m, int B, hipStream_t s) {
    const artalk_config& c = m->cfg;
    Workspace& w = m->view ? *m->view : m->ws;
    const int H = c.vae_hidden, T = 100;
    Range r_re("artalk.vae.reencode_bsq");              // K16-K17: encoder, multi-scale BSQ, history features
    kbucket(m, KB_REENC);
    audit(m, w.enc_in, B * T, 128, 128, false, s, &m->ex.vae_enc_in);
    linear(m, w.enc_in, 128, m->enc.in_w, m->enc.in_b, w.vh, H, B * T, H, 128, ACT_LEAKY02, nullptr, s, 0, nullptr, m->ex.vae_enc_in);
    run_vae_stack(m, m->enc, B, T, 0, s);
    linear(m, w.vh, H, m->enc.out_w, m->enc.out_b, w.enc_out, c.code_dim, B * T, c.code_dim, H, ACT_NONE, nullptr, s, LF_EXACT);
    launch_bsq_history(w.enc_out, w.hist_bits, w.prev_fdec, w.msfeat, B, s, w.status);
    launch_vq_embed(w.msfeat, kNTok - 1, m->vq_w, m->vq_b, m->prev_lvl_pos + kE, w.prev_in, kNTok, 1, w.style_cond,
                    m->prev_lvl_pos, B, s);
}

}  // namespace

namespace artalk {      // called from other files: declared in model.h
// Initial history of B clips (app/models.py:86-89) from the per-model cache (artalk_model::init_hist).
int run_init_history(artalk_model* m, int B, hipStream_t s) {
    const artalk_config& c = m->cfg;
    struct Restore { artalk_model* m; ~Restore() { kbucket(m, KB_OTHER); } } restore{m};
    Workspace& w = m->ws;
    artalk_model::InitHistory& ih = m->init_hist[m->precision];
    const long nb = (long)kNTok * c.code_dim, nf = 100L * c.code_dim * 4, nm = 180L * c.code_dim * 4;
    if (!ih.valid) {
        if (!ih.bits) {
            ih.bits = dalloc<uint8_t>(m, nb); ih.fdec = dalloc<float>(m, nf / 4); ih.msfeat = dalloc<float>(m, nm / 4);
            if (!ih.bits || !ih.fdec || !ih.msfeat) return fail(m, ARTALK_EHIP, "hipMalloc failed for the initial-history cache");
            HIPCHK(m, hipDeviceSynchronize());      // (dalloc's zero fill runs on the null stream)
        }
        launch_enc_input_zero(m->vae_mean, m->vae_std, m->enc_pos, w.enc_in, 1, s);
        run_reencode(m, 1, s);
        HIPCHK(m, hipMemcpyAsync(ih.bits, w.hist_bits, nb, hipMemcpyDeviceToDevice, s));
        HIPCHK(m, hipMemcpyAsync(ih.fdec, w.prev_fdec, nf, hipMemcpyDeviceToDevice, s));
        HIPCHK(m, hipMemcpyAsync(ih.msfeat, w.msfeat, nm, hipMemcpyDeviceToDevice, s));
        // The cache is complete before this call returns to its caller's enqueue loop: a later call on ANOTHER stream reads it with no
        // ordering against this fill otherwise.  Once per model and mode, beside the allocation above.  A fill that raised a
        // health flag (the range guard of the P8 format, a non-finite value) is NOT kept: every later call would reuse the damaged
        // history with a clean status word; it is recomputed - and flagged again - by the next call instead.
        int flags[4] = {0, 0, 0, 0};
        HIPCHK(m, hipMemcpyAsync(flags, w.status, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(m, hipStreamSynchronize(s));
        ih.valid = flags[0] == 0;
    }
    launch_broadcast16(ih.bits, w.hist_bits, nb, B, s);
    launch_broadcast16(ih.fdec, w.prev_fdec, nf, B, s);
    launch_broadcast16(ih.msfeat, w.msfeat, nm, B, s);
    launch_vq_embed(w.msfeat, kNTok - 1, m->vq_w, m->vq_b, m->prev_lvl_pos + kE, w.prev_in, kNTok, 1, w.style_cond, m->prev_lvl_pos, B, s);
    return ARTALK_OK;
}

}  // namespace artalk

namespace {
// Everything of one chunk index that depends only on (B, fixed workspace pointers): capturable as one hipGraph.
// n_reencode: clips (a prefix of the B) whose generated motion is re-encoded into the next history - the clips that HAVE a next chunk.
// The reference re-encodes after every chunk (app/models.py:111-114), the last one included, and throws that result away.
void run_chunk_body(artalk_model* m, int B, hipStream_t s, int n_reencode = -1) {
    struct BodyScope { artalk_model* m; BodyScope(artalk_model* x) : m(x) { m->in_body = true; } ~BodyScope() { m->in_body = false; } } scope(m);
    const artalk_config& c = m->cfg;
    Workspace& w = m->view ? *m->view : m->ws;
    const long ldada = m->ada_n;
    const long cache_l = (long)w.maxB * 2 * kNTok * 3 * kE;   // floats per layer
    // f16x3 mode: the block's GEMM-only activations (modulated LN output, attention output, FFN hidden) are written in the P8 split
    // format by their producers, which lets every block GEMM use the LDS-DMA kernels (gemm_p8_sm_kernel at these grid sizes)
    const int p8 = m->precision == 1 ? 1 : 0;
    // K/V of the 181 history tokens, once per layer (raw prev tokens, not modulated: app/transformer.py:68-70)
    kbucket(m, KB_AR_MISC);
    tap_copy(m, TAP_PREV_IN, 0, w.prev_in, kNTok, kE, B, s);      // prev_attn_feat + prev_lvl_pos_embed (app/models.py:101, 2nd argument)
    roctxRangePushA("artalk.ar.history_kv");
    SiteExps& ex = m->ex;
    if (p8) launch_pack_split(w.prev_in, reinterpret_cast<unsigned int*>(w.prev_in_p8), (long)B * kNTok * kE, false, s, w.status, ex.hist_tok);   // one split for the 12 layers
    audit(m, p8 ? w.prev_in_p8 : w.prev_in, B * kNTok, kE, kE, p8, s, &ex.hist_tok);
    {
        // all blocks in one launch: N = depth x (E keys + E values), column group l = block l's weight rows / cache columns
        GemmArgs g;
        g.A = p8 ? w.prev_in_p8 : w.prev_in; g.a_packed = p8; g.a_exp = ex.hist_tok;
        g.lda = kE; g.W = m->ar_qkv_w + (long)kE * kE; g.ldw = kE; g.bias = m->ar_qkv_b + kE;
        g.C = w.cache + kE; g.ldc = 3 * kE; g.cmap = rowmap(kNTok, 2 * kNTok, 0);
        g.M = B * kNTok; g.N = c.ar_depth * 2 * kE; g.K = kE;
        g.ngrp = 2 * kE; g.grpW = (long)3 * kE * kE; g.grpB = 3 * kE; g.grpC = cache_l;
        g.Wp = packed_of(m, g.W);
        if (p8 && gemm_p8_eligible(g)) {
            gemm(m, g, s);
        } else {
            for (int l = 0; l < c.ar_depth; ++l) {          // exact-f32 mode / small batches: one launch per block
                const ARLayer& L = m->ar[l];
                GemmArgs q = g;
                q.Wp = nullptr; q.ngrp = 0; q.grpW = q.grpB = q.grpC = 0;
                q.W = L.qkv_w + (long)kE * kE; q.bias = L.qkv_b + kE; q.C = w.cache + l * cache_l + kE; q.N = 2 * kE;
                gemm(m, q, s);
            }
        }
    }
    roctxRangePop();
    launch_ar_begin(w.style_cond, m->lvl_pos, w.x, w.fhat, B, s);
    static const char* const kLevelName[kMaxLv] = {"artalk.ar.scale_step0", "artalk.ar.scale_step1", "artalk.ar.scale_step2",
                                                   "artalk.ar.scale_step3", "artalk.ar.scale_step4"};
    for (int p = 0; p < c.n_levels; ++p) {
        Range r_lv(kLevelName[p]);                       // K8-K14 of one scale step: 12 blocks, head, bits, next-scale features
        kbucket(m, KB_LEVEL0 + p);
        const int pn = m->pn[p], off = m->off[p], M = B * pn;
        const RowMap amap = rowmap(pn, kNTok, off);            // rows of the AdaLN table for this level's tokens
        // AdaLN-modulated LayerNorm into w.xmod: block l's first (which = 0) / second (1) norm, or the head's (l = depth).  Each is
        // either its own launch or - when the GEMM that produces x is split over K - written by that GEMM's reduce pass.
        auto ln_args = [&](int l, int which) {
            LnArgs n;
            n.X = w.x; n.ldx = kE; n.Y = w.xmod; n.ldy = kE; n.ldm = ldada; n.mmap = amap; n.M = M; n.D = kE; n.eps = 1e-6f;
            n.status = p8 ? w.status : nullptr;
            if (l < c.ar_depth) {
                const float* ada = w.ada + (long)l * 6 * kE;   // gamma1,gamma2,scale1,scale2,shift1,shift2 (app/transformer.py:32)
                n.scale = ada + (2 + which) * kE; n.shift = ada + (4 + which) * kE; n.out_p8 = p8;
                n.p8_exp = which == 0 ? ex.ar[l].ln1 : ex.ar[l].ln2;
            } else {                                           // head (app/models.py:145-148): scale, shift = split2; fp32 (exact logits GEMM)
                const float* hada = w.ada + (long)c.ar_depth * 6 * kE;
                n.scale = hada; n.shift = hada + kE; n.out_p8 = 0;
            }
            return n;
        };
        bool have_ln = false;                                  // w.xmod already holds the norm the next GEMM reads
        for (int l = 0; l < c.ar_depth; ++l) {
            const ARLayer& L = m->ar[l];
            const float* ada = w.ada + (long)l * 6 * kE;
            float* cache = w.cache + l * cache_l;
            SiteExps::AR& E = ex.ar[l];
            if (l == 0) tap_copy(m, TAP_BLK0_IN, off, w.x, pn, kE, B, s);        // attn_feat entering attn_blocks[0] (app/models.py:100)
            if (!have_ln) launch_layernorm(ln_args(l, 0), s);
            audit(m, w.xmod, M, kE, kE, p8, s, &E.ln1);
            GemmArgs q;
            q.A = w.xmod; q.lda = kE; q.W = L.qkv_w; q.ldw = kE; q.bias = L.qkv_b; q.C = cache; q.ldc = 3 * kE;
            q.cmap = rowmap(pn, 2 * kNTok, kNTok + off); q.M = M; q.N = 3 * kE; q.K = kE; q.a_packed = p8; q.a_exp = E.ln1;
            gemm(m, q, s);
            AttnArgs a;
            a.Q = cache + (long)(kNTok + off) * 3 * kE; a.K = cache + kE; a.V = cache + 2 * kE;
            a.ldq = a.ldk = a.ldv = 3 * kE; a.q_bstride = a.k_bstride = a.v_bstride = (long)2 * kNTok * 3 * kE;
            a.O = w.attn_out; a.ldo = kE; a.o_bstride = (long)pn * kE;
            a.B = B; a.H = c.ar_heads; a.HD = kE / c.ar_heads; a.Lq = pn; a.Lk = kNTok + off + pn; a.scale = 1.0f;
            a.l2norm = 1; a.qscale = L.qscale; a.out_p8 = p8; a.split16 = p8; a.status = p8 ? w.status : nullptr; a.o_exp = E.attn;
            launch_attention(a, s);
            audit(m, w.attn_out, M, kE, kE, p8, s, &E.attn);
            GemmArgs pj;
            pj.A = w.attn_out; pj.lda = kE; pj.W = L.proj_w; pj.ldw = kE; pj.bias = L.proj_b; pj.C = w.x; pj.ldc = kE;
            pj.gate = ada; pj.ldg = ldada; pj.gmap = amap; pj.R = w.x; pj.ldr = kE; pj.M = M; pj.N = kE; pj.K = kE; pj.a_packed = p8; pj.a_exp = E.attn;
            const LnArgs n2 = ln_args(l, 1);
            if (!gemm(m, pj, s, &n2)) launch_layernorm(n2, s);
            audit(m, w.xmod, M, kE, kE, p8, s, &E.ln2);
            linear(m, w.xmod, kE, L.ffn1_w, L.ffn1_b, w.ffn_h, 4 * kE, M, 4 * kE, kE, ACT_GELU_TANH, nullptr, s, p8 ? (LF_A_P8 | LF_C_P8) : 0, nullptr, E.ln2, E.ffn);
            audit(m, w.ffn_h, M, 4 * kE, 4 * kE, p8, s, &E.ffn);
            GemmArgs f2;
            f2.A = w.ffn_h; f2.lda = 4 * kE; f2.W = L.ffn2_w; f2.ldw = 4 * kE; f2.bias = L.ffn2_b; f2.C = w.x; f2.ldc = kE;
            f2.gate = ada + kE; f2.ldg = ldada; f2.gmap = amap; f2.R = w.x; f2.ldr = kE; f2.M = M; f2.N = kE; f2.K = 4 * kE; f2.a_packed = p8; f2.a_exp = E.ffn;
            const LnArgs nn = ln_args(l + 1, 0);               // next block's first norm, or the head's after the last block
            have_ln = gemm(m, f2, s, &nn);
            if (l == 0) tap_copy(m, TAP_BLK0_OUT, off, w.x, pn, kE, B, s);        // output of attn_blocks[0] (app/transformer.py:43)
            if (l == c.ar_depth - 1) tap_copy(m, TAP_BLKL_OUT, off, w.x, pn, kE, B, s);   // output of the last block (app/models.py:102)
        }
        if (!have_ln) launch_layernorm(ln_args(c.ar_depth, 0), s);
        linear(m, w.xmod, kE, m->logits_w, m->logits_b, w.logits, 2 * c.code_dim, M, 2 * c.code_dim, kE, ACT_NONE, nullptr, s, LF_EXACT);
        tap_copy(m, TAP_LOGITS, off, w.logits, pn, 2 * c.code_dim, B, s);          // pred_motion_logits (app/models.py:103), fp32
        launch_ar_bits_next(w.logits, w.bits, w.fhat, w.nextfeat, B, p, s, w.status);
        if (p + 1 < c.n_levels)
            launch_vq_embed(w.nextfeat, m->pn[p + 1], m->vq_w, m->vq_b, m->lvl_pos + (long)m->off[p + 1] * kE, w.x, m->pn[p + 1], 0,
                            nullptr, nullptr, B, s);
    }
    stage_mark(m, s, PB_AR);
    // ---- VAE decode of [history | current] (bitwise_vae.py:105-113) ----
    const int H = c.vae_hidden;
    roctxRangePushA("artalk.vae.decode");               // K15
    kbucket(m, KB_VAE_DEC);
    launch_dec_input(w.prev_fdec, w.fhat, w.bits, m->dec_pos, w.dec_x, B, s);
    audit(m, w.dec_x, B * 200, c.code_dim, c.code_dim, false, s, &ex.vae_dec_in);
    linear(m, w.dec_x, c.code_dim, m->dec.in_w, m->dec.in_b, w.vh, H, B * 200, H, c.code_dim, ACT_LEAKY02, nullptr, s, 0, nullptr, ex.vae_dec_in);
    run_vae_stack(m, m->dec, B, 200, 100, s);
    audit(m, w.vh, B * 200, H, H, false, s, &ex.vae_dec_head);
    linear(m, w.vh, H, m->dec.out_w, m->dec.out_b, w.dec_out, c.motion_dim, B * 200, c.motion_dim, H, ACT_NONE, nullptr, s, 0, nullptr, ex.vae_dec_head);
    tap_copy(m, TAP_DEC_OUT, 0, w.dec_out, 200, c.motion_dim, B, s);               // dec_out before unnorm_with_stats (bitwise_vae.py:111)
    launch_dec_finish(w.dec_out, m->vae_mean, m->vae_std, m->enc_pos, w.motion_chunk, 100L * c.motion_dim, 0, w.enc_in, B, s, w.status);
    roctxRangePop();
    // ---- re-encode the generated motion into the next history (app/models.py:111-114) ----
    if (n_reencode < 0 || n_reencode > B) n_reencode = B;
    if (n_reencode > 0) run_reencode(m, n_reencode, s);
    stage_mark(m, s, PB_VAE);
}

// A view of the workspace for clips [b0, ...): every per-clip buffer pointer advanced by b0 clips (compact step buffers get a
// fixed 100-row region per clip so the two halves never overlap), its own split-K scratch.
Workspace clip_view(const artalk_model* m, int b0, int branch) {
    Workspace v = m->ws;
    for (const ClipBuf& cb : clip_buffers(m)) {
        if (cb.f) v.*cb.f += b0 * cb.n; else v.*cb.u8 += b0 * cb.n;
    }
    v.splitk = m->ws.splitk_b[branch];
    return v;
}

// The AR/VAE body of one chunk index for B clips.  The small scale steps leave most CUs idle, and clips are independent, so the
// batch is cut into n clip groups (1, 2 or 4: body_branches), each with its own workspace view and split-K scratch, that run as
// parallel branches on stream s and m->side_stream: one group's GPU-filling step overlaps the others' latency-bound ones.  With
// graphs on every group is one hipGraph (a single captured graph with a fork/join ran almost serially).
// HIP multiplexes streams onto a few hardware queues (4 by default): every extra stream a process creates can end up sharing a
// queue with the caller's stream and serialise the branches, so side streams are created lazily and only as many as are used.
int ensure_side_streams(artalk_model* m, int n) {
    bool ok = m->fork_ev.create(hipEventDisableTiming);
    for (int i = 0; ok && i < n && i < 3; ++i)      // (a create on a member that holds something keeps it)
        ok = (m->cu_mask.empty() ? m->side_stream[i].create() : m->side_stream[i].create_masked(m->cu_mask.data(), (int)m->cu_mask.size())) &&
             m->join_ev[i].create(hipEventDisableTiming);
    return ok ? ARTALK_OK : fail(m, ARTALK_EHIP, "creating the side streams of the clip groups and their events failed");
}
int body_branches(const artalk_model* m, int B) {
    // measured at batch 32: 1 branch 54.9 ms, 2 branches 49.5 ms, 4 branches 77-120 ms (queue sharing / contention)
    const int want = m->branches > 0 ? m->branches : (B >= 8 ? 2 : 1);
    return B >= 2 * want ? want : (B >= 8 ? 2 : 1);
}
// Replay captured graphs, or launch eagerly?  The one rule, for the batch call and the streaming calls alike: the audit and the taps
// are launches of their own that a replay would not make (or would make forever), profiling levels 2 and 3 time the single launches.
bool body_uses_graphs(const artalk_model* m) { return m->use_graphs && m->profiling < 2 && !m->audit && !m->tap; }
// Graph cache: one hipGraphExec per (active clips, clip group, precision, re-encoded clips of the group).  The key space is bounded
// (ADVICE r4): the re-encode count of a group is rounded UP to a multiple of 8 (re-encoding a clip without a next chunk is what the
// reference does anyway, app/models.py:111-114; its history is never read), so a group contributes at most 1 + size / 8 keys per
// active-batch size instead of one per (B_j, B_j+1) pair; and the cache holds at most kMaxGraphs executables, least recently used
// evicted (a serving loop with ever-changing ragged batches re-captures instead of growing without bound).
constexpr size_t kMaxGraphs = 96;
int evict_graphs(artalk_model* m, const long long* keep, int n_keep) {
    while (m->graphs.size() >= kMaxGraphs) {
        auto victim = m->graphs.end();
        for (auto it = m->graphs.begin(); it != m->graphs.end(); ++it) {
            bool pinned = false;
            for (int i = 0; i < n_keep; ++i) pinned |= it->first == keep[i];
            if (!pinned && (victim == m->graphs.end() || it->second.last_use < victim->second.last_use)) victim = it;
        }
        if (victim == m->graphs.end()) break;
        HIPCHK(m, hipDeviceSynchronize());      // the victim may still be running on a side stream of an earlier call
        m->graphs.erase(victim);
    }
    return ARTALK_OK;
}
// The clip groups of one chunk index: group h holds clips [b0[h], b0[h + 1]) and re-encodes its first nre[h] (n_next = clips of the B,
// a prefix, that have a next chunk; < 0 = all).  The only place that cuts a batch: graph replay, the eager streams and the kernel
// timer run the same groups, so the body's GEMMs get the same M - the same tiles, split-K and summation order - in all three.
struct BodyGroups { bool graphs; int n; int b0[5]; int nre[4]; long long key[4]; };
BodyGroups plan_body(const artalk_model* m, int B, int n_next) {
    BodyGroups g;
    if (n_next < 0 || n_next > B) n_next = B;
    g.graphs = body_uses_graphs(m) && B <= 4095;      // (graph keys hold 12 bits of clip counts)
    // one group: the audit and the taps address the batch as a whole, level 2 times whole stages; body_branches covers m->branches == 1
    const bool whole = m->audit || m->tap || m->profiling == 2 || (body_uses_graphs(m) && !g.graphs);
    g.n = whole ? 1 : body_branches(m, B);
    for (int h = 0; h <= g.n; ++h) g.b0[h] = (int)((long)B * h / g.n);
    for (int h = 0; h < g.n; ++h) {
        const int gsz = g.b0[h + 1] - g.b0[h];
        const int need = std::max(0, std::min(n_next - g.b0[h], gsz));      // clips of this group that have a next chunk
        g.nre[h] = g.graphs ? std::min(gsz, (need + 7) / 8 * 8) : need;     // rounded only where it bounds the key space
        g.key[h] = ((long long)(((B * 8 + g.n) * 4 + h) * 3 + m->precision)) * 4096 + g.nre[h];     // (3 precision modes)
    }
    return g;
}
// Runs the groups: replay of their graphs on n streams (captured on a miss), eagerly on n streams (graphs off), or - kernel timer,
// profiling level 3 - eagerly one after the other on s: the sums are then those of the production launches, without their overlap.
int run_body(artalk_model* m, int B, hipStream_t s, int n_next) {
    const BodyGroups g = plan_body(m, B, n_next);
    const bool fork = g.n > 1 && m->profiling != 3;
    if (fork) { if (int rc = ensure_side_streams(m, g.n - 1)) return rc; }
    hipStream_t st[4] = {s, s, s, s};
    for (int h = 1; fork && h < g.n; ++h) st[h] = m->side_stream[h - 1].get();
    Workspace views[4];
    for (int h = 0; h < g.n; ++h) views[h] = clip_view(m, g.b0[h], h);
    auto launch_group = [&](int h) { m->view = &views[h]; run_chunk_body(m, g.b0[h + 1] - g.b0[h], st[h], g.nre[h]); m->view = nullptr; };
    for (int h = 0; g.graphs && h < g.n; ++h) {      // capture what the cache lacks, before anything of this chunk index is launched
        auto hit = m->graphs.find(g.key[h]);
        if (hit != m->graphs.end()) { hit->second.last_use = ++m->graph_clock; continue; }
        if (int rc = evict_graphs(m, g.key, g.n)) return rc;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        HIPCHK(m, hipStreamBeginCapture(st[h], hipStreamCaptureModeThreadLocal));
        m->in_graph_body = true;
        launch_group(h);
        m->in_graph_body = false;
        HIPCHK(m, hipStreamEndCapture(st[h], &graph));
        HIPCHK(m, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        (void)hipGraphDestroy(graph);
        m->graphs.emplace(g.key[h], artalk_model::GraphEntry{GraphExec(exec), ++m->graph_clock});
        ++m->graph_captures;
    }
    if (fork) {
        HIPCHK(m, hipEventRecord(m->fork_ev.get(), s));
        for (int h = 1; h < g.n; ++h) HIPCHK(m, hipStreamWaitEvent(st[h], m->fork_ev.get(), 0));
    }
    for (int h = 0; h < g.n; ++h) {
        if (g.graphs) HIPCHK(m, hipGraphLaunch(m->graphs[g.key[h]].exec.get(), st[h]));
        else launch_group(h);
    }
    for (int h = 1; fork && h < g.n; ++h) {
        HIPCHK(m, hipEventRecord(m->join_ev[h - 1].get(), st[h]));
        HIPCHK(m, hipStreamWaitEvent(s, m->join_ev[h - 1].get(), 0));
    }
    return ARTALK_OK;
}

}  // namespace

namespace artalk {      // called from other files: declared in model.h
// Start of a call for B clips: the style flags go through the pinned slot `stg` (its event then covers every copy the caller staged
// in it before), the status word is reset, the style conditions are computed.
int begin_clips(artalk_model* m, hipStream_t s, int B, const float* style_motion_dev, const uint8_t* has_style, bool encode_style,
                artalk_model::Stage* stg) {
    Workspace& w = m->ws;
    if (!has_style) style_motion_dev = nullptr;
    if (style_motion_dev) {
        std::memcpy(stg->has.get(), has_style, (size_t)B);
        HIPCHK(m, hipMemcpyAsync(w.has_style, stg->has.get(), B, hipMemcpyHostToDevice, s));
    }
    HIPCHK(m, hipEventRecord(stg->done.get(), s));   // pinned slot: no synchronisation, the slot is reused kStageSlots calls later
    stg->used = true;
    HIPCHK(m, hipMemsetAsync(w.status, 0, 4 * sizeof(int), s));
    stage_mark(m, s, PB_OTHER);
    run_style(m, style_motion_dev, B, s, encode_style);
    stage_mark(m, s, PB_STYLE);
    return ARTALK_OK;
}
// One chunk index of Bn clips whose SiLU(cond) rows start at row cond_row0 * 181 of w.silu_cond: the AdaLN table of all blocks + head,
// SiLU(cond) @ [W_0;...;W_11;W_head]^T, in line in front of the body that reads it, the body, and the chunk's motion to the caller
// ([Bn][out_stride] floats).  tap_chunk = the chunk's row of slots in the tap buffer (m->tap_maxch: none).
// (The table of chunk index j + 1 on a stream of its own beside body j was measured in round 4 and removed in round 5: the bodies slow
// down by what the table GEMM takes, profiles/r04_ada_overlap_sweep.log.)
int chunk_step(artalk_model* m, hipStream_t s, int cond_row0, int Bn, int n_next, int tap_chunk, float* out_motion_dev, int64_t out_stride) {
    Workspace& w = m->ws;
    m->tap_chunk = tap_chunk;
    roctxRangePushA("artalk.ar.adaln_table");
    kbucket(m, KB_ADA);
    linear(m, w.silu_cond + (long)cond_row0 * kNTok * kCond, kCond, m->ada_w, m->ada_b, w.ada, m->ada_n, Bn * kNTok, m->ada_n, kCond,
           ACT_NONE, nullptr, s, m->precision == 1 ? LF_A_P8 : 0, nullptr, m->ex.silu_cond);
    roctxRangePop();
    stage_mark(m, s, PB_ADA);
    if (body_uses_graphs(m)) {
        Range r_body("artalk.body.graph");
        if (int rc = run_body(m, Bn, s, n_next)) return rc;
        stage_mark(m, s, PB_AR);   // light profiling: the whole captured body (AR steps + VAE) is charged to the AR bucket
    } else {
        if (int rc = run_body(m, Bn, s, n_next)) return rc;
    }
    const size_t mrow = (size_t)100 * m->cfg.motion_dim * 4;
    HIPCHK(m, hipMemcpy2DAsync(out_motion_dev, (size_t)out_stride * 4, w.motion_chunk, mrow, mrow, Bn, hipMemcpyDeviceToDevice, s));
    return ARTALK_OK;
}

}  // namespace artalk
