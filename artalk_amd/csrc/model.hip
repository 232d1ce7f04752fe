// Model lifetime and state behind the C ABI (model.h): the weight registry in the reference's key names and the derived layouts, the
// packed and bf16 weight copies, workspace and pinned staging ring, the site table and its scales, settings, calibration, status and
// profile.  Nothing here launches the path: that is engine.hip.
#include "model.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace artalk;

namespace {
thread_local std::string g_create_error;

float* walloc(artalk_model* m, int64_t n) {
    m->weight_bytes += n * 4;
    float* p = dalloc<float>(m, n);
    m->wranges.push_back({p, n, nullptr, nullptr});
    return p;
}

}  // namespace

namespace artalk {      // called from other files: declared in model.h
const unsigned int* packed_of(const artalk_model* m, const float* w) {
    for (const auto& r : m->wranges)
        if (r.packed && w >= r.base && w < r.base + r.n) return r.packed + (w - r.base);
    return nullptr;
}

// the bf16 copy of a weight (same indexing), or null before ensure_bf16_copy / for a pointer that is no weight
const void* bf16_of(const artalk_model* m, const float* w) {
    for (const auto& r : m->wranges)
        if (r.bf16 && w >= r.base && w < r.base + r.n) return r.bf16 + (w - r.base);
    return nullptr;
}

}  // namespace artalk

namespace {
// Precision mode 2 reads every weight from a bf16 copy: built once, on the first switch to the mode (a model that never runs bf16
// allocates nothing for it).  One allocation, each weight at a 64-element aligned offset; weight_bytes counts 2 bytes per parameter.
int ensure_bf16_copy(artalk_model* m) {
    if (m->have_bf16) return ARTALK_OK;
    int64_t total = 0;
    for (const auto& r : m->wranges) total += (r.n + 63) / 64 * 64;
    uint16_t* base = dalloc<uint16_t>(m, total);
    if (!base) return fail(m, ARTALK_EHIP, "hipMalloc failed for the bf16 weight copy");
    HIPCHK(m, hipDeviceSynchronize());      // (dalloc's zero fill runs on the null stream)
    int64_t off = 0;
    for (auto& r : m->wranges) {
        r.bf16 = base + off;
        launch_pack_bf16(r.base, r.bf16, r.n, nullptr);
        off += (r.n + 63) / 64 * 64;
    }
    HIPCHK(m, hipDeviceSynchronize());
    for (const auto& r : m->wranges) m->weight_bytes += r.n * 2;     // counted once the copy exists
    m->have_bf16 = true;
    return ARTALK_OK;
}

void add_slot(artalk_model* m, const std::string& key, std::vector<int64_t> shape, SlotKind kind, float* dst,
              int64_t pad_to = 0, int dtype = ARTALK_DTYPE_F32) {
    Slot s;
    s.shape = std::move(shape); s.kind = kind; s.dst = dst; s.pad_to = pad_to; s.dtype = dtype;
    m->slots[key] = std::move(s);
}

// Linear: weight [out,in] (+bias) copied as is.
void add_linear(artalk_model* m, const std::string& p, int out_f, int in_f, float*& w, float*& b, bool bias = true) {
    w = walloc(m, (int64_t)out_f * in_f);
    add_slot(m, p + ".weight", {out_f, in_f}, SK_DIRECT, w);
    if (bias) { b = walloc(m, out_f); add_slot(m, p + ".bias", {out_f}, SK_DIRECT, b); } else b = nullptr;
}
void add_vec(artalk_model* m, const std::string& key, int n, float*& v) {
    v = walloc(m, n);
    add_slot(m, key, {n}, SK_DIRECT, v);
}
void add_ln(artalk_model* m, const std::string& p, int n, float*& w, float*& b) {
    add_vec(m, p + ".weight", n, w);
    add_vec(m, p + ".bias", n, b);
}

int build_registry(artalk_model* m) {
    const artalk_config& c = m->cfg;
    const int NT = kNTok;
    // ---- top level (app/models.py:19-56) ----
    add_slot(m, "null_style_cond", {1, 1, kE}, SK_DIRECT, m->null_style = walloc(m, kE));
    add_slot(m, "pos_embed", {1, NT, kE}, SK_HOST, nullptr);
    add_slot(m, "prev_pos_embed", {1, NT, kE}, SK_HOST, nullptr);
    add_slot(m, "attn_bias_for_masking", {1, 1, NT, 2 * NT}, SK_HOST, nullptr);
    add_slot(m, "lvl_idx", {1, NT}, SK_HOST, nullptr, 0, ARTALK_DTYPE_I64);
    add_slot(m, "lvl_embed.weight", {c.n_levels, kE}, SK_HOST, nullptr);
    m->lvl_pos = walloc(m, (int64_t)NT * kE);
    m->prev_lvl_pos = walloc(m, (int64_t)NT * kE);
    add_linear(m, "vqfeat_embed", kE, c.code_dim, m->vq_w, m->vq_b);
    add_linear(m, "style_cond_embed", kE, c.style_dim, m->sc_w, m->sc_b);
    add_linear(m, "logits_head", 2 * c.code_dim, kE, m->logits_w, m->logits_b);
    // fused AdaLN table: rows [l*6E, (l+1)*6E) = block l, rows [depth*6E, depth*6E+2E) = head
    m->ada_n = c.ar_depth * 6 * kE + 2 * kE;
    m->ada_w = walloc(m, (int64_t)m->ada_n * kCond);
    m->ada_b = walloc(m, m->ada_n);
    add_slot(m, "cond_logits_head.ada_lin.1.weight", {2 * kE, kCond}, SK_DIRECT, m->ada_w + (int64_t)c.ar_depth * 6 * kE * kCond);
    add_slot(m, "cond_logits_head.ada_lin.1.bias", {2 * kE}, SK_DIRECT, m->ada_b + c.ar_depth * 6 * kE);
    m->ar.resize(c.ar_depth);
    // q|k|v weights of all blocks in ONE allocation ([depth][3E][E]): the K/V projections of the 181 history tokens are the same
    // input through every block's key / value weights, and run as one GEMM over column groups (run_chunk_body)
    m->ar_qkv_w = walloc(m, (int64_t)c.ar_depth * 3 * kE * kE);
    m->ar_qkv_b = walloc(m, (int64_t)c.ar_depth * 3 * kE);
    for (int i = 0; i < c.ar_depth; ++i) {
        ARLayer& L = m->ar[i];
        const std::string p = "attn_blocks." + std::to_string(i);
        add_slot(m, p + ".attn.scale_mul_1H11", {1, c.ar_heads, 1, 1}, SK_HOST, nullptr);
        L.qscale = walloc(m, c.ar_heads);
        L.qkv_w = m->ar_qkv_w + (int64_t)i * 3 * kE * kE;
        L.qkv_b = m->ar_qkv_b + (int64_t)i * 3 * kE;     // key has no bias (app/transformer.py:61): stays zero
        add_slot(m, p + ".attn.query.weight", {kE, kE}, SK_DIRECT, L.qkv_w);
        add_slot(m, p + ".attn.query.bias", {kE}, SK_DIRECT, L.qkv_b);
        add_slot(m, p + ".attn.key.weight", {kE, kE}, SK_DIRECT, L.qkv_w + (int64_t)kE * kE);
        add_slot(m, p + ".attn.value.weight", {kE, kE}, SK_DIRECT, L.qkv_w + (int64_t)2 * kE * kE);
        add_slot(m, p + ".attn.value.bias", {kE}, SK_DIRECT, L.qkv_b + 2 * kE);
        add_linear(m, p + ".attn.proj", kE, kE, L.proj_w, L.proj_b);
        add_linear(m, p + ".ffn.0", 4 * kE, kE, L.ffn1_w, L.ffn1_b);
        add_linear(m, p + ".ffn.2", kE, 4 * kE, L.ffn2_w, L.ffn2_b);
        add_slot(m, p + ".ada_lin.1.weight", {6 * kE, kCond}, SK_DIRECT, m->ada_w + (int64_t)i * 6 * kE * kCond);
        add_slot(m, p + ".ada_lin.1.bias", {6 * kE}, SK_DIRECT, m->ada_b + i * 6 * kE);
    }
    // ---- VAE (app/modules/bitwise_vae.py) ----
    const int H = c.vae_hidden, T2 = 2 * c.patch_nums[c.n_levels - 1], MD = c.motion_dim;
    add_slot(m, "basic_vae.enc_pos_embed", {1, T2, MD}, SK_DIRECT, m->enc_pos = walloc(m, (int64_t)T2 * MD));
    add_slot(m, "basic_vae.dec_pos_embed", {1, T2, c.code_dim}, SK_DIRECT, m->dec_pos = walloc(m, (int64_t)T2 * c.code_dim));
    add_slot(m, "basic_vae.attn_mask", {1, 1, T2, T2}, SK_HOST, nullptr);
    add_vec(m, "basic_vae.motion_mean", MD, m->vae_mean);
    add_vec(m, "basic_vae.motion_std", MD, m->vae_std);
    m->enc.in_w = walloc(m, (int64_t)H * 128);
    add_slot(m, "basic_vae.encoder.inp_mapping.0.weight", {H, MD}, SK_PADK, m->enc.in_w, 128);
    add_vec(m, "basic_vae.encoder.inp_mapping.0.bias", H, m->enc.in_b);
    add_linear(m, "basic_vae.encoder.code_mapping", c.code_dim, H, m->enc.out_w, m->enc.out_b);
    add_linear(m, "basic_vae.decoder.inp_mapping.0", H, c.code_dim, m->dec.in_w, m->dec.in_b);
    add_linear(m, "basic_vae.decoder.out_mapping", MD, H, m->dec.out_w, m->dec.out_b);
    for (int side = 0; side < 2; ++side) {
        VAESide& S = side == 0 ? m->enc : m->dec;
        const std::string base = side == 0 ? "basic_vae.encoder.encoder_transformer." : "basic_vae.decoder.decoder_transformer.";
        S.layers.resize(c.vae_depth);
        for (int i = 0; i < c.vae_depth; ++i) {
            VAELayer& L = S.layers[i];
            const std::string a = base + std::to_string(2 * i), f = base + std::to_string(2 * i + 1);
            add_ln(m, a + ".norm", H, L.lnw, L.lnb);
            float* nb = nullptr;
            add_linear(m, a + ".to_qkv", 3 * H, H, L.qkv_w, nb, false);
            add_linear(m, a + ".to_out", H, H, L.out_w, L.out_b);
            add_linear(m, f + ".0", H * 3 / 2, H, L.m1_w, L.m1_b);
            add_linear(m, f + ".2", H, H * 3 / 2, L.m2_w, L.m2_b);
        }
    }
    // ---- style encoder (app/modules/style_encoder.py) ----
    const int S = c.style_dim;
    add_vec(m, "style_encoder.motion_mean", MD, m->st_mean);
    add_vec(m, "style_encoder.motion_std", MD, m->st_std);
    add_slot(m, "style_encoder.PE.pe", {1, 600, S}, SK_HOST, nullptr);
    m->st_pe = walloc(m, S);
    m->st_proj_w = walloc(m, (int64_t)S * 128);
    add_slot(m, "style_encoder.encoder.motion_proj.weight", {S, MD}, SK_PADK, m->st_proj_w, 128);
    add_vec(m, "style_encoder.encoder.motion_proj.bias", S, m->st_proj_b);
    m->style.resize(c.style_layers);
    for (int i = 0; i < c.style_layers; ++i) {
        StyleLayer& L = m->style[i];
        const std::string p = "style_encoder.encoder.transformer.layers." + std::to_string(i);
        L.in_w = walloc(m, (int64_t)3 * S * S); L.in_b = walloc(m, 3 * S);
        add_slot(m, p + ".self_attn.in_proj_weight", {3 * S, S}, SK_DIRECT, L.in_w);
        add_slot(m, p + ".self_attn.in_proj_bias", {3 * S}, SK_DIRECT, L.in_b);
        add_linear(m, p + ".self_attn.out_proj", S, S, L.out_w, L.out_b);
        add_linear(m, p + ".linear1", c.style_ffn, S, L.l1_w, L.l1_b);
        add_linear(m, p + ".linear2", S, c.style_ffn, L.l2_w, L.l2_b);
        add_ln(m, p + ".norm1", S, L.n1w, L.n1b);
        add_ln(m, p + ".norm2", S, L.n2w, L.n2b);
    }
    // ---- wav2vec2 ----
    const int Hs = c.w2v_hidden, Fi = c.w2v_ffn, CD = c.w2v_conv_dim;
    add_slot(m, "audio_encoder.masked_spec_embed", {Hs}, SK_IGNORE, nullptr);   // dead in inference
    int cin = 1;
    for (int i = 0; i < c.w2v_n_conv; ++i) {
        const std::string p = "audio_encoder.feature_extractor.conv_layers." + std::to_string(i);
        const int k = c.w2v_conv_kernel[i];
        m->conv_w[i] = walloc(m, (int64_t)CD * cin * k);
        add_slot(m, p + ".conv.weight", {CD, cin, k}, i == 0 ? SK_DIRECT : SK_CONV, m->conv_w[i]);
        add_vec(m, p + ".conv.bias", CD, m->conv_b[i]);
        add_ln(m, p + ".layer_norm", CD, m->conv_lnw[i], m->conv_lnb[i]);
        cin = CD;
    }
    m->conv0_w = m->conv_w[0];
    add_ln(m, "audio_encoder.feature_projection.layer_norm", CD, m->fp_lnw, m->fp_lnb);
    add_linear(m, "audio_encoder.feature_projection.projection", Hs, CD, m->fp_w, m->fp_b);
    const std::string pc = "audio_encoder.encoder.pos_conv_embed.conv";
    add_vec(m, pc + ".bias", Hs, m->pos_b);
    add_slot(m, pc + ".parametrizations.weight.original0", {1, 1, c.w2v_pos_kernel}, SK_HOST, nullptr);
    add_slot(m, pc + ".parametrizations.weight.original1", {Hs, Hs / c.w2v_pos_groups, c.w2v_pos_kernel}, SK_HOST, nullptr);
    m->pos_w = walloc(m, (int64_t)Hs * (Hs / c.w2v_pos_groups) * c.w2v_pos_kernel);
    add_ln(m, "audio_encoder.encoder.layer_norm", Hs, m->enc_lnw, m->enc_lnb);
    m->w2v.resize(c.w2v_layers);
    for (int i = 0; i < c.w2v_layers; ++i) {
        W2VLayer& L = m->w2v[i];
        const std::string p = "audio_encoder.encoder.layers." + std::to_string(i);
        L.qkv_w = walloc(m, (int64_t)3 * Hs * Hs); L.qkv_b = walloc(m, 3 * Hs);
        const char* names[3] = {"q_proj", "k_proj", "v_proj"};
        for (int j = 0; j < 3; ++j) {
            add_slot(m, p + ".attention." + names[j] + ".weight", {Hs, Hs}, SK_DIRECT, L.qkv_w + (int64_t)j * Hs * Hs);
            add_slot(m, p + ".attention." + names[j] + ".bias", {Hs}, SK_DIRECT, L.qkv_b + j * Hs);
        }
        add_linear(m, p + ".attention.out_proj", Hs, Hs, L.out_w, L.out_b);
        add_ln(m, p + ".layer_norm", Hs, L.ln1w, L.ln1b);
        add_ln(m, p + ".final_layer_norm", Hs, L.ln2w, L.ln2b);
        add_linear(m, p + ".feed_forward.intermediate_dense", Fi, Hs, L.ff1_w, L.ff1_b);
        add_linear(m, p + ".feed_forward.output_dense", Hs, Fi, L.ff2_w, L.ff2_b);
    }
    if (!m->weights.ok()) return fail(m, ARTALK_EHIP, "hipMalloc failed while allocating weights");
    return ARTALK_OK;
}

int upload(artalk_model* m, float* dst, const float* src, int64_t n) {
    HIPCHK(m, hipMemcpy(dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return ARTALK_OK;
}

// the captured body graphs (engine.hip: run_body) hold workspace pointers, site exponents and grid sizes: dropped when one changes
void drop_graphs(artalk_model* m) { m->graphs.clear(); }
}  // namespace

namespace artalk {      // called from other files: declared in model.h
// The status slots once, and a ring of pinned slots for maxB clips and maxC chunks: a whole ring, or a failure with the caps at 0 (the
// next call builds it again).  The slots' `done` events live through a regrow.
int ensure_stage(artalk_model* m, int maxB, int maxC) {
    if (!m->h_status.get()) {
        bool ok = true;
        for (auto& e : m->status_ev) ok = ok && e.create(hipEventDisableTiming);
        if (!ok || !m->h_status.alloc(artalk_model::kStatusSlots)) return fail(m, ARTALK_EHIP, "the pinned status slots or their events could not be taken from the runtime");
        std::memset(m->h_status.get(), 0, artalk_model::kStatusSlots * sizeof(int));
    }
    if (maxB <= m->stage_cap_b && maxC <= m->stage_cap_c) return ARTALK_OK;
    for (auto& st : m->stage) if (st.used) HIPCHK(m, hipEventSynchronize(st.done.get()));
    m->stage_cap_c = m->stage_cap_b = 0;
    bool ok = true;
    for (auto& st : m->stage) {      // (alloc gives the old block back first)
        st.used = false;
        ok = ok && st.src.alloc((size_t)3 * maxC) && st.has.alloc((size_t)maxB) && st.slots.alloc((size_t)maxB) && st.smooth.alloc((size_t)maxB) &&
             st.done.create(hipEventDisableTiming);
    }
    if (!ok) return fail(m, ARTALK_EHIP, "the pinned staging ring or its events could not be taken from the runtime");
    m->stage_cap_b = maxB; m->stage_cap_c = maxC;
    return ARTALK_OK;
}
// next slot of the ring; waits only if the call that last used it has not consumed its copies yet
int next_stage(artalk_model* m, artalk_model::Stage** out) {
    artalk_model::Stage& st = m->stage[m->stage_next];
    m->stage_next = (m->stage_next + 1) % artalk_model::kStageSlots;
    if (st.used) HIPCHK(m, hipEventSynchronize(st.done.get()));
    *out = &st;
    return ARTALK_OK;
}
// end of a call: hand the device status word to the host asynchronously (artalk_get_status / artalk_poll_status read it)
int publish_status(artalk_model* m, hipStream_t s) {
    const int slot = (int)(m->ticket % artalk_model::kStatusSlots);
    // the slot's previous user is kStatusSlots calls back: its copy has long landed unless the caller queued more calls than slots
    if (m->ticket >= artalk_model::kStatusSlots) HIPCHK(m, hipEventSynchronize(m->status_ev[slot].get()));
    HIPCHK(m, hipMemcpyAsync(m->h_status.get() + slot, m->ws.status, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(m, hipEventRecord(m->status_ev[slot].get(), s));
    ++m->ticket;
    m->status_pending = true;
    HIPCHK(m, hipGetLastError());
    return ARTALK_OK;
}

// Every per-clip buffer of the workspace with its elements per clip, in allocation order (the compact step buffers x .. nextfeat get a
// fixed 100-row region per clip).  The one statement of these extents: reserve() allocates maxB clips of each, clip_view() (engine.hip)
// advances each by the clips in front of a clip group.
std::vector<ClipBuf> clip_buffers(const artalk_model* m) {
    const artalk_config& c = m->cfg;
    const int64_t cd = c.code_dim, md = c.motion_dim, H = c.vae_hidden;
    using W = Workspace;
    auto f = [](float* W::*p, int64_t n) { return ClipBuf{p, nullptr, n}; };
    auto u8 = [](uint8_t* W::*p, int64_t n) { return ClipBuf{nullptr, p, n}; };
    return {f(&W::ada, (int64_t)kNTok * m->ada_n), f(&W::style_cond, kE), f(&W::prev_in, kNTok * kE), f(&W::prev_in_p8, kNTok * kE),
            f(&W::cache, 2 * kNTok * 3 * kE), f(&W::x, 100 * kE), f(&W::xmod, 100 * kE), f(&W::attn_out, 100 * kE), f(&W::ffn_h, 100 * 4 * kE),
            f(&W::logits, 100 * 2 * cd), f(&W::fhat, 100 * cd), f(&W::nextfeat, 100 * cd),
            u8(&W::bits, kNTok * cd), u8(&W::hist_bits, kNTok * cd),
            f(&W::prev_fdec, 100 * cd), f(&W::msfeat, 180 * cd), f(&W::dec_x, 200 * cd),
            f(&W::vh, 200 * H), f(&W::vln, 200 * H), f(&W::vqkv, 200 * 3 * H), f(&W::vatt, 200 * H), f(&W::vmlp, 200 * H * 3 / 2),
            f(&W::dec_out, 200 * md), f(&W::enc_in, 100 * 128), f(&W::enc_out, 100 * cd), f(&W::motion_chunk, 100 * md)};
}

int reserve(artalk_model* m, int maxB, int maxC) {
    const artalk_config& c = m->cfg;
    if (maxB <= m->ws.maxB && maxC <= m->ws.maxC) return ensure_stage(m, m->ws.maxB, m->ws.maxC);
    // grow: drop the old workspace (and the graphs that captured its pointers) and allocate the larger one
    maxB = std::max(maxB, m->ws.maxB); maxC = std::max(maxC, m->ws.maxC);
    (void)hipDeviceSynchronize();
    drop_graphs(m);
    m->ws_pool.clear();
    m->ws = Workspace();
    m->stream_B = 0; m->stream_scales_ended = false;          // the streaming history lived in the workspace that was just dropped: a session must begin again
    m->status_pending = false;
    Workspace& w = m->ws;
    const int CD = c.w2v_conv_dim, Hs = c.w2v_hidden;
    w.maxB = maxB; w.maxC = maxC; w.G = std::min(maxC, 96);
    auto F = [&](int64_t n) { w.bytes += n * 4; return m->ws_pool.take<float>(n); };
    const int G = w.G;
    w.src_off = m->ws_pool.take<long>((int64_t)3 * maxC);      // chunk table of a call [C] | in pass order [C] | gather table [C] (ConvPasses)
    w.xnorm = F((int64_t)G * kSamplesPerChunk);
    w.convA = F(((int64_t)G * m->conv_S[0] + 16) * CD);
    w.convB = F(((int64_t)G * m->conv_S[1] + 16) * CD);
    const int64_t M = (int64_t)G * m->Ts;
    w.h0 = F(M * Hs); w.h1 = F(M * Hs); w.xln = F(M * Hs); w.qkv = F(M * 3 * Hs); w.att = F(M * Hs); w.ffn = F(M * c.w2v_ffn);
    w.silu_cond = F((int64_t)maxC * kNTok * kCond);
    for (const ClipBuf& cb : clip_buffers(m)) {      // maxB clips of each; the buffers that are not per clip keep their place between them
        const int64_t n = (cb.f == &Workspace::cache ? c.ar_depth : 1) * maxB * cb.n;      // the cache: [depth][maxB][...]
        if (cb.f) w.*cb.f = F(n); else w.*cb.u8 = m->ws_pool.take<uint8_t>(n);
        if (cb.f == &Workspace::logits) {
            w.splitk_floats = (int64_t)8 << 20; w.splitk = F(w.splitk_floats); w.splitk_b[0] = w.splitk;
            for (int i = 1; i < 4; ++i) w.splitk_b[i] = F(w.splitk_floats);
        }
        if (cb.u8 == &Workspace::hist_bits) {
            w.has_style = m->ws_pool.take<uint8_t>(maxB);
            w.status = m->ws_pool.take<int>(4);
            w.sess_slots = m->ws_pool.take<float*>(maxB);
        }
    }
    const int S = c.style_dim, SL = c.style_len;
    w.s_in = F((int64_t)maxB * SL * 128); w.s_h = F((int64_t)maxB * SL * S); w.s_qkv = F((int64_t)maxB * SL * 3 * S);
    w.s_att = F((int64_t)maxB * SL * S); w.s_ffn = F((int64_t)maxB * SL * c.style_ffn); w.s_tmp = F((int64_t)maxB * SL * S);
    if (!m->ws_pool.ok()) return fail(m, ARTALK_EHIP, "hipMalloc failed while reserving workspace");
    // the zero fills above run on the null stream; callers use non-blocking streams, which do not order against it
    HIPCHK(m, hipDeviceSynchronize());
    return ensure_stage(m, maxB, maxC);
}

}  // namespace artalk

namespace {
// The P8 producer sites this configuration can run, named as the audit reports them.  Built once from the config (artalk_create):
// unlike the audit's first-seen order it does not depend on which clips ran, so it is what a saved calibration is keyed by.
void build_site_table(artalk_model* m) {
    const artalk_config& c = m->cfg;
    SiteExps& ex = m->ex;
    auto add = [m](std::string name, int* e) {
        m->site_of.emplace(e, (int)m->sites.size());
        m->sites.push_back({std::move(name), e});
    };
    for (int i = 0; i + 1 < c.w2v_n_conv; ++i) add("w2v.conv" + std::to_string(i) + ".ln_gelu", &ex.conv[i]);
    add("w2v.feature_projection.ln", &ex.fp_ln);
    add("w2v.posconv.input(fp32 A)", &ex.posconv_in);
    for (int i = 0; i < c.w2v_layers; ++i) {
        const std::string p = "w2v.layer" + std::to_string(i);
        SiteExps::W2V& E = ex.w2v[i];
        add(p + ".ln1", &E.ln1); add(p + ".qkv", &E.qkv); add(p + ".attn_out", &E.attn); add(p + ".ln2", &E.ln2); add(p + ".ffn_hidden", &E.ffn);
    }
    add("ar.silu_cond", &ex.silu_cond);
    add("ar.history_tokens", &ex.hist_tok);
    for (int l = 0; l < c.ar_depth; ++l) {
        const std::string p = "ar.block" + std::to_string(l);
        SiteExps::AR& E = ex.ar[l];
        add(p + ".ln1_mod", &E.ln1); add(p + ".attn_out", &E.attn); add(p + ".ln2_mod", &E.ln2); add(p + ".ffn_hidden", &E.ffn);
    }
    for (int sd = 0; sd < 2; ++sd)
        for (int i = 0; i < c.vae_depth; ++i) {
            const std::string p = std::string(sd == 0 ? "vae.encoder.layer" : "vae.decoder.layer") + std::to_string(i);
            SiteExps::VAE& E = ex.vae[sd][i];
            add(p + ".ln", &E.ln); add(p + ".qkv", &E.qkv); add(p + ".attn_out", &E.attn); add(p + ".residual", &E.resid); add(p + ".mlp_hidden", &E.mlp);
        }
    add("vae.encoder.input(fp32 A)", &ex.vae_enc_in);
    add("vae.decoder.input(fp32 A)", &ex.vae_dec_in);
    add("vae.decoder.output_head(fp32 A)", &ex.vae_dec_head);
    add("style.input(fp32 A)", &ex.style_in);
    for (int i = 0; i < c.style_layers; ++i) {
        const std::string p = "style.layer" + std::to_string(i);
        SiteExps::ST& E = ex.style[i];
        add(p + ".in(fp32 A)", &E.h); add(p + ".attn_out(fp32 A)", &E.attn); add(p + ".norm1(fp32 A)", &E.h1); add(p + ".ffn_hidden(fp32 A)", &E.ffn);
    }
}

// A change of site scales closes every open session (the device is idle: the caller synchronised): their history was written under the
// old exponents' arithmetic, and a session never mixes exponents.  The ids are remembered so that a later step can say why it fails.
void end_sessions_by_scales(artalk_model* m) {
    for (const auto& kv : m->sess.open) { m->sess.ended_by_scales.insert(kv.first); m->sess.owner[kv.second.slot] = 0; }
    m->sess.open.clear();
}
// The one way new site exponents take effect (artalk_set_site_scales, artalk_calibrate): `next` is a complete SiteExps.  When anything
// differs, the device is synchronised, the captured graphs (the exponents are kernel arguments of their launches) and the initial-history
// cache are dropped, and an open streaming session ends - a session never mixes exponents.  Returns the number of sites changed.
int commit_scales(artalk_model* m, const SiteExps& next) {
    const int* a = reinterpret_cast<const int*>(&m->ex);
    const int* b = reinterpret_cast<const int*>(&next);
    int changed = 0;
    for (size_t i = 0; i < sizeof(SiteExps) / sizeof(int); ++i) changed += a[i] != b[i];
    if (changed) {
        (void)hipSetDevice(m->device); (void)hipDeviceSynchronize();
        drop_graphs(m);
        m->invalidate_init_hist();
        if (m->stream_B > 0) { m->stream_B = 0; m->stream_scales_ended = true; }
        end_sessions_by_scales(m);
        m->ex = next;
    }
    m->scales_changed = 0;
    for (size_t i = 0; i < sizeof(SiteExps) / sizeof(int); ++i) m->scales_changed += a[i] != kActExp;
    return changed;
}

}  // namespace

// =================================================================================================== C ABI
extern "C" {

const char* artalk_last_error(const artalk_model* m) { return m ? m->err.c_str() : g_create_error.c_str(); }

// Conv stack geometry of a chunk with `valid` real samples in front of zero padding (host only).  Row t of layer i starts at sample
// J_i t (J_i = product of the strides up to i): from t_const[i] = ceil(valid / J_i) on, a row sees the padding alone, and all such rows
// of a layer are equal.  Rows to compute: the last layer's rows 0 .. t_c = t_const[last] (one representative of the constant rows),
// counted back as Tp[i-1] = (Tp[i] - 1) stride + kernel; row strides Sp[last] = Tp[last] + 1, Sp[i-1] = 2 Sp[i] (the full chunk's
// rule, artalk_create).  Returns 1 and that geometry, or 0 and the whole chunk's when t_c leaves no constant row to skip.
int artalk_conv_tail_geometry(int64_t valid, int samples_per_chunk, int n_conv, const int* kernel, const int* stride, int* t_const, int* Tp,
                              int* Sp, int* samples_read) {
    if (!kernel || !stride || !t_const || !Tp || !Sp || !samples_read || n_conv < 2 || n_conv > 8 || samples_per_chunk <= 0 || valid < 1 ||
        valid > samples_per_chunk)
        return ARTALK_EINVAL;
    int T[8], J = 1, t = samples_per_chunk;
    for (int i = 0; i < n_conv; ++i) {
        if (kernel[i] <= 0 || stride[i] <= 0 || (i > 0 && stride[i] != 2) || t < kernel[i]) return ARTALK_EINVAL;
        t = (t - kernel[i]) / stride[i] + 1; T[i] = t;
        J *= stride[i];
        t_const[i] = (int)((valid + J - 1) / J);
    }
    const int L = n_conv - 1;
    const bool partial = t_const[L] < T[L] - 1;
    Tp[L] = partial ? t_const[L] + 1 : T[L];
    Sp[L] = Tp[L] + 1;
    for (int i = L; i > 0; --i) {
        Tp[i - 1] = partial ? (Tp[i] - 1) * stride[i] + kernel[i] : T[i - 1];
        Sp[i - 1] = 2 * Sp[i];
        if (Tp[i - 1] > Sp[i - 1] || Tp[i - 1] > T[i - 1]) return ARTALK_EINVAL;
    }
    *samples_read = partial ? (Tp[0] - 1) * stride[0] + kernel[0] : samples_per_chunk;
    return partial ? 1 : 0;
}
// The length class of such a chunk: classes are quarters of a chunk, and a chunk runs at its class's upper bound, which is returned
// (samples_per_chunk: the whole chunk).
int64_t artalk_conv_tail_class(int64_t valid, int samples_per_chunk) {
    if (samples_per_chunk <= 0 || valid < 1 || valid > samples_per_chunk) return ARTALK_EINVAL;
    if (samples_per_chunk % 4) return samples_per_chunk;
    const int64_t q = samples_per_chunk / 4;
    return (valid + q - 1) / q * q;
}

int artalk_create(int device_id, const artalk_config* cfg, artalk_model** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ARTALK_EINVAL; }
    const artalk_config& c = *cfg;
    static const int want_pn[5] = {1, 5, 25, 50, 100};
    bool ok = c.n_levels == 5 && c.code_dim == 32 && c.motion_dim == 106 && c.vae_hidden == 512 && c.w2v_hidden == kCond &&
              c.w2v_conv_dim == 512 && c.w2v_n_conv >= 2 && c.w2v_n_conv <= 8 && c.ar_heads * 64 == kE && c.vae_heads * 64 == c.vae_hidden &&
              c.w2v_heads * 64 == c.w2v_hidden && c.style_dim == 128 && c.style_heads * 32 == c.style_dim && c.style_len == 50 &&
              c.w2v_conv_kernel[0] == 10 && c.w2v_conv_stride[0] == 5 && c.w2v_ffn % 32 == 0 && c.style_ffn % 32 == 0 &&
              c.w2v_layers >= 1 && c.w2v_layers <= 64 && c.ar_depth >= 1 && c.ar_depth <= 32 && c.vae_depth >= 1 && c.vae_depth <= 16 && c.style_layers >= 1 && c.style_layers <= 8;      // (SiteExps tables)
    for (int i = 0; ok && i < 5; ++i) ok = c.patch_nums[i] == want_pn[i];
    if (!ok) { g_create_error = "unsupported configuration (kernels are specialised for assets/config.json + XLS-R-300M widths)"; return ARTALK_EINVAL; }
    if (hipSetDevice(device_id) != hipSuccess) { g_create_error = "hipSetDevice failed"; return ARTALK_EHIP; }
    artalk_model* m = new artalk_model();
    m->cfg = c; m->device = device_id;
    // conv stack geometry: T_l valid frames; row stride S_l per chunk with S_l = 2*S_{l+1} so that one GEMM covers all chunks
    int T = kSamplesPerChunk;
    for (int i = 0; i < c.w2v_n_conv; ++i) { T = (T - c.w2v_conv_kernel[i]) / c.w2v_conv_stride[i] + 1; m->conv_T[i] = T; }
    m->n_conv = c.w2v_n_conv; m->Tw = T; m->Ts = T + 1;
    int S = m->Ts;
    for (int i = c.w2v_n_conv - 1; i >= 0; --i) {
        m->conv_S[i] = S;
        if (i > 0) {
            if (c.w2v_conv_stride[i] != 2 || m->conv_T[i - 1] > 2 * S) { g_create_error = "conv stack geometry unsupported"; delete m; return ARTALK_EINVAL; }
            S *= 2;
        }
    }
    for (int q = 1; q <= 4 && kSamplesPerChunk % 4 == 0; ++q) {
        artalk_model::TailGeo& tg = m->tail_geo[q - 1];
        int tconst[8], read = 0;
        const int rc = artalk_conv_tail_geometry((int64_t)q * (kSamplesPerChunk / 4), kSamplesPerChunk, c.w2v_n_conv, c.w2v_conv_kernel, c.w2v_conv_stride,
                                                 tconst, tg.T, tg.S, &read);
        tg.partial = rc == 1;      // (a geometry the function rejects runs whole chunks)
        tg.tc = tconst[c.w2v_n_conv - 1];
    }
    for (int i = 0; i < 5; ++i) { m->pn[i] = c.patch_nums[i]; m->off[i + 1] = m->off[i] + c.patch_nums[i]; }
    if (init_ms_tables() != 0) { g_create_error = "uploading the interpolation tables to the device failed"; delete m; return ARTALK_EHIP; }
    attention_prepare();
    gemm_p8_prepare();
    build_site_table(m);
    const int rc = build_registry(m);
    if (rc != ARTALK_OK) { g_create_error = m->err; artalk_destroy(m); return rc; }
    *out = m;
    return ARTALK_OK;
}

void artalk_destroy(artalk_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    delete m;      // (every member that holds something of the runtime's gives it back: device_mem.h)
}

int artalk_set_tensor(artalk_model* m, const char* key, const void* host_ptr, int dtype, int ndim, const int64_t* shape) {
    if (!m || !key || !host_ptr || !shape) return ARTALK_EINVAL;
    if (m->finalized) return fail(m, ARTALK_ESTATE, "weights are final after artalk_finalize_weights (derived layouts and packed copies exist); create a new model");
    auto it = m->slots.find(key);
    if (it == m->slots.end()) return fail(m, ARTALK_EKEY, std::string("Unexpected key in state_dict: ") + key);
    Slot& s = it->second;
    bool same = (int)s.shape.size() == ndim && dtype == s.dtype;
    for (int i = 0; same && i < ndim; ++i) same = s.shape[i] == shape[i];
    if (!same) return fail(m, ARTALK_EINVAL, std::string("size mismatch for ") + key);
    (void)hipSetDevice(m->device);
    const int64_t n = s.numel();
    if (dtype == ARTALK_DTYPE_I64) {
        s.host_i64.assign((const int64_t*)host_ptr, (const int64_t*)host_ptr + n);
        s.set = true;
        return ARTALK_OK;
    }
    const float* src = (const float*)host_ptr;
    if (s.kind == SK_HOST || n <= 4096) s.host.assign(src, src + n);
    int rc = ARTALK_OK;
    switch (s.kind) {
        case SK_DIRECT: rc = upload(m, s.dst, src, n); break;
        case SK_PADK: {   // [out, in] -> [out, pad_to], zero padded
            const int64_t o = s.shape[0], in = s.shape[1];
            std::vector<float> t((size_t)o * s.pad_to, 0.f);
            for (int64_t r = 0; r < o; ++r) std::memcpy(&t[r * s.pad_to], src + r * in, in * sizeof(float));
            rc = upload(m, s.dst, t.data(), (int64_t)t.size());
            break;
        }
        case SK_CONV: {   // [out, cin, k] -> [out, k, cin]: the K index of the conv-as-GEMM is tap*cin + ci
            const int64_t o = s.shape[0], ci = s.shape[1], k = s.shape[2];
            std::vector<float> t((size_t)n);
            for (int64_t a = 0; a < o; ++a)
                for (int64_t b = 0; b < ci; ++b)
                    for (int64_t d = 0; d < k; ++d) t[(a * k + d) * ci + b] = src[(a * ci + b) * k + d];
            rc = upload(m, s.dst, t.data(), n);
            break;
        }
        default: break;
    }
    if (rc == ARTALK_OK) s.set = true;
    return rc;
}

int artalk_finalize_weights(artalk_model* m) {
    if (!m) return ARTALK_EINVAL;
    (void)hipSetDevice(m->device);
    std::string missing;
    int nmiss = 0;
    for (auto& kv : m->slots)
        if (!kv.second.set) { if (nmiss++ < 8) missing += (missing.empty() ? "" : ", ") + kv.first; }
    if (nmiss) return fail(m, ARTALK_EMISSING, "Missing key(s) in state_dict: " + missing + (nmiss > 8 ? ", ..." : ""));
    const artalk_config& c = m->cfg;
    // level / position tables (app/models.py:74-75)
    {
        const Slot& li = m->slots["lvl_idx"]; const Slot& le = m->slots["lvl_embed.weight"];
        const Slot& pe = m->slots["pos_embed"]; const Slot& ppe = m->slots["prev_pos_embed"];
        std::vector<float> a((size_t)kNTok * kE), b((size_t)kNTok * kE);
        int tok = 0;
        for (int p = 0; p < c.n_levels; ++p)
            for (int i = 0; i < c.patch_nums[p]; ++i, ++tok)
                if (li.host_i64[tok] != p) return fail(m, ARTALK_EINVAL, "lvl_idx does not match V_PATCH_NUMS");
        for (int t = 0; t < kNTok; ++t)
            for (int e = 0; e < kE; ++e) {
                const float lv = le.host[(size_t)li.host_i64[t] * kE + e];
                a[(size_t)t * kE + e] = lv + pe.host[(size_t)t * kE + e];
                b[(size_t)t * kE + e] = lv + ppe.host[(size_t)t * kE + e];
            }
        if (int rc = upload(m, m->lvl_pos, a.data(), (int64_t)a.size())) return rc;
        if (int rc = upload(m, m->prev_lvl_pos, b.data(), (int64_t)b.size())) return rc;
        // the masks are implied by patch_nums (block-causal by level; VAE: history rows see history only); verify
        const Slot& mk = m->slots["attn_bias_for_masking"];
        for (int q = 0; q < kNTok; ++q)
            for (int k = 0; k < 2 * kNTok; ++k) {
                const float v = mk.host[(size_t)q * 2 * kNTok + k];
                const bool vis = k < kNTok || li.host_i64[q] >= li.host_i64[k - kNTok];
                if (vis ? (v != 0.f) : !(std::isinf(v) && v < 0)) return fail(m, ARTALK_EINVAL, "attn_bias_for_masking is not the level-causal mask");
            }
        const Slot& vm = m->slots["basic_vae.attn_mask"];
        for (int q = 0; q < 200; ++q)
            for (int k = 0; k < 200; ++k) {
                const float v = vm.host[(size_t)q * 200 + k];
                const bool vis = !(q < 100 && k >= 100);
                if (vis ? (v != 0.f) : !(std::isinf(v) && v < 0)) return fail(m, ARTALK_EINVAL, "basic_vae.attn_mask is not the expected mask");
            }
    }
    // learned attention scale: exp(min(scale_mul, log 100))  (app/transformer.py:72)
    for (int i = 0; i < c.ar_depth; ++i) {
        const Slot& sm = m->slots["attn_blocks." + std::to_string(i) + ".attn.scale_mul_1H11"];
        std::vector<float> q(c.ar_heads);
        for (int h = 0; h < c.ar_heads; ++h) q[h] = std::exp(std::min(sm.host[h], (float)std::log(100.0)));
        if (int rc = upload(m, m->ar[i].qscale, q.data(), c.ar_heads)) return rc;
    }
    // style PE row pe[:, seq_len]  (style_encoder.py:59)
    {
        const Slot& pe = m->slots["style_encoder.PE.pe"];
        if (int rc = upload(m, m->st_pe, pe.host.data() + (size_t)c.style_len * c.style_dim, c.style_dim)) return rc;
    }
    // pos-conv weight-norm fold (dim=2): w[o,i,k] = g[k] * v[o,i,k] / ||v[:,:,k]||, re-laid out [o][k][i]
    {
        const std::string pc = "audio_encoder.encoder.pos_conv_embed.conv.parametrizations.weight.";
        const Slot& g = m->slots[pc + "original0"]; const Slot& v = m->slots[pc + "original1"];
        const int64_t O = v.shape[0], I = v.shape[1], K = v.shape[2];
        std::vector<double> nrm(K, 0.0);
        for (int64_t o = 0; o < O; ++o)
            for (int64_t i = 0; i < I; ++i)
                for (int64_t k = 0; k < K; ++k) { const double x = v.host[(o * I + i) * K + k]; nrm[k] += x * x; }
        std::vector<float> t((size_t)O * I * K);
        for (int64_t k = 0; k < K; ++k) {
            const float nk = (float)std::sqrt(nrm[k]);
            for (int64_t o = 0; o < O; ++o)
                for (int64_t i = 0; i < I; ++i) t[(o * K + k) * I + i] = v.host[(o * I + i) * K + k] * (g.host[k] / nk);
        }
        if (int rc = upload(m, m->pos_w, t.data(), (int64_t)t.size())) return rc;
    }
    for (auto& kv : m->slots) { std::vector<float>().swap(kv.second.host); }
    // packed f16x3 copies of every weight matrix (same size and indexing as the fp32 original)
    for (auto& r : m->wranges) {
        if (r.n < 1024 || r.packed) continue;
        r.packed = dalloc<unsigned int>(m, r.n);
        if (!r.packed) return fail(m, ARTALK_EHIP, "hipMalloc failed for packed weights");
        launch_pack_split(r.base, r.packed, r.n, true, nullptr);
    }
    HIPCHK(m, hipDeviceSynchronize());
    if (m->precision == 2) { if (int rc = ensure_bf16_copy(m)) return rc; }
    m->finalized = true;
    return ARTALK_OK;
}

int artalk_reserve(artalk_model* m, int max_batch, int max_total_chunks) {
    if (!m || max_batch <= 0 || max_total_chunks < max_batch) return ARTALK_EINVAL;
    (void)hipSetDevice(m->device);
    return reserve(m, max_batch, max_total_chunks);
}
int64_t artalk_workspace_bytes(const artalk_model* m) { return m ? m->ws.bytes : 0; }
int64_t artalk_weight_bytes(const artalk_model* m) { return m ? m->weight_bytes : 0; }

int artalk_set_profiling(artalk_model* m, int level) { if (!m || level < 0 || level > 3) return ARTALK_EINVAL; m->profiling = level; return ARTALK_OK; }
int artalk_set_precision(artalk_model* m, int mode) {
    if (!m || mode < 0 || mode > 2) return ARTALK_EINVAL;
    if (mode == 2 && m->finalized) {      // (before finalize: artalk_finalize_weights builds the copy)
        (void)hipSetDevice(m->device);
        if (int rc = ensure_bf16_copy(m)) return rc;
    }
    m->precision = mode;   // captured graphs are keyed by mode: switching costs nothing and keeps every set
    return ARTALK_OK;
}
int artalk_set_tail_skip(artalk_model* m, int on) { if (!m) return ARTALK_EINVAL; m->tail_skip = on != 0; return ARTALK_OK; }
int artalk_set_graphs(artalk_model* m, int enable) {
    if (!m) return ARTALK_EINVAL;
    m->use_graphs = (enable & 0xff) != 0;
    const int br = (enable >> 8) & 0xff;          // tuning: enable | (branches << 8) forces 1 / 2 / 4 concurrent clip groups
    if (br >= 0 && br <= 4) m->branches = br; else return ARTALK_EINVAL;
    if ((enable >> 16) & 0xffff) {                // tuning: split-K thresholds, (tiles/16) << 16 | (target/16) << 24
        m->splitk_tiles = ((enable >> 16) & 0xff) * 16; m->splitk_target = ((enable >> 24) & 0xff) * 16;
    }
    (void)hipSetDevice(m->device); (void)hipDeviceSynchronize();
    drop_graphs(m);
    m->invalidate_init_hist();      // "the same run_reencode as every later history": the split-K tuning changed
    return ARTALK_OK;
}
// number of captured body graphs the model holds (bounded: run_body) / captures since the model was created
int artalk_graph_count(const artalk_model* m, long long* captures) {
    if (!m) return ARTALK_EINVAL;
    if (captures) *captures = m->graph_captures;
    return (int)m->graphs.size();
}

// Headroom audit of the f16x3 operand format (tools/p8_headroom.py): while enabled, every artalk_infer runs without graphs and
// records, per producer site of a P8 operand, max |x| * 16 (the value that must stay below fp16's 65504).  artalk_get_audit
// synchronises the device and returns the number of sites; names are written NUL-separated into names_buf.
int artalk_set_audit(artalk_model* m, int enable) {
    if (!m) return ARTALK_EINVAL;
    (void)hipSetDevice(m->device);
    if (enable && !m->audit_vals) {
        m->audit_vals = dalloc<unsigned int>(m, kAuditSlots);
        if (!m->audit_vals) return fail(m, ARTALK_EHIP, "hipMalloc failed for the audit block");
    }
    if (enable) {
        HIPCHK(m, hipDeviceSynchronize());
        HIPCHK(m, hipMemset(m->audit_vals, 0, kAuditSlots * sizeof(unsigned int)));
        m->audit_names.clear(); m->audit_index.clear(); m->audit_exp.clear();
    }
    m->audit = enable != 0;
    return ARTALK_OK;
}
// Per-site operand scales of the f16x3 format from the audit's maxima (SiteExps): after artalk_infer calls with the audit on - in EXACT-F32
// mode, where no site can overflow on the way to a later one - every site whose max |x| * 2^e * headroom exceeds fp16's 65504 gets the
// largest exponent e (<= the default 4, >= -8) that fits.  Exponents only go down (a later calibration on tamer inputs never undoes an
// earlier one; artalk_reset_scales does).  All or nothing: the new exponents are computed into a copy and committed (commit_scales:
// graphs, initial-history cache and streaming session dropped when anything changed) only after every site has passed.
// Returns the number of sites changed (>= 0), or a negative error with the model untouched: ARTALK_ESTATE without audit data,
// ARTALK_EINVAL for a non-finite maximum (run the pass in f32 mode) or one that no exponent >= -8 can hold.
int artalk_calibrate(artalk_model* m, float headroom) {
    if (!m || !(headroom >= 1.0f)) return ARTALK_EINVAL;
    if (!m->audit_vals || m->audit_names.empty()) { m->err = "artalk_calibrate: no audit data (artalk_set_audit(1), then artalk_infer in f32 mode)"; return ARTALK_ESTATE; }
    (void)hipSetDevice(m->device);
    if (hipDeviceSynchronize() != hipSuccess) return ARTALK_EHIP;
    const int n = (int)m->audit_names.size();
    std::vector<unsigned int> bits((size_t)n);
    if (hipMemcpy(bits.data(), m->audit_vals, n * sizeof(unsigned int), hipMemcpyDeviceToHost) != hipSuccess) return ARTALK_EHIP;
    SiteExps next = m->ex;
    int* const base = reinterpret_cast<int*>(&m->ex);
    int* const nbase = reinterpret_cast<int*>(&next);
    for (int i = 0; i < n; ++i) {
        if (!m->audit_exp[i]) continue;
        int* ex = nbase + (m->audit_exp[i] - base);      // the same member of the copy
        float mx;
        std::memcpy(&mx, &bits[i], sizeof(float));
        if (!std::isfinite(mx)) { m->err = "artalk_calibrate: site " + m->audit_names[i] + " is not finite (calibrate in f32 mode)"; return ARTALK_EINVAL; }
        if (mx <= 0.f) continue;
        int e = *ex;
        while (e > -8 && (double)mx * std::ldexp(1.0, e) * headroom > 65504.0) --e;
        if ((double)mx * std::ldexp(1.0, e) > 65504.0) { m->err = "artalk_calibrate: site " + m->audit_names[i] + " exceeds every supported scale"; return ARTALK_EINVAL; }
        *ex = e;
    }
    return commit_scales(m, next);
}
int artalk_reset_scales(artalk_model* m) {
    if (!m) return ARTALK_EINVAL;
    (void)hipSetDevice(m->device); (void)hipDeviceSynchronize();
    if (m->scales_changed) end_sessions_by_scales(m);      // (the lockstep session keeps its old rule)
    m->ex = SiteExps();
    m->scales_changed = 0;
    drop_graphs(m);
    m->invalidate_init_hist();
    return ARTALK_OK;
}
// exps[i] = exponent of audit site i (the order of artalk_get_audit); returns the number written
int artalk_get_scales(artalk_model* m, int* exps, int max_n) {
    if (!m || !exps || max_n <= 0) return ARTALK_EINVAL;
    const int n = std::min<int>((int)m->audit_names.size(), max_n);
    for (int i = 0; i < n; ++i) exps[i] = m->audit_exp[i] ? *m->audit_exp[i] : kActExp;
    return n;
}
// The static site table (build_site_table): names NUL-separated in table order; names_buf = NULL returns the count only.
int artalk_scale_sites(const artalk_model* m, char* names_buf, int buf_len) {
    if (!m) return ARTALK_EINVAL;
    const int n = (int)m->sites.size();
    if (!names_buf) return n;
    int need = 0;
    for (const auto& st : m->sites) need += (int)st.name.size() + 1;
    if (buf_len < need) { const_cast<artalk_model*>(m)->err = "artalk_scale_sites: names need " + std::to_string(need) + " bytes"; return ARTALK_EINVAL; }
    int pos = 0;
    for (const auto& st : m->sites) { std::memcpy(names_buf + pos, st.name.c_str(), st.name.size() + 1); pos += (int)st.name.size() + 1; }
    return n;
}
int artalk_get_site_scales(artalk_model* m, int* exps, int n) {
    if (!m || !exps) return ARTALK_EINVAL;
    if (n != (int)m->sites.size()) return fail(m, ARTALK_EINVAL, "artalk_get_site_scales: n must equal the site count " + std::to_string(m->sites.size()));
    for (int i = 0; i < n; ++i) exps[i] = *m->sites[i].ex;
    return ARTALK_OK;
}
// Validates every value before it changes anything, then commits through commit_scales (as artalk_calibrate does).
int artalk_set_site_scales(artalk_model* m, const int* exps, int n) {
    if (!m || !exps) return ARTALK_EINVAL;
    if (n != (int)m->sites.size()) return fail(m, ARTALK_EINVAL, "artalk_set_site_scales: n must equal the site count " + std::to_string(m->sites.size()));
    for (int i = 0; i < n; ++i)
        if (exps[i] < -8 || exps[i] > kActExp)
            return fail(m, ARTALK_EINVAL, "artalk_set_site_scales: exponent " + std::to_string(exps[i]) + " of site " + m->sites[i].name + " is outside [-8, 4]");
    SiteExps next = m->ex;
    int* const base = reinterpret_cast<int*>(&m->ex);
    int* const nbase = reinterpret_cast<int*>(&next);
    for (int i = 0; i < n; ++i) nbase[m->sites[i].ex - base] = exps[i];
    return commit_scales(m, next);
}
int artalk_get_audit(artalk_model* m, char* names_buf, int buf_len, float* values, int max_n) {
    if (!m || !names_buf || !values || buf_len <= 0 || max_n <= 0) return ARTALK_EINVAL;
    if (!m->audit_vals) return 0;
    (void)hipSetDevice(m->device);
    if (hipDeviceSynchronize() != hipSuccess) return ARTALK_EHIP;
    const int n = std::min<int>((int)m->audit_names.size(), max_n);
    std::vector<unsigned int> bits((size_t)std::max(n, 1));
    if (n && hipMemcpy(bits.data(), m->audit_vals, n * sizeof(unsigned int), hipMemcpyDeviceToHost) != hipSuccess) return ARTALK_EHIP;
    int pos = 0, written = 0;
    for (int i = 0; i < n; ++i) {
        const std::string& nm = m->audit_names[i];
        if (pos + (int)nm.size() + 1 > buf_len) break;
        std::memcpy(names_buf + pos, nm.c_str(), nm.size() + 1);
        pos += (int)nm.size() + 1;
        std::memcpy(&values[i], &bits[i], sizeof(float));
        ++written;
    }
    return written;
}

// Intermediate taps for the parity tests (SURVEY.md 8c "reference-captured intermediates"): while a tap buffer is set, artalk_infer runs
// the AR/VAE body eagerly as ONE clip group (no graphs) and copies, per chunk index j and clip position b (sorted order), into slot
// (j * max_batch + b) of `tap_dev`: the layout of artalk_tap_layout().  tap_dev = NULL switches it off.
int artalk_set_tap(artalk_model* m, float* tap_dev, int max_batch, int max_chunks) {
    if (!m || max_batch < 0 || max_chunks < 0) return ARTALK_EINVAL;
    (void)hipSetDevice(m->device); (void)hipDeviceSynchronize();
    m->tap = tap_dev; m->tap_B = tap_dev ? max_batch : 0; m->tap_maxch = tap_dev ? max_chunks : 0; m->tap_chunk = 0;
    return ARTALK_OK;
}
// out[0..6] = float offsets of the fields blk0_in, blk0_out, blkL_out, prev_in, logits, dec_out inside a slot, out[6] = floats per slot
int artalk_tap_layout(int64_t* out, int n) {
    if (!out || n < 7) return ARTALK_EINVAL;
    const int64_t v[7] = {TAP_BLK0_IN, TAP_BLK0_OUT, TAP_BLKL_OUT, TAP_PREV_IN, TAP_LOGITS, TAP_DEC_OUT, TAP_SLOT};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
    return ARTALK_OK;
}

// Restrict the model to a set of compute units (bit i of mask = CU i / 8 of XCD i % 8 on MI355X): the streams the library creates
// itself (the second clip group of the AR/VAE body) get the mask, the persistent GEMM kernels size their grids to it.  The caller
// passes a stream with the same mask to artalk_infer (artalk_op_create_masked_stream).  n_words = 0 clears the mask.
int artalk_set_cu_mask(artalk_model* m, const uint32_t* mask, int n_words) {
    if (!m || n_words < 0 || (n_words > 0 && !mask)) return ARTALK_EINVAL;
    (void)hipSetDevice(m->device); (void)hipDeviceSynchronize();
    m->cu_mask.assign(mask, mask + n_words);
    int n = 0;
    for (uint32_t w : m->cu_mask) n += __builtin_popcount(w);
    if (n_words > 0 && n < 8) { m->cu_mask.clear(); m->n_cus = 0; return fail(m, ARTALK_EINVAL, "a CU partition needs at least 8 compute units"); }
    int dev_cus = 0;      // mask bits beyond the device's CUs select nothing: the grids must not count them
    if (hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, m->device) == hipSuccess && dev_cus > 0) n = std::min(n, dev_cus);
    m->n_cus = n;
    for (int i = 0; i < 3; ++i) {      // side streams are re-created (masked) on demand
        m->side_stream[i].reset();
        m->join_ev[i].reset();
    }
    drop_graphs(m);      // the GEMM grids were captured for the old CU count
    m->invalidate_init_hist();
    return ARTALK_OK;
}


// Numerical health of the work enqueued since the last artalk_infer / artalk_stream_begin started.  Every call ends with an
// asynchronous copy of the device status word into pinned host memory; artalk_get_status waits for that copy (the only
// synchronisation on this boundary, and only if the caller asks), artalk_poll_status never blocks (ARTALK_EBUSY while the call is
// still running).  Bits: 0 = a logit was NaN/Inf (the pairwise argmax would have turned it into a 0 bit), 1 = a re-encoder
// output was NaN/Inf, 2 = a FLAME code was NaN/Inf, 3 = an activation left the range of the P8 split format at its producer.
// Non-zero in f16x3 mode means an activation left fp16's range: redo the call in f32 mode.
int artalk_get_status(artalk_model* m, int* flags, void* stream) {
    (void)stream;      // kept for ABI compatibility: the wait is on the library's own event, not on a stream
    if (!m || !flags) return ARTALK_EINVAL;
    if (!m->status_pending) { *flags = 0; return ARTALK_OK; }
    (void)hipSetDevice(m->device);
    const int slot = (int)((m->ticket - 1) % artalk_model::kStatusSlots);
    HIPCHK(m, hipEventSynchronize(m->status_ev[slot].get()));
    *flags = m->h_status.get()[slot];
    return ARTALK_OK;
}
long long artalk_last_ticket(artalk_model* m) { return m ? m->ticket : -1; }
int artalk_get_status_of(artalk_model* m, long long ticket, int* flags) {
    if (!m || !flags || ticket <= 0 || ticket > m->ticket) return ARTALK_EINVAL;
    if (ticket + artalk_model::kStatusSlots <= m->ticket) { m->err = "artalk_get_status_of: that call's status slot has been reused"; return ARTALK_EINVAL; }
    if (!m->status_pending) { *flags = 0; return ARTALK_OK; }      // the workspace was re-created since: nothing of that call is left
    (void)hipSetDevice(m->device);
    const int slot = (int)((ticket - 1) % artalk_model::kStatusSlots);
    HIPCHK(m, hipEventSynchronize(m->status_ev[slot].get()));
    *flags = m->h_status.get()[slot];
    return ARTALK_OK;
}
int artalk_poll_status(artalk_model* m, int* flags) {
    if (!m || !flags) return ARTALK_EINVAL;
    if (!m->status_pending) { *flags = 0; return ARTALK_OK; }
    (void)hipSetDevice(m->device);
    const int slot = (int)((m->ticket - 1) % artalk_model::kStatusSlots);
    const hipError_t e = hipEventQuery(m->status_ev[slot].get());
    if (e == hipErrorNotReady) return ARTALK_EBUSY;
    if (e != hipSuccess) { m->err = std::string("hipEventQuery: ") + hipGetErrorString(e); return ARTALK_EHIP; }
    *flags = m->h_status.get()[slot];
    return ARTALK_OK;
}

int artalk_get_profile(artalk_model* m, double* out, int n) {
    if (!m || !out || n < 10) return ARTALK_EINVAL;
    if (!m->profiling || m->marks.size() < 2) return fail(m, ARTALK_ESTATE, "profiling was not enabled for the last artalk_infer");
    (void)hipSetDevice(m->device);
    HIPCHK(m, hipStreamSynchronize(m->prof_stream));
    auto ms = [&](size_t a, size_t b) { float t = 0.f; (void)hipEventElapsedTime(&t, m->ev_pool[a].get(), m->ev_pool[b].get()); return (double)t; };
    double r[10] = {0};
    for (size_t i = 1; i < m->marks.size(); ++i) {
        const int b = m->marks[i].first;
        if (b >= 0 && b < 6) r[b] += ms(m->marks[i - 1].second, m->marks[i].second);
    }
    r[6] = ms(m->marks.front().second, m->marks.back().second);
    for (auto& d : m->dom_events) { r[7] += 1.0; r[8] += ms(d.first, d.first + 1); r[9] += d.second; }
    for (int i = 0; i < 10; ++i) out[i] = r[i];
    return ARTALK_OK;
}

// Kernel-time budget of the last artalk_infer run at profiling level 3: out[b] = sum of the durations (ms) of the kernels launched in
// bucket b - 0 style, 1 conv stack, 2 encoder, 3 AdaLN tables, 4 history K/V + glue, 5..9 scale steps 0..4, 10 VAE decode, 11 re-encode,
// 12 other - and out[13] = number of kernels timed.  Durations are the dispatches' own begin / end timestamps (hipExtLaunchKernelGGL
// events), i.e. without launch gaps: stage event time minus this sum is the time the stage's stream sat idle.  n >= 14.
int artalk_get_kernel_sums(artalk_model* m, double* out, int n) {
    if (!m || !out || n < KB_N + 1) return ARTALK_EINVAL;
    if (m->ktimer.recs.empty()) return fail(m, ARTALK_ESTATE, "no kernel was timed (artalk_set_profiling(3) before artalk_infer)");
    (void)hipSetDevice(m->device);
    HIPCHK(m, hipDeviceSynchronize());
    for (int i = 0; i <= KB_N; ++i) out[i] = 0.0;
    for (const auto& r : m->ktimer.recs) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, m->ktimer.pool[r.second].get(), m->ktimer.pool[r.second + 1].get()) != hipSuccess) continue;
        const int b = r.first >= 0 && r.first < KB_N ? r.first : KB_OTHER;
        out[b] += t;
        out[KB_N] += 1.0;
    }
    return ARTALK_OK;
}

}  // extern "C"
