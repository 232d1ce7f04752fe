// Model object behind the C ABI (include/artalk_hip.h): weight table in the reference's key names, derived
// layouts, workspace, and the launch sequence of the audio->motion path.
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
#include "kernels.h"
#include "../../include/artalk_hip.h"

#include <hip/hip_ext.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace artalk;

namespace artalk {
thread_local KernelTimer* g_ktimer = nullptr;
bool ktimer_events(hipEvent_t* e0, hipEvent_t* e1) {
    KernelTimer* t = g_ktimer;
    if (!t) return false;
    while (t->pool.size() < t->used + 2) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return false;
        t->pool.push_back(e);
    }
    *e0 = t->pool[t->used]; *e1 = t->pool[t->used + 1];
    t->recs.emplace_back(t->bucket, t->used);
    t->used += 2;
    return true;
}
}  // namespace artalk

namespace {
// buckets of the kernel timer (artalk_get_kernel_sums): stages of the path, the scale steps of the body
enum { KB_STYLE = 0, KB_CONV = 1, KB_ENC = 2, KB_ADA = 3, KB_AR_MISC = 4, KB_LEVEL0 = 5, KB_VAE_DEC = 10, KB_REENC = 11, KB_OTHER = 12, KB_N = 13 };

thread_local std::string g_create_error;

constexpr int kSamplesPerChunk = 64000;
constexpr int kE = 768;      // embed dim (app/models.py:19)
constexpr int kCond = 1024;  // audio feature dim (app/models.py:27)
constexpr int kNTok = 181;
constexpr int kMaxLv = 5;

// roctx range around one kernel group of the path (SURVEY.md section 5, K-groups): visible with `rocprofv3 --marker-trace`.
// Host-side ranges: they bracket the ENQUEUE of the group (the path is asynchronous); inside a hipGraph capture nothing is
// enqueued at replay time, so the captured body shows up as one "body.graph" range per clip group and its inner ranges
// appear only when graphs are off (artalk_set_graphs(0) / profiling level 2).
struct Range {
    explicit Range(const char* name) { roctxRangePushA(name); }
    ~Range() { roctxRangePop(); }
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
};

enum SlotKind { SK_DIRECT, SK_PADK, SK_CONV, SK_HOST, SK_IGNORE };

struct Slot {
    std::vector<int64_t> shape;
    int dtype = ARTALK_DTYPE_F32;
    SlotKind kind = SK_DIRECT;
    float* dst = nullptr;      // device destination (DIRECT/PADK/CONV)
    int64_t pad_to = 0;        // PADK: padded inner size
    bool set = false;
    std::vector<float> host;   // SK_HOST (and every small tensor) keeps a host copy
    std::vector<int64_t> host_i64;
    int64_t numel() const { int64_t n = 1; for (auto d : shape) n *= d; return n; }
};

struct W2VLayer { float *qkv_w, *qkv_b, *out_w, *out_b, *ln1w, *ln1b, *ln2w, *ln2b, *ff1_w, *ff1_b, *ff2_w, *ff2_b; };
struct ARLayer { float *qkv_w, *qkv_b, *proj_w, *proj_b, *ffn1_w, *ffn1_b, *ffn2_w, *ffn2_b, *qscale; };
struct VAELayer { float *lnw, *lnb, *qkv_w, *out_w, *out_b, *m1_w, *m1_b, *m2_w, *m2_b; };
struct VAESide { float *in_w, *in_b, *out_w, *out_b; std::vector<VAELayer> layers; };
struct StyleLayer { float *in_w, *in_b, *out_w, *out_b, *l1_w, *l1_b, *l2_w, *l2_b, *n1w, *n1b, *n2w, *n2b; };

// Site exponents of the P8 operand format (common.h): every producer of a P8 operand writes it with scale 2^e and every consumer removes
// the same scale, e = kActExp (16) by default.  artalk_calibrate lowers the exponent of a site whose activations need the range
// (a real XLS-R-class checkpoint: FFN hidden channels of 1e4 and more) - per SITE, so that one outlier channel in a few layers
// does not cost the whole model its fast mode.  Named by the site table (build_site_table).
struct SiteExps {
    int conv[8]; int fp_ln, posconv_in;
    struct W2V { int ln1, qkv, attn, ln2, ffn; } w2v[64];
    int silu_cond, hist_tok;
    struct AR { int ln1, attn, ln2, ffn; } ar[32];
    struct VAE { int ln, qkv, attn, resid, mlp; } vae[2][16];
    int vae_enc_in, vae_dec_in, vae_dec_head;
    int style_in; struct ST { int h, attn, h1, ffn; } style[8];      // style encoder: fp32 A rows split while staging
    SiteExps() { int* p = reinterpret_cast<int*>(this); for (size_t i = 0; i < sizeof(SiteExps) / sizeof(int); ++i) p[i] = kActExp; }
};

struct Workspace {
    int maxB = 0, maxC = 0, G = 0;   // G = wav2vec2 chunk-group size
    // wav2vec2
    long* src_off = nullptr; float *xnorm = nullptr, *convA = nullptr, *convB = nullptr;
    float *h0 = nullptr, *h1 = nullptr, *xln = nullptr, *qkv = nullptr, *att = nullptr, *ffn = nullptr;
    float* silu_cond = nullptr;     // [maxC*181, 1024]
    // AR
    float *ada = nullptr, *style_cond = nullptr, *prev_in = nullptr, *prev_in_p8 = nullptr, *cache = nullptr;
    float *x = nullptr, *xmod = nullptr, *attn_out = nullptr, *ffn_h = nullptr, *logits = nullptr;
    float *fhat = nullptr, *nextfeat = nullptr;
    float* splitk = nullptr; int64_t splitk_floats = 0;   // partial sums of split-K GEMMs
    float* splitk_b[4] = {nullptr, nullptr, nullptr, nullptr};   // one scratch per concurrent branch of the AR body (splitk_b[0] == splitk)
    uint8_t *bits = nullptr, *hist_bits = nullptr, *has_style = nullptr;
    int* status = nullptr;           // device word: bit 0 non-finite logit, bit 1 non-finite re-encoder output (see artalk_get_status)
    float** sess_slots = nullptr;    // [maxB] pool slots of the sessions of the current artalk_session_open / _step, row order (launch_session_gather)
    // VAE
    float *prev_fdec = nullptr, *msfeat = nullptr, *dec_x = nullptr, *vh = nullptr, *vln = nullptr, *vqkv = nullptr;
    float *vatt = nullptr, *vmlp = nullptr, *dec_out = nullptr, *enc_in = nullptr, *enc_out = nullptr, *motion_chunk = nullptr;
    // style
    float *s_in = nullptr, *s_h = nullptr, *s_qkv = nullptr, *s_att = nullptr, *s_ffn = nullptr, *s_tmp = nullptr;
    int64_t bytes = 0;
};

}  // namespace

// where the smoother's carry starts in a pool slot, in floats: behind [style kE | prev_in kNTok x kE | prev_fdec 100 x code_dim]
constexpr int64_t slot_carry_off(int code_dim) { return kE + (int64_t)kNTok * kE + 100LL * code_dim; }
constexpr int kOpCodeDim = 32, kOpMotionDim = 106;      // the only widths artalk_create accepts: what the model-free entry points assume

struct artalk_model {
    artalk_config cfg{};
    int device = 0;
    std::string err;
    bool finalized = false;
    std::map<std::string, Slot> slots;
    std::vector<void*> allocs;      // weights (model lifetime)
    std::vector<void*> ws_allocs;   // workspace (re-allocated when a larger batch arrives)
    int64_t weight_bytes = 0;
    struct PackRange { const float* base; int64_t n; unsigned int* packed; uint16_t* bf16; };
    std::vector<PackRange> wranges;   // every weight allocation, its packed f16x3 copy (built at finalize) and its bf16 copy (built on
                                      // the first switch to precision mode 2: ensure_bf16_copy)
    int precision = 0;                // 0: fp32 MFMA everywhere, 1: f16x3 split GEMMs, 2: bf16 GEMMs (heads stay fp32 in 1 and 2)
    bool have_bf16 = false;           // the bf16 weight copy exists
    int splitk_tiles = 192, splitk_target = 384;   // split-K when the grid has fewer tiles than splitk_tiles; aim at splitk_target workgroups
    // headroom audit (artalk_set_audit): max |x| * 16 at every producer of a P8 operand, by site name
    bool audit = false;
    unsigned int* audit_vals = nullptr;            // device, kAuditSlots floats (as bits)
    std::vector<std::string> audit_names;
    std::map<std::string, int> audit_index;
    std::vector<int*> audit_exp;                   // the site's exponent (SiteExps member) per audit slot: what artalk_calibrate adjusts
    SiteExps ex;                                   // site exponents of the P8 format (all kActExp until a calibration lowers some)
    int scales_changed = 0;                        // sites whose exponent differs from kActExp
    // every P8 producer site the configuration can run, built from the config alone at artalk_create (build_site_table): the one
    // place the site names are defined (the audit looks its names up here by exponent pointer) and the order of artalk_*_site_scales
    struct Site { std::string name; int* ex; };
    std::vector<Site> sites;
    std::map<const int*, int> site_of;             // exponent pointer -> index into sites
    bool stream_scales_ended = false;              // a scale change ended the streaming session (artalk_stream_chunk says so)
    // The INITIAL history of a clip (app/models.py:86-89: encode + quantise an all-zero motion) is a function of the weights only - the
    // same bits, decoder features and history tokens for every clip of every call.  It is computed once per precision mode (for ONE
    // clip, through the same run_reencode as every later history) and broadcast to the batch afterwards; only the style token in
    // front of the history tokens differs per clip (launch_vq_embed).  Indexed by precision mode: [0] exact f32, [1] f16x3, [2] bf16.
    struct InitHistory { uint8_t* bits = nullptr; float *fdec = nullptr, *msfeat = nullptr; bool valid = false; } init_hist[3];
    void invalidate_init_hist() { for (auto& ih : init_hist) ih.valid = false; }
    // intermediate taps (artalk_set_tap): parity tests compare these device buffers with intermediates captured from the reference
    float* tap = nullptr; int tap_B = 0, tap_maxch = 0, tap_chunk = 0;
    std::vector<uint32_t> cu_mask;    // artalk_set_cu_mask: the library's own streams are restricted to these compute units
    int n_cus = 0;                    // their number (0 = the whole device): grid of the persistent one-workgroup-per-CU kernels
    int stream_B = 0;                 // streams opened by artalk_stream_begin (history lives in the workspace)
    // Independent streaming sessions (artalk_session_*).  What a stream carries from chunk to chunk - style condition [768], history
    // tokens prev_in [181][768], decoder features prev_fdec [100][32], plain fp32 in every precision mode - lives in a pool slot, OUTSIDE
    // the workspace: device memory in blocks of kSessBlock slots that are never moved or freed before artalk_destroy, so growing the
    // pool touches no open session.  A step gathers the listed sessions into workspace rows 0..n-1, runs the chunk step of lockstep
    // streaming there and scatters the new history back.  INVARIANT: between library calls the workspace holds nothing a session
    // needs - it is scratch, and the batch call, lockstep streaming, artalk_style_encode and workspace growth may use it freely.
    static constexpr int kSessBlock = 32;
    struct Sessions {
        std::vector<float*> blocks;                // device blocks of kSessBlock slots
        std::vector<int64_t> owner;                // per slot: the id of the session that holds it, 0 = free
        // an open session: its slot, and where its streaming smoother stands (artalk_session_smooth): raw frames consumed, and whether
        // a `last` call has emitted the tail.  Born zero with the id, dropped with it: a slot reused under a new id starts clean.
        struct Open { int slot = 0; int64_t seen = 0; bool smooth_done = false; };
        std::map<int64_t, Open> open;              // id -> state
        std::set<int64_t> ended_by_scales;         // ids a change of site scales closed (a step on one says so; artalk_session_close forgets it)
        int64_t next_id = 1;                       // ids are never reused during the model's life
        void* smooth_tab = nullptr; int64_t smooth_cap = 0;      // device table of one artalk_session_smooth call: [cap slot pointers | cap int4]
    } sess;
    // slot: [style | prev_in | prev_fdec | smoother carry]; the carry (the last 9 raw frames, padded to 16 bytes) is read and written in
    // place by savgol_stream_kernel and never visits the workspace: SessionRows and the gather / scatter cover the first three fields only
    int64_t sess_carry_off() const { return slot_carry_off(cfg.code_dim); }
    int64_t sess_slot_floats() const { return sess_carry_off() + (kSavgolCarry * (int64_t)cfg.motion_dim + 3) / 4 * 4; }
    float* sess_slot(int i) const { return sess.blocks[i / kSessBlock] + (int64_t)(i % kSessBlock) * sess_slot_floats(); }
    Workspace* view = nullptr;        // workspace view (clip sub-range) the body launchers currently work on; null = m->ws
    bool sticky_error = false;        // set by internal consistency checks inside the launch sequence; reported by artalk_infer
    // derived sizes
    int n_conv = 0; int conv_T[8]{}; int conv_S[8]{};   // valid frames / padded row stride per conv layer output
    int Tw = 0, Ts = 0;                                 // 199, 200
    // Conv stack over the frames that hear real audio (run_wav2vec): a chunk whose tail is zero padding runs the stack up to ONE frame
    // of the padded region.  Chunks fall into length classes by quarter of a chunk and run at their class's upper bound: tail_geo[q - 1]
    // for a chunk with valid samples in ((q - 1) / 4, q / 4] of a chunk (artalk_conv_tail_geometry of the bound; partial = false: the
    // whole chunk, conv_T / conv_S).
    struct TailGeo { bool partial = false; int tc = 0; int T[8]{}, S[8]{}; } tail_geo[4];
    bool tail_skip = true;                              // artalk_set_tail_skip
    int ada_n = 0;                                      // 12*4608 + 1536
    int pn[kMaxLv]{}, off[kMaxLv + 1]{};
    // weights
    float *conv0_w = nullptr, *conv_b[8]{}, *conv_lnw[8]{}, *conv_lnb[8]{}, *conv_w[8]{};
    float *fp_lnw = nullptr, *fp_lnb = nullptr, *fp_w = nullptr, *fp_b = nullptr;
    float *pos_w = nullptr, *pos_b = nullptr, *enc_lnw = nullptr, *enc_lnb = nullptr;
    std::vector<W2VLayer> w2v;
    float *ada_w = nullptr, *ada_b = nullptr;
    float *ar_qkv_w = nullptr, *ar_qkv_b = nullptr;   // [depth][3E][E] / [depth][3E]: every block's q|k|v weights, contiguous
    std::vector<ARLayer> ar;
    float *logits_w = nullptr, *logits_b = nullptr, *vq_w = nullptr, *vq_b = nullptr, *sc_w = nullptr, *sc_b = nullptr;
    float *null_style = nullptr, *lvl_pos = nullptr, *prev_lvl_pos = nullptr;
    float *enc_pos = nullptr, *dec_pos = nullptr, *vae_mean = nullptr, *vae_std = nullptr;
    VAESide enc, dec;
    float *st_mean = nullptr, *st_std = nullptr, *st_pe = nullptr, *st_proj_w = nullptr, *st_proj_b = nullptr;
    std::vector<StyleLayer> style;
    Workspace ws;
    // profiling
    int profiling = 0;        // 0 off, 1 light (graphs stay on; events around eager launches only), 2 full (graphs off), 3 kernel timer (graphs off, one clip group, every launch timed)
    KernelTimer ktimer;       // level 3: per-kernel durations by bucket (artalk_get_kernel_sums)
    bool use_graphs = true;
    bool in_graph_body = false;   // capturing: no events
    bool in_body = false;         // inside run_chunk_body (captured or eager)
    std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
    std::vector<std::pair<size_t, double>> dom_events;   // (event index of start, flops)
    std::vector<std::pair<int, size_t>> marks;          // (bucket of the interval ending here, event index), caller's stream
    hipStream_t prof_stream = nullptr;
    hipStream_t side_stream[3] = {nullptr, nullptr, nullptr};   // extra branches of the AR body (run_body)
    hipEvent_t fork_ev = nullptr, join_ev[3] = {nullptr, nullptr, nullptr};
    int branches = 0;                 // 0 = automatic (2 for B >= 8), else forced 1/2/4
    hipStream_t own_stream = nullptr;   // used when the caller passes stream == NULL (graph capture needs a real stream)
    // graphs: one per (active batch size, clip group, precision, re-encoded clips), LRU-bounded (run_body)
    struct GraphEntry { hipGraphExec_t exec = nullptr; long long last_use = 0; };
    std::map<long long, GraphEntry> graphs;
    long long graph_clock = 0, graph_captures = 0;
    // Pinned host staging for the small per-call tables (chunk offsets, style flags): a ring of slots, each guarded by an event
    // recorded after its H2D copies, so artalk_infer never has to wait for its own copies (it blocks only if kStageSlots calls
    // are still in flight).  h_status receives the device status word at the end of every call (async), status_ev marks it.
    static constexpr int kStageSlots = 4;
    struct Stage { long* src = nullptr; uint8_t* has = nullptr; float** slots = nullptr; int4* smooth = nullptr; hipEvent_t done = nullptr; bool used = false; };
    Stage stage[kStageSlots];
    int stage_cap_c = 0, stage_cap_b = 0, stage_next = 0;
    // one slot per call in flight (ring of kStatusSlots, indexed by the call's ticket): a caller that keeps several calls queued reads
    // each call's own word (artalk_get_status_of)
    static constexpr int kStatusSlots = 4;
    int* h_status = nullptr; hipEvent_t status_ev[kStatusSlots] = {nullptr, nullptr, nullptr, nullptr}; bool status_pending = false;
    long long ticket = 0;          // number of calls that have published a status word; the last one's ticket is `ticket`, slot (ticket - 1) % kStatusSlots
};

namespace {

#define HIPCHK(m, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (m)->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            return ARTALK_EHIP;                                                                 \
        }                                                                                       \
    } while (0)

int fail(artalk_model* m, int code, const std::string& msg) { m->err = msg; return code; }
// the streaming / style-encode entry points run without stage events; the level comes back on every exit path
struct ProfilingOff {
    artalk_model* m; int saved;
    explicit ProfilingOff(artalk_model* x) : m(x), saved(x->profiling) { m->profiling = 0; }
    ~ProfilingOff() { m->profiling = saved; }
    ProfilingOff(const ProfilingOff&) = delete;
    ProfilingOff& operator=(const ProfilingOff&) = delete;
};

template <typename T>
T* dalloc_in(std::vector<void*>& pool, int64_t n) {
    void* p = nullptr;
    if (n <= 0) n = 1;
    if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) { pool.push_back(nullptr); return nullptr; }
    (void)hipMemset(p, 0, n * sizeof(T));
    pool.push_back(p);
    return reinterpret_cast<T*>(p);
}
template <typename T>
T* dalloc(artalk_model* m, int64_t n) { return dalloc_in<T>(m->allocs, n); }

float* walloc(artalk_model* m, int64_t n) {
    m->weight_bytes += n * 4;
    float* p = dalloc<float>(m, n);
    m->wranges.push_back({p, n, nullptr, nullptr});
    return p;
}

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
    for (void* p : m->allocs) if (!p) return fail(m, ARTALK_EHIP, "hipMalloc failed while allocating weights");
    return ARTALK_OK;
}

int upload(artalk_model* m, float* dst, const float* src, int64_t n) {
    HIPCHK(m, hipMemcpy(dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return ARTALK_OK;
}

// ------------------------------------------------------------------------------------------------ profiling
hipEvent_t next_event(artalk_model* m, hipStream_t s, size_t* idx) {
    if (m->ev_used == m->ev_pool.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        m->ev_pool.push_back(e);
    }
    *idx = m->ev_used++;
    (void)hipEventRecord(m->ev_pool[*idx], s);
    return m->ev_pool[*idx];
}
// profile buckets (artalk_get_profile): the interval that ENDS at a mark is charged to the mark's bucket
enum { PB_STYLE = 0, PB_CONV = 1, PB_ENC = 2, PB_ADA = 3, PB_AR = 4, PB_VAE = 5, PB_OTHER = 6 };
void kbucket(artalk_model* m, int b) { m->ktimer.bucket = b; }
void stage_mark(artalk_model* m, hipStream_t s, int bucket) {
    if (!m->profiling || m->in_graph_body) return;
    size_t i;
    next_event(m, s, &i);
    m->marks.emplace_back(bucket, i);
}

// fuse_ln: the AdaLN-modulated LayerNorm that consumes this GEMM's (768-wide, residual-stream) result.  If the GEMM is split
// over K, its reduce pass also writes that LayerNorm's output (one launch instead of two) and gemm() returns true; otherwise
// the caller launches the LayerNorm itself.
constexpr int kAuditSlots = 1024;
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
    const bool timed = m->profiling && plan.dominant && !m->in_body;
    size_t i0 = 0, i1 = 0;
    if (timed) next_event(m, s, &i0);
    run_gemm(g, plan, fuse_ln, s);
    if (timed) {
        next_event(m, s, &i1);
        m->dom_events.emplace_back(i0, gemm_flops(g));
    }
    return plan.fused_ln;
}

// ---- intermediate taps (include/artalk_hip.h: artalk_set_tap) ----
// slot (chunk index j, clip position b) of the tap buffer, fields in floats:
enum { TAP_BLK0_IN = 0, TAP_BLK0_OUT = kNTok * kE, TAP_BLKL_OUT = 2 * kNTok * kE, TAP_PREV_IN = 3 * kNTok * kE,
       TAP_LOGITS = 4 * kNTok * kE, TAP_DEC_OUT = 4 * kNTok * kE + kNTok * 64, TAP_SLOT = 4 * kNTok * kE + kNTok * 64 + 200 * 106 };
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

// ------------------------------------------------------------------------------------------------ stages
// The conv stack's passes over the chunks of one run_wav2vec call (tail skip): pass p holds n[p] chunks, `off[p]` chunks into the pass
// order, at the geometry of tail_geo[cls[p]] (cls 3: whole chunks).  The chunk table of the pass order and the gather table that
// brings the result back to the call's order (launch_conv_tail_gather) are rows `perm` and `tab` of the device chunk table.
struct ConvPasses { int np = 0; int off[4]{}, n[4]{}, cls[4]{}; const long* perm = nullptr; const long* tab = nullptr; };

// wav2vec2 on chunks [c0, c0+n) of the chunk list (app/modules/wav2vec.py:11-20); writes SiLU(pooled cond) rows c0*181..
void run_wav2vec(artalk_model* m, const float* audio, int c0, int n, float* out_w2v, hipStream_t s, const ConvPasses* tail = nullptr) {
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
void run_style(artalk_model* m, const float* style_motion, int B, hipStream_t s, bool encode = true) {
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
        // ordering against this fill otherwise.  Once per model and mode, beside the hipMalloc above.  A fill that raised a
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
    const artalk_config& c = m->cfg;
    Workspace v = m->ws;
    const long b = b0;
    v.ada += b * kNTok * m->ada_n; v.style_cond += b * kE; v.prev_in += b * kNTok * kE; v.prev_in_p8 += b * kNTok * kE;
    v.cache += b * 2 * kNTok * 3 * kE;
    v.x += b * 100 * kE; v.xmod += b * 100 * kE; v.attn_out += b * 100 * kE; v.ffn_h += b * 100 * 4 * kE;
    v.logits += b * 100 * 2 * c.code_dim; v.fhat += b * 100 * c.code_dim; v.nextfeat += b * 100 * c.code_dim;
    v.bits += b * kNTok * c.code_dim; v.hist_bits += b * kNTok * c.code_dim;
    v.prev_fdec += b * 100 * c.code_dim; v.msfeat += b * 180 * c.code_dim; v.dec_x += b * 200 * c.code_dim;
    const long H = c.vae_hidden;
    v.vh += b * 200 * H; v.vln += b * 200 * H; v.vqkv += b * 200 * 3 * H; v.vatt += b * 200 * H; v.vmlp += b * 200 * H * 3 / 2;
    v.dec_out += b * 200 * c.motion_dim; v.enc_in += b * 100 * 128; v.enc_out += b * 100 * c.code_dim;
    v.motion_chunk += b * 100 * c.motion_dim;
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
    if (!m->fork_ev) HIPCHK(m, hipEventCreateWithFlags(&m->fork_ev, hipEventDisableTiming));
    for (int i = 0; i < n && i < 3; ++i) {
        if (m->side_stream[i]) continue;
        if (m->cu_mask.empty()) HIPCHK(m, hipStreamCreateWithFlags(&m->side_stream[i], hipStreamNonBlocking));
        else HIPCHK(m, hipExtStreamCreateWithCUMask(&m->side_stream[i], (uint32_t)m->cu_mask.size(), m->cu_mask.data()));
        HIPCHK(m, hipEventCreateWithFlags(&m->join_ev[i], hipEventDisableTiming));
    }
    return ARTALK_OK;
}
int body_branches(const artalk_model* m, int B) {
    // measured at batch 32: 1 branch 54.9 ms, 2 branches 49.5 ms, 4 branches 77-120 ms (queue sharing / contention)
    const int want = m->branches > 0 ? m->branches : (B >= 8 ? 2 : 1);
    return B >= 2 * want ? want : (B >= 8 ? 2 : 1);
}
// Replay captured graphs, or launch eagerly?  The one rule, for the batch call and the streaming calls alike: the audit and the taps
// are launches of their own that a replay would not make (or would make forever), profiling levels 2 and 3 time the single launches.
bool body_uses_graphs(const artalk_model* m) { return m->use_graphs && m->profiling < 2 && !m->audit && !m->tap; }
void drop_graphs(artalk_model* m) {
    for (auto& g : m->graphs) (void)hipGraphExecDestroy(g.second.exec);
    m->graphs.clear();
}
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
        (void)hipGraphExecDestroy(victim->second.exec);
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
    for (int h = 1; fork && h < g.n; ++h) st[h] = m->side_stream[h - 1];
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
        m->graphs.emplace(g.key[h], artalk_model::GraphEntry{exec, ++m->graph_clock});
        ++m->graph_captures;
    }
    if (fork) {
        HIPCHK(m, hipEventRecord(m->fork_ev, s));
        for (int h = 1; h < g.n; ++h) HIPCHK(m, hipStreamWaitEvent(st[h], m->fork_ev, 0));
    }
    for (int h = 0; h < g.n; ++h) {
        if (g.graphs) HIPCHK(m, hipGraphLaunch(m->graphs[g.key[h]].exec, st[h]));
        else launch_group(h);
    }
    for (int h = 1; fork && h < g.n; ++h) {
        HIPCHK(m, hipEventRecord(m->join_ev[h - 1], st[h]));
        HIPCHK(m, hipStreamWaitEvent(s, m->join_ev[h - 1], 0));
    }
    return ARTALK_OK;
}

void free_stage(artalk_model* m) {
    for (auto& st : m->stage) {
        if (st.src) (void)hipHostFree(st.src);
        if (st.has) (void)hipHostFree(st.has);
        if (st.slots) (void)hipHostFree(st.slots);
        if (st.smooth) (void)hipHostFree(st.smooth);
        st.src = nullptr; st.has = nullptr; st.slots = nullptr; st.smooth = nullptr; st.used = false;
    }
    m->stage_cap_c = m->stage_cap_b = 0;
}
int ensure_stage(artalk_model* m, int maxB, int maxC) {
    if (!m->h_status) {
        HIPCHK(m, hipHostMalloc(reinterpret_cast<void**>(&m->h_status), artalk_model::kStatusSlots * sizeof(int), hipHostMallocDefault));
        std::memset(m->h_status, 0, artalk_model::kStatusSlots * sizeof(int));
        for (auto& e : m->status_ev) HIPCHK(m, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (maxB <= m->stage_cap_b && maxC <= m->stage_cap_c) return ARTALK_OK;
    for (auto& st : m->stage) if (st.used) HIPCHK(m, hipEventSynchronize(st.done));
    free_stage(m);
    for (auto& st : m->stage) {
        HIPCHK(m, hipHostMalloc(reinterpret_cast<void**>(&st.src), (size_t)3 * maxC * sizeof(long), hipHostMallocDefault));
        HIPCHK(m, hipHostMalloc(reinterpret_cast<void**>(&st.has), (size_t)maxB, hipHostMallocDefault));
        HIPCHK(m, hipHostMalloc(reinterpret_cast<void**>(&st.slots), (size_t)maxB * sizeof(float*), hipHostMallocDefault));
        HIPCHK(m, hipHostMalloc(reinterpret_cast<void**>(&st.smooth), (size_t)maxB * sizeof(int4), hipHostMallocDefault));
        if (!st.done) HIPCHK(m, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    }
    m->stage_cap_b = maxB; m->stage_cap_c = maxC;
    return ARTALK_OK;
}
// next slot of the ring; waits only if the call that last used it has not consumed its copies yet
int next_stage(artalk_model* m, artalk_model::Stage** out) {
    artalk_model::Stage& st = m->stage[m->stage_next];
    m->stage_next = (m->stage_next + 1) % artalk_model::kStageSlots;
    if (st.used) HIPCHK(m, hipEventSynchronize(st.done));
    *out = &st;
    return ARTALK_OK;
}
// end of a call: hand the device status word to the host asynchronously (artalk_get_status / artalk_poll_status read it)
int publish_status(artalk_model* m, hipStream_t s) {
    const int slot = (int)(m->ticket % artalk_model::kStatusSlots);
    // the slot's previous user is kStatusSlots calls back: its copy has long landed unless the caller queued more calls than slots
    if (m->ticket >= artalk_model::kStatusSlots) HIPCHK(m, hipEventSynchronize(m->status_ev[slot]));
    HIPCHK(m, hipMemcpyAsync(m->h_status + slot, m->ws.status, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(m, hipEventRecord(m->status_ev[slot], s));
    ++m->ticket;
    m->status_pending = true;
    HIPCHK(m, hipGetLastError());
    return ARTALK_OK;
}

int reserve(artalk_model* m, int maxB, int maxC) {
    const artalk_config& c = m->cfg;
    if (maxB <= m->ws.maxB && maxC <= m->ws.maxC) return ensure_stage(m, m->ws.maxB, m->ws.maxC);
    // grow: drop the old workspace (and the graphs that captured its pointers) and allocate the larger one
    maxB = std::max(maxB, m->ws.maxB); maxC = std::max(maxC, m->ws.maxC);
    (void)hipDeviceSynchronize();
    drop_graphs(m);
    for (void* p : m->ws_allocs) if (p) (void)hipFree(p);
    m->ws_allocs.clear();
    m->ws = Workspace();
    m->stream_B = 0; m->stream_scales_ended = false;          // the streaming history lived in the workspace that was just dropped: a session must begin again
    m->status_pending = false;
    Workspace& w = m->ws;
    const int CD = c.w2v_conv_dim, Hs = c.w2v_hidden;
    w.maxB = maxB; w.maxC = maxC; w.G = std::min(maxC, 96);
    auto F = [&](int64_t n) { w.bytes += n * 4; return dalloc_in<float>(m->ws_allocs, n); };
    const int G = w.G;
    w.src_off = dalloc_in<long>(m->ws_allocs, (int64_t)3 * maxC);      // chunk table of a call [C] | in pass order [C] | gather table [C] (ConvPasses)
    w.xnorm = F((int64_t)G * kSamplesPerChunk);
    w.convA = F(((int64_t)G * m->conv_S[0] + 16) * CD);
    w.convB = F(((int64_t)G * m->conv_S[1] + 16) * CD);
    const int64_t M = (int64_t)G * m->Ts;
    w.h0 = F(M * Hs); w.h1 = F(M * Hs); w.xln = F(M * Hs); w.qkv = F(M * 3 * Hs); w.att = F(M * Hs); w.ffn = F(M * c.w2v_ffn);
    w.silu_cond = F((int64_t)maxC * kNTok * kCond);
    w.ada = F((int64_t)maxB * kNTok * m->ada_n);
    w.style_cond = F((int64_t)maxB * kE);
    w.prev_in = F((int64_t)maxB * kNTok * kE); w.prev_in_p8 = F((int64_t)maxB * kNTok * kE);
    w.cache = F((int64_t)c.ar_depth * maxB * 2 * kNTok * 3 * kE);
    w.x = F((int64_t)maxB * 100 * kE); w.xmod = F((int64_t)maxB * 100 * kE); w.attn_out = F((int64_t)maxB * 100 * kE);
    w.ffn_h = F((int64_t)maxB * 100 * 4 * kE); w.logits = F((int64_t)maxB * 100 * 2 * c.code_dim);
    w.splitk_floats = (int64_t)8 << 20; w.splitk = F(w.splitk_floats); w.splitk_b[0] = w.splitk;
    for (int i = 1; i < 4; ++i) w.splitk_b[i] = F(w.splitk_floats);
    w.fhat = F((int64_t)maxB * 100 * c.code_dim); w.nextfeat = F((int64_t)maxB * 100 * c.code_dim);
    w.bits = dalloc_in<uint8_t>(m->ws_allocs, (int64_t)maxB * kNTok * c.code_dim);
    w.hist_bits = dalloc_in<uint8_t>(m->ws_allocs, (int64_t)maxB * kNTok * c.code_dim);
    w.has_style = dalloc_in<uint8_t>(m->ws_allocs, maxB);
    w.status = dalloc_in<int>(m->ws_allocs, 4);
    w.sess_slots = dalloc_in<float*>(m->ws_allocs, maxB);
    w.prev_fdec = F((int64_t)maxB * 100 * c.code_dim); w.msfeat = F((int64_t)maxB * 180 * c.code_dim);
    const int H = c.vae_hidden;
    w.dec_x = F((int64_t)maxB * 200 * c.code_dim); w.vh = F((int64_t)maxB * 200 * H); w.vln = F((int64_t)maxB * 200 * H);
    w.vqkv = F((int64_t)maxB * 200 * 3 * H); w.vatt = F((int64_t)maxB * 200 * H); w.vmlp = F((int64_t)maxB * 200 * H * 3 / 2);
    w.dec_out = F((int64_t)maxB * 200 * c.motion_dim); w.enc_in = F((int64_t)maxB * 100 * 128);
    w.enc_out = F((int64_t)maxB * 100 * c.code_dim); w.motion_chunk = F((int64_t)maxB * 100 * c.motion_dim);
    const int S = c.style_dim, SL = c.style_len;
    w.s_in = F((int64_t)maxB * SL * 128); w.s_h = F((int64_t)maxB * SL * S); w.s_qkv = F((int64_t)maxB * SL * 3 * S);
    w.s_att = F((int64_t)maxB * SL * S); w.s_ffn = F((int64_t)maxB * SL * c.style_ffn); w.s_tmp = F((int64_t)maxB * SL * S);
    for (void* p : m->ws_allocs)
        if (!p) return fail(m, ARTALK_EHIP, "hipMalloc failed while reserving workspace");
    // the zero fills above run on the null stream; callers use non-blocking streams, which do not order against it
    HIPCHK(m, hipDeviceSynchronize());
    return ensure_stage(m, maxB, maxC);
}

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

// ---------------------------------------------------------------------------------- shared by the batch call and the streaming calls
// device of the model and the stream of this call: the caller's, or the model's own (graph capture needs a real stream)
int call_stream(artalk_model* m, void* stream, hipStream_t* s) {
    (void)hipSetDevice(m->device);
    if (!stream && !m->own_stream) HIPCHK(m, hipStreamCreate(&m->own_stream));
    *s = stream ? (hipStream_t)stream : m->own_stream;
    return ARTALK_OK;
}
// the style flags of a call, checked before anything is enqueued or any state changes; *encode = some clip brings a style clip (flag 1)
int check_has_style(artalk_model* m, const float* style_motion_dev, const uint8_t* has_style, int B, bool* encode) {
    *encode = false;
    for (int b = 0; style_motion_dev && has_style && b < B; ++b) {
        if (has_style[b] > 2) return fail(m, ARTALK_EINVAL, "has_style entries must be 0, 1 or 2");
        *encode |= has_style[b] == 1;
    }
    return ARTALK_OK;
}
// Start of a call for B clips: the style flags go through the pinned slot `stg` (its event then covers every copy the caller staged
// in it before), the status word is reset, the style conditions are computed.
int begin_clips(artalk_model* m, hipStream_t s, int B, const float* style_motion_dev, const uint8_t* has_style, bool encode_style,
                artalk_model::Stage* stg) {
    Workspace& w = m->ws;
    if (!has_style) style_motion_dev = nullptr;
    if (style_motion_dev) {
        std::memcpy(stg->has, has_style, (size_t)B);
        HIPCHK(m, hipMemcpyAsync(w.has_style, stg->has, B, hipMemcpyHostToDevice, s));
    }
    HIPCHK(m, hipEventRecord(stg->done, s));   // pinned slot: no synchronisation, the slot is reused kStageSlots calls later
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

// ---------------------------------------------------------------------------------- session pool (artalk_session_*)
SessionRows session_rows(const artalk_model* m) {
    const Workspace& w = m->ws;
    SessionRows r;
    r.style = reinterpret_cast<uint4*>(w.style_cond); r.prev_in = reinterpret_cast<uint4*>(w.prev_in); r.prev_fdec = reinterpret_cast<uint4*>(w.prev_fdec);
    r.s16 = kE / 4; r.p16 = kNTok * kE / 4; r.f16 = 100 * m->cfg.code_dim / 4;
    return r;
}
// at least n_slots slots: new blocks only, nothing is moved (the slots are written by a scatter before anything reads them: no fill)
int grow_sessions(artalk_model* m, int64_t n_slots) {
    artalk_model::Sessions& ss = m->sess;
    if (m->cfg.code_dim % 4) return fail(m, ARTALK_EINVAL, "sessions need a code_dim that is a multiple of 4 (16-byte rows)");
    while ((int64_t)ss.owner.size() < n_slots) {
        void* p = nullptr;
        HIPCHK(m, hipMalloc(&p, (size_t)artalk_model::kSessBlock * m->sess_slot_floats() * sizeof(float)));
        ss.blocks.push_back(static_cast<float*>(p));
        ss.owner.resize(ss.owner.size() + artalk_model::kSessBlock, 0);
    }
    if (ss.smooth_cap < (int64_t)ss.owner.size()) {      // the table of artalk_session_smooth: one row per slot is always enough (hipFree waits for the device)
        if (ss.smooth_tab) (void)hipFree(ss.smooth_tab);
        ss.smooth_tab = nullptr; ss.smooth_cap = 0;
        HIPCHK(m, hipMalloc(&ss.smooth_tab, ss.owner.size() * (sizeof(float*) + sizeof(int4))));
        ss.smooth_cap = (int64_t)ss.owner.size();
    }
    return ARTALK_OK;
}

// ---------------------------------------------------------------------------------- streaming smoother: the checks, on the host alone
// Which stream frames a smoother call emits: [max(0, seen - 4), last ? seen + nf : seen + nf - 4)  (model.py: smooth_span)
void smooth_span(int64_t seen, int nf, bool last, int* first, int* count) {
    const int64_t f = seen > kSavgolLag ? seen - kSavgolLag : 0;
    *first = (int)f;
    *count = (int)((last ? seen + nf : seen + nf - kSavgolLag) - f);
}
// one row of a smoother call, in two parts (a finished smoother is refused between them); `who` names the row in the message
int smooth_row_range(const std::string& who, int nf, bool last, std::string* err) {
    if (nf < 0 || nf > 100) { *err = who + ": n_frames " + std::to_string(nf) + " is outside 0..100"; return ARTALK_EINVAL; }
    if (nf < 100 && !last) { *err = who + ": fewer than 100 frames (" + std::to_string(nf) + ") without `last`"; return ARTALK_EINVAL; }
    return ARTALK_OK;
}
int smooth_row_length(const std::string& who, int64_t seen, int nf, bool last, std::string* err) {
    if (seen < 0 || seen > INT_MAX - 2 * kSavgolMaxOut) { *err = who + ": frame count out of range"; return ARTALK_EINVAL; }
    if (last && seen + nf < kSavgolCarry) { *err = who + ": savgol (mode='interp') needs window_length <= T (T >= 9)"; return ARTALK_EINVAL; }
    return ARTALK_OK;
}
int smooth_stride_check(const char* fn, bool have_raw, bool need_raw, int64_t raw_stride, int64_t out_stride, int D, std::string* err) {
    if (need_raw && !have_raw) { *err = std::string(fn) + ": no raw frames given"; return ARTALK_EINVAL; }
    if (need_raw && raw_stride < 100LL * D) { *err = std::string(fn) + ": raw_stride is below 100 x " + std::to_string(D); return ARTALK_EINVAL; }
    if (out_stride < (int64_t)kSavgolMaxOut * D) { *err = std::string(fn) + ": out_stride is below 104 x " + std::to_string(D); return ARTALK_EINVAL; }
    return ARTALK_OK;
}
// every check of artalk_session_smooth, in the order the header lists them; on success st[i] is the state of ids[i].  Nothing is changed.
int smooth_check(artalk_model::Sessions& ss, const int64_t* ids, int n, bool have_raw, int64_t raw_stride, const int* n_frames,
                 const uint8_t* last, int64_t out_stride, int D, std::vector<artalk_model::Sessions::Open*>* st, std::string* err) {
    st->assign((size_t)n, nullptr);
    std::set<int64_t> listed;
    for (int i = 0; i < n; ++i) {
        const auto it = ss.open.find(ids[i]);
        if (it == ss.open.end()) {
            if (ss.ended_by_scales.count(ids[i])) {
                *err = "session " + std::to_string(ids[i]) + ": the site scales changed since artalk_session_open; open the session again";
                return ARTALK_ESTATE;
            }
            *err = "artalk_session_smooth: " + std::to_string(ids[i]) + " is not an open session";
            return ARTALK_EINVAL;
        }
        if (!listed.insert(ids[i]).second) { *err = "artalk_session_smooth: session " + std::to_string(ids[i]) + " is listed twice"; return ARTALK_EINVAL; }
        (*st)[i] = &it->second;
    }
    bool need_raw = false;
    for (int i = 0; i < n; ++i) {
        const int nf = n_frames ? n_frames[i] : 100;
        const bool lst = last && last[i];
        const std::string who = "artalk_session_smooth: session " + std::to_string(ids[i]);
        if (int rc = smooth_row_range(who, nf, lst, err)) return rc;
        if ((*st)[i]->smooth_done) { *err = who + " has been smoothed to its end (a `last` call was made)"; return ARTALK_ESTATE; }
        if (int rc = smooth_row_length(who, (*st)[i]->seen, nf, lst, err)) return rc;
        need_raw |= nf > 0;
    }
    return smooth_stride_check("artalk_session_smooth", have_raw, need_raw, raw_stride, out_stride, D, err);
}
// the device table of this call's slots (row i = slot[i]) through the pinned slot `stg`; the caller records stg->done afterwards
int stage_session_slots(artalk_model* m, hipStream_t s, artalk_model::Stage* stg, const int* slot, int n) {
    for (int i = 0; i < n; ++i) stg->slots[i] = m->sess_slot(slot[i]);
    HIPCHK(m, hipMemcpyAsync(m->ws.sess_slots, stg->slots, (size_t)n * sizeof(float*), hipMemcpyHostToDevice, s));
    return ARTALK_OK;
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
    drop_graphs(m);
    for (auto e : m->ev_pool) (void)hipEventDestroy(e);
    for (auto e : m->ktimer.pool) (void)hipEventDestroy(e);
    if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
    for (int i = 0; i < 3; ++i) {
        if (m->side_stream[i]) (void)hipStreamDestroy(m->side_stream[i]);
        if (m->join_ev[i]) (void)hipEventDestroy(m->join_ev[i]);
    }
    if (m->fork_ev) (void)hipEventDestroy(m->fork_ev);
    free_stage(m);
    for (auto& st : m->stage) if (st.done) (void)hipEventDestroy(st.done);
    if (m->h_status) (void)hipHostFree(m->h_status);
    for (auto& e : m->status_ev) if (e) (void)hipEventDestroy(e);
    for (void* p : m->allocs) if (p) (void)hipFree(p);
    for (void* p : m->ws_allocs) if (p) (void)hipFree(p);
    for (float* p : m->sess.blocks) if (p) (void)hipFree(p);
    if (m->sess.smooth_tab) (void)hipFree(m->sess.smooth_tab);
    delete m;
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
        HIPCHK(m, hipMalloc(reinterpret_cast<void**>(&m->audit_vals), kAuditSlots * sizeof(unsigned int)));
        m->allocs.push_back(m->audit_vals);
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
        if (m->side_stream[i]) { (void)hipStreamDestroy(m->side_stream[i]); m->side_stream[i] = nullptr; }
        if (m->join_ev[i]) { (void)hipEventDestroy(m->join_ev[i]); m->join_ev[i] = nullptr; }
    }
    drop_graphs(m);      // the GEMM grids were captured for the old CU count
    m->invalidate_init_hist();
    return ARTALK_OK;
}

int artalk_infer(artalk_model* m, const float* audio_dev, int64_t audio_clip_stride, const int64_t* n_chunks, int B,
                 const float* style_motion_dev, const uint8_t* has_style, float* out_motion_dev, int64_t out_clip_stride,
                 uint8_t* out_bits_dev, uint8_t* out_hist_bits_dev, float* out_w2v_dev, void* stream) {
    return artalk_infer_samples(m, audio_dev, audio_clip_stride, n_chunks, nullptr, B, style_motion_dev, has_style, out_motion_dev, out_clip_stride,
                                out_bits_dev, out_hist_bits_dev, out_w2v_dev, stream);
}

// artalk_infer for clips whose length is known: n_samples[b] real samples, zeros behind them up to n_chunks[b] whole chunks.  The conv
// stack then skips the frames that hear the padding alone (run_wav2vec); n_samples = NULL: every chunk is full.
int artalk_infer_samples(artalk_model* m, const float* audio_dev, int64_t audio_clip_stride, const int64_t* n_chunks, const int64_t* n_samples,
                         int B, const float* style_motion_dev, const uint8_t* has_style, float* out_motion_dev, int64_t out_clip_stride,
                         uint8_t* out_bits_dev, uint8_t* out_hist_bits_dev, float* out_w2v_dev, void* stream) {
    if (!m || !audio_dev || !n_chunks || !out_motion_dev || B <= 0) return ARTALK_EINVAL;
    if (!m->finalized) return fail(m, ARTALK_ESTATE, "artalk_infer before artalk_finalize_weights");
    for (int b = 0; n_samples && b < B; ++b)
        if (n_chunks[b] > 0 && (n_samples[b] < 1 || n_samples[b] > n_chunks[b] * kSamplesPerChunk))
            return fail(m, ARTALK_EINVAL, "n_samples[" + std::to_string(b) + "] must be in 1 .. n_chunks * " + std::to_string(kSamplesPerChunk));
    hipStream_t s;
    if (int rc = call_stream(m, stream, &s)) return rc;
    const artalk_config& c = m->cfg;
    int64_t C = 0, maxch = n_chunks[0];
    for (int b = 0; b < B; ++b) {
        if (n_chunks[b] <= 0 || (b > 0 && n_chunks[b] > n_chunks[b - 1])) return fail(m, ARTALK_EINVAL, "n_chunks must be positive and non-increasing");
        C += n_chunks[b];
    }
    bool encode_style;
    if (int rc = check_has_style(m, style_motion_dev, has_style, B, &encode_style)) return rc;
    if (m->tap && (B > m->tap_B || maxch > m->tap_maxch)) return fail(m, ARTALK_EINVAL, "the tap buffer (artalk_set_tap) is smaller than this call");
    if (B > m->ws.maxB || C > m->ws.maxC) { if (int rc = reserve(m, B, (int)C)) return rc; }
    Workspace& w = m->ws;
    // chunk list, chunk-index major: chunk (j, b) for all b with n_chunks[b] > j  -> active clips are a prefix
    artalk_model::Stage* stg = nullptr;
    if (int rc = next_stage(m, &stg)) return rc;
    long* src = stg->src;
    std::vector<int> base((size_t)maxch + 1, 0), Bj((size_t)maxch, 0);
    {
        int idx = 0;
        for (int64_t j = 0; j < maxch; ++j) {
            base[j] = idx;
            for (int b = 0; b < B && n_chunks[b] > j; ++b) { src[idx++] = (long)b * audio_clip_stride + (long)j * kSamplesPerChunk; Bj[j]++; }
        }
        base[maxch] = idx;
    }
    // Tail skip: the length class of every chunk (3: the whole chunk - also a chunk wholly behind the clip's end, which cannot arise from
    // a count that matches its chunk count), and per run_wav2vec group with a partial chunk its passes, the chunk table in pass order
    // (src[C ..]) and the gather table (src[2 C ..]): launch_conv_tail_gather.
    std::vector<ConvPasses> passes;
    bool any_tail = false;
    if (n_samples && m->tail_skip) {
        std::vector<int> cls((size_t)C, 3);
        for (int64_t j = 0, idx = 0; j < maxch; ++j)
            for (int b = 0; b < B && n_chunks[b] > j; ++b, ++idx) {
                const int64_t v = std::min<int64_t>(n_samples[b] - j * kSamplesPerChunk, kSamplesPerChunk);
                const int64_t bound = v >= 1 ? artalk_conv_tail_class(v, kSamplesPerChunk) : 0;
                const int q = bound >= 1 && kSamplesPerChunk % 4 == 0 ? (int)(bound / (kSamplesPerChunk / 4)) : 4;
                cls[idx] = m->tail_geo[q - 1].partial ? q - 1 : 3;
            }
        const int last = m->n_conv - 1;
        for (int c0 = 0; c0 < C; c0 += w.G) {
            const int n = (int)std::min<int64_t>(w.G, C - c0);
            ConvPasses cp;
            static const int order[4] = {3, 0, 1, 2};      // whole chunks first, then the classes
            int pos = 0;
            long row0 = 0;                                 // where the pass's rows of the last layer start (run_wav2vec)
            for (int k = 0; k < 4; ++k) {
                const int cl = order[k], off = pos;
                const artalk_model::TailGeo& tg = m->tail_geo[cl];
                const long rows = cl == 3 ? m->Ts : tg.S[last], tc = cl == 3 ? m->Tw - 1 : tg.tc;
                for (int i = 0; i < n; ++i)
                    if (cls[c0 + i] == cl) {
                        src[C + c0 + pos] = src[c0 + i];
                        src[2 * C + c0 + i] = (row0 + (pos - off) * rows) | (tc << 32);
                        ++pos;
                    }
                if (pos > off) { cp.off[cp.np] = off; cp.n[cp.np] = pos - off; cp.cls[cp.np] = cl; ++cp.np; row0 += (pos - off) * rows; }
            }
            if (cp.np == 1 && cp.cls[0] == 3) cp.np = 0;      // whole chunks only: the launches of a call without counts, no gather
            else { cp.perm = w.src_off + C + c0; cp.tab = w.src_off + 2 * C + c0; any_tail = true; }
            passes.push_back(cp);
        }
    }
    HIPCHK(m, hipMemcpyAsync(w.src_off, src, (any_tail ? 3 : 1) * C * sizeof(long), hipMemcpyHostToDevice, s));
    m->stream_B = 0; m->stream_scales_ended = false;   // the batch call reuses the workspace that holds the streaming history
    m->ev_used = 0; m->dom_events.clear(); m->marks.clear(); m->prof_stream = s;
    // level 3: every kernel of this call is launched with its own start / stop events (kernels.h ARTALK_LAUNCH) - on this thread, for the
    // duration of the call; the body then runs eagerly, its clip groups one after the other (run_body)
    struct TimerScope { bool on; TimerScope(artalk_model* x) : on(x->profiling == 3) { if (on) { x->ktimer.used = 0; x->ktimer.recs.clear(); x->ktimer.bucket = KB_OTHER; g_ktimer = &x->ktimer; } }
                        ~TimerScope() { if (on) g_ktimer = nullptr; } } timer_scope(m);
    if (int rc = begin_clips(m, s, B, style_motion_dev, has_style, encode_style, stg)) return rc;
    // (wav2vec2 of chunk index j + 1 on a stream of its own beside the AR/VAE body of index j was an option until round 3: with the
    // persistent one-workgroup-per-CU GEMM kernels, whose workgroups hold a CU's LDS for a whole launch, the body's short kernels wait
    // behind them - 82 -> 128 ms per step; removed)
    for (int c0 = 0, gi = 0; c0 < C; c0 += w.G, ++gi)
        run_wav2vec(m, audio_dev, c0, (int)std::min<int64_t>(w.G, C - c0), out_w2v_dev, s, !passes.empty() && passes[gi].np ? &passes[gi] : nullptr);
    // initial history: encode + quantise an all-zero motion (app/models.py:86-89) - the same for every clip: cached per model
    if (int rc = run_init_history(m, B, s)) return rc;
    const size_t bits_row = (size_t)kNTok * c.code_dim;
    if (out_hist_bits_dev)
        HIPCHK(m, hipMemcpy2DAsync(out_hist_bits_dev, (size_t)(maxch + 1) * bits_row, w.hist_bits, bits_row, bits_row, B,
                                   hipMemcpyDeviceToDevice, s));
    stage_mark(m, s, PB_VAE);
    for (int64_t j = 0; j < maxch; ++j) {
        const int Bn = Bj[j];
        // clips whose motion must be re-encoded into a history: those with a chunk j + 1 (a prefix: clips are sorted by length) - all of
        // them when the caller asked for the history bits of every chunk (the reference computes the trailing ones too and drops them)
        const int n_next = out_hist_bits_dev ? Bn : (j + 1 < maxch ? Bj[j + 1] : 0);
        if (int rc = chunk_step(m, s, base[j], Bn, n_next, (int)j, out_motion_dev + j * 100 * c.motion_dim, out_clip_stride)) return rc;
        if (out_bits_dev)
            HIPCHK(m, hipMemcpy2DAsync(out_bits_dev + j * bits_row, (size_t)maxch * bits_row, w.bits, bits_row, bits_row, Bn,
                                       hipMemcpyDeviceToDevice, s));
        if (out_hist_bits_dev)
            HIPCHK(m, hipMemcpy2DAsync(out_hist_bits_dev + (j + 1) * bits_row, (size_t)(maxch + 1) * bits_row, w.hist_bits, bits_row,
                                       bits_row, Bn, hipMemcpyDeviceToDevice, s));
    }
    stage_mark(m, s, PB_OTHER);
    if (int rc = publish_status(m, s)) return rc;
    if (m->sticky_error) { m->sticky_error = false; return ARTALK_ESTATE; }
    return ARTALK_OK;
}

// Style-clip cache support: the style condition of app/models.py:67-73 depends on the style clip only,
// and the reference's engine keeps ONE style clip across many inference calls (inference.py:41-45,115-118).  This computes the
// conditions of n clips once; a later artalk_infer / artalk_stream_begin takes such a condition in place of the clip (flag 2).
int artalk_style_encode(artalk_model* m, const float* style_motion_dev, int n, float* out_cond_dev, void* stream) {
    if (!m || !style_motion_dev || !out_cond_dev || n <= 0) return ARTALK_EINVAL;
    if (!m->finalized) return fail(m, ARTALK_ESTATE, "artalk_style_encode before artalk_finalize_weights");
    hipStream_t s;
    if (int rc = call_stream(m, stream, &s)) return rc;
    if (m->stream_B > 0) return fail(m, ARTALK_ESTATE, "artalk_style_encode during a streaming session (it shares the workspace)");
    if (n > m->ws.maxB) { if (int rc = reserve(m, n, std::max(n, m->ws.maxC))) return rc; }
    Workspace& w = m->ws;
    HIPCHK(m, hipMemsetAsync(w.has_style, 1, n, s));
    {
        ProfilingOff quiet(m);
        run_style(m, style_motion_dev, n, s, true);
    }
    HIPCHK(m, hipMemcpyAsync(out_cond_dev, w.style_cond, (size_t)n * kE * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(m, hipGetLastError());
    return ARTALK_OK;
}

// ---------------------------------------------------------------------------------- streaming
// The path already produces 4-second blocks causally (app/models.py:92-114: chunk j needs only the re-encoded motion of
// chunk j-1); these two calls expose that with the history kept in the model's workspace between calls.
int artalk_stream_begin(artalk_model* m, int B, const float* style_motion_dev, const uint8_t* has_style, void* stream) {
    if (!m || B <= 0) return ARTALK_EINVAL;
    if (!m->finalized) return fail(m, ARTALK_ESTATE, "artalk_stream_begin before artalk_finalize_weights");
    bool encode_style;
    if (int rc = check_has_style(m, style_motion_dev, has_style, B, &encode_style)) return rc;
    hipStream_t s;
    if (int rc = call_stream(m, stream, &s)) return rc;
    if (B > m->ws.maxB || B > m->ws.maxC) { if (int rc = reserve(m, B, B)) return rc; }
    if (int rc = ensure_stage(m, m->ws.maxB, m->ws.maxC)) return rc;
    artalk_model::Stage* stg = nullptr;
    if (int rc = next_stage(m, &stg)) return rc;
    {
        ProfilingOff quiet(m);
        if (int rc = begin_clips(m, s, B, style_motion_dev, has_style, encode_style, stg)) return rc;   // the status word covers the whole session
        if (int rc = run_init_history(m, B, s)) return rc;
    }
    m->stream_B = B; m->stream_scales_ended = false;
    if (int rc = publish_status(m, s)) return rc;
    return ARTALK_OK;
}

// audio_dev: [B][chunk_stride] f32, the next 64000 samples of every stream (zero padded by the caller at the end of a
// clip); out_motion_dev: [B][out_stride] receives 100 x 106 codes per stream.
int artalk_stream_chunk(artalk_model* m, const float* audio_dev, int64_t chunk_stride, float* out_motion_dev, int64_t out_stride,
                        void* stream) {
    if (!m || !audio_dev || !out_motion_dev) return ARTALK_EINVAL;
    if (m->stream_B <= 0)
        return fail(m, ARTALK_ESTATE, m->stream_scales_ended ? "the site scales changed since artalk_stream_begin; begin again"
                                                             : "artalk_stream_chunk before artalk_stream_begin");
    hipStream_t s;
    if (int rc = call_stream(m, stream, &s)) return rc;
    const int B = m->stream_B;
    Workspace& w = m->ws;
    if (B > w.maxB) return fail(m, ARTALK_ESTATE, "workspace was re-reserved since artalk_stream_begin; begin again");
    artalk_model::Stage* stg = nullptr;
    if (int rc = next_stage(m, &stg)) return rc;
    for (int b = 0; b < B; ++b) stg->src[b] = (long)b * chunk_stride;
    HIPCHK(m, hipMemcpyAsync(w.src_off, stg->src, B * sizeof(long), hipMemcpyHostToDevice, s));
    HIPCHK(m, hipEventRecord(stg->done, s));
    stg->used = true;
    ProfilingOff quiet(m);      // restored on every exit path
    for (int c0 = 0; c0 < B; c0 += w.G) run_wav2vec(m, audio_dev, c0, std::min(w.G, B - c0), nullptr, s);
    // every stream has a next chunk; no taps: their slots belong to the chunk indices of a batch call
    if (int rc = chunk_step(m, s, 0, B, B, m->tap_maxch, out_motion_dev, out_stride)) return rc;
    if (int rc = publish_status(m, s)) return rc;
    return ARTALK_OK;
}

int artalk_stream_end(artalk_model* m) {
    if (!m) return ARTALK_EINVAL;
    m->stream_B = 0; m->stream_scales_ended = false;      // the history in the workspace is dead; artalk_style_encode / artalk_reserve may use the workspace again
    return ARTALK_OK;
}

// ---------------------------------------------------------------------------------- independent sessions
// The same chunk step for streams that join and leave between steps: the history of every session lives in the session pool
// (artalk_model::Sessions) and visits the workspace only for the duration of a call.
int artalk_sessions_reserve(artalk_model* m, int max_sessions) {
    if (!m || max_sessions <= 0) return ARTALK_EINVAL;
    (void)hipSetDevice(m->device);
    return grow_sessions(m, max_sessions);
}

int artalk_session_count(const artalk_model* m) { return m ? (int)m->sess.open.size() : ARTALK_EINVAL; }

int artalk_session_open(artalk_model* m, int n, const float* style_motion_dev, const uint8_t* has_style, int64_t* ids_out, void* stream) {
    if (!m || n <= 0 || !ids_out) return ARTALK_EINVAL;
    if (!m->finalized) return fail(m, ARTALK_ESTATE, "artalk_session_open before artalk_finalize_weights");
    bool encode_style;
    if (int rc = check_has_style(m, style_motion_dev, has_style, n, &encode_style)) return rc;
    hipStream_t s;
    if (int rc = call_stream(m, stream, &s)) return rc;
    artalk_model::Sessions& ss = m->sess;
    if (int rc = grow_sessions(m, (int64_t)ss.open.size() + n)) return rc;
    if (n > m->ws.maxB || n > m->ws.maxC) { if (int rc = reserve(m, n, n)) return rc; }
    if (int rc = ensure_stage(m, m->ws.maxB, m->ws.maxC)) return rc;
    std::vector<int> slot;
    for (int i = 0; i < (int)ss.owner.size() && (int)slot.size() < n; ++i)
        if (!ss.owner[i]) slot.push_back(i);
    artalk_model::Stage* stg = nullptr;
    if (int rc = next_stage(m, &stg)) return rc;
    if (int rc = stage_session_slots(m, s, stg, slot.data(), n)) return rc;
    m->stream_B = 0; m->stream_scales_ended = false;      // rows 0..n-1 of the workspace are rewritten: a lockstep session ends, as under artalk_infer
    {
        ProfilingOff quiet(m);
        if (int rc = begin_clips(m, s, n, style_motion_dev, has_style, encode_style, stg)) return rc;
        if (int rc = run_init_history(m, n, s)) return rc;
    }
    launch_session_scatter(m->ws.sess_slots, session_rows(m), n, true, s);
    if (int rc = publish_status(m, s)) return rc;
    for (int i = 0; i < n; ++i) {
        ids_out[i] = ss.next_id++;
        ss.owner[slot[i]] = ids_out[i];
        ss.open.emplace(ids_out[i], artalk_model::Sessions::Open{slot[i]});
    }
    return ARTALK_OK;
}

int artalk_session_step(artalk_model* m, const int64_t* ids, int n, const float* audio_dev, int64_t chunk_stride, float* out_motion_dev,
                        int64_t out_stride, uint8_t* out_bits_dev, uint8_t* out_hist_bits_dev, void* stream) {
    if (!m || !ids || n <= 0 || !audio_dev || !out_motion_dev) return ARTALK_EINVAL;
    artalk_model::Sessions& ss = m->sess;
    // every id is checked before anything is enqueued or any session changes
    std::vector<int> slot((size_t)n);
    std::set<int64_t> seen;
    for (int i = 0; i < n; ++i) {
        const auto it = ss.open.find(ids[i]);
        if (it == ss.open.end()) {
            if (ss.ended_by_scales.count(ids[i]))
                return fail(m, ARTALK_ESTATE, "session " + std::to_string(ids[i]) + ": the site scales changed since artalk_session_open; open the session again");
            return fail(m, ARTALK_EINVAL, "artalk_session_step: " + std::to_string(ids[i]) + " is not an open session");
        }
        if (!seen.insert(ids[i]).second) return fail(m, ARTALK_EINVAL, "artalk_session_step: session " + std::to_string(ids[i]) + " is listed twice");
        slot[i] = it->second.slot;
    }
    hipStream_t s;
    if (int rc = call_stream(m, stream, &s)) return rc;
    if (n > m->ws.maxB || n > m->ws.maxC) { if (int rc = reserve(m, n, n)) return rc; }
    Workspace& w = m->ws;
    artalk_model::Stage* stg = nullptr;
    if (int rc = next_stage(m, &stg)) return rc;
    for (int b = 0; b < n; ++b) stg->src[b] = (long)b * chunk_stride;
    HIPCHK(m, hipMemcpyAsync(w.src_off, stg->src, n * sizeof(long), hipMemcpyHostToDevice, s));
    if (int rc = stage_session_slots(m, s, stg, slot.data(), n)) return rc;
    HIPCHK(m, hipEventRecord(stg->done, s));
    stg->used = true;
    m->stream_B = 0; m->stream_scales_ended = false;      // (see artalk_session_open)
    HIPCHK(m, hipMemsetAsync(w.status, 0, 4 * sizeof(int), s));      // every step has a status word, and a ticket, of its own
    const SessionRows rows = session_rows(m);
    ProfilingOff quiet(m);      // restored on every exit path
    launch_session_gather(w.sess_slots, rows, n, s);
    for (int c0 = 0; c0 < n; c0 += w.G) run_wav2vec(m, audio_dev, c0, std::min(w.G, n - c0), nullptr, s);
    // the chunk step of artalk_stream_chunk for n streams: same rows, same graphs; every session has a next chunk
    if (int rc = chunk_step(m, s, 0, n, n, m->tap_maxch, out_motion_dev, out_stride)) return rc;
    launch_session_scatter(w.sess_slots, rows, n, false, s);
    const size_t bits_n = (size_t)n * kNTok * m->cfg.code_dim;
    if (out_bits_dev) HIPCHK(m, hipMemcpyAsync(out_bits_dev, w.bits, bits_n, hipMemcpyDeviceToDevice, s));
    if (out_hist_bits_dev) HIPCHK(m, hipMemcpyAsync(out_hist_bits_dev, w.hist_bits, bits_n, hipMemcpyDeviceToDevice, s));
    if (int rc = publish_status(m, s)) return rc;
    return ARTALK_OK;
}

int artalk_session_close(artalk_model* m, const int64_t* ids, int n) {
    if (!m || !ids || n <= 0) return ARTALK_EINVAL;
    artalk_model::Sessions& ss = m->sess;
    std::set<int64_t> seen;
    for (int i = 0; i < n; ++i)
        if ((!ss.open.count(ids[i]) && !ss.ended_by_scales.count(ids[i])) || !seen.insert(ids[i]).second)
            return fail(m, ARTALK_EINVAL, "artalk_session_close: " + std::to_string(ids[i]) + " is not an open session (or is listed twice)");
    for (int i = 0; i < n; ++i) {
        const auto it = ss.open.find(ids[i]);
        if (it != ss.open.end()) { ss.owner[it->second.slot] = 0; ss.open.erase(it); }
        ss.ended_by_scales.erase(ids[i]);      // a session the scale change closed: only the note is dropped
    }
    return ARTALK_OK;
}

// The Savitzky-Golay filter of artalk_savgol for live sessions (savgol_stream_kernel): row i of raw_dev holds the n_frames[i] codes the last
// artalk_session_step produced for ids[i]; the frames that have become final - everything up to 4 frames behind the newest, or up to the
// end with last[i] - land in row i of out_dev, and first_out / count_out say which they are.  Two small table copies (slot pointers,
// frame counts) through the pinned ring and one launch; no synchronisation, no status word, no workspace row: a lockstep session lives on, and the precision mode plays no part.
int artalk_session_smooth(artalk_model* m, const int64_t* ids, int n, const float* raw_dev, int64_t raw_stride, const int* n_frames,
                          const uint8_t* last, float* out_dev, int64_t out_stride, int* first_out, int* count_out, void* stream) {
    if (!m || !ids || n <= 0 || !out_dev || !first_out || !count_out) return ARTALK_EINVAL;
    artalk_model::Sessions& ss = m->sess;
    // everything is checked before anything is enqueued or any session changes
    std::vector<artalk_model::Sessions::Open*> st;
    std::string err;
    if (int rc = smooth_check(ss, ids, n, raw_dev != nullptr, raw_stride, n_frames, last, out_stride, m->cfg.motion_dim, &st, &err)) return fail(m, rc, err);
    hipStream_t s;
    if (int rc = call_stream(m, stream, &s)) return rc;
    if (n > m->stage_cap_b) { if (int rc = ensure_stage(m, n, m->stage_cap_c)) return rc; }      // pinned tables only: the workspace stays
    artalk_model::Stage* stg = nullptr;
    if (int rc = next_stage(m, &stg)) return rc;
    for (int i = 0; i < n; ++i) {
        stg->slots[i] = m->sess_slot(st[i]->slot);
        stg->smooth[i] = make_int4((int)st[i]->seen, n_frames ? n_frames[i] : 100, last && last[i] ? 1 : 0, 0);
    }
    float** slots_dev = static_cast<float**>(ss.smooth_tab);
    int4* meta_dev = reinterpret_cast<int4*>(slots_dev + ss.smooth_cap);
    HIPCHK(m, hipMemcpyAsync(slots_dev, stg->slots, (size_t)n * sizeof(float*), hipMemcpyHostToDevice, s));
    HIPCHK(m, hipMemcpyAsync(meta_dev, stg->smooth, (size_t)n * sizeof(int4), hipMemcpyHostToDevice, s));
    HIPCHK(m, hipEventRecord(stg->done, s));
    stg->used = true;
    launch_savgol_stream(slots_dev, meta_dev, (long)m->sess_carry_off(), raw_dev, (long)raw_stride, out_dev, (long)out_stride, n,
                         m->cfg.motion_dim, s);
    HIPCHK(m, hipGetLastError());
    for (int i = 0; i < n; ++i) {
        const int nf = n_frames ? n_frames[i] : 100;
        const bool lst = last && last[i];
        smooth_span(st[i]->seen, nf, lst, &first_out[i], &count_out[i]);
        st[i]->seen += nf;
        st[i]->smooth_done = lst;
    }
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
    HIPCHK(m, hipEventSynchronize(m->status_ev[slot]));
    *flags = m->h_status[slot];
    return ARTALK_OK;
}
long long artalk_last_ticket(artalk_model* m) { return m ? m->ticket : -1; }
int artalk_get_status_of(artalk_model* m, long long ticket, int* flags) {
    if (!m || !flags || ticket <= 0 || ticket > m->ticket) return ARTALK_EINVAL;
    if (ticket + artalk_model::kStatusSlots <= m->ticket) { m->err = "artalk_get_status_of: that call's status slot has been reused"; return ARTALK_EINVAL; }
    if (!m->status_pending) { *flags = 0; return ARTALK_OK; }      // the workspace was re-created since: nothing of that call is left
    (void)hipSetDevice(m->device);
    const int slot = (int)((ticket - 1) % artalk_model::kStatusSlots);
    HIPCHK(m, hipEventSynchronize(m->status_ev[slot]));
    *flags = m->h_status[slot];
    return ARTALK_OK;
}
int artalk_poll_status(artalk_model* m, int* flags) {
    if (!m || !flags) return ARTALK_EINVAL;
    if (!m->status_pending) { *flags = 0; return ARTALK_OK; }
    (void)hipSetDevice(m->device);
    const int slot = (int)((m->ticket - 1) % artalk_model::kStatusSlots);
    const hipError_t e = hipEventQuery(m->status_ev[slot]);
    if (e == hipErrorNotReady) return ARTALK_EBUSY;
    if (e != hipSuccess) { m->err = std::string("hipEventQuery: ") + hipGetErrorString(e); return ARTALK_EHIP; }
    *flags = m->h_status[slot];
    return ARTALK_OK;
}

int artalk_get_profile(artalk_model* m, double* out, int n) {
    if (!m || !out || n < 10) return ARTALK_EINVAL;
    if (!m->profiling || m->marks.size() < 2) return fail(m, ARTALK_ESTATE, "profiling was not enabled for the last artalk_infer");
    (void)hipSetDevice(m->device);
    HIPCHK(m, hipStreamSynchronize(m->prof_stream));
    auto ms = [&](size_t a, size_t b) { float t = 0.f; (void)hipEventElapsedTime(&t, m->ev_pool[a], m->ev_pool[b]); return (double)t; };
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
        if (hipEventElapsedTime(&t, m->ktimer.pool[r.second], m->ktimer.pool[r.second + 1]) != hipSuccess) continue;
        const int b = r.first >= 0 && r.first < KB_N ? r.first : KB_OTHER;
        out[b] += t;
        out[KB_N] += 1.0;
    }
    return ARTALK_OK;
}

int artalk_savgol(artalk_model* m, const float* in_dev, float* out_dev, int T, void* stream) {
    if (!m || !in_dev || !out_dev) return ARTALK_EINVAL;
    if (T < 9) return fail(m, ARTALK_EINVAL, "savgol (mode='interp') needs window_length <= T (T >= 9)");
    (void)hipSetDevice(m->device);
    launch_savgol(in_dev, out_dev, T, m->cfg.motion_dim, (hipStream_t)stream);
    return ARTALK_OK;
}

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
    unsigned int* wp = nullptr;
    if (hipMalloc(&wp, (size_t)N * K * 4) != hipSuccess) return ARTALK_EHIP;
    launch_pack_split(W, wp, (long)N * K, true, s);
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = W; g.Wp = wp; g.ldw = K; g.bias = bias; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = act;
    g.force_cfg = force_cfg & 0xff;
    g.a_exp = a_exp; g.status = status_dev;
    unsigned int* ap = nullptr;
    if (force_cfg >= 0 && (force_cfg & 0x100)) {   // tuning: pre-packed A (what a fused producer would hand over)
        if (hipMalloc(&ap, (size_t)M * lda * 4) != hipSuccess) { (void)hipFree(wp); return ARTALK_EHIP; }
        launch_pack_split(A, ap, (long)M * lda, false, s, status_dev, a_exp);
        g.A = reinterpret_cast<const float*>(ap); g.a_packed = 1;
    }
    run_gemm(g, plan_gemm(g, GemmPolicy{1, true}, nullptr), nullptr, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(wp);
    if (ap) (void)hipFree(ap);
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
    void* wb = nullptr;
    float* part = nullptr;
    if (hipMalloc(&wb, (size_t)nb * N * K * 2) != hipSuccess) return ARTALK_EHIP;
    if (S > 1 && hipMalloc(&part, (size_t)S * nb * M * N * 4) != hipSuccess) { (void)hipFree(wb); return ARTALK_EHIP; }
    launch_pack_bf16(W, wb, (long)nb * N * K, s);
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = W; g.Wb = wb; g.ldw = K; g.bias = bias; g.C = C; g.ldc = N; g.gate = gate; g.ldg = N; g.R = R; g.ldr = N;
    g.M = M; g.N = N; g.K = K; g.act = act; g.force_cfg = cfg == 0xff ? -1 : cfg;
    g.batch = nb; g.sA = am ? 64 : (long)M * lda; g.sW = (long)N * K; g.sBias = bias ? N : 0; g.sC = (long)M * N; g.sR = R ? (long)M * N : 0;
    if (am) { g.amode = 1; g.pc_T = T; g.pc_tstride = T; g.pc_pad = K / 64 / 2; g.pc_cin = 64; }
    if (S > 1) {
        if (nb > 1 || am) { (void)hipFree(wb); (void)hipFree(part); return ARTALK_EINVAL; }     // (split-K is a batch-1 plain-window form)
        g.splitk = S; g.partial = part;
    }
    run_gemm(g, plan_gemm(g, GemmPolicy{2}, nullptr), nullptr, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(wb);
    if (part) (void)hipFree(part);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

// split-K scratch of the tuning entry point below (never used by the model path): the current buffer and the ones it outgrew
static float* g_op_scratch = nullptr;
static size_t g_op_scratch_cap = 0;
static std::vector<float*> g_op_retired;
// Frees every scratch buffer of artalk_op_gemm_f16s_packed (current and retired).  The caller guarantees that no captured graph
// that replays such a launch is used afterwards (tools/* destroy their graphs first; pytest calls it at session end).
int artalk_op_release_scratch(void) {
    if (hipDeviceSynchronize() != hipSuccess) return ARTALK_EHIP;
    for (float* p : g_op_retired) (void)hipFree(p);
    g_op_retired.clear();
    if (g_op_scratch) (void)hipFree(g_op_scratch);
    g_op_scratch = nullptr; g_op_scratch_cap = 0;
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
                const size_t need = (size_t)S * M * N * 4;
                if (need > g_op_scratch_cap) {
                    // a smaller scratch is NOT freed here: graphs captured from earlier calls (tools/gemm_f16s_bench.py replays one per
                    // variant) still write to it - freeing it turned their replay into a memory fault.  It is RETIRED instead and freed by
                    // artalk_op_release_scratch(), which the owner of those graphs calls once they are gone.  At least 64 MB, so that it rarely grows.
                    const size_t cap = std::max(need, (size_t)64 << 20);
                    float* fresh = nullptr;
                    if (hipMalloc(&fresh, cap) != hipSuccess) return ARTALK_EHIP;
                    if (g_op_scratch) g_op_retired.push_back(g_op_scratch);
                    g_op_scratch = fresh; g_op_scratch_cap = cap;
                }
                g.splitk = S; g.partial = g_op_scratch;
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
    void* wcopy = nullptr;
    float* part = nullptr;
    if (a->mode != 0 && hipMalloc(&wcopy, (size_t)w_last * (p8 ? 4 : 2)) != hipSuccess) return ARTALK_EHIP;
    if (g.splitk > 1 && hipMalloc(&part, (size_t)g.splitk * M * N * 4) != hipSuccess) { if (wcopy) (void)hipFree(wcopy); return ARTALK_EHIP; }
    g.partial = part;
    if (p8) { launch_pack_split(a->W, (unsigned int*)wcopy, w_last, true, s); g.Wp = (const unsigned int*)wcopy; }
    if (a->mode == 2) { launch_pack_bf16(a->W, wcopy, w_last, s); g.Wb = wcopy; }
    run_gemm(g, plan, &ln, s);
    if (a->ln_Y && !plan.fused_ln) launch_layernorm(ln, s);
    const hipError_t e1 = hipStreamSynchronize(s);
    if (wcopy) (void)hipFree(wcopy);
    if (part) (void)hipFree(part);
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
    long* doff = nullptr;
    if (hipMalloc(&doff, C * sizeof(long)) != hipSuccess) return ARTALK_EHIP;
    (void)hipMemcpy(doff, off.data(), C * sizeof(long), hipMemcpyHostToDevice);
    const int T = (n - 10) / 5 + 1;
    launch_audio_normalize(audio, doff, xnorm_out, C, n, s);
    launch_conv0(xnorm_out, n, w, bias, lnw, lnb, Y, C, T, T, s, out_p8 ? 1 : 0, out_p8 ? status_dev : nullptr, p8_exp);
    (void)hipStreamSynchronize(s);
    (void)hipFree(doff);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_resample_mean(const float* x, int nch, int n, const float* taps, int orig, int nw, int width, float* out, int n_out,
                            void* stream) {
    if (!x || !taps || !out || nch <= 0 || n <= 0 || orig <= 0 || nw <= 0 || width < 0) return ARTALK_EINVAL;
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
    long* doff = nullptr;
    if (hipMalloc(&doff, C * sizeof(long)) != hipSuccess) return ARTALK_EHIP;
    if (hipMemcpy(doff, off.data(), C * sizeof(long), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(doff); return ARTALK_EHIP; }
    launch_audio_normalize(audio, doff, xnorm_out, C, n, s);
    launch_conv0(xnorm_out, n, w, bias, lnw, lnb, Y, C, T, (int)row_stride, s, out_p8 ? 1 : 0, out_p8 ? status_dev : nullptr, p8_exp);
    const hipError_t e1 = hipStreamSynchronize(s);
    (void)hipFree(doff);
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
    void* wcopy = nullptr;
    if (mode != 0 && hipMalloc(&wcopy, (size_t)(H * K) * (mode == 1 ? 4 : 2)) != hipSuccess) return ARTALK_EHIP;
    GemmArgs g;
    g.A = X; g.lda = H; g.W = W; g.ldw = K; g.bias = bias; g.C = C; g.ldc = H; g.R = R; g.ldr = H;
    g.M = (int)M; g.act = act; g.a_exp = a_exp; g.K = (int)K;
    if (mode == 1) {
        launch_pack_split(W, (unsigned int*)wcopy, H * K, true, s);
        g.N = (int)H; g.Wp = (const unsigned int*)wcopy; g.status = status_dev;
        launch_posconv_p8(g, n_chunks, T, Ts, s);
    } else {
        // the grouped GEMM over grid.z of run_wav2vec (amode 1)
        g.amode = 1; g.pc_T = T; g.pc_tstride = Ts; g.pc_pad = taps / 2; g.pc_cin = cg;
        g.N = cg; g.force_cfg = force_cfg;
        g.batch = groups; g.sA = cg; g.sW = (long)cg * K; g.sBias = bias ? cg : 0; g.sC = cg; g.sR = R ? cg : 0;
        if (mode == 2) { launch_pack_bf16(W, wcopy, H * K, s); g.Wb = wcopy; }
        run_gemm(g, plan_gemm(g, GemmPolicy{mode}, nullptr), nullptr, s);
    }
    const hipError_t e1 = hipStreamSynchronize(s);
    if (wcopy) (void)hipFree(wcopy);
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
    int4* dmeta = nullptr;
    if (hipMalloc(&dmeta, (size_t)n * sizeof(int4)) != hipSuccess) return ARTALK_EHIP;
    if (hipMemcpy(dmeta, meta.data(), (size_t)n * sizeof(int4), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dmeta); return ARTALK_EHIP; }
    launch_savgol_stream(slots_dev, dmeta, (long)slot_carry_off(kOpCodeDim), raw, (long)raw_stride, out, (long)out_stride, n, kOpMotionDim, s);
    const hipError_t e1 = hipStreamSynchronize(s);
    (void)hipFree(dmeta);
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

// ---------------------------------------------------------------------------------- FLAME vertices
struct artalk_flame {
    int device = 0, V = 0, NB = 0, NBp = 0, P = 0, Pp = 0, cap = 0;
    float scale = 1.f;
    float *v_template = nullptr, *shapedirs = nullptr, *posedirs = nullptr, *jreg = nullptr, *weights = nullptr;
    int* parents = nullptr;
    float *betas = nullptr, *feat = nullptr, *rot = nullptr, *J = nullptr, *vshaped = nullptr, *vposed = nullptr;
    std::vector<void*> allocs, ws;
    std::string err;
};

static thread_local std::string g_flame_error;
const char* artalk_flame_last_error(const artalk_flame* f) { return f ? f->err.c_str() : g_flame_error.c_str(); }

void artalk_flame_destroy(artalk_flame* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    (void)hipDeviceSynchronize();
    for (void* p : f->allocs) if (p) (void)hipFree(p);
    for (void* p : f->ws) if (p) (void)hipFree(p);
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
    auto up = [&](const float* h, int64_t rows, int64_t cols, int64_t cols_pad) -> float* {
        float* d = dalloc_in<float>(f->allocs, rows * cols_pad);
        if (!d) return nullptr;
        if (cols == cols_pad) { (void)hipMemcpy(d, h, rows * cols * 4, hipMemcpyHostToDevice); }
        else (void)hipMemcpy2D(d, cols_pad * 4, h, cols * 4, cols * 4, rows, hipMemcpyHostToDevice);
        return d;
    };
    f->v_template = up(v_template, 1, (int64_t)V * 3, (int64_t)V * 3);
    f->shapedirs = up(shapedirs, (int64_t)V * 3, NB, f->NBp);       // GEMM weight [N = 3V][K = NB padded]
    f->posedirs = up(posedirs_t, (int64_t)V * 3, P, f->Pp);
    f->jreg = up(J_regressor, 5, V, V);
    f->weights = up(lbs_weights, V, 5, 5);
    f->parents = dalloc_in<int>(f->allocs, 5);
    for (void* p : f->allocs) if (!p) { g_flame_error = "hipMalloc failed"; artalk_flame_destroy(f); return ARTALK_EHIP; }
    (void)hipMemcpy(f->parents, parents, 5 * sizeof(int), hipMemcpyHostToDevice);
    if (hipDeviceSynchronize() != hipSuccess) { g_flame_error = "upload failed"; artalk_flame_destroy(f); return ARTALK_EHIP; }
    *out = f;
    return ARTALK_OK;
}

// betas_dev [T][NB] (shape ++ expression), full_pose_dev [T][15] (global, neck, jaw, eye_l, eye_r axis-angles: FLAME.py:131-136)
// -> out_dev [T][V][3] = vertices * scale
int artalk_flame_verts(artalk_flame* f, const float* betas_dev, const float* full_pose_dev, int T, float* out_dev, void* stream) {
    if (!f || !betas_dev || !full_pose_dev || !out_dev || T <= 0) return ARTALK_EINVAL;
    (void)hipSetDevice(f->device);
    hipStream_t s = (hipStream_t)stream;
    if (T > f->cap) {
        (void)hipDeviceSynchronize();
        for (void* p : f->ws) if (p) (void)hipFree(p);
        f->ws.clear();
        const int64_t N = (int64_t)f->V * 3;
        f->betas = dalloc_in<float>(f->ws, (int64_t)T * f->NBp);
        f->feat = dalloc_in<float>(f->ws, (int64_t)T * f->Pp);
        f->rot = dalloc_in<float>(f->ws, (int64_t)T * 45);
        f->J = dalloc_in<float>(f->ws, (int64_t)T * 15);
        f->vshaped = dalloc_in<float>(f->ws, T * N);
        f->vposed = dalloc_in<float>(f->ws, T * N);
        for (void* p : f->ws) if (!p) { f->err = "hipMalloc failed"; f->cap = 0; return ARTALK_EHIP; }
        (void)hipDeviceSynchronize();   // zero fills run on the null stream
        f->cap = T;
    }
    const int N = f->V * 3;
    // betas into the K-padded GEMM operand (pad columns stay zero from allocation)
    if (hipMemcpy2DAsync(f->betas, (size_t)f->NBp * 4, betas_dev, (size_t)f->NB * 4, (size_t)f->NB * 4, T, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        f->err = "copy failed"; return ARTALK_EHIP;
    }
    GemmArgs g;     // v_shaped = v_template + betas . shapedirs^T      (exact fp32 MFMA)
    g.A = f->betas; g.lda = f->NBp; g.W = f->shapedirs; g.ldw = f->NBp; g.C = f->vshaped; g.ldc = N; g.R = f->v_template; g.ldr = 0;
    g.M = T; g.N = N; g.K = f->NBp;
    launch_gemm(g, s);
    launch_flame_joints(f->vshaped, f->jreg, f->J, T, f->V, s);
    launch_flame_pose(full_pose_dev, f->rot, f->feat, T, f->Pp, s);
    GemmArgs p;     // v_posed = v_shaped + pose_feature . posedirs
    p.A = f->feat; p.lda = f->Pp; p.W = f->posedirs; p.ldw = f->Pp; p.C = f->vposed; p.ldc = N; p.R = f->vshaped; p.ldr = N;
    p.M = T; p.N = N; p.K = f->Pp;
    launch_gemm(p, s);
    launch_flame_skin(f->vposed, f->rot, f->J, f->parents, f->weights, out_dev, T, f->V, f->scale, s);
    if (hipGetLastError() != hipSuccess) { f->err = "kernel launch failed"; return ARTALK_EHIP; }
    return ARTALK_OK;
}

}  // extern "C"
