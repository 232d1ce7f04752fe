// The model object behind the C ABI (include/artalk_hip.h) - weight table in the reference's key names, derived layouts, workspace -
// and what the files that implement it need from one another:
//   engine.hip   the launch sequence of the audio->motion path
//   model.hip    model lifetime and state: weight registry, workspace and staging ring, site table, settings, status, profile
//   calls.hip    the batch, streaming and session calls
//   ops.hip      the single-kernel entry points of tests and tuning tools (no artalk_model)
// Private to csrc/: what one file alone uses stays in that file's anonymous namespace.
#pragma once
#include "device_mem.h"
#include "kernels.h"
#include "../../include/artalk_hip.h"

#include <rocprofiler-sdk-roctx/roctx.h>

#include <cstdint>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace artalk {

// buckets of the kernel timer (artalk_get_kernel_sums): stages of the path, the scale steps of the body
enum { KB_STYLE = 0, KB_CONV = 1, KB_ENC = 2, KB_ADA = 3, KB_AR_MISC = 4, KB_LEVEL0 = 5, KB_VAE_DEC = 10, KB_REENC = 11, KB_OTHER = 12, KB_N = 13 };
// profile buckets (artalk_get_profile): the interval that ENDS at a mark is charged to the mark's bucket
enum { PB_STYLE = 0, PB_CONV = 1, PB_ENC = 2, PB_ADA = 3, PB_AR = 4, PB_VAE = 5, PB_OTHER = 6 };

constexpr int kSamplesPerChunk = 64000;
constexpr int kE = 768;      // embed dim (app/models.py:19)
constexpr int kCond = 1024;  // audio feature dim (app/models.py:27)
constexpr int kNTok = 181;
constexpr int kMaxLv = 5;
constexpr int kAuditSlots = 1024;      // sites the headroom audit can record (artalk_set_audit)

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

// One per-clip buffer of the workspace: the member (fp32 `f`, or bytes `u8`) and its elements per clip (clip_buffers)
struct ClipBuf { float* Workspace::*f; uint8_t* Workspace::*u8; int64_t n; };

// The conv stack's passes over the chunks of one run_wav2vec call (tail skip): pass p holds n[p] chunks, `off[p]` chunks into the pass
// order, at the geometry of tail_geo[cls[p]] (cls 3: whole chunks).  The chunk table of the pass order and the gather table that
// brings the result back to the call's order (launch_conv_tail_gather) are rows `perm` and `tab` of the device chunk table.
struct ConvPasses { int np = 0; int off[4]{}, n[4]{}, cls[4]{}; const long* perm = nullptr; const long* tab = nullptr; };

// ---- intermediate taps (include/artalk_hip.h: artalk_set_tap) ----
// slot (chunk index j, clip position b) of the tap buffer, fields in floats:
enum { TAP_BLK0_IN = 0, TAP_BLK0_OUT = kNTok * kE, TAP_BLKL_OUT = 2 * kNTok * kE, TAP_PREV_IN = 3 * kNTok * kE,
       TAP_LOGITS = 4 * kNTok * kE, TAP_DEC_OUT = 4 * kNTok * kE + kNTok * 64, TAP_SLOT = 4 * kNTok * kE + kNTok * 64 + 200 * 106 };

// where the smoother's carry starts in a pool slot, in floats: behind [style kE | prev_in kNTok x kE | prev_fdec 100 x code_dim]
constexpr int64_t slot_carry_off(int code_dim) { return kE + (int64_t)kNTok * kE + 100LL * code_dim; }
constexpr int kOpCodeDim = 32, kOpMotionDim = 106;      // the only widths artalk_create accepts: what the model-free entry points assume

}  // namespace artalk

using namespace artalk;      // (private header: every file that includes it implements the library)

struct artalk_model {
    artalk_config cfg{};
    int device = 0;
    std::string err;
    bool finalized = false;
    std::map<std::string, Slot> slots;
    DevPool weights;                // weights and what lives as long: packed and bf16 copies, audit block, initial-history cache
    DevPool ws_pool;                // workspace (re-allocated when a larger batch arrives)
    int64_t weight_bytes = 0;
    struct PackRange { const float* base; int64_t n; unsigned int* packed; uint16_t* bf16; };
    std::vector<PackRange> wranges;   // every weight allocation, its packed f16x3 copy (built at finalize) and its bf16 copy (built on
                                      // the first switch to precision mode 2: ensure_bf16_copy)
    int precision = 0;                // 0: fp32 MFMA everywhere, 1: f16x3 split GEMMs, 2: bf16 GEMMs (heads stay fp32 in 1 and 2)
    bool have_bf16 = false;           // the bf16 weight copy exists
    int splitk_tiles = 192, splitk_target = 384;   // split-K when the grid has fewer tiles than splitk_tiles; aim at splitk_target workgroups
    // headroom audit (artalk_set_audit): max |x| * 16 at every producer of a P8 operand, by site name
    bool audit = false;
    unsigned int* audit_vals = nullptr;            // device (of `weights`), kAuditSlots floats (as bits)
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
        std::vector<DevBuf<float>> blocks;         // device blocks of kSessBlock slots
        std::vector<int64_t> owner;                // per slot: the id of the session that holds it, 0 = free
        // an open session: its slot, and where its streaming smoother stands (artalk_session_smooth): raw frames consumed, and whether
        // a `last` call has emitted the tail.  Born zero with the id, dropped with it: a slot reused under a new id starts clean.
        struct Open { int slot = 0; int64_t seen = 0; bool smooth_done = false; };
        std::map<int64_t, Open> open;              // id -> state
        std::set<int64_t> ended_by_scales;         // ids a change of site scales closed (a step on one says so; artalk_session_close forgets it)
        int64_t next_id = 1;                       // ids are never reused during the model's life
        DevBuf<unsigned char> smooth_tab; int64_t smooth_cap = 0;      // device table of one artalk_session_smooth call: [cap slot pointers | cap int4]
    } sess;
    // slot: [style | prev_in | prev_fdec | smoother carry]; the carry (the last 9 raw frames, padded to 16 bytes) is read and written in
    // place by savgol_stream_kernel and never visits the workspace: SessionRows and the gather / scatter cover the first three fields only
    int64_t sess_carry_off() const { return slot_carry_off(cfg.code_dim); }
    int64_t sess_slot_floats() const { return sess_carry_off() + (kSavgolCarry * (int64_t)cfg.motion_dim + 3) / 4 * 4; }
    float* sess_slot(int i) const { return sess.blocks[i / kSessBlock].get() + (int64_t)(i % kSessBlock) * sess_slot_floats(); }
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
    int profiling = 0;        // 0 off, 1 light (graphs stay on; events around eager launches only), 2 full (graphs off), 3 kernel timer (graphs off, the production clip groups one after the other on one stream, every launch timed: run_body)
    KernelTimer ktimer;       // level 3: per-kernel durations by bucket (artalk_get_kernel_sums)
    bool use_graphs = true;
    bool in_graph_body = false;   // capturing: no events
    bool in_body = false;         // inside run_chunk_body (captured or eager)
    std::vector<Event> ev_pool; size_t ev_used = 0;
    std::vector<std::pair<size_t, double>> dom_events;   // (event index of start, flops)
    std::vector<std::pair<int, size_t>> marks;          // (bucket of the interval ending here, event index), caller's stream
    hipStream_t prof_stream = nullptr;
    Stream side_stream[3];            // extra branches of the AR body (run_body)
    Event fork_ev, join_ev[3];
    int branches = 0;                 // 0 = automatic (2 for B >= 8), else forced 1/2/4
    Stream own_stream;                // used when the caller passes stream == NULL (graph capture needs a real stream)
    // graphs: one per (active batch size, clip group, precision, re-encoded clips), LRU-bounded (run_body)
    struct GraphEntry { GraphExec exec; long long last_use = 0; };
    std::map<long long, GraphEntry> graphs;
    long long graph_clock = 0, graph_captures = 0;
    // Pinned host staging for the small per-call tables (chunk offsets, style flags): a ring of slots, each guarded by an event
    // recorded after its H2D copies, so artalk_infer never has to wait for its own copies (it blocks only if kStageSlots calls
    // are still in flight).  h_status receives the device status word at the end of every call (async), status_ev marks it.
    static constexpr int kStageSlots = 4;
    struct Stage { PinnedBuf<long> src; PinnedBuf<uint8_t> has; PinnedBuf<float*> slots; PinnedBuf<int4> smooth; Event done; bool used = false; };
    Stage stage[kStageSlots];
    int stage_cap_c = 0, stage_cap_b = 0, stage_next = 0;
    // one slot per call in flight (ring of kStatusSlots, indexed by the call's ticket): a caller that keeps several calls queued reads
    // each call's own word (artalk_get_status_of)
    static constexpr int kStatusSlots = 4;
    PinnedBuf<int> h_status; Event status_ev[kStatusSlots]; bool status_pending = false;
    long long ticket = 0;          // number of calls that have published a status word; the last one's ticket is `ticket`, slot (ticket - 1) % kStatusSlots
};

#define HIPCHK(m, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (m)->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            return ARTALK_EHIP;                                                                 \
        }                                                                                       \
    } while (0)

namespace artalk {

inline int fail(artalk_model* m, int code, const std::string& msg) { m->err = msg; return code; }
// the streaming / style-encode entry points run without stage events; the level comes back on every exit path
struct ProfilingOff {
    artalk_model* m; int saved;
    explicit ProfilingOff(artalk_model* x) : m(x), saved(x->profiling) { m->profiling = 0; }
    ~ProfilingOff() { m->profiling = saved; }
    ProfilingOff(const ProfilingOff&) = delete;
    ProfilingOff& operator=(const ProfilingOff&) = delete;
};

template <typename T>
T* dalloc(artalk_model* m, int64_t n) { return m->weights.take<T>(n); }

// ---- the functions that cross a file boundary, by the file that defines them
// engine.hip: the stages of the path and the chunk step (calls.hip runs them)
void stage_mark(artalk_model* m, hipStream_t s, int bucket);
void run_wav2vec(artalk_model* m, const float* audio, int c0, int n, float* out_w2v, hipStream_t s, const ConvPasses* tail = nullptr);
void run_style(artalk_model* m, const float* style_motion, int B, hipStream_t s, bool encode = true);
int run_init_history(artalk_model* m, int B, hipStream_t s);
int begin_clips(artalk_model* m, hipStream_t s, int B, const float* style_motion_dev, const uint8_t* has_style, bool encode_style,
                artalk_model::Stage* stg);
int chunk_step(artalk_model* m, hipStream_t s, int cond_row0, int Bn, int n_next, int tap_chunk, float* out_motion_dev, int64_t out_stride);
// model.hip: the weight copies a GEMM reads (engine.hip), workspace, staging ring and status word (calls.hip), per-clip extents (engine.hip)
const unsigned int* packed_of(const artalk_model* m, const float* w);
const void* bf16_of(const artalk_model* m, const float* w);
int ensure_stage(artalk_model* m, int maxB, int maxC);
int next_stage(artalk_model* m, artalk_model::Stage** out);
int publish_status(artalk_model* m, hipStream_t s);
std::vector<ClipBuf> clip_buffers(const artalk_model* m);
int reserve(artalk_model* m, int maxB, int maxC);
// calls.hip: the smoother's host checks (ops.hip exposes them to the CPU tests)
void smooth_span(int64_t seen, int nf, bool last, int* first, int* count);
int smooth_row_range(const std::string& who, int nf, bool last, std::string* err);
int smooth_row_length(const std::string& who, int64_t seen, int nf, bool last, std::string* err);
int smooth_stride_check(const char* fn, bool have_raw, bool need_raw, int64_t raw_stride, int64_t out_stride, int D, std::string* err);
int smooth_check(artalk_model::Sessions& ss, const int64_t* ids, int n, bool have_raw, int64_t raw_stride, const int* n_frames,
                 const uint8_t* last, int64_t out_stride, int D, std::vector<artalk_model::Sessions::Open*>* st, std::string* err);

}  // namespace artalk
