// The calls of the C ABI that run the path (engine.hip) on a model (model.h): the batch call, style encoding, lockstep streaming, the
// independent sessions with their pool, and the streaming smoother with its host checks.
#include "model.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <set>
#include <string>
#include <vector>

using namespace artalk;

namespace {
// ---------------------------------------------------------------------------------- shared by the batch call and the streaming calls
// device of the model and the stream of this call: the caller's, or the model's own (graph capture needs a real stream)
int call_stream(artalk_model* m, void* stream, hipStream_t* s) {
    (void)hipSetDevice(m->device);
    if (!stream && !m->own_stream.create(hipStreamDefault)) return fail(m, ARTALK_EHIP, "creating the model's own stream failed");
    *s = stream ? (hipStream_t)stream : m->own_stream.get();
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
        DevBuf<float> block;
        if (!block.alloc((size_t)artalk_model::kSessBlock * m->sess_slot_floats())) return fail(m, ARTALK_EHIP, "hipMalloc failed for a block of session slots");
        ss.blocks.emplace_back(std::move(block));      // (the vector may move its owners; the device blocks stay where they are)
        ss.owner.resize(ss.owner.size() + artalk_model::kSessBlock, 0);
    }
    if (ss.smooth_cap < (int64_t)ss.owner.size()) {      // the table of artalk_session_smooth: one row per slot is always enough (freeing the old one waits for the device)
        ss.smooth_cap = 0;
        if (!ss.smooth_tab.alloc(ss.owner.size() * (sizeof(float*) + sizeof(int4)))) return fail(m, ARTALK_EHIP, "hipMalloc failed for the table of artalk_session_smooth");
        ss.smooth_cap = (int64_t)ss.owner.size();
    }
    return ARTALK_OK;
}
// The sessions a call names: (*st)[i] = the state of ids[i], every one open and none listed twice, or the error of the first id that is
// not (`fn`: the calling function, as the messages name it).  Nothing is changed.
int resolve_sessions(artalk_model::Sessions& ss, const char* fn, const int64_t* ids, int n, std::vector<artalk_model::Sessions::Open*>* st,
                     std::string* err) {
    st->assign((size_t)n, nullptr);
    std::set<int64_t> listed;
    for (int i = 0; i < n; ++i) {
        const auto it = ss.open.find(ids[i]);
        if (it == ss.open.end()) {
            if (ss.ended_by_scales.count(ids[i])) {
                *err = "session " + std::to_string(ids[i]) + ": the site scales changed since artalk_session_open; open the session again";
                return ARTALK_ESTATE;
            }
            *err = std::string(fn) + ": " + std::to_string(ids[i]) + " is not an open session";
            return ARTALK_EINVAL;
        }
        if (!listed.insert(ids[i]).second) { *err = std::string(fn) + ": session " + std::to_string(ids[i]) + " is listed twice"; return ARTALK_EINVAL; }
        (*st)[i] = &it->second;
    }
    return ARTALK_OK;
}

}  // namespace

namespace artalk {      // called from other files: declared in model.h
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
    if (int rc = resolve_sessions(ss, "artalk_session_smooth", ids, n, st, err)) return rc;
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
}  // namespace artalk

namespace {
// the device table of this call's slots (row i = slot[i]) through the pinned slot `stg`; the caller records stg->done afterwards
int stage_session_slots(artalk_model* m, hipStream_t s, artalk_model::Stage* stg, const int* slot, int n) {
    for (int i = 0; i < n; ++i) stg->slots.get()[i] = m->sess_slot(slot[i]);
    HIPCHK(m, hipMemcpyAsync(m->ws.sess_slots, stg->slots.get(), (size_t)n * sizeof(float*), hipMemcpyHostToDevice, s));
    return ARTALK_OK;
}

}  // namespace

extern "C" {

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
    long* src = stg->src.get();
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
    for (int b = 0; b < B; ++b) stg->src.get()[b] = (long)b * chunk_stride;
    HIPCHK(m, hipMemcpyAsync(w.src_off, stg->src.get(), B * sizeof(long), hipMemcpyHostToDevice, s));
    HIPCHK(m, hipEventRecord(stg->done.get(), s));
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
    std::vector<artalk_model::Sessions::Open*> st;
    std::string err;
    if (int rc = resolve_sessions(ss, "artalk_session_step", ids, n, &st, &err)) return fail(m, rc, err);
    std::vector<int> slot((size_t)n);
    for (int i = 0; i < n; ++i) slot[i] = st[i]->slot;
    hipStream_t s;
    if (int rc = call_stream(m, stream, &s)) return rc;
    if (n > m->ws.maxB || n > m->ws.maxC) { if (int rc = reserve(m, n, n)) return rc; }
    Workspace& w = m->ws;
    artalk_model::Stage* stg = nullptr;
    if (int rc = next_stage(m, &stg)) return rc;
    for (int b = 0; b < n; ++b) stg->src.get()[b] = (long)b * chunk_stride;
    HIPCHK(m, hipMemcpyAsync(w.src_off, stg->src.get(), n * sizeof(long), hipMemcpyHostToDevice, s));
    if (int rc = stage_session_slots(m, s, stg, slot.data(), n)) return rc;
    HIPCHK(m, hipEventRecord(stg->done.get(), s));
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
        stg->slots.get()[i] = m->sess_slot(st[i]->slot);
        stg->smooth.get()[i] = make_int4((int)st[i]->seen, n_frames ? n_frames[i] : 100, last && last[i] ? 1 : 0, 0);
    }
    float** slots_dev = reinterpret_cast<float**>(ss.smooth_tab.get());
    int4* meta_dev = reinterpret_cast<int4*>(slots_dev + ss.smooth_cap);
    HIPCHK(m, hipMemcpyAsync(slots_dev, stg->slots.get(), (size_t)n * sizeof(float*), hipMemcpyHostToDevice, s));
    HIPCHK(m, hipMemcpyAsync(meta_dev, stg->smooth.get(), (size_t)n * sizeof(int4), hipMemcpyHostToDevice, s));
    HIPCHK(m, hipEventRecord(stg->done.get(), s));
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

int artalk_savgol(artalk_model* m, const float* in_dev, float* out_dev, int T, void* stream) {
    if (!m || !in_dev || !out_dev) return ARTALK_EINVAL;
    if (T < 9) return fail(m, ARTALK_EINVAL, "savgol (mode='interp') needs window_length <= T (T >= 9)");
    (void)hipSetDevice(m->device);
    launch_savgol(in_dev, out_dev, T, m->cfg.motion_dim, (hipStream_t)stream);
    return ARTALK_OK;
}

}  // extern "C"
