// Live audio in ("Live audio in"): raw PCM packets -> the model's 16 kHz mono blocks, per stream, on the device.
//
//   pcm_push_kernel   one launch for the packets of any number of streams (one descriptor a packet, any mix of rates): the streaming form
//                     of resample_mean_kernel (w2v_front.hip).  Output i = j nw + p of a stream is
//                         s = fmaf(taps[p][k], x_c[j orig - width + k], s), k ascending, indices outside the signal skipped;
//                         acc += s over the channels in order; acc / (float)nch
//                     - the same operations in the same order as the whole-clip kernel, so the same bits whatever the packet sizes.
//   pcm_take_kernel   the oldest `block` samples of each listed ring -> row i of an (n, block) tensor, zero past the last real sample.
//
// A descriptor speaks of its SPAN: the frames the stream still holds (its carry: every frame from j_next orig - width on, fewer than
// ntaps a channel) followed by the packet's frames.  Span frame v stands for signal frame v + j_next orig - width, so group g of the
// launch reads span frames g orig .. g orig + ntaps - 1; v < lead are frames before the signal's first (skipped), v >= lead + carry_n
// + frames are frames that have not arrived (never read by a push, which emits final groups only; skipped by the end).
// A workgroup takes a tile of tile_groups groups of one packet, stages the span frames they read into LDS once - de-interleaved, converted
// to float - and computes the tile's outputs from there; taps come from global memory (L1 / L2: 41 taps at 48 kHz, 76 000 at 44.1 kHz).
// The packet's last tile writes the new carry, from global memory, into the OTHER carry buffer of the stream: no tile reads what
// another writes.  No atomics, no reductions: bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "artalk_hip.h"
#include "device_mem.h"
#include "kernels.h"

namespace artalk {

namespace {

constexpr int kPcmLds = 12288;          // floats of LDS a tile stages into (48 KB); 8 channels x 1024 taps fit with one group a tile
constexpr int kPcmThreads = 256;
constexpr int64_t kPcmMaxTapTable = 1 << 24;      // artalk_amd.audio.MAX_TAP_TABLE

// span frame v (lead <= v < lead + carry_n + frames) of channel c, as float
__device__ __forceinline__ float pcm_span_frame(const artalk_pcm_desc& d, int v, int c) {
    const int r = v - d.lead;
    if (r < d.carry_n) return d.carry_in[(long)c * d.carry_stride + r];
    const long e = (long)(r - d.carry_n) * d.nch + c;
    if (d.format == ARTALK_PCM_S16) return (float)static_cast<const int16_t*>(d.data)[e] * (1.0f / 32768.0f);      // exact, = / 32768
    return static_cast<const float*>(d.data)[e];
}

__global__ __launch_bounds__(kPcmThreads) void pcm_push_kernel(const artalk_pcm_desc* __restrict__ descs) {
    __shared__ float lds[kPcmLds];
    const artalk_pcm_desc d = descs[blockIdx.y];
    const int tile = blockIdx.x;
    if (tile >= d.n_tiles) return;
    const int ntaps = 2 * d.width + d.orig, nch = d.nch;
    const int V = d.lead + d.carry_n + d.frames;                       // end of the span: frames that have arrived
    const int o0 = min(d.n_out, tile * d.tile_groups * d.nw), o1 = min(d.n_out, o0 + d.tile_groups * d.nw);
    // the span frames this tile's groups read, clipped to what exists: [s0, s1)
    int s0 = 0, s1 = 0;
    if (o1 > o0) {
        s0 = max((o0 / d.nw) * d.orig, d.lead);
        s1 = min(((o1 - 1) / d.nw) * d.orig + ntaps, V);
        if (s1 < s0) s1 = s0;
    }
    const int span = s1 - s0;                                          // <= (tile_groups - 1) orig + ntaps: nch x span fits the LDS block
    for (int idx = threadIdx.x; idx < span * nch; idx += kPcmThreads) {      // in the packet's order: neighbouring lanes, neighbouring samples
        const int f = idx / nch, c = idx - f * nch;
        lds[c * span + f] = pcm_span_frame(d, s0 + f, c);
    }
    __syncthreads();
    for (int o = o0 + threadIdx.x; o < o1; o += kPcmThreads) {
        const int j = o / d.nw, p = o - j * d.nw;
        const float* tp = d.taps + (long)p * ntaps;
        const int base = j * d.orig;
        const int k0 = max(0, s0 - base), k1 = min(ntaps, s1 - base);  // the terms whose frame exists, in ascending k
        float acc = 0.f;
        for (int c = 0; c < nch; ++c) {
            const float* xc = lds + c * span + (base - s0);
            float s = 0.f;
            for (int k = k0; k < k1; ++k) s = fmaf(tp[k], xc[k], s);
            acc += s;
        }
        int pos = d.ring_pos + o;
        if (pos >= d.ring_cap) pos -= d.ring_cap;
        d.ring[pos] = acc / (float)nch;
    }
    if (tile == d.n_tiles - 1) {
        for (int idx = threadIdx.x; idx < d.carry_out_n * nch; idx += kPcmThreads) {
            const int f = idx / nch, c = idx - f * nch;
            d.carry_out[(long)c * d.carry_stride + f] = pcm_span_frame(d, d.carry_from + f, c);
        }
    }
}

__global__ __launch_bounds__(kPcmThreads) void pcm_take_kernel(const artalk_pcm_take_desc* __restrict__ descs, float* __restrict__ out,
                                                                long out_stride, int block) {
    const artalk_pcm_take_desc d = descs[blockIdx.y];
    const int i = blockIdx.x * kPcmThreads + threadIdx.x;
    if (i >= block) return;
    float v = 0.f;
    if (i < d.n_valid) {
        int pos = d.read_pos + i;
        if (pos >= d.ring_cap) pos -= d.ring_cap;
        v = d.ring[pos];
    }
    out[(long)blockIdx.y * out_stride + i] = v;
}

// ---- host arithmetic --------------------------------------------------------------------------------------------------------------
int64_t pcm_final_groups(int64_t n_in, int orig, int width) { return n_in < width ? 0 : (n_in - width) / orig; }

struct PcmPlan { int64_t n_out, lead, carry_n, carry_from, carry_out_n, groups; };

// what a push of `frames` frames (end: the end of the signal) does to a stream that has taken n_before frames
PcmPlan pcm_plan(int64_t n_before, int64_t frames, bool end, int orig, int nw, int width) {
    PcmPlan q;
    const int64_t j0 = pcm_final_groups(n_before, orig, width);
    const int64_t a0 = j0 * orig - width;                              // the signal's frame that span frame 0 stands for
    q.lead = a0 < 0 ? -a0 : 0;
    q.carry_n = n_before - (a0 < 0 ? 0 : a0);
    if (end) {
        const int64_t total = (n_before * nw + orig - 1) / orig;
        q.n_out = total - j0 * nw;
        q.groups = (q.n_out + nw - 1) / nw;
        q.carry_from = q.lead; q.carry_out_n = 0;
        return q;
    }
    const int64_t n_after = n_before + frames, j1 = pcm_final_groups(n_after, orig, width);
    q.groups = j1 - j0;
    q.n_out = q.groups * nw;
    const int64_t a1 = j1 * orig - width, keep = a1 < 0 ? 0 : a1;
    q.carry_from = keep - a0;
    q.carry_out_n = n_after - keep;
    return q;
}

int pcm_rate_check(int orig, int nw, int width, std::string* err) {
    if (orig < 1 || nw < 1 || width < 0) { *err = "orig and new must be positive, width not negative"; return ARTALK_EINVAL; }
    const int64_t ntaps = 2 * (int64_t)width + orig;
    if (ntaps > ARTALK_PCM_MAX_TAPS) {
        *err = "the ratio " + std::to_string(orig) + ":" + std::to_string(nw) + " has " + std::to_string(ntaps) + " taps a phase (limit " +
               std::to_string(ARTALK_PCM_MAX_TAPS) + "); resample to a rate with a larger common divisor first";
        return ARTALK_EINVAL;
    }
    if (nw * ntaps > kPcmMaxTapTable) { *err = "the tap table has more than 2^24 elements"; return ARTALK_EINVAL; }
    return ARTALK_OK;
}

int pcm_format_bytes(int format) { return format == ARTALK_PCM_S16 ? 2 : format == ARTALK_PCM_F32 ? 4 : 0; }

// checks one descriptor and fills tile_groups / n_tiles.  Everything the kernel indexes with is bounded here.  (pointers = false: a
// handle without a device, whose descriptors hold no addresses)
int pcm_desc_check(artalk_pcm_desc* d, std::string* err, bool pointers = true) {
    const int rc = pcm_rate_check(d->orig, d->nw, d->width, err);
    if (rc != ARTALK_OK) return rc;
    const int ntaps = 2 * d->width + d->orig;
    if (d->nch < 1 || d->nch > ARTALK_PCM_MAX_CHANNELS) { *err = "channels must be in 1..8"; return ARTALK_EINVAL; }
    const int eb = pcm_format_bytes(d->format);
    if (!eb) { *err = "unknown sample format " + std::to_string(d->format) + " (ARTALK_PCM_S16 = 1, ARTALK_PCM_F32 = 2)"; return ARTALK_EINVAL; }
    if (d->frames < 0 || (int64_t)d->frames * d->nch > (1 << 30)) { *err = "a packet holds 0 .. 2^30 samples"; return ARTALK_EINVAL; }
    if (pointers && !d->taps) { *err = "taps must not be NULL"; return ARTALK_EINVAL; }
    if (pointers && d->frames > 0 && (!d->data || (uintptr_t)d->data % eb)) { *err = "a packet must not be NULL and must be aligned to its samples"; return ARTALK_EINVAL; }
    if (d->lead < 0 || d->lead > d->width) { *err = "lead must be in 0..width"; return ARTALK_EINVAL; }
    if (d->carry_stride < 0 || d->carry_n < 0 || d->carry_n >= ntaps || d->carry_n > d->carry_stride || (pointers && d->carry_n > 0 && !d->carry_in)) {
        *err = "the carry in holds fewer than ntaps frames, within its stride"; return ARTALK_EINVAL;
    }
    const int64_t V = (int64_t)d->lead + d->carry_n + d->frames;
    if (d->carry_out_n < 0 || d->carry_out_n >= ntaps || d->carry_out_n > d->carry_stride || (pointers && d->carry_out_n > 0 && !d->carry_out) ||
        d->carry_from < d->lead || (int64_t)d->carry_from + d->carry_out_n > V) {
        *err = "the carry out holds fewer than ntaps frames of the span, within its stride"; return ARTALK_EINVAL;
    }
    if (d->ring_cap < 1 || d->ring_cap > (1 << 30) || d->ring_pos < 0 || d->ring_pos >= d->ring_cap || d->n_out < 0 || d->n_out > d->ring_cap ||
        (pointers && d->n_out > 0 && !d->ring)) {
        *err = "the outputs must fit the ring"; return ARTALK_EINVAL;
    }
    const int64_t groups = ((int64_t)d->n_out + d->nw - 1) / d->nw;
    if (groups * d->orig > (1 << 30)) { *err = "the launch's groups reach past 2^30 frames"; return ARTALK_EINVAL; }
    int g = (kPcmLds / d->nch - ntaps) / d->orig + 1;                  // nch ((g - 1) orig + ntaps) <= kPcmLds
    g = std::min(g, std::max(1, kPcmThreads / d->nw));
    d->tile_groups = g;
    d->n_tiles = (int)std::max<int64_t>(1, (groups + g - 1) / g);
    return ARTALK_OK;
}

void launch_pcm_push(const artalk_pcm_desc* table_dev, int n, int max_tiles, hipStream_t s) {
    ARTALK_LAUNCH(pcm_push_kernel, dim3(max_tiles, n), dim3(kPcmThreads), 0, s, table_dev);
}

void launch_pcm_take(const artalk_pcm_take_desc* table_dev, int n, float* out, int64_t out_stride, int block, hipStream_t s) {
    ARTALK_LAUNCH(pcm_take_kernel, dim3((block + kPcmThreads - 1) / kPcmThreads, n), dim3(kPcmThreads), 0, s, table_dev, out, (long)out_stride, block);
}

int pcm_take_desc_check(const artalk_pcm_take_desc* d, int block, std::string* err, bool pointers = true) {
    if ((pointers && !d->ring) || d->ring_cap < 1 || d->ring_cap > (1 << 30) || d->read_pos < 0 || d->read_pos >= d->ring_cap || d->n_valid < 0 ||
        d->n_valid > block || d->n_valid > d->ring_cap) {
        *err = "a take reads 0 .. block samples of a ring, from a position inside it"; return ARTALK_EINVAL;
    }
    return ARTALK_OK;
}

}  // namespace

struct PcmRate {
    int sample_rate = 0, orig = 1, nw = 1, width = 0;
    DevBuf<float> taps;
};

struct PcmStream {
    int64_t id = -1;                    // -1: the slot is free
    const PcmRate* rate = nullptr;
    int nch = 1, format = ARTALK_PCM_S16;
    int64_t n_in = 0, written = 0, taken = 0;
    bool ended = false;
    int cur = 0;                        // the carry buffer the next launch reads
};

}  // namespace artalk

using namespace artalk;

struct artalk_pcm {
    int device = 0;                                     // ARTALK_PCM_NO_DEVICE: every call checks and counts, nothing is allocated or enqueued
    bool dry() const { return device == ARTALK_PCM_NO_DEVICE; }
    int block = 0, ring_blocks = 0, max_streams = 0;
    int64_t cap = 0;                                    // samples of one ring
    DevBuf<float> ring, carry;                          // [max_streams][cap]; [max_streams][2][8][ARTALK_PCM_MAX_TAPS]
    std::vector<PcmStream> slots;
    std::unordered_map<int64_t, int> by_id;
    int64_t next_id = 1;
    std::vector<std::unique_ptr<PcmRate>> rates;
    PinnedBuf<uint8_t> pin[2];                          // descriptor table, then the call's host packets
    Event ev[2];
    bool in_flight[2] = {false, false};
    int next_pin = 0;
    DevBuf<uint8_t> stage;                              // where the staged bytes land; read by the launch that follows the copy
    std::string err;

    // (a handle without a device has no buffers: its descriptors hold no addresses)
    float* ring_of(int slot) { return dry() ? nullptr : ring.get() + (int64_t)slot * cap; }
    float* carry_of(int slot, int which) {
        return dry() ? nullptr : carry.get() + ((int64_t)slot * 2 + which) * ARTALK_PCM_MAX_CHANNELS * ARTALK_PCM_MAX_TAPS;
    }
};

namespace {

thread_local std::string g_pcm_error;

int fail(artalk_pcm* p, int rc, const std::string& msg) { p->err = msg; return rc; }

// resolves ids to slots; refuses an unknown or closed id and an id listed twice
int pcm_resolve(artalk_pcm* p, const int64_t* ids, int n, std::vector<int>* slots) {
    if (n < 1 || !ids) return fail(p, ARTALK_EINVAL, "a call lists at least one stream");
    slots->clear();
    for (int i = 0; i < n; ++i) {
        const auto it = p->by_id.find(ids[i]);
        if (it == p->by_id.end()) return fail(p, ARTALK_EINVAL, "stream " + std::to_string(ids[i]) + " is not open (unknown or closed)");
        if (std::find(slots->begin(), slots->end(), it->second) != slots->end())
            return fail(p, ARTALK_EINVAL, "stream " + std::to_string(ids[i]) + " is listed twice");
        slots->push_back(it->second);
    }
    return ARTALK_OK;
}

// a free pinned staging buffer of `bytes` (waits at most for that buffer's own last copy); null: the runtime refused
uint8_t* pcm_stage_begin(artalk_pcm* p, size_t bytes, int* which, hipStream_t s) {
    const int k = p->next_pin;
    if (p->in_flight[k]) { (void)hipEventSynchronize(p->ev[k].get()); p->in_flight[k] = false; }
    if (p->pin[k].capacity() < bytes && !p->pin[k].alloc(bytes + bytes / 2)) return nullptr;
    if (!p->stage.grow(bytes, 1, 2, s)) return nullptr;
    if (!p->ev[k].create()) return nullptr;
    *which = k;
    return p->pin[k].get();
}

bool pcm_stage_commit(artalk_pcm* p, int k, size_t bytes, hipStream_t s) {
    if (hipMemcpyAsync(p->stage.get(), p->pin[k].get(), bytes, hipMemcpyHostToDevice, s) != hipSuccess) { (void)hipGetLastError(); return false; }
    (void)hipEventRecord(p->ev[k].get(), s);
    p->in_flight[k] = true;
    p->next_pin = k ^ 1;
    return true;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
alignas(16) const unsigned char kAligned[16] = {0};

// push (data != null) or end (data == null) of the listed streams: one staging copy, one launch
int pcm_push_or_end(artalk_pcm* p, const int64_t* ids, int n, const void* const* data, const int64_t* frames, bool on_device, hipStream_t s) {
    const bool end = data == nullptr;
    std::vector<int> slots;
    int rc = pcm_resolve(p, ids, n, &slots);
    if (rc != ARTALK_OK) return rc;
    if (!end && !frames) return fail(p, ARTALK_EINVAL, "frames must not be NULL");
    std::vector<artalk_pcm_desc> descs((size_t)n);
    std::vector<PcmPlan> plans((size_t)n);
    size_t bytes = align16((size_t)n * sizeof(artalk_pcm_desc));
    std::vector<size_t> at((size_t)n, 0);
    int max_tiles = 1;
    for (int i = 0; i < n; ++i) {
        PcmStream& st = p->slots[slots[i]];
        const std::string who = "stream " + std::to_string(st.id);
        if (st.ended) return fail(p, ARTALK_ESTATE, who + " has ended: " + (end ? "it ends once" : "no push after end"));
        const int64_t fr = end ? 0 : frames[i];
        if (fr < 0 || fr * st.nch > (1 << 30)) return fail(p, ARTALK_EINVAL, who + ": a packet holds 0 .. 2^30 samples");
        if (fr > 0 && !data[i]) return fail(p, ARTALK_EINVAL, who + ": the packet is NULL");
        const PcmRate& r = *st.rate;
        const PcmPlan q = plans[i] = pcm_plan(st.n_in, fr, end, r.orig, r.nw, r.width);
        const int64_t free_space = p->cap - (st.written - st.taken);
        if (q.n_out > free_space)
            return fail(p, ARTALK_ECAPACITY, who + ": " + std::to_string(q.n_out) + " new samples do not fit the ring's free space (" +
                                                 std::to_string(free_space) + "); take a block first");
        artalk_pcm_desc& d = descs[i];
        std::memset(&d, 0, sizeof(d));
        d.taps = r.taps.get();
        d.orig = r.orig; d.nw = r.nw; d.width = r.width; d.nch = st.nch; d.format = st.format; d.frames = (int32_t)fr;
        d.lead = (int32_t)q.lead; d.carry_n = (int32_t)q.carry_n; d.carry_from = (int32_t)q.carry_from; d.carry_out_n = (int32_t)q.carry_out_n;
        d.carry_stride = ARTALK_PCM_MAX_TAPS;
        d.carry_in = p->carry_of(slots[i], st.cur); d.carry_out = p->carry_of(slots[i], st.cur ^ 1);
        d.ring = p->ring_of(slots[i]); d.ring_cap = (int32_t)p->cap; d.ring_pos = (int32_t)(st.written % p->cap); d.n_out = (int32_t)q.n_out;
        if (fr > 0 && !on_device) {      // a host packet: its place in the staging buffer, and for the check a stand-in address
            at[i] = bytes; bytes += align16((size_t)fr * st.nch * pcm_format_bytes(st.format));
            d.data = kAligned;
        } else {
            d.data = fr > 0 ? data[i] : nullptr;
        }
        rc = pcm_desc_check(&d, &p->err, !p->dry());
        if (rc != ARTALK_OK) return rc;
        max_tiles = std::max(max_tiles, d.n_tiles);
    }
    // checked whole; from here on the call enqueues
    if (!p->dry()) {
        DeviceGuard guard(p->device);
        int k = 0;
        uint8_t* host = pcm_stage_begin(p, bytes, &k, s);
        if (!host) return fail(p, ARTALK_EHIP, "no staging memory for the call");
        for (int i = 0; i < n; ++i) {
            if (at[i]) {
                std::memcpy(host + at[i], data[i], (size_t)descs[i].frames * descs[i].nch * pcm_format_bytes(descs[i].format));
                descs[i].data = p->stage.get() + at[i];
            }
        }
        std::memcpy(host, descs.data(), (size_t)n * sizeof(artalk_pcm_desc));
        if (!pcm_stage_commit(p, k, bytes, s)) return fail(p, ARTALK_EHIP, "the staging copy failed");
        launch_pcm_push(reinterpret_cast<const artalk_pcm_desc*>(p->stage.get()), n, max_tiles, s);
        if (hipGetLastError() != hipSuccess) return fail(p, ARTALK_EHIP, "the launch failed");
    }
    for (int i = 0; i < n; ++i) {
        PcmStream& st = p->slots[slots[i]];
        st.n_in += descs[i].frames;
        st.written += plans[i].n_out;
        st.cur ^= 1;
        if (end) st.ended = true;
    }
    return ARTALK_OK;
}

}  // namespace

extern "C" {

const char* artalk_pcm_last_error(artalk_pcm* p) { return p ? p->err.c_str() : g_pcm_error.c_str(); }

int artalk_pcm_create(int device, int block, int ring_blocks, int max_streams, artalk_pcm** out) {
    if (!out) { g_pcm_error = "out must not be NULL"; return ARTALK_EINVAL; }
    *out = nullptr;
    if (device < ARTALK_PCM_NO_DEVICE || block < 1 || ring_blocks < 2 || max_streams < 1 || max_streams > 4096 || (int64_t)block * ring_blocks >= (1 << 30)) {
        g_pcm_error = "artalk_pcm_create needs block >= 1, ring_blocks >= 2, max_streams in 1..4096 and a ring below 2^30 samples";
        return ARTALK_EINVAL;
    }
    std::unique_ptr<artalk_pcm> p(new artalk_pcm);
    p->device = device; p->block = block; p->ring_blocks = ring_blocks; p->max_streams = max_streams;
    p->cap = (int64_t)block * ring_blocks;
    p->slots.resize((size_t)max_streams);
    if (p->dry()) { *out = p.release(); return ARTALK_OK; }
    DeviceGuard guard(device);
    const size_t stage0 = (size_t)max_streams * (sizeof(artalk_pcm_desc) + 8192) + 4096;      // a 20 ms packet of 48 kHz stereo s16 is 3840 bytes
    if (!p->ring.alloc((size_t)max_streams * p->cap) ||
        !p->carry.alloc_zero((size_t)max_streams * 2 * ARTALK_PCM_MAX_CHANNELS * ARTALK_PCM_MAX_TAPS) || !p->stage.alloc(stage0) ||
        !p->pin[0].alloc(stage0) || !p->pin[1].alloc(stage0) || !p->ev[0].create() || !p->ev[1].create()) {
        g_pcm_error = "artalk_pcm_create: the device refused the rings or the staging buffers";
        return ARTALK_EHIP;
    }
    *out = p.release();
    return ARTALK_OK;
}

void artalk_pcm_destroy(artalk_pcm* p) {
    if (!p) return;
    if (p->dry()) { delete p; return; }
    DeviceGuard guard(p->device);
    for (int k = 0; k < 2; ++k)
        if (p->in_flight[k]) (void)hipEventSynchronize(p->ev[k].get());
    delete p;
}

int artalk_pcm_set_rate(artalk_pcm* p, int sample_rate, const float* taps_host, int orig, int nw, int width) {
    if (!p) { g_pcm_error = "the handle is NULL"; return ARTALK_EINVAL; }
    if (sample_rate < 1 || !taps_host) return fail(p, ARTALK_EINVAL, "a rate needs a positive sample rate and its tap table");
    const int rc = pcm_rate_check(orig, nw, width, &p->err);
    if (rc != ARTALK_OK) return rc;
    for (const auto& r : p->rates)
        if (r->sample_rate == sample_rate) {
            if (r->orig == orig && r->nw == nw && r->width == width) return ARTALK_OK;
            return fail(p, ARTALK_EINVAL, "rate " + std::to_string(sample_rate) + " was set before with another geometry");
        }
    std::unique_ptr<PcmRate> r(new PcmRate);
    r->sample_rate = sample_rate; r->orig = orig; r->nw = nw; r->width = width;
    if (p->dry()) { p->rates.push_back(std::move(r)); return ARTALK_OK; }
    DeviceGuard guard(p->device);
    if (!r->taps.upload(taps_host, (size_t)nw * (2 * (size_t)width + orig))) { (void)hipGetLastError(); return fail(p, ARTALK_EHIP, "the tap table could not be uploaded"); }
    p->rates.push_back(std::move(r));
    return ARTALK_OK;
}

int artalk_pcm_open(artalk_pcm* p, int sample_rate, int channels, int format, int64_t* id_out) {
    if (!p) { g_pcm_error = "the handle is NULL"; return ARTALK_EINVAL; }
    if (!id_out) return fail(p, ARTALK_EINVAL, "id_out must not be NULL");
    if (channels < 1 || channels > ARTALK_PCM_MAX_CHANNELS) return fail(p, ARTALK_EINVAL, "channels must be in 1..8 (got " + std::to_string(channels) + ")");
    if (!pcm_format_bytes(format)) return fail(p, ARTALK_EINVAL, "unknown sample format " + std::to_string(format) + " (ARTALK_PCM_S16 = 1, ARTALK_PCM_F32 = 2)");
    const PcmRate* rate = nullptr;
    for (const auto& r : p->rates)
        if (r->sample_rate == sample_rate) rate = r.get();
    if (!rate) return fail(p, ARTALK_EINVAL, "rate " + std::to_string(sample_rate) + " has no tap table yet (artalk_pcm_set_rate)");
    for (int i = 0; i < p->max_streams; ++i) {
        if (p->slots[i].id >= 0) continue;
        PcmStream st;
        st.id = p->next_id++; st.rate = rate; st.nch = channels; st.format = format;
        p->slots[i] = st;
        p->by_id[st.id] = i;
        *id_out = st.id;
        return ARTALK_OK;
    }
    return fail(p, ARTALK_ECAPACITY, "all " + std::to_string(p->max_streams) + " streams are open");
}

int artalk_pcm_close(artalk_pcm* p, int64_t id) {
    if (!p) { g_pcm_error = "the handle is NULL"; return ARTALK_EINVAL; }
    const auto it = p->by_id.find(id);
    if (it == p->by_id.end()) return fail(p, ARTALK_EINVAL, "stream " + std::to_string(id) + " is not open (unknown or closed)");
    p->slots[it->second] = PcmStream();
    p->by_id.erase(it);
    return ARTALK_OK;
}

int artalk_pcm_push(artalk_pcm* p, const int64_t* ids, int n, const void* const* data, const int64_t* frames, int on_device, void* stream) {
    if (!p) { g_pcm_error = "the handle is NULL"; return ARTALK_EINVAL; }
    if (!data) return fail(p, ARTALK_EINVAL, "data must not be NULL");
    return pcm_push_or_end(p, ids, n, data, frames, on_device != 0, (hipStream_t)stream);
}

int artalk_pcm_end(artalk_pcm* p, const int64_t* ids, int n, void* stream) {
    if (!p) { g_pcm_error = "the handle is NULL"; return ARTALK_EINVAL; }
    return pcm_push_or_end(p, ids, n, nullptr, nullptr, false, (hipStream_t)stream);
}

int artalk_pcm_available(artalk_pcm* p, int64_t id, int64_t* samples, int* ended) {
    if (!p) { g_pcm_error = "the handle is NULL"; return ARTALK_EINVAL; }
    const auto it = p->by_id.find(id);
    if (it == p->by_id.end()) return fail(p, ARTALK_EINVAL, "stream " + std::to_string(id) + " is not open (unknown or closed)");
    const PcmStream& st = p->slots[it->second];
    if (samples) *samples = st.written - st.taken;
    if (ended) *ended = st.ended ? 1 : 0;
    return ARTALK_OK;
}

int artalk_pcm_take(artalk_pcm* p, const int64_t* ids, int n, float* out_dev, int64_t out_stride, int64_t* n_valid_host, void* stream) {
    if (!p) { g_pcm_error = "the handle is NULL"; return ARTALK_EINVAL; }
    std::vector<int> slots;
    int rc = pcm_resolve(p, ids, n, &slots);
    if (rc != ARTALK_OK) return rc;
    if ((!out_dev && !p->dry()) || !n_valid_host || out_stride < p->block) return fail(p, ARTALK_EINVAL, "take needs out, n_valid and a row stride of a block or more");
    std::vector<artalk_pcm_take_desc> descs((size_t)n);
    for (int i = 0; i < n; ++i) {
        const PcmStream& st = p->slots[slots[i]];
        const int64_t have = st.written - st.taken;
        if (have < p->block && !(st.ended && have >= 1))
            return fail(p, ARTALK_ESTATE, "stream " + std::to_string(st.id) + " holds " + std::to_string(have) + " samples: neither a block of " +
                                              std::to_string(p->block) + " nor the rest of an ended stream");
        descs[i].ring = p->ring_of(slots[i]); descs[i].ring_cap = (int32_t)p->cap; descs[i].read_pos = (int32_t)(st.taken % p->cap);
        descs[i].n_valid = (int32_t)std::min<int64_t>(have, p->block); descs[i].reserved = 0;
        rc = pcm_take_desc_check(&descs[i], p->block, &p->err, !p->dry());
        if (rc != ARTALK_OK) return rc;
    }
    if (!p->dry()) {
        hipStream_t s = (hipStream_t)stream;
        DeviceGuard guard(p->device);
        const size_t bytes = (size_t)n * sizeof(artalk_pcm_take_desc);
        int k = 0;
        uint8_t* host = pcm_stage_begin(p, bytes, &k, s);
        if (!host) return fail(p, ARTALK_EHIP, "no staging memory for the call");
        std::memcpy(host, descs.data(), bytes);
        if (!pcm_stage_commit(p, k, bytes, s)) return fail(p, ARTALK_EHIP, "the staging copy failed");
        launch_pcm_take(reinterpret_cast<const artalk_pcm_take_desc*>(p->stage.get()), n, out_dev, out_stride, p->block, s);
        if (hipGetLastError() != hipSuccess) return fail(p, ARTALK_EHIP, "the launch failed");
    }
    for (int i = 0; i < n; ++i) {
        p->slots[slots[i]].taken += descs[i].n_valid;
        n_valid_host[i] = descs[i].n_valid;
    }
    return ARTALK_OK;
}

int artalk_op_pcm_plan(int64_t n_before, int64_t frames, int end, int orig, int nw, int width, int64_t* out6) {
    if (!out6 || n_before < 0 || frames < 0 || pcm_rate_check(orig, nw, width, &g_pcm_error) != ARTALK_OK) return ARTALK_EINVAL;
    const PcmPlan q = pcm_plan(n_before, frames, end != 0, orig, nw, width);
    out6[0] = q.n_out; out6[1] = q.lead; out6[2] = q.carry_n; out6[3] = q.carry_from; out6[4] = q.carry_out_n; out6[5] = q.groups;
    return ARTALK_OK;
}

int artalk_op_pcm_desc_bytes(int which) { return which == 0 ? (int)sizeof(artalk_pcm_desc) : which == 1 ? (int)sizeof(artalk_pcm_take_desc) : ARTALK_EINVAL; }

int artalk_op_pcm_push(artalk_pcm_desc* descs_host, int n, void* table_dev, int64_t table_bytes, void* stream) {
    if (!descs_host || n < 1 || n > 65535 || !table_dev || table_bytes < (int64_t)n * (int64_t)sizeof(artalk_pcm_desc)) {
        g_pcm_error = "artalk_op_pcm_push needs 1..65535 descriptors and a device table that holds them"; return ARTALK_EINVAL;
    }
    int max_tiles = 1;
    for (int i = 0; i < n; ++i) {
        if (pcm_desc_check(&descs_host[i], &g_pcm_error) != ARTALK_OK) return ARTALK_EINVAL;
        max_tiles = std::max(max_tiles, descs_host[i].n_tiles);
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(table_dev, descs_host, (size_t)n * sizeof(artalk_pcm_desc), hipMemcpyHostToDevice, s) != hipSuccess) { (void)hipGetLastError(); return ARTALK_EHIP; }
    launch_pcm_push(static_cast<const artalk_pcm_desc*>(table_dev), n, max_tiles, s);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

int artalk_op_pcm_take(const artalk_pcm_take_desc* descs_host, int n, void* table_dev, int64_t table_bytes, float* out_dev, int64_t out_stride,
                       int block, void* stream) {
    if (!descs_host || n < 1 || n > 65535 || !table_dev || table_bytes < (int64_t)n * (int64_t)sizeof(artalk_pcm_take_desc) || !out_dev || block < 1 ||
        out_stride < block) {
        g_pcm_error = "artalk_op_pcm_take needs 1..65535 descriptors, a device table that holds them and rows of a block or more"; return ARTALK_EINVAL;
    }
    for (int i = 0; i < n; ++i)
        if (pcm_take_desc_check(&descs_host[i], block, &g_pcm_error) != ARTALK_OK) return ARTALK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(table_dev, descs_host, (size_t)n * sizeof(artalk_pcm_take_desc), hipMemcpyHostToDevice, s) != hipSuccess) { (void)hipGetLastError(); return ARTALK_EHIP; }
    launch_pcm_take(static_cast<const artalk_pcm_take_desc*>(table_dev), n, out_dev, out_stride, block, s);
    return hipGetLastError() == hipSuccess ? ARTALK_OK : ARTALK_EHIP;
}

}  // extern "C"
