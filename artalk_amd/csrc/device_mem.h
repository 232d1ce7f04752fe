// Owners of what the host side takes from the HIP runtime: device blocks and pools of them, pinned host blocks, events, streams, graph
// executables, the events of a stage or call timer.
// Host code only.  Every type is move-only, takes nothing in its constructor and gives back what it holds in its destructor, so an
// object made of them is destroyed by `delete` and an early return leaks nothing.  A call that fails leaves its object empty
// (capacity 0), clears the runtime's last error - the caller reports the failure once, and it does not come back from a later
// hipGetLastError() as a failed launch - and returns false.  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

namespace artalk {

// One block of T, in device memory or (kPinned) in pinned host memory.  A request for 0 elements takes 1.
template <typename T, bool kPinned>
class Block {
public:
    T* get() const { return p_.get(); }
    size_t capacity() const { return p_ ? cap_ : 0; }      // elements
    void reset() { p_.reset(); }
    bool alloc(size_t n) { return take((n ? n : 1) * sizeof(T)); }
    // bytes that grow(n, slack_num, slack_den, ..) asks for: n elements and slack_num / slack_den of them on top
    static size_t grown_bytes(size_t n, size_t slack_num, size_t slack_den) { return (n ? n : 1) * sizeof(T) * (slack_den + slack_num) / slack_den; }
    // Nothing when n fits.  Else: wait for `wait`, the stream whose earlier work may still read the block, free it, and take n
    // elements plus the slack (the contents are not kept).
    bool grow(size_t n, size_t slack_num, size_t slack_den, hipStream_t wait) {
        if (p_ && n <= cap_) return true;
        if (p_) (void)hipStreamSynchronize(wait);
        return take(grown_bytes(n, slack_num, slack_den));
    }

private:
    bool take(size_t bytes) {
        reset();
        void* p = nullptr;
        if ((kPinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes)) != hipSuccess) { (void)hipGetLastError(); return false; }
        p_.reset(static_cast<T*>(p)); cap_ = bytes / sizeof(T);
        return true;
    }
    struct Free { void operator()(T* p) const { if (kPinned) (void)hipHostFree(p); else (void)hipFree(p); } };
    std::unique_ptr<T, Free> p_;
    size_t cap_ = 0;
};

template <typename T>
using PinnedBuf = Block<T, true>;

template <typename T>
class DevBuf : public Block<T, false> {
public:
    bool alloc_zero(size_t n) {      // the fill runs on the null stream
        if (!this->alloc(n)) return false;
        (void)hipMemset(this->get(), 0, (n ? n : 1) * sizeof(T));
        return true;
    }
    bool upload(const T* host, size_t n) {
        return this->alloc(n) && (n == 0 || hipMemcpy(this->get(), host, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    }
};

// Device blocks that live and die together (the engine's weights, its workspace): take() hands out zero-filled blocks, the first
// failure is remembered in ok() - as WeightStore does for uploads - and clear() frees every block and forgets it.
class DevPool {
public:
    // zero-filled block of max(n, 1) elements (the fill runs on the null stream), or null
    template <typename T>
    T* take(int64_t n) {
        DevBuf<unsigned char> b;
        if (!b.alloc_zero((size_t)(n > 0 ? n : 1) * sizeof(T))) { ok_ = false; return nullptr; }
        blocks_.push_back(std::move(b));
        return reinterpret_cast<T*>(blocks_.back().get());
    }
    bool ok() const { return ok_; }
    void clear() { blocks_.clear(); ok_ = true; }

private:
    std::vector<DevBuf<unsigned char>> blocks_;
    bool ok_ = true;
};

class Event {
public:
    hipEvent_t get() const { return e_.get(); }
    void reset() { e_.reset(); }
    // flags: hipEventDefault (the event can be timed) or hipEventDisableTiming
    bool create(unsigned flags = hipEventDefault) {
        if (e_) return true;
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, flags) != hipSuccess) { (void)hipGetLastError(); return false; }
        e_.reset(e);
        return true;
    }

private:
    struct Destroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
    std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Destroy> e_;
};

// A stream of the current device: non-blocking (a copy stream beside the caller's), blocking (the engine's own stream for callers
// that pass none), or restricted to the compute units of a mask
class Stream {
public:
    hipStream_t get() const { return s_.get(); }
    void reset() { s_.reset(); }
    bool create(unsigned flags = hipStreamNonBlocking) {
        hipStream_t s = nullptr;
        return s_ || keep(hipStreamCreateWithFlags(&s, flags), s);
    }
    bool create_masked(const uint32_t* words, int n) {
        hipStream_t s = nullptr;
        return s_ || keep(hipExtStreamCreateWithCUMask(&s, (uint32_t)n, words), s);
    }

private:
    bool keep(hipError_t e, hipStream_t s) {
        if (e != hipSuccess) { (void)hipGetLastError(); return false; }
        s_.reset(s);
        return true;
    }
    struct Destroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
    std::unique_ptr<std::remove_pointer_t<hipStream_t>, Destroy> s_;
};

// One instantiated graph
class GraphExec {
public:
    GraphExec() = default;
    explicit GraphExec(hipGraphExec_t g) : g_(g) {}
    hipGraphExec_t get() const { return g_.get(); }
    void reset() { g_.reset(); }

private:
    struct Destroy { void operator()(hipGraphExec_t g) const { (void)hipGraphExecDestroy(g); } };
    std::unique_ptr<std::remove_pointer_t<hipGraphExec_t>, Destroy> g_;
};

// A handle's device for the length of a call: made current in the constructor, the caller's put back in the destructor
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev); else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Time per stage of one call, from events on the call's stream: the interval that ENDS at a mark belongs to the mark's stage
// (stage < 0: to none).  A mark whose event cannot be made is skipped.  Disabled, no method makes a HIP call.
class StageTimer {
public:
    void start(hipStream_t s, bool enabled) { s_ = s; on_ = enabled; ev_.clear(); stage_.clear(); }
    void mark(int stage) {
        Event e;
        if (!on_ || !e.create()) return;
        (void)hipEventRecord(e.get(), s_);
        ev_.push_back(std::move(e)); stage_.push_back(stage);
    }
    // waits for the last mark, then adds every interval to stage_ms[its stage] (n stages)
    void finish(double* stage_ms, int n) {
        if (!ev_.empty()) (void)hipEventSynchronize(ev_.back().get());
        for (size_t k = 1; k < ev_.size(); ++k) {
            float ms = 0.f;
            if (stage_[k] >= 0 && stage_[k] < n && hipEventElapsedTime(&ms, ev_[k - 1].get(), ev_[k].get()) == hipSuccess) stage_ms[stage_[k]] += ms;
        }
        ev_.clear(); stage_.clear();
    }

private:
    hipStream_t s_ = nullptr;
    bool on_ = false;
    std::vector<Event> ev_;      // ev_[k] closes an interval of stage stage_[k]
    std::vector<int> stage_;
};

// Time of one call on its stream, and of the launches inside it that ask for a start / stop pair of events (launch_conv takes one).
// The pairs come from a pool kept from call to call.  total_ms() and pair_ms() are those of the last call that end() saw through with
// the timer enabled.  Disabled, no method makes a HIP call.
class CallTimer {
public:
    // records the call's start; false: the call's own two events cannot be made (nothing is timed then)
    bool begin(hipStream_t s, bool enabled) {
        s_ = s; on_ = enabled; used_ = 0;
        if (!on_) return true;
        if (!t0_.create() || !t1_.create()) { on_ = false; return false; }
        (void)hipEventRecord(t0_.get(), s_);
        return true;
    }
    // the next pair of the pool, which grows by two events when it has none left; null pointers when disabled or when an event
    // cannot be made.  true: a pair was handed out
    bool pair(hipEvent_t* e0, hipEvent_t* e1) {
        *e0 = *e1 = nullptr;
        if (!on_) return false;
        if (used_ + 2 > pool_.size()) {
            Event a0, a1;
            if (a0.create() && a1.create()) { pool_.push_back(std::move(a0)); pool_.push_back(std::move(a1)); }
        }
        if (used_ + 2 > pool_.size()) return false;
        *e0 = pool_[used_].get(); *e1 = pool_[used_ + 1].get(); used_ += 2;
        return true;
    }
    // records the call's end and waits for it; false: the device reported a failure.  A pair whose time cannot be read counts 0.
    bool end() {
        if (!on_) return true;
        (void)hipEventRecord(t1_.get(), s_);
        if (hipEventSynchronize(t1_.get()) != hipSuccess) { (void)hipGetLastError(); return false; }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t0_.get(), t1_.get()) != hipSuccess) (void)hipGetLastError();
        total_ms_ = ms;
        pair_ms_.assign(used_ / 2, 0.0);
        for (size_t i = 0; i + 1 < used_; i += 2) {
            float k = 0.f;
            if (hipEventElapsedTime(&k, pool_[i].get(), pool_[i + 1].get()) == hipSuccess) pair_ms_[i / 2] = k; else (void)hipGetLastError();
        }
        return true;
    }
    double total_ms() const { return total_ms_; }
    const std::vector<double>& pair_ms() const { return pair_ms_; }      // in the order the pairs were handed out
    double pairs_ms() const { double t = 0; for (double v : pair_ms_) t += v; return t; }
    bool empty() const { return pool_.empty() && !t0_.get() && !t1_.get(); }      // nothing was ever taken from the device

private:
    hipStream_t s_ = nullptr;
    bool on_ = false;
    Event t0_, t1_;
    std::vector<Event> pool_;      // start / stop pairs, the first used_ of them handed out in this call
    size_t used_ = 0;
    double total_ms_ = 0;
    std::vector<double> pair_ms_;
};

// Offsets of the blocks of a workspace, in floats, every block 16-byte aligned (vector loads)
struct WsLayout {
    int64_t off = 0;
    int64_t take(int64_t n) { const int64_t at = off; off += (n + 3) & ~(int64_t)3; return at; }
};

}  // namespace artalk
