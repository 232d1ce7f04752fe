// Walks the owner types of artalk_amd/csrc/device_mem.h (blocks, pools, events, streams, graph executables, timers) on the host, built
// with -fsanitize=address,undefined (Makefile beside this file; tests/test_device_mem_cpu.py builds and runs it).  Without a usable device every HIP call fails, which is exactly the failure
// path of every method: the object must then be empty, its capacity 0, and the runtime's last error cleared.  With a device the same
// walk checks the success path.  Exit status 0 and no sanitizer output: all held.
// "Cleared" where the runtime cannot initialise for want of a device: there hipGetLastError() itself answers hipErrorNoDevice on
// every call, whatever came before (it remembers nothing).  main() takes the answer of a second hipGetLastError() in a row, which is
// hipSuccess or that, as what "no error is left behind" reads like in this process (g_quiet).
#include "../../artalk_amd/csrc/device_mem.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

using namespace artalk;

// the HIP runtime keeps its own allocations until the process ends: they are not this program's to free
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

static int g_checks = 0;
static hipError_t g_quiet = hipSuccess;      // what hipGetLastError() answers when no error is remembered (main)
static int g_taken = 0;                      // calls that did get something from the runtime
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// after a call that returned `ok` for a request of n elements
template <typename B>
static void check_state(const B& b, bool ok, size_t n) {
    if (ok) {
        ++g_taken;
        CHECK(b.get() != nullptr && b.capacity() >= (n ? n : 1));
    } else {
        CHECK(b.get() == nullptr && b.capacity() == 0);
        CHECK(hipGetLastError() == g_quiet);
    }
}

template <typename B>
static void walk_block() {
    B a;
    CHECK(a.get() == nullptr && a.capacity() == 0);
    check_state(a, a.alloc(100), 100);
    check_state(a, a.alloc(0), 0);                       // 0 elements take 1
    const bool grown = a.grow(1000, 1, 4, nullptr);
    check_state(a, grown, 1000);
    if (grown) {
        CHECK(a.capacity() == 1250);
        auto* before = a.get();
        CHECK(a.grow(1250, 1, 4, nullptr) && a.get() == before && a.capacity() == 1250);      // fits: nothing happens
        CHECK(a.grow(10, 1, 4, nullptr) && a.get() == before);
    }
    CHECK(B::grown_bytes(0, 0, 1) == sizeof(*a.get()) && B::grown_bytes(8, 1, 4) == 10 * sizeof(*a.get()));
    B b(std::move(a));                                   // move-construct
    CHECK(a.get() == nullptr && a.capacity() == 0);
    check_state(b, grown, 1000);
    B c;
    check_state(c, c.alloc(7), 7);
    c = std::move(b);                                    // move-assign over a block that may hold something
    CHECK(b.get() == nullptr && b.capacity() == 0);
    check_state(c, grown, 1000);
    c.reset();
    c.reset();                                           // double reset
    CHECK(c.get() == nullptr && c.capacity() == 0);
    check_state(c, c.grow(0, 0, 1, nullptr), 0);         // grow on an empty block takes, also for 0 elements
}

static void walk_devbuf() {
    DevBuf<float> d;
    check_state(d, d.alloc_zero(33), 33);
    const float host[5] = {1.f, 2.f, 3.f, 4.f, 5.f};
    const bool up = d.upload(host, 5);
    if (up) {
        float back[5] = {};
        CHECK(hipMemcpy(back, d.get(), sizeof(back), hipMemcpyDeviceToHost) == hipSuccess);
        for (int i = 0; i < 5; ++i) CHECK(back[i] == host[i]);
    } else {
        (void)hipGetLastError();                         // (a failed copy into a block that was taken is the caller's to report)
        if (!d.get()) CHECK(d.capacity() == 0);
    }
    check_state(d, d.upload(nullptr, 0), 0);             // nothing to copy: a block of 1 all the same
}

static void walk_pool() {
    DevPool p;
    CHECK(p.ok());
    float* a = p.take<float>(100);
    CHECK(p.ok() == (a != nullptr));
    if (a) ++g_taken;
    else CHECK(hipGetLastError() == g_quiet);
    unsigned char* z = p.take<unsigned char>(0);         // 0 elements take 1
    CHECK(p.ok() == (a != nullptr && z != nullptr) && (!a || !z || (void*)z != (void*)a));
    if (a) {
        float back[100];
        CHECK(hipDeviceSynchronize() == hipSuccess);      // (the zero fill runs on the null stream)
        CHECK(hipMemcpy(back, a, sizeof(back), hipMemcpyDeviceToHost) == hipSuccess);
        for (float v : back) CHECK(v == 0.f);
    }
    const bool was_ok = p.ok();
    DevPool q(std::move(p));                             // the blocks and the remembered failure move together
    CHECK(q.ok() == was_ok);
    q.clear();
    CHECK(q.ok());                                       // clear() forgets the failure
    q.clear();                                           // double clear
    long* l = q.take<long>(-5);                          // a negative count takes 1 as well
    CHECK(q.ok() == (l != nullptr));
    if (!l) CHECK(hipGetLastError() == g_quiet);
}

static void walk_graph_exec() {
    GraphExec g;                                         // (instantiating a graph needs a device: the empty owner's moves and resets)
    CHECK(g.get() == nullptr);
    GraphExec h(std::move(g));
    CHECK(g.get() == nullptr && h.get() == nullptr);
    GraphExec k{nullptr};
    k = std::move(h);
    CHECK(k.get() == nullptr);
    k.reset();
    k.reset();
    CHECK(k.get() == nullptr);
    CHECK(hipGetLastError() == g_quiet);
}

static void walk_event(unsigned flags) {
    Event e;
    CHECK(e.get() == nullptr);
    const bool ok = flags == hipEventDefault ? e.create() : e.create(flags);
    CHECK(ok == (e.get() != nullptr));
    if (ok) ++g_taken;
    else CHECK(hipGetLastError() == g_quiet);
    hipEvent_t h = e.get();
    CHECK(e.create() == ok && e.get() == h);             // a second create keeps the event
    Event f(std::move(e));
    CHECK(e.get() == nullptr && f.get() == h);
    Event g;
    (void)g.create();
    g = std::move(f);
    CHECK(f.get() == nullptr && g.get() == h);
    g.reset();
    g.reset();
    CHECK(g.get() == nullptr);
}

static void walk_stream() {
    Stream s;
    CHECK(s.get() == nullptr);
    const bool ok = s.create();
    CHECK(ok == (s.get() != nullptr));
    if (ok) ++g_taken;
    else CHECK(hipGetLastError() == g_quiet);
    hipStream_t h = s.get();
    CHECK(s.create() == ok && s.get() == h);             // a second create keeps the stream
    Stream t(std::move(s));
    CHECK(s.get() == nullptr && t.get() == h);
    Stream u;
    u = std::move(t);
    CHECK(t.get() == nullptr && u.get() == h);
    u.reset();
    u.reset();                                           // double reset
    CHECK(u.get() == nullptr);
    const uint32_t words[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0};
    const bool masked = u.create_masked(words, 8);       // a stream on half of the compute units
    CHECK(masked == (u.get() != nullptr));
    if (masked) ++g_taken;
    else CHECK(hipGetLastError() == g_quiet);
    h = u.get();
    CHECK(u.create_masked(words, 8) == masked && u.create() == masked && u.get() == h);      // a second create of either kind keeps the stream
    Stream b;
    const bool blocking = b.create(hipStreamDefault);    // the flags of the plain create
    CHECK(blocking == (b.get() != nullptr));
    if (!blocking) CHECK(hipGetLastError() == g_quiet);
}

static void walk_timer() {
    double ms[3] = {0, 0, 0};
    {
        StageTimer off;                                  // disabled: no HIP call, nothing counted
        off.start(nullptr, false);
        off.mark(-1); off.mark(0); off.mark(2);
        off.finish(ms, 3);
        CHECK(ms[0] == 0 && ms[1] == 0 && ms[2] == 0);
    }
    {
        StageTimer on;
        on.start(nullptr, true);
        on.mark(-1); on.mark(0); on.mark(1); on.mark(-1); on.mark(1); on.mark(7);      // (stage 7 of 3 counts to none)
        on.finish(ms, 3);
        CHECK(ms[0] >= 0 && ms[1] >= 0 && ms[2] == 0);
        CHECK(hipGetLastError() == g_quiet);
        on.finish(ms, 3);                                // a second finish has nothing left
    }
    {
        StageTimer abandoned;                            // never finished: the destructor gives the events back
        abandoned.start(nullptr, true);
        abandoned.mark(-1); abandoned.mark(0);
    }
    CHECK(hipGetLastError() == g_quiet);
}

int main() {
    int n_dev = 0;
    (void)hipGetDeviceCount(&n_dev);
    (void)hipGetLastError();
    g_quiet = hipGetLastError();
    CHECK(g_quiet == hipSuccess || g_quiet == hipErrorNoDevice);
    walk_block<DevBuf<float>>();
    walk_block<DevBuf<unsigned long long>>();
    walk_block<PinnedBuf<char>>();
    walk_block<PinnedBuf<float>>();
    walk_devbuf();
    walk_pool();
    walk_event(hipEventDefault);
    walk_event(hipEventDisableTiming);
    walk_stream();
    walk_graph_exec();
    walk_timer();
    std::printf("device_mem_check: %d checks held (%s)\n", g_checks, g_taken ? "with a device" : "no device: failure paths");
    return 0;
}
