// Walks WeightStore and pack_conv_weight of artalk_amd/csrc/weight_store.h and the CallTimer and WsLayout of device_mem.h on the
// host, built with -fsanitize=address,undefined (Makefile beside this file; tests/test_weight_store_cpu.py builds and runs it).  The
// intake - declare, set, missing, host, shape, release_host - and the repack never touch the runtime and are checked to the byte.
// upload and the timer do: without a usable device every HIP call fails and they must fail quietly (null pointers, ok() false, 0 ms,
// no error left behind, "quiet" as device_mem_check.cpp defines it); with a device the same walk checks the success path.  Exit
// status 0 and no sanitizer output: all held.
#include "../../artalk_amd/csrc/weight_store.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

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

static std::vector<float> ramp(size_t n, float first) {
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = first + (float)i;
    return v;
}

static void walk_intake() {
    WeightStore st;
    const std::vector<std::string> names = {"z.weight", "a.bias", "m.gamma", "b.weight"};      // (not sorted: the order is the caller's)
    st.declare(names[0], {2, 3});
    st.declare(names[1], {3});
    st.declare(names[2], {1, 4}, true);
    st.declare(names[3], {2, 1, 1, 2});
    CHECK(st.keys() == names);
    CHECK(st.shape("z.weight") == (std::vector<int64_t>{2, 3}) && st.shape("nothing").empty() && st.host("nothing").empty());

    std::string msg = "untouched";
    const std::vector<float> a = ramp(6, 1.f), b = ramp(6, 100.f);
    const int64_t s23[2] = {2, 3}, s32[2] = {3, 2}, s3[1] = {3}, s14[2] = {1, 4}, s2112[4] = {2, 1, 1, 2};
    CHECK(st.set("y.weight", a.data(), 2, s23, &msg) == ARTALK_EKEY && msg == "Unexpected key in state_dict: y.weight");
    CHECK(st.set("z.weight", a.data(), 1, s3, &msg) == ARTALK_EINVAL && msg == "size mismatch for z.weight");      // ndim
    CHECK(st.set("z.weight", a.data(), 2, s32, &msg) == ARTALK_EINVAL && msg == "size mismatch for z.weight");     // an extent
    CHECK(st.host("z.weight").empty());
    msg = "untouched";
    CHECK(st.set("z.weight", a.data(), 2, s23, &msg) == ARTALK_OK && msg == "untouched" && st.host("z.weight") == a);
    CHECK(st.set("z.weight", b.data(), 2, s23, &msg) == ARTALK_OK && st.host("z.weight") == b);      // the later data stays
    CHECK(st.missing(&msg) && msg == "Missing key(s) in state_dict: a.bias, b.weight");               // in order, the optional one left out
    CHECK(st.set("b.weight", a.data(), 4, s2112, &msg) == ARTALK_OK && st.host("b.weight") == ramp(4, 1.f));
    CHECK(st.set("a.bias", a.data(), 1, s3, &msg) == ARTALK_OK);
    msg = "untouched";
    CHECK(!st.missing(&msg) && msg == "untouched");                                                   // m.gamma is optional
    CHECK(st.set("m.gamma", a.data(), 2, s14, &msg) == ARTALK_OK && !st.missing(&msg));

    CHECK(st.ok() && !st.on_device());
    st.release_host();
    for (const std::string& k : names) CHECK(st.host(k).empty());
    CHECK(st.shape("b.weight") == (std::vector<int64_t>{2, 1, 1, 2}) && st.keys() == names && !st.missing(&msg));
}

// n required keys k0 .. k(n-1) and an optional one, none set
static std::string missing_of(int n) {
    WeightStore st;
    st.declare("opt", {1}, true);
    for (int i = 0; i < n; ++i) st.declare("k" + std::to_string(i), {1});
    std::string msg;
    CHECK(st.missing(&msg) == (n > 0));
    return msg;
}

static void walk_missing() {
    CHECK(missing_of(0).empty());
    CHECK(missing_of(1) == "Missing key(s) in state_dict: k0");
    CHECK(missing_of(8) == "Missing key(s) in state_dict: k0, k1, k2, k3, k4, k5, k6, k7");
    CHECK(missing_of(9) == "Missing key(s) in state_dict: k0, k1, k2, k3, k4, k5, k6, k7, ...");
}

static void walk_pack() {
    const int cout = 5, cin = 3;
    for (int k : {1, 3})
        for (int cinp : {3, 8}) {
            const int kk = k * k;
            const std::vector<float> w = ramp((size_t)cout * cin * kk, 1.f);      // distinct, none 0
            const std::vector<float> t = pack_conv_weight(w, cout, cin, cinp, k);
            CHECK(t.size() == (size_t)kk * cinp * cout);
            for (int q = 0; q < kk; ++q)
                for (int i = 0; i < cinp; ++i)
                    for (int o = 0; o < cout; ++o) {
                        const float want = i < cin ? w[((size_t)o * cin + i) * kk + q] : 0.f;
                        CHECK(t[((size_t)q * cinp + i) * cout + o] == want);
                    }
        }
}

static void walk_upload() {
    WeightStore st;
    st.declare("w", {5});
    const std::vector<float> host = ramp(5, 1.f);
    const int64_t s5[1] = {5};
    std::string msg;
    CHECK(st.set("w", host.data(), 1, s5, &msg) == ARTALK_OK);
    const float* byvec = st.upload(std::vector<float>{7.f, 8.f, 9.f});
    const float* bykey = st.upload("w");
    CHECK(st.on_device());
    CHECK(hipGetLastError() == g_quiet);
    if (st.ok()) {
        ++g_taken;
        CHECK(byvec && bykey && byvec != bykey);
        float back[5] = {};
        CHECK(hipMemcpy(back, bykey, sizeof(back), hipMemcpyDeviceToHost) == hipSuccess);
        for (int i = 0; i < 5; ++i) CHECK(back[i] == host[i]);
        CHECK(hipMemcpy(back, byvec, 3 * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess && back[0] == 7.f && back[2] == 9.f);
    } else {
        CHECK(!byvec && !bykey);
    }
    const bool was = st.ok();
    st.release_host();
    (void)st.upload("w");                                // (an empty tensor takes a block of 1 all the same)
    CHECK(st.ok() == was && hipGetLastError() == g_quiet);
}

static void walk_timer() {
    hipEvent_t e0 = (hipEvent_t)&g_checks, e1 = (hipEvent_t)&g_checks;
    {
        CallTimer off;                                   // disabled: no HIP call, null events, 0 ms
        CHECK(off.begin(nullptr, false));
        CHECK(!off.pair(&e0, &e1) && !e0 && !e1);
        CHECK(off.end());
        CHECK(off.total_ms() == 0 && off.pairs_ms() == 0 && off.pair_ms().empty() && off.empty());
    }
    {
        CallTimer on;
        const bool began = on.begin(nullptr, true);
        CHECK(hipGetLastError() == g_quiet);
        const bool p0 = on.pair(&e0, &e1);
        CHECK(p0 == (e0 != nullptr) && p0 == (e1 != nullptr) && (!p0 || e0 != e1));
        if (p0) { (void)hipEventRecord(e0, nullptr); (void)hipEventRecord(e1, nullptr); }
        hipEvent_t f0 = nullptr, f1 = nullptr;
        const bool p1 = on.pair(&f0, &f1);               // (never recorded: its time cannot be read and counts 0)
        CHECK(!p1 || (f0 != e0 && f0 != e1 && f1 != f0));
        const bool ended = on.end();
        CHECK(hipGetLastError() == g_quiet);
        if (began) {
            ++g_taken;
            CHECK(p0 && p1 && ended && !on.empty());
            CHECK(on.pair_ms().size() == 2 && on.pair_ms()[0] >= 0 && on.pair_ms()[1] == 0);
            CHECK(on.total_ms() >= 0 && on.pairs_ms() == on.pair_ms()[0]);
            // the next call takes the pool's pairs again, and a disabled call keeps the last timed figures
            CHECK(on.begin(nullptr, true) && on.pair(&f0, &f1) && f0 == e0 && f1 == e1 && on.end() && on.pair_ms().size() == 1);
            CHECK(on.begin(nullptr, false) && !on.pair(&f0, &f1) && on.end() && on.pair_ms().size() == 1);
        } else {
            CHECK(!p0 && !p1 && ended && on.empty());    // nothing is timed, nothing fails twice
            CHECK(on.total_ms() == 0 && on.pairs_ms() == 0 && on.pair_ms().empty());
        }
    }
    {
        CallTimer abandoned;                             // begun, never ended: the destructor gives the events back
        (void)abandoned.begin(nullptr, true);
        (void)abandoned.pair(&e0, &e1);
    }
    CHECK(hipGetLastError() == g_quiet);
}

static void walk_layout() {
    WsLayout w;
    CHECK(w.take(1) == 0 && w.take(4) == 4 && w.take(0) == 8 && w.take(5) == 8 && w.off == 16);
}

int main() {
    int n_dev = 0;
    (void)hipGetDeviceCount(&n_dev);
    (void)hipGetLastError();
    g_quiet = hipGetLastError();
    CHECK(g_quiet == hipSuccess || g_quiet == hipErrorNoDevice);
    walk_intake();
    walk_missing();
    walk_pack();
    walk_upload();
    walk_timer();
    walk_layout();
    std::printf("weight_store_check: %d checks held (%s)\n", g_checks, g_taken ? "with a device" : "no device: failure paths");
    return 0;
}
