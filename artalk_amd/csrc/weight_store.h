// The weight intake of an object that loads a PyTorch state_dict (artalk_styleunet, artalk_gsgen, artalk_dino): the manifest of
// declared tensors, their host copies while the dict comes in, torch's wording for what is wrong with it, and the device copies
// afterwards.  Host code only, private to csrc/, in the manner of device_mem.h.  A module declares its keys in the order of the
// reference module's state_dict(), hands every artalk_X_set_tensor to set(), and in artalk_X_finalize asks missing(), uploads - a key
// as it came, or a vector it repacked from host(key) - and releases the host copies.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "artalk_hip.h"
#include "device_mem.h"

namespace artalk {

class WeightStore {
public:
    void declare(const std::string& name, std::vector<int64_t> shape, bool optional = false) {
        Slot& s = slots_[name];
        s.shape = std::move(shape); s.optional = optional;
        order_.push_back(name);
    }
    const std::vector<std::string>& keys() const { return order_; }      // in declaration order

    // One tensor of the dict, fp32 and contiguous at host_ptr.  ARTALK_EKEY for a key that was not declared, ARTALK_EINVAL for
    // another shape than the declared one, with torch's message in *msg.  A key set twice keeps the later data.
    int set(const char* key, const void* host_ptr, int ndim, const int64_t* shape, std::string* msg) {
        auto it = slots_.find(key);
        if (it == slots_.end()) { *msg = std::string("Unexpected key in state_dict: ") + key; return ARTALK_EKEY; }
        Slot& sl = it->second;
        bool same = (int)sl.shape.size() == ndim;
        for (int i = 0; same && i < ndim; ++i) same = sl.shape[i] == shape[i];
        if (!same) { *msg = std::string("size mismatch for ") + key; return ARTALK_EINVAL; }
        int64_t n = 1;
        for (int64_t v : sl.shape) n *= v;
        sl.host.assign((const float*)host_ptr, (const float*)host_ptr + n);
        sl.set = true;
        return ARTALK_OK;
    }
    // true when a key that is not optional was never set: *msg names the first 8 of them, in declaration order
    bool missing(std::string* msg) const {
        std::string names;
        int n = 0;
        for (const std::string& k : order_) {
            const Slot& sl = slots_.at(k);
            if (!sl.set && !sl.optional) { if (n++ < 8) names += (names.empty() ? "" : ", ") + k; }
        }
        if (n) *msg = "Missing key(s) in state_dict: " + names + (n > 8 ? ", ..." : "");
        return n != 0;
    }
    // for the repacks that are a module's own (a key that was not declared: empty)
    const std::vector<float>& host(const std::string& key) const { return slot(key).host; }
    const std::vector<int64_t>& shape(const std::string& key) const { return slot(key).shape; }

    // One device block per call, kept until the store goes.  Null after a failure, which ok() remembers.
    const float* upload(const std::vector<float>& v) {
        dev_.emplace_back();
        if (!dev_.back().upload(v.data(), v.size())) { (void)hipGetLastError(); ok_ = false; }
        return dev_.back().get();
    }
    const float* upload(const std::string& key) { return upload(host(key)); }
    bool ok() const { return ok_; }
    bool on_device() const { return !dev_.empty(); }      // an upload was tried: the owner's destroy waits for the device first
    void release_host() { for (auto& kv : slots_) std::vector<float>().swap(kv.second.host); }

private:
    struct Slot { std::vector<int64_t> shape; std::vector<float> host; bool set = false, optional = false; };
    const Slot& slot(const std::string& key) const {
        static const Slot none;
        auto it = slots_.find(key);
        return it == slots_.end() ? none : it->second;
    }
    std::map<std::string, Slot> slots_;
    std::vector<std::string> order_;
    std::vector<DevBuf<float>> dev_;
    bool ok_ = true;
};

// torch's conv weight [cout][cin][k][k] (a Linear: k = 1) -> [k k][cinp][cout], the layout launch_conv reads; the rows of the padded
// input channels cin .. cinp - 1 are zero
inline std::vector<float> pack_conv_weight(const std::vector<float>& w, int cout, int cin, int cinp, int k) {
    const int kk = k * k;
    std::vector<float> t((size_t)kk * cinp * cout, 0.f);
    for (int o = 0; o < cout; ++o)
        for (int i = 0; i < cin; ++i)
            for (int q = 0; q < kk; ++q) t[((size_t)q * cinp + i) * cout + o] = w[((size_t)o * cin + i) * kk + q];
    return t;
}

}  // namespace artalk
