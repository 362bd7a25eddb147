// launch_cache_core.h -- what the library remembers about a kernel's launch attributes: plain C++17, no HIP include or call.
// A kernel's dynamic-LDS limit and its occupancy belong to ONE device's copy of the kernel, so every key starts with the device
// ordinal.  The runtime calls come in as callables: runtime.cpp passes the real ones, tests/host_sim/sim_launch_cache.cpp counting ones.
#pragma once
#include <cstddef>
#include <map>
#include <mutex>
#include <tuple>

namespace bdsp {

class LaunchCache {
public:
    // Makes the dynamic-LDS limit of `kernel` on `device` at least `bytes`: raise() (0, or an error code, which is returned and
    // not remembered) runs only if the limit is not known to be that large -- under the lock, so limits only grow
    template <typename Raise>
    int lds_limit(int device, const void* kernel, size_t bytes, Raise&& raise)
    {
        std::lock_guard<std::mutex> lk(mu_);
        size_t& have = limit_[std::make_tuple(device, kernel)];
        if (have >= bytes) return 0;
        const int c = raise();
        if (c == 0) have = bytes;
        return c;
    }

    // The resident workgroups per CU for the key, at least 1: query() runs once per key, under the lock (no two first callers ask)
    template <typename Query>
    int slots(int device, const void* kernel, int threads, size_t lds, Query&& query)
    {
        std::lock_guard<std::mutex> lk(mu_);
        const auto key = std::make_tuple(device, kernel, threads, lds);
        auto it = slots_.find(key);
        if (it == slots_.end()) {
            const int o = query();
            it = slots_.emplace(key, o < 1 ? 1 : o).first;
        }
        return it->second;
    }

private:
    std::mutex mu_;
    std::map<std::tuple<int, const void*>, size_t> limit_;
    std::map<std::tuple<int, const void*, int, size_t>, int> slots_;
};

} // namespace bdsp
