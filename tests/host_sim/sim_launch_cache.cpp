// sim_launch_cache.cpp -- basic_dsp_amd/csrc/launch_cache_core.h on the host, with counting stand-ins for the two runtime
// calls (tests/test_launch_cache_abi.py builds this plainly and with -fsanitize=thread and runs both).
//   8 threads x 1000 lookups, interleaved over 3 device ordinals x 4 (kernel, threads, lds) keys:
//     * the occupancy query runs exactly 12 times, once per (device, key), whoever comes first;
//     * every lookup returns the value of the device it named (the stand-in's values differ per device);
//     * a query result below 1 (key 3 answers 0, -1, -2 on devices 0, 1, 2) comes back as 1;
//     * the LDS limit is raised once per (device, kernel) and again only for a byte count above what was raised before; a
//       failed raise is reported and not remembered; nothing leaks from one device to another.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../basic_dsp_amd/csrc/launch_cache_core.h"

namespace {

constexpr int THREADS = 8, LOOKUPS = 1000, DEVICES = 3, KEYS = 4;

struct Key {
    const void* kernel;
    int threads;
    size_t lds;
};

int g_kernels[3]; // three addresses to stand for kernels; keys 1 and 2 share a kernel and differ in threads / lds

const Key g_keys[KEYS] = {{&g_kernels[0], 256, 69632}, {&g_kernels[1], 512, 148000}, {&g_kernels[1], 256, 148000}, {&g_kernels[2], 256, 1024}};

// what the "runtime" answers: differs per device and per key; key 3 answers below 1
int device_answer(int dev, int key) { return key == 3 ? -dev : 1 + dev * 10 + key; }
int expected(int dev, int key) { return key == 3 ? 1 : device_answer(dev, key); }

int g_failures = 0;
void check(bool ok, const char* what)
{
    if (!ok) { std::printf("FAIL: %s\n", what); ++g_failures; }
}

} // namespace

int main()
{
    bdsp::LaunchCache cache;
    std::atomic<int> queries{0}, raises{0}, wrong{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; ++t)
        pool.emplace_back([&, t] {
            for (int i = 0; i < LOOKUPS; ++i) {
                // interleaved: consecutive lookups of a thread name different devices and keys, and the threads start apart
                const int dev = (i + t) % DEVICES, key = (i / DEVICES + t) % KEYS;
                const Key& k = g_keys[key];
                const int c = cache.lds_limit(dev, k.kernel, k.lds, [&] { ++raises; return 0; });
                const int got = cache.slots(dev, k.kernel, k.threads, k.lds, [&] { ++queries; return device_answer(dev, key); });
                if (c != 0 || got != expected(dev, key)) ++wrong;
            }
        });
    for (auto& th : pool) th.join();
    std::printf("%d threads x %d lookups over %d devices x %d keys: %d queries, %d raises, %d wrong values\n", THREADS, LOOKUPS, DEVICES,
                KEYS, queries.load(), raises.load(), wrong.load());
    check(queries.load() == DEVICES * KEYS, "the query runs exactly once per (device, key): 12 times");
    check(wrong.load() == 0, "every lookup returns the value of its own device, floored at 1");
    // three distinct kernels, one byte count each: one raise per (device, kernel)
    check(raises.load() == DEVICES * 3, "the limit is raised once per (device, kernel)");

    // the limit only grows, per device: a smaller request is served by what is there, a larger one raises again
    int n = 0;
    auto raise = [&] { ++n; return 0; };
    check(cache.lds_limit(0, &g_kernels[0], 65537, raise) == 0 && n == 0, "a smaller request does not lower the limit");
    check(cache.lds_limit(0, &g_kernels[0], 160000, raise) == 0 && n == 1, "a larger request raises it");
    check(cache.lds_limit(0, &g_kernels[0], 148000, raise) == 0 && n == 1, "... and is remembered");
    check(cache.lds_limit(1, &g_kernels[0], 148000, raise) == 0 && n == 2, "... on that device only");
    check(cache.lds_limit(7, &g_kernels[0], 69632, raise) == 0 && n == 3, "a device nobody has used knows nothing");
    // a failed raise is reported and not remembered
    check(cache.lds_limit(2, &g_kernels[0], 200000, [&] { ++n; return -7; }) == -7 && n == 4, "a failed raise returns its code");
    check(cache.lds_limit(2, &g_kernels[0], 200000, raise) == 0 && n == 5, "... and is tried again");
    // a new device asks the occupancy again and gets its own answer, once; another byte count is another key
    int q = 0;
    auto five = [&] { ++q; return 5; };
    const Key& k = g_keys[0];
    check(cache.slots(8, k.kernel, k.threads, k.lds, five) == 5 && q == 1, "a new device asks");
    check(cache.slots(8, k.kernel, k.threads, k.lds, five) == 5 && q == 1, "... once");
    check(cache.slots(0, k.kernel, k.threads, k.lds, five) == expected(0, 0) && q == 1, "... and the first device keeps its own answer");
    check(cache.slots(0, k.kernel, k.threads, k.lds + 16, five) == 5 && q == 2, "another byte count is another key");
    std::printf("%d failures\n%s\n", g_failures, g_failures ? "FAILED" : "ok");
    return g_failures ? 1 : 0;
}
