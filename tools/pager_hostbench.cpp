// pager_hostbench -- the host side that tools/bench_pager.py measures beside the page bank: fmd_pocsag_decoder_push over the busy
// rows of a call (those with a record, or whose decoder is locked or searching), on `threads` threads (each a contiguous share of
// the listed rows), timed in here so that no interpreter stands between two pushes.  Built by the tool into tools/pager_hostbench.so
// against libfmd_hip.so.
#include "../include/fmd.h"

#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>

extern "C" double hostbench_push(fmd_pocsag_decoder** decs, const int16_t* soft, size_t n, size_t cap, const uint32_t* counts,
                                 const fmd_fsk_hit* hits, size_t hit_cap, const uint32_t* busy, size_t n_busy, unsigned threads,
                                 uint64_t* msgs)
{
    std::vector<uint64_t> found(threads, 0);
    std::vector<std::thread> pool;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            fmd_pocsag_msg buf[16];
            const size_t lo = n_busy * t / threads, hi = n_busy * (t + 1) / threads;
            for (size_t b = lo; b < hi; ++b) {
                const size_t r = busy[b];
                size_t k = 0;
                if (fmd_pocsag_decoder_push(decs[r], soft + r * cap, n, hits + r * hit_cap, std::min<size_t>(counts[r], hit_cap), buf, 16, &k) == FMD_OK)
                    found[t] += k;
            }
        });
    for (std::thread& th : pool) th.join();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t sum = 0;
    for (uint64_t f : found) sum += f;
    if (msgs) *msgs = sum;
    return s;
}
