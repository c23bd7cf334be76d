// hdlc_hostbench -- the host side that tools/bench_hdlc.py measures beside the frame bank: fmd_ax25_decoder_push over every row of a
// call, on `threads` threads (each a contiguous share of the rows), timed in here so that no interpreter stands between two pushes.
// Built by the tool into tools/hdlc_hostbench.so against libfmd_hip.so.
#include "../include/fmd.h"

#include <chrono>
#include <thread>
#include <vector>

extern "C" double hostbench_push(fmd_ax25_decoder** decs, const int16_t* soft, size_t rows, size_t n, size_t cap, unsigned threads,
                                 uint64_t* frames)
{
    std::vector<uint64_t> found(threads, 0);
    std::vector<std::thread> pool;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            fmd_ax25_frame buf[16];
            const size_t lo = rows * t / threads, hi = rows * (t + 1) / threads;
            for (size_t r = lo; r < hi; ++r) {
                size_t k = 0;
                if (fmd_ax25_decoder_push(decs[r], soft + r * cap, n, buf, 16, &k) == FMD_OK) found[t] += k;
            }
        });
    for (std::thread& th : pool) th.join();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t sum = 0;
    for (uint64_t f : found) sum += f;
    if (frames) *frames = sum;
    return s;
}
