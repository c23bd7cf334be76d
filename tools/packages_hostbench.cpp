// packages_hostbench -- the host side that tools/bench_packages.py measures beside the package bank: an fmd_pulse_slicer per stream,
// pushed the stream's records of a call, given the idle test and emptied, on `threads` threads (each a contiguous share of the
// streams), timed in here so that no interpreter stands between two pushes.  Built by the tool into tools/packages_hostbench.so
// against libfmd_hip.so.
#include "../include/fmd.h"

#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>

extern "C" double hostbench_push(fmd_pulse_slicer** slicers, const uint32_t* counts, const fmd_pulses_rec* recs, size_t rec_cap,
                                 const fmd_pulses_totals* totals, uint64_t n_samples, size_t n_streams, unsigned threads, uint64_t* packages)
{
    std::vector<uint64_t> found(threads, 0);
    std::vector<std::thread> pool;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            fmd_pulse_package buf[64];
            const size_t lo = n_streams * t / threads, hi = n_streams * (t + 1) / threads;
            for (size_t s = lo; s < hi; ++s) {
                fmd_pulse_slicer_push(slicers[s], recs + s * rec_cap, std::min<size_t>(counts[s], rec_cap), totals[s].samples - n_samples);
                fmd_pulse_slicer_idle(slicers[s], totals[s].state, totals[s].run);
                size_t k = 0;
                while (fmd_pulse_slicer_take(slicers[s], buf, 64, &k) == FMD_OK && k) found[t] += k;
            }
        });
    for (std::thread& th : pool) th.join();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t sum = 0;
    for (uint64_t f : found) sum += f;
    if (packages) *packages = sum;
    return s;
}
