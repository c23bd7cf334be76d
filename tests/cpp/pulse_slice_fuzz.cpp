// pulse_slice_fuzz.cpp -- a program of its own over csrc/fmd_pulse_slice.cpp (host only), for the address and undefined-behaviour
// sanitizers: random record lists, with widths and gaps on every side of the windows and at both ends of their range, through
// fmd_pulse_slicer_push, _idle and _take, with buffers of exactly the size each call may touch.  Prints `ok packages N bits N`.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fmd.h"

void fmd_internal_set_err(const char*) {}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

int main()
{
    unsigned long long packages = 0, bits = 0;
    fmd_pulse_slicer* bad = nullptr;
    const fmd_pulse_slicer_config none{2, 1, 1, 0, 1};
    if (fmd_pulse_slicer_new(&none, &bad) != FMD_ERR_UNSUPPORTED || bad) return 1;
    if (fmd_pulse_slicer_new(nullptr, &bad) != FMD_ERR_INVALID_ARG) return 1;
    for (int it = 0; it < 400; ++it) {
        const fmd_pulse_slicer_config cfg{rnd() & 1u, 1u + rnd() % 40u, 1u + rnd() % 80u, it % 9 == 0 ? 0xFFFFFFFFu : rnd() % 8u, 1u + rnd() % 200u};
        fmd_pulse_slicer* p = nullptr;
        if (fmd_pulse_slicer_new(&cfg, &p) != FMD_OK || !p) return 2;
        uint64_t pos = it % 5 == 0 ? 0xFFFFFFFFFFFF0000ull : 0;
        for (int call = 0; call < 60; ++call) {
            const size_t n = rnd() % 50;
            std::vector<fmd_pulses_rec> recs(n);                 // (exactly n: a read beyond it is an error)
            for (fmd_pulses_rec& r : recs) {
                const uint32_t pick[6] = {cfg.short_w, cfg.long_w, cfg.short_w + cfg.tol, rnd() % 300u, 0xFFFFFFFFu, 0u};
                r.k_rel = (int32_t)(rnd() % 100000u);
                r.width = pick[rnd() % 6];
                r.gap = it % 7 == 0 ? rnd() % cfg.reset : pick[rnd() % 6];      // (some runs keep one package open: truncation)
                r.level = rnd();
            }
            if (fmd_pulse_slicer_push(p, recs.data(), n, pos) != FMD_OK) return 3;
            if (fmd_pulse_slicer_idle(p, rnd() & 1u, rnd() % 400u) != FMD_OK) return 4;
            if (call % 4 == 3) {
                const size_t cap = rnd() % 70;
                std::vector<fmd_pulse_package> out(cap);
                size_t got = 99999;
                if (fmd_pulse_slicer_take(p, out.data(), cap, &got) != FMD_OK || got > cap || got > 64) return 5;
                for (size_t i = 0; i < got; ++i) {
                    if (out[i].n_bits > 256 || out[i].n_pulses == 0 || (out[i].flags & ~3u) || out[i].rsv) return 6;
                    for (uint32_t b = out[i].n_bits; b < 256; ++b)
                        if (out[i].bits[b >> 3] & (0x80u >> (b & 7u))) return 7;                 // nothing set behind the bits
                    ++packages; bits += out[i].n_bits;
                }
            }
            pos += 100000;
        }
        fmd_pulse_slicer_free(p);
    }
    fmd_pulse_slicer_free(nullptr);
    printf("ok packages %llu bits %llu\n", packages, bits);
    return 0;
}
