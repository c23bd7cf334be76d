// resample_probe.cpp -- prints what fm::resample_taps and fm::resample_ratio of csrc/demod.hpp compute, one `name v0 v1 ...` line
// each, for tests/test_resample.py to compare with the Python package.  Needs the library but no device.
#include <cstdio>

#include "demod.hpp"

int main()
{
    const uint32_t shapes[][3] = {{15, 16, 32}, {3, 16, 64}, {441, 512, 24}, {160, 147, 48}, {6, 1, 8}, {1, 32, 256}, {1, 1, 1}, {1024, 1023, 16}};
    for (const auto& s : shapes) {
        const auto g = fm::resample_taps(s[0], s[1], s[2]);
        printf("taps_%u_%u_%u %u", s[0], s[1], s[2], g.second);
        for (int16_t v : g.first) printf(" %d", (int)v);
        printf("\n");
    }
    const uint64_t rates[][3] = {{51200, 1, 48000}, {1020000, 6, 48000}, {2400000, 40, 48000}, {2048000, 40, 48000}, {44100, 1, 48000}};
    for (const auto& r : rates) {
        const auto lm = fm::resample_ratio(r[0], r[1], r[2]);
        printf("ratio_%llu_%llu_%llu %u %u\n", (unsigned long long)r[0], (unsigned long long)r[1], (unsigned long long)r[2], lm.first, lm.second);
    }
    return 0;
}
