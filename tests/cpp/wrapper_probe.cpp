// wrapper_probe.cpp -- prints what the host-side designers and defaults of csrc/demod.hpp compute, one `name v0 v1 ...` line
// each, for tests/test_cpp_wrapper.py to compare with the Python package.  Needs the library but no device.
#include <cstdio>

#include "demod.hpp"

static void dump(const char* name, const std::vector<int16_t>& v)
{
    printf("%s", name);
    for (int16_t x : v) printf(" %d", (int)x);
    printf("\n");
}

static void dump_narrow(const char* name, double rate, double lo, double hi)
{
    const auto g = fm::narrow_taps(rate, 256, lo, hi);
    dump((std::string(name) + "_re").c_str(), g.first);
    dump((std::string(name) + "_im").c_str(), g.second);
}

int main()
{
    for (const int f_m : {170000, 240000}) {
        const std::string r = std::to_string(f_m);
        dump(("stereo_" + r).c_str(), fm::stereo_taps(f_m, 127));
        const auto g = fm::rds_taps(f_m, 255);
        dump(("rds_" + r).c_str(), g.first);
        printf("rds_shift_%s %u\n", r.c_str(), g.second);
        // the CLI's default bands (-N am / iq and fm / usb / lsb) and the issue's two
        dump_narrow(("narrow_am_" + r).c_str(), f_m, -4000, 4000);
        dump_narrow(("narrow_fm_" + r).c_str(), f_m, -6000, 6000);
        dump_narrow(("narrow_usb_" + r).c_str(), f_m, 300, 3000);
        dump_narrow(("narrow_lsb_" + r).c_str(), f_m, -3000, -300);
    }
    const auto u = fm::uniform_taps(16, 8);
    dump("uniform_16_8", u);
    printf("uniform_shift_16_8 %u\n", fm::uniform_auto_shift(u, 16));
    printf("uniform_shift_16_8_sel %u\n", fm::uniform_auto_shift(u, 16, {0, 3, 15}));
    // the named defaults at the example's capture rates: -s values whose downsample is 2, 6, 10 and 64
    for (const uint32_t rate : {600000u, 170000u, 110000u, 15800u}) {
        const auto settings = fm::optimal_settings(94900000, rate);
        const uint32_t capture = settings.first.capture_rate, D = settings.second.downsample, f_m = capture / D;
        const std::string r = std::to_string(rate);
        const uint32_t shift = fm::boxcar_shift(D, 16384);
        printf("front_%s %u %u %u %u %llu\n", r.c_str(), capture, D, fm::boxcar_shift(D, 256), shift,
               (unsigned long long)fm::boxcar_y_bound(D, shift));
        printf("pilot_min_%s %u\n", r.c_str(), fm::default_pilot_min(capture, D));
        printf("audio_shift_%s %u\n", r.c_str(), fm::default_audio_shift(fm::stereo_taps(f_m, 127), capture, D));
        const struct { const char* mode; double lo, hi; uint64_t limit; } bands[] = {
            {"am", -4000, 4000, 16384}, {"fm", -6000, 6000, 256}, {"usb", 300, 3000, 16384}, {"lsb", -3000, -300, 16384}};
        for (const auto& b : bands) {
            const auto g = fm::narrow_taps(f_m, 256, b.lo, b.hi);
            printf("chan_shift_%s_%s %u\n", b.mode, r.c_str(), fm::narrow_chan_shift(fm::boxcar_y_bound(D, shift), g.first, g.second, b.limit));
        }
        const auto h = fm::rds_front_taps(capture);
        dump(("rds_front_" + r).c_str(), h.first);
        printf("rds_front_shift_%s %u\n", r.c_str(), h.second);
    }
    return 0;
}
