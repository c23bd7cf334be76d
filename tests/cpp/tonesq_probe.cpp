// tonesq_probe.cpp -- for tests/test_tonesq.py.  Without arguments: what fm::ToneSquelch of csrc/demod.hpp answers to configurations
// on both sides of domain edges, one `name status` line each (status 0: a handle was made; FMD_ERR_NO_DEVICE: the arguments passed
// and only the device was missing).  With `table rate block f0 f1 ...`: fm::tone_table's entries, one `c s` line per (tone, r).
// Needs the library but no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "demod.hpp"

static void probe(const char* name, fmd_tonesq_config cfg, uint32_t n_tones, uint32_t rows, uint32_t width)
{
    int status = 0;
    try {
        fm::ToneSquelch sq(cfg, std::vector<int16_t>((size_t)n_tones * cfg.block * 2, 1023), rows, width);
        status = sq.block() == cfg.block ? 0 : 1;
    } catch (const fm::Error& e) {
        status = e.status;
    }
    printf("%s %d\n", name, status);
}

int main(int argc, char** argv)
{
    if (argc > 4 && !strcmp(argv[1], "table")) {
        std::vector<double> freqs;
        for (int i = 4; i < argc; ++i) freqs.push_back(strtod(argv[i], nullptr));
        const uint32_t block = (uint32_t)strtoul(argv[3], nullptr, 10);
        const std::vector<int16_t> tab = fm::tone_table(strtod(argv[2], nullptr), freqs, block);
        for (size_t i = 0; i < tab.size(); i += 2) printf("%d %d\n", tab[i], tab[i + 1]);
        return 0;
    }
    const fmd_tonesq_config ok{4096, 1, 3, 2, 2, 64, 20000000ull, ~0ull};
    probe("defaults", ok, 38, 3, 2);
    probe("width_3", ok, 38, 1, 3);
    probe("rows_0", ok, 38, 0, 1);
    probe("tones_65", ok, 65, 1, 1);
    fmd_tonesq_config c = ok;
    c.block = 48; probe("block_48", c, 2, 1, 1);
    c = ok; c.block = 8192; c.ramp = 8192; probe("block_8192", c, 32, 1, 1);
    c = ok; c.block = 8192; probe("product_33", c, 33, 1, 1);
    c = ok; c.guard = 64; probe("guard_64", c, 38, 1, 1);
    c = ok; c.dom_shift = 33; probe("dom_shift_33", c, 38, 1, 2);
    c = ok; c.min_power = 0; probe("min_power_0", c, 38, 1, 1);
    c = ok; c.confirm = 256; probe("confirm_256", c, 38, 1, 1);
    c = ok; c.hang = 65536; probe("hang_65536", c, 38, 1, 1);
    c = ok; c.ramp = 48; probe("ramp_48", c, 38, 1, 1);
    c = ok; c.guard = 63; c.dom_shift = 32; c.confirm = 255; c.hang = 65535; c.ramp = 1; c.block = 64; probe("largest", c, 64, 1, 2);
    return 0;
}
