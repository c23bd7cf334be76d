// pocsag_probe.cpp -- for tests/test_fsk.py and tests/test_pocsag.py.  Without arguments: what fm::FskDemod of csrc/demod.hpp answers
// to configurations on both sides of the library's domain (name and status per line; with no device the inside ones are
// FMD_ERR_NO_DEVICE).  `design rate baud`: fm::fsk_design as numbers, or `refused`.  `text baud mode address function n_bits hex`:
// fm::pocsag_text of that message.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "demod.hpp"

static void probe(const char* name, const fmd_fsk_config& cfg, uint32_t rows, uint32_t width)
{
    int rc = FMD_OK;
    try { fm::FskDemod d(cfg, rows, width); }
    catch (const fm::Error& e) { rc = e.status; }
    printf("%s %d\n", name, rc);
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "design")) {
        try {
            const fmd_fsk_config c = fm::fsk_design(strtod(argv[2], nullptr), strtod(argv[3], nullptr));
            printf("%u %u %u %u %u %d %u", c.D, c.W, c.shift, c.sync, c.tol, c.min_corr, c.hit_cap);
            for (uint32_t j = 0; j < 32; ++j) printf(" %u", c.tap[j]);
            printf("\n");
        } catch (const std::invalid_argument&) { printf("refused\n"); }
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "text")) {
        fmd_pocsag_msg m{};
        m.address = (uint32_t)strtoul(argv[4], nullptr, 10); m.function = (uint32_t)strtoul(argv[5], nullptr, 10);
        m.n_bits = (uint32_t)strtoul(argv[6], nullptr, 10);
        const size_t len = strlen(argv[7]) / 2;
        for (size_t i = 0; i < len && i < sizeof m.bits; ++i) {
            const char b[3] = {argv[7][2 * i], argv[7][2 * i + 1], 0};
            m.bits[i] = (uint8_t)strtoul(b, nullptr, 16);
        }
        printf("%s\n", fm::pocsag_text(m, (uint32_t)strtoul(argv[2], nullptr, 10), atoi(argv[3])).c_str());
        return 0;
    }
    const fmd_fsk_config ok = fm::fsk_design(12000, 1200);
    probe("defaults", ok, 1, 1);
    fmd_fsk_config c = ok;
    c.D = 64; c.W = 16; c.shift = 10; c.tap[31] = 255; c.tol = 15; c.min_corr = 1 << 20; c.hit_cap = 64;
    probe("largest", c, 3, 1);
    c = ok; c.D = 65; c.shift = 10; probe("D_65", c, 1, 1);
    c = ok; c.W = 17; c.shift = 10; probe("W_17", c, 1, 1);
    c = ok; c.shift = 2; probe("shift_2", c, 1, 1);
    c = ok; c.shift = 11; probe("shift_11", c, 1, 1);
    c = ok; c.tap[31] = 256; probe("tap_256", c, 1, 1);
    c = ok; c.tol = 16; probe("tol_16", c, 1, 1);
    c = ok; c.min_corr = -1; probe("min_corr_neg", c, 1, 1);
    c = ok; c.hit_cap = 65; probe("hit_cap_65", c, 1, 1);
    probe("rows_0", ok, 0, 1);
    probe("width_2", ok, 1, 2);
    return 0;
}
