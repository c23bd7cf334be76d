// dcs_probe.cpp -- for tests/test_dcs.py.  Without arguments: what fm::CodeSquelch of csrc/demod.hpp answers to configurations on both
// sides of domain edges, one `name status` line each (status 0: a handle was made; FMD_ERR_NO_DEVICE: the arguments passed and only
// the device was missing).  With `design rate`: fm::dcs_design's entries, one line: block box n_taps lshift tol min_hits confirm hang
// ramp, then the 32 lp, then the 23 tap.  With `words`: fm::dcs_codeword and fm::dcs_word (plain and inverted) of the 104 codes, one
// `code codeword word inverted` line each.  Needs the library but no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "demod.hpp"

static void probe(const char* name, const fmd_dcs_config& cfg, uint32_t n_words, uint32_t rows, uint32_t width)
{
    int status = 0;
    try {
        fm::CodeSquelch sq(cfg, std::vector<uint32_t>(n_words, 0x7FFFFFu), rows, width);
        status = sq.block() == cfg.block ? 0 : 1;
    } catch (const fm::Error& e) {
        status = e.status;
    }
    printf("%s %d\n", name, status);
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "design")) {
        const fmd_dcs_config c = fm::dcs_design(strtod(argv[2], nullptr));
        printf("%u %u %u %u %u %u %u %u %u", c.block, c.box, c.n_taps, c.lshift, c.tol, c.min_hits, c.confirm, c.hang, c.ramp);
        for (uint32_t t = 0; t < c.n_taps; ++t) printf(" %d", c.lp[t]);
        for (uint32_t j = 0; j < 23; ++j) printf(" %u", c.tap[j]);
        printf("\n");
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "words")) {
        for (uint32_t code : fm::dcs_codes())
            printf("%u %u %u %u\n", code, fm::dcs_codeword(code), fm::dcs_word(code), fm::dcs_word(code, true));
        return 0;
    }
    const fmd_dcs_config ok = fm::dcs_design(12000);
    probe("defaults", ok, 104, 3, 2);
    probe("width_3", ok, 104, 1, 3);
    probe("rows_0", ok, 104, 0, 1);
    probe("words_129", ok, 129, 1, 1);
    fmd_dcs_config c = ok;
    c.block = 4100; probe("block_4100", c, 2, 1, 1);
    c = ok; c.block = 32768; probe("block_32768", c, 128, 1, 1);
    c = ok; c.box = 3; probe("box_3", c, 104, 1, 1);
    c = ok; c.n_taps = 65; probe("n_taps_65", c, 104, 1, 1);
    c = ok; c.lp[0] = 1024; probe("lp_1024", c, 104, 1, 1);
    c = ok; c.lshift = 32; probe("lshift_32", c, 104, 1, 1);
    c = ok; c.tap[22] = 512; probe("tap_512", c, 104, 1, 1);
    c = ok; c.tol = 24; probe("tol_24", c, 104, 1, 2);
    c = ok; c.min_hits = 0; probe("min_hits_0", c, 104, 1, 1);
    c = ok; c.confirm = 256; probe("confirm_256", c, 104, 1, 1);
    c = ok; c.hang = 65536; probe("hang_65536", c, 104, 1, 1);
    c = ok; c.ramp = 48; probe("ramp_48", c, 104, 1, 1);
    c = ok; c.tol = 23; c.confirm = 255; c.hang = 65535; c.ramp = 1; c.block = 64; c.box = 64; c.n_taps = 64; c.lshift = 31;
    for (uint32_t j = 1; j < 23; ++j) c.tap[j] = 511;
    probe("largest", c, 128, 1, 2);
    return 0;
}
