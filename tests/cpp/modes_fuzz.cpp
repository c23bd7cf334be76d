// modes_fuzz.cpp -- a program of its own over csrc/fmd_modes_decode.cpp (host only), for the address and undefined-behaviour
// sanitizers: random and published messages, damaged and of every length, through fmd_modes_syndrome, fmd_modes_table,
// fmd_modes_decode and fmd_modes_cpr_global, with buffers of exactly the size each call may touch.  Prints `ok decoded N solved N`.
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
    static const char* const kKnown[4] = {"8D4840D6202CC371C32CE0576098", "8D40621D58C382D690C8AC2863A7", "8D40621D58C386435CC412692AD6",
                                          "8D485020994409940838175B284F"};
    unsigned decoded = 0, solved = 0;
    for (uint32_t n_bits : {0u, 55u, 56u, 57u, 112u, 113u}) {
        std::vector<uint32_t> t(n_bits ? n_bits : 1);
        const int rc = fmd_modes_table(n_bits, t.data());
        if ((rc == FMD_OK) != (n_bits == 56 || n_bits == 112)) return 1;
    }
    for (int it = 0; it < 200000; ++it) {
        const size_t len = it % 7 == 0 ? rnd() % 20 : (it & 1 ? 14 : 7);
        std::vector<uint8_t> msg(len ? len : 1);
        if (it % 3 == 0 && len == 14) {
            for (size_t i = 0; i < 14; ++i) { unsigned v; sscanf(kKnown[it % 4] + 2 * i, "%2x", &v); msg[i] = (uint8_t)v; }
            if (it % 6 == 0) msg[4 + rnd() % 7] = (uint8_t)rnd();                      // the ME field, at random
        } else {
            for (uint8_t& b : msg) b = (uint8_t)rnd();
            if (len == 14 && it % 5) msg[0] = (uint8_t)((17 + (rnd() & 1)) << 3 | (rnd() & 7));
        }
        uint32_t syn = 0;
        const int rs = fmd_modes_syndrome(msg.data(), len, &syn);
        if ((rs == FMD_OK) != (len == 7 || len == 14) || syn >> 24) return 2;
        fmd_modes_fields f;
        if (fmd_modes_decode(msg.data(), len, &f) == FMD_OK) {
            ++decoded;
            if (f.callsign[15] != 0 || f.type_code > 31 || f.icao >> 24) return 3;
        }
        double lat = 0, lon = 0;
        const int rc = fmd_modes_cpr_global(rnd() & 0x1FFFF, rnd() & 0x1FFFF, rnd() & 0x1FFFF, rnd() & 0x1FFFF, it & 1, &lat, &lon);
        if (rc == FMD_OK) {
            ++solved;
            if (!(lat >= -90.0001 && lat <= 90.0001 && lon >= -180.0 && lon < 180.0001)) return 4;
        } else if (rc != FMD_ERR_BAD_STATE) return 5;
    }
    if (fmd_modes_cpr_global(1u << 17, 0, 0, 0, 0, nullptr, nullptr) != FMD_ERR_INVALID_ARG) return 6;
    printf("ok decoded %u solved %u\n", decoded, solved);
    return 0;
}
