// fmd_stations_common.h -- host plan of the station bank (fmd_stations.hip): the NCO table, the complex taps of every
// (stream, station), the matrix-core A fragments and the domain bound.  Definition: include/fmd.h, "station bank".
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

// TAB[i] = round(16384 cos(2 pi i / 1024)); no entry lies near a rounding tie, so any libm gives the same table.
inline void fmd_st_nco_table(int16_t* tab)
{
    const double two_pi = 6.28318530717958647692528676655900577;
    for (int i = 0; i < 1024; ++i) tab[i] = (int16_t)std::lround(16384.0 * std::cos(two_pi * i / 1024.0));
}
inline int fmd_st_cosq(const int16_t* tab, uint32_t phi) { return tab[phi >> 22]; }
inline int fmd_st_sinq(const int16_t* tab, uint32_t phi) { return tab[((phi >> 22) - 256u) & 1023u]; }

// W[t] = rnd(h[t] cosq(t inc)) + j rnd(-h[t] sinq(t inc)), rnd(v) = (v + 8192) >> 14 (arithmetic shift): |W| <= 2047.
inline void fmd_st_complex_taps(const int16_t* h, uint32_t n_taps, uint32_t inc, const int16_t* tab, int32_t* wr, int32_t* wi)
{
    for (uint32_t t = 0; t < n_taps; ++t) {
        const uint32_t phi = t * inc;                                    // mod 2^32
        wr[t] = (h[t] * fmd_st_cosq(tab, phi) + 8192) >> 14;
        wi[t] = (-h[t] * fmd_st_sinq(tab, phi) + 8192) >> 14;
    }
}

// The tap matrix of one stream on the matrix cores (v_mfma_i32_16x16x64_i8, A = 16 rows x 64 bytes per K chunk).  Rows:
//   two digits (any |W| <= 2047): row 4 i + (zr_lo, zr_hi, zi_lo, zi_hi) of station 4 rt + i, W = 128 hi + lo (|lo| <= 64, |hi| <= 16);
//   one digit (every |W| <= 127): row 2 i + (zr, zi) of station 8 rt + i.
// K index = byte offset from a 16-byte aligned LDS address; the window of the column's output starts `delta` bytes (0, 4, 8, 12)
// further, byte 2 t is I and 2 t + 1 is Q of sample t.  With B = b - 128 (the staged bytes xor 0x80, as s8) the sample is
// c = (B_I + 1) + j (B_Q + 1), so
//   zr = sum Wr cI - Wi cQ  -> I weight Wr, Q weight -Wi, constant sum (Wr - Wi)
//   zi = sum Wi cI + Wr cQ  -> I weight Wi, Q weight  Wr, constant sum (Wr + Wi).
struct FmdStationsPlan {
    uint32_t K = 0, T = 0, S = 0;
    uint32_t digits = 2;              // i8 digits per tap
    uint32_t spt = 4;                 // stations per row tile (4: two digits, 8: one)
    uint32_t nrt = 0, nkc = 0;        // row tiles, 64-byte K chunks
    std::vector<uint32_t> amat;       // [S][4 deltas][nrt][nkc][64 lanes][4 dwords]
    std::vector<int32_t> kconst;      // [S][K][2]: the additive constants of zr, zi
    std::vector<uint32_t> dinc;       // [S][K]: decim * inc mod 2^32 (output rotation step)
    uint64_t max_gain = 0;            // max over (stream, station) of sum_t |Wr| + |Wi|
};

inline int fmd_st_a_entry(const int32_t* wr, const int32_t* wi, uint32_t T, uint32_t comp, uint32_t kb, uint32_t delta)
{
    if (kb < delta || kb - delta >= 2u * T) return 0;
    const uint32_t u = kb - delta, t = u >> 1, q = u & 1u;
    return comp == 0u ? (q ? -wi[t] : wr[t]) : (q ? wr[t] : wi[t]);
}

inline void fmd_st_build_plan(const int16_t* h, uint32_t T, uint32_t decim, const uint32_t* inc, uint32_t S, uint32_t K,
                              FmdStationsPlan& P)
{
    int16_t tab[1024];
    fmd_st_nco_table(tab);
    P.K = K; P.T = T; P.S = S;
    std::vector<int32_t> wr((size_t)S * K * T), wi((size_t)S * K * T);
    bool small = true;
    P.max_gain = 0;
    P.kconst.assign((size_t)S * K * 2, 0);
    P.dinc.assign((size_t)S * K, 0u);
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t k = 0; k < K; ++k) {
            const size_t sk = (size_t)s * K + k;
            int32_t* r = &wr[sk * T];
            int32_t* i = &wi[sk * T];
            fmd_st_complex_taps(h, T, inc[sk], tab, r, i);
            uint64_t g = 0;
            int64_t cre = 0, cim = 0;
            for (uint32_t t = 0; t < T; ++t) {
                g += (uint64_t)(r[t] < 0 ? -r[t] : r[t]) + (uint64_t)(i[t] < 0 ? -i[t] : i[t]);
                if (r[t] > 127 || r[t] < -127 || i[t] > 127 || i[t] < -127) small = false;
                cre += r[t] - i[t];
                cim += r[t] + i[t];
            }
            if (g > P.max_gain) P.max_gain = g;
            P.kconst[2 * sk] = (int32_t)cre;
            P.kconst[2 * sk + 1] = (int32_t)cim;
            P.dinc[sk] = decim * inc[sk];
        }
    P.digits = small ? 1u : 2u;
    P.spt = small ? 8u : 4u;
    P.nrt = (K + P.spt - 1u) / P.spt;
    P.nkc = (12u + 2u * T + 63u) / 64u;
    P.amat.assign((size_t)S * 4 * P.nrt * P.nkc * 64 * 4, 0u);
    uint8_t* ab = reinterpret_cast<uint8_t*>(P.amat.data());
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t dl = 0; dl < 4; ++dl)
            for (uint32_t rt = 0; rt < P.nrt; ++rt)
                for (uint32_t kc = 0; kc < P.nkc; ++kc)
                    for (uint32_t lane = 0; lane < 64; ++lane) {
                        const uint32_t row = lane & 15u, q = lane >> 4;
                        uint32_t k, comp, dsel;
                        if (small) { k = 8u * rt + (row >> 1); comp = row & 1u; dsel = 0u; }
                        else { k = 4u * rt + (row >> 2); comp = (row >> 1) & 1u; dsel = 1u + (row & 1u); }
                        if (k >= K) continue;
                        const size_t sk = (size_t)s * K + k;
                        const size_t base = ((((((size_t)s * 4 + dl) * P.nrt + rt) * P.nkc + kc) * 64) + lane) * 16;
                        for (uint32_t b = 0; b < 16; ++b) {
                            const int v = fmd_st_a_entry(&wr[sk * T], &wi[sk * T], T, comp, 64u * kc + 16u * q + b, 4u * dl);
                            const int lo = ((v + 64) & 127) - 64, hi = (v - lo) / 128;
                            ab[base + b] = (uint8_t)(int8_t)(dsel == 0u ? v : (dsel == 1u ? lo : hi));
                        }
                    }
}
