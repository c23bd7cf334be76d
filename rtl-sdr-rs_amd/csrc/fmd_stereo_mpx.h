// fmd_stereo_mpx.h -- the multiplex pass (fmd_sto::fmd_stereo_mpx_kernel, fmd_stereo.hip) as the handles that start from the
// multiplex use it: the stereo station bank (fmd_stereo.hip) and the RDS bank (fmd_rds.hip).  The kernel is compiled once, in
// fmd_stereo.hip; this header holds its launch struct, its tiling plan, the launch itself and the host side of the pilot report.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "fmd_ddc.h"

namespace fmd_sto {

struct MpxLaunch {
    const uint8_t* iq;         // [S][nbytes]
    uint64_t nbytes;
    const uint8_t* hist_in;    // [S][HB]
    uint8_t* hist_out;
    uint32_t HB;
    uint32_t vb_first;         // virtual byte of the window of the call's first output
    uint64_t m0;               // global index of the call's first output
    uint32_t M;                // outputs of this call per (stream, station)
    uint32_t D, T, K, S, shift;
    uint32_t nrt, nkc, digits;
    uint32_t tile, cols;       // outputs per tile (cols - 1), LDS row length
    uint32_t ntiles, raw_bytes;
    uint32_t pshift, inc_p;    // log2 P, pilot step
    uint64_t jfirst;           // block of the call's first output
    const uint32_t* amat;
    const int32_t* kconst;
    const uint32_t* dinc;
    const uint32_t* tab;
    const uint32_t* ylast_in;  // [S K]: y[m0 - 1], packed
    uint32_t* ylast_out;
    int16_t* x;                // [S K][M]
    unsigned long long* sums;  // [nbc][S K][2]: I, Q of block jfirst + i, this call's samples only
};

// grid (A.ntiles, A.S), `lds` bytes of dynamic LDS (mpx_tiling), on `stream`; A.sums zeroed by the caller
hipError_t launch_mpx(const MpxLaunch& A, size_t lds, hipStream_t stream);

constexpr size_t kMpxLdsBudget = 40960;

inline size_t mpx_lds(uint32_t D, uint32_t nkc, uint32_t T, uint32_t K, uint32_t G, uint32_t* raw_bytes)
{
    const uint64_t cap = 64ull * G;                       // contracted outputs per tile (the tile's and the one before)
    const uint64_t reads = 12 + 6ull * D + 8ull * D * (16 * G - 1) + 64ull * nkc;
    const uint64_t staged = 12 + 2ull * D * (cap - 1) + 2ull * T + 15;
    const uint64_t raw = ((reads > staged ? reads : staged) + 15) & ~15ull;
    *raw_bytes = (uint32_t)raw;
    return (size_t)(raw + fmd_ddc::kTableBytes + 4ull * K * cap);
}

// the largest tile whose LDS stays within the budget
struct MpxTiling { uint32_t groups = 0, tile = 0, cols = 0, raw_bytes = 0; size_t lds = 0; };
inline MpxTiling mpx_tiling(uint32_t D, uint32_t nkc, uint32_t T, uint32_t K)
{
    MpxTiling t;
    for (uint32_t G = fmd_ddc::kGroups; G >= 1; --G) {
        uint32_t rb;
        const size_t l = mpx_lds(D, nkc, T, K, G, &rb);
        if (l <= kMpxLdsBudget || G == 1) { t.groups = G; t.cols = 64u * G; t.tile = 64u * G - 1u; t.raw_bytes = rb; t.lds = l; break; }
    }
    return t;
}

inline uint64_t isqrt_u128(unsigned __int128 v)
{
    uint64_t r = (uint64_t)std::sqrt((double)v);
    while ((unsigned __int128)r * r > v) --r;
    while ((unsigned __int128)(r + 1) * (r + 1) <= v) ++r;
    return r;
}

// present_j and the level of the block whose correlations are I, Q (include/fmd.h, fmd_stereo_pilot)
inline void pilot_report(long long I, long long Q, uint32_t pilot_min, uint32_t P, int* present, uint32_t* level)
{
    const unsigned __int128 e2 = (unsigned __int128)((__int128)I * I) + (unsigned __int128)((__int128)Q * Q);
    const uint64_t thr = (uint64_t)pilot_min * P * 8192u;
    *present = thr != 0 && e2 >= (unsigned __int128)thr * thr ? 1 : 0;
    *level = (uint32_t)(isqrt_u128(e2) / ((uint64_t)P * 8192u));
}

}  // namespace fmd_sto
