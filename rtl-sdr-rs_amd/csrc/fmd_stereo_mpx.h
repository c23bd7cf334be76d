// fmd_stereo_mpx.h -- the multiplex pass (fmd_sto::fmd_stereo_mpx_kernel, fmd_stereo.hip) as the handles that start from the
// multiplex use it: the stereo station bank (fmd_stereo.hip) and the RDS bank (fmd_rds.hip).  The kernel is compiled once, in
// fmd_stereo.hip; this header holds its launch struct, its tiling plan, the launch itself, the host state and call plan of the
// multiplex stage, the pilot report, and the device side of the block sums that both second passes continue.
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

// the largest tile whose LDS stays within the budget: the front end contracts the tile's outputs and the one before them, so a
// tile of the shared sizing (cols = 64 G contracted outputs, the LDS row length) yields cols - 1 outputs
struct MpxTiling { uint32_t groups = 0, tile = 0, cols = 0, raw_bytes = 0; size_t lds = 0; };
inline MpxTiling mpx_tiling(uint32_t D, uint32_t nkc, uint32_t T, uint32_t K)
{
    const FmdDdcTiling t = fmd_ddc_tiling(D, nkc, T, K);
    return MpxTiling{t.groups, t.tile - 1u, t.tile, t.raw_bytes, t.lds};
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

// ---- host state and call plan of the multiplex stage -----------------------------------------------------------------------------

// What a handle that starts from the multiplex holds for it, next to its FmdDdcBank.
struct MpxState {
    MpxTiling tl;
    uint32_t P = 0, pshift = 0;                           // pilot block, log2 of it
    uint32_t pilot_min = 0, inc_p = 0;
    FmdDdcPair ylast;                                     // [S K] packed y
    FmdDdcPair carry;                                     // [S K][4] block carry (long long)
    void* d_x = nullptr; size_t d_x_cap = 0;              // the call's MPX samples
    void* d_sums = nullptr; size_t d_sums_cap = 0;        // the call's block sums
};

// In a *_new, after the bank's front step and before its device step.
inline void mpx_init(FmdDdcBank& b, MpxState& m, uint32_t block, uint32_t pilot_min, uint32_t capture_rate)
{
    m.tl = mpx_tiling(b.D, b.plan.nkc, b.T, b.K);
    m.P = block; m.pilot_min = pilot_min;
    while ((1u << m.pshift) < block) ++m.pshift;
    (void)fmd_stereo_pilot_inc(capture_rate, b.D, &m.inc_p);
    const size_t SK = (size_t)b.S * b.K;
    fmd_ddc_add_pair(b.core, m.ylast, SK * 4);
    fmd_ddc_add_pair(b.core, m.carry, SK * 32);
    fmd_ddc_add_owned(b.core, m.d_x);
    fmd_ddc_add_owned(b.core, m.d_sums);
}

// The counts of one call of a handle whose second filter has Ta taps at stride R and tiles of `na` outputs.
struct MpxCall {
    uint64_t ns;               // samples per stream of the call
    uint64_t mS, mE, M;        // MPX samples before / after the call, of the call
    uint64_t nS, NA;           // second-stage outputs before the call, of the call
    uint64_t jfirst, nbc;      // block of mS, blocks the call touches
    uint64_t SK, nt2;          // rows, second-stage tiles per row
    size_t sums_bytes;
};

// The start of an enqueue: the call checks, the counts, the grid checks, the call-sized scratch, the multiplex pass's launch.
inline int mpx_plan_call(FmdDdcBank& b, MpxState& m, uint32_t Ta, uint32_t R, uint32_t na, const void* d_iq, size_t nbytes,
                         const void* d_out, size_t out_cap, MpxCall& q, MpxLaunch& A)
{
    if (const int rc = fmd_ddc_check_call(nbytes, d_iq, d_out, 4u)) return rc;
    const FmdDdcCore& c = b.core;
    q.ns = nbytes / 2;
    q.mS = fmd_ddc_outputs(b.T, b.D, c.pos); q.mE = fmd_ddc_outputs(b.T, b.D, c.pos + q.ns); q.M = q.mE - q.mS;
    q.nS = fmd_ddc_fir_outputs(Ta, R, q.mS); q.NA = fmd_ddc_fir_outputs(Ta, R, q.mE) - q.nS;
    if (q.NA < 1) { fmd_internal_set_err("the call completes no output"); return FMD_ERR_TOO_SHORT; }
    if (q.NA > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    q.SK = (uint64_t)b.S * b.K;
    const uint64_t nt1 = (q.M + m.tl.tile - 1) / m.tl.tile;
    q.nt2 = (q.NA + na - 1) / na;
    if (nt1 > (1u << 30) || b.S > 65535u || q.nt2 * q.SK > 0x7FFFFFFFull) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }
    q.jfirst = q.mS >> m.pshift; q.nbc = ((q.mE - 1) >> m.pshift) - q.jfirst + 1;
    q.sums_bytes = (size_t)(q.nbc * q.SK * 16);
    FMD_DDC_TRY(fmd_ddc_grow(m.d_x, m.d_x_cap, (size_t)(q.SK * q.M * 2)));
    FMD_DDC_TRY(fmd_ddc_grow(m.d_sums, m.d_sums_cap, q.sums_bytes));

    fmd_ddc_fill_front(A, b, d_iq, nbytes, q.mS);
    A.m0 = q.mS; A.M = (uint32_t)q.M;
    A.tile = m.tl.tile; A.cols = m.tl.cols; A.ntiles = (uint32_t)nt1; A.raw_bytes = m.tl.raw_bytes;
    A.pshift = m.pshift; A.inc_p = m.inc_p; A.jfirst = q.jfirst;
    A.ylast_in = m.ylast.in<uint32_t>(c.cur); A.ylast_out = m.ylast.out<uint32_t>(c.cur);
    A.x = static_cast<int16_t*>(m.d_x);
    A.sums = static_cast<unsigned long long*>(m.d_sums);
    return FMD_OK;
}

// The multiplex pass of the planned call on `stream`, behind the handle's earlier launches.
inline int mpx_enqueue(FmdDdcBank& b, MpxState& m, const MpxCall& q, const MpxLaunch& A, hipStream_t stream)
{
    FMD_DDC_TRY(b.core.order.before(stream));
    FMD_DDC_TRY(hipMemsetAsync(m.d_sums, 0, q.sums_bytes, stream));
    FMD_DDC_TRY(launch_mpx(A, m.tl.lds, stream));
    return FMD_OK;
}

// The fields of a second pass's launch struct that continue the pilot's block sums (same names in both).
template <class Launch>
inline void mpx_fill_blocks(Launch& B, const FmdDdcBank& b, const MpxState& m, const MpxCall& q)
{
    B.x = static_cast<const int16_t*>(m.d_x); B.M = (uint32_t)q.M;
    B.sums = static_cast<const long long*>(m.d_sums);
    B.carry_in = m.carry.in<long long>(b.core.cur); B.carry_out = m.carry.out<long long>(b.core.cur);
    B.SK = (uint32_t)q.SK;
    B.mS = q.mS; B.mE = q.mE; B.jfirst = q.jfirst; B.nS = q.nS;
    B.NA = (uint32_t)q.NA; B.ntiles = (uint32_t)q.nt2;
    B.pshift = m.pshift;
    B.tab = b.core.d_tab;
}

// fmd_stereo_pilot / fmd_rds_pilot: the last complete block of (stream, station)
inline int mpx_pilot(const FmdDdcBank& b, const MpxState& m, uint32_t stream, uint32_t station, int* present, uint32_t* level)
{
    if (!present || !level) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (stream >= b.S || station >= b.K) { fmd_internal_set_err("stream or station out of range"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(b.core.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    long long c[4];
    FMD_DDC_TRY(hipMemcpy(c, m.carry.in<long long>(b.core.cur) + 4ull * ((size_t)stream * b.K + station), sizeof c, hipMemcpyDeviceToHost));
    pilot_report(c[0], c[1], m.pilot_min, m.P, present, level);
    return FMD_OK;
}

// ---- device: the block sums as a second pass reads them ------------------------------------------------------------------------
// `Launch` is the second pass's launch struct; sums, carry_in, carry_out, SK, jfirst, mE and pshift have the same names in both.

// I, Q of block j (>= jfirst - 1, every sample of it already in the sums)
template <class Launch>
__device__ __forceinline__ void block_iq(const Launch& L, uint32_t row, int64_t j, long long& I, long long& Q)
{
    const int64_t jf = (int64_t)L.jfirst;
    if (j < 0) { I = 0; Q = 0; return; }
    if (j == jf - 1) { I = L.carry_in[4u * row]; Q = L.carry_in[4u * row + 1u]; return; }
    const long long* p = L.sums + ((uint64_t)(j - jf) * L.SK + row) * 2u;
    I = p[0]; Q = p[1];
    if (j == jf) { I += L.carry_in[4u * row + 2u]; Q += L.carry_in[4u * row + 3u]; }
}

// the next call's block carry of `row`: the sums of the last complete block, the partial sums of a block that straddles calls
template <class Launch>
__device__ __forceinline__ void write_block_carry(const Launch& L, uint32_t row)
{
    const int64_t jn = (int64_t)(L.mE >> L.pshift);
    long long I = 0, Q = 0, Ip = 0, Qp = 0;
    if (jn >= 1) block_iq(L, row, jn - 1, I, Q);
    if (L.mE & ((1ull << L.pshift) - 1u)) block_iq(L, row, jn, Ip, Qp);
    long long* const c = L.carry_out + 4u * row;
    c[0] = I; c[1] = Q; c[2] = Ip; c[3] = Qp;
}

}  // namespace fmd_sto
