// fmd_stereo_mpx.h -- the multiplex stage and the second stage over it, as the handles that start from the multiplex use them: the
// stereo station bank (fmd_stereo.hip), the RDS bank (fmd_rds.hip) and the receiver bank (fmd_receiver.hip), which runs both second
// stages over one multiplex.
//
// The multiplex pass (fmd_sto::fmd_stereo_mpx_kernel) is compiled once, in fmd_stereo.hip; this header holds its launch struct, its
// tiling plan, the launch itself, the host state and call plan of the multiplex stage and the pilot report.
//
// The second stage is a real FIR at stride R over pairs that a bank forms from the multiplex sample x[m] and the NCO table, with the
// last Ta - 1 pairs carried from call to call.  The banks keep their own pass kernels; the two sides of a second pass and their launch
// structs are in fmd_mpx_passes.h; this header holds what is the same around and inside them: the constructor's checks and steps, the host state, the launch fields both kernels read, the
// enqueue, the entry points' one-liners, and the device skeleton of a second-pass tile (stage_tile) with the block sums it continues.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <new>

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

// ---- the second stage over the multiplex: host ------------------------------------------------------------------------------------

constexpr uint32_t kStageTile = 256;                      // outputs per second-pass tile (at most)

// What a handle holds for a second stage, and the handle with one of them: fmd_stereo and fmd_rds are one each.  The receiver
// (fmd_receiver.hip) holds two stages over the one multiplex.
struct MpxStage {
    uint32_t Ta = 0, R = 0, shift = 0;                    // taps, stride, the output's shift
    uint32_t HX = 0, HXS = 0, na = 0;                     // Ta - 1, its row stride (>= 1), outputs per tile
    void* d_g = nullptr;                                  // int16 taps
    FmdDdcPair ph;                                        // [S K][HXS][2] pair history (int32)
};
struct MpxHandle {
    FmdDdcBank bank;
    MpxState mpx;
    MpxStage st;
};

// The counts of one call: of the multiplex stage, and of a second stage of Ta taps at stride R and tiles of `na` outputs.
struct MpxCall {
    uint64_t ns;               // samples per stream of the call
    uint64_t mS, mE, M;        // MPX samples before / after the call, of the call
    uint64_t jfirst, nbc;      // block of mS, blocks the call touches
    uint64_t SK;               // rows
    size_t sums_bytes;
};
struct StageCall {
    uint64_t nS, NA;           // the stage's outputs before the call, of the call
    uint64_t nt;               // its tiles per row
};

// One output of a call: the stage that forms it and the caller's buffer; mpx_plan_call adds the stage's counts.
struct StageOut {
    const MpxStage* st;
    void* d_out; size_t out_cap;
    StageCall c;
};

// The start of an enqueue of a handle with N second stages over its multiplex: the call checks, the counts, the grid checks, the
// call-sized scratch, the multiplex pass's launch.  A call is accepted only if it completes an output of EVERY stage, so that the
// first output of each stage's first tile is complete (stage_tile).
template <size_t N>
inline int mpx_plan_call(FmdDdcBank& b, MpxState& m, StageOut (&so)[N], const void* d_iq, size_t nbytes, MpxCall& q, MpxLaunch& A)
{
    for (const StageOut& o : so)
        if (const int rc = fmd_ddc_check_call(nbytes, d_iq, o.d_out, 4u)) return rc;
    const FmdDdcCore& c = b.core;
    q.ns = nbytes / 2;
    q.mS = fmd_ddc_outputs(b.T, b.D, c.pos); q.mE = fmd_ddc_outputs(b.T, b.D, c.pos + q.ns); q.M = q.mE - q.mS;
    for (StageOut& o : so) {
        o.c.nS = fmd_ddc_fir_outputs(o.st->Ta, o.st->R, q.mS); o.c.NA = fmd_ddc_fir_outputs(o.st->Ta, o.st->R, q.mE) - o.c.nS;
        if (o.c.NA < 1) { fmd_internal_set_err("the call completes no output"); return FMD_ERR_TOO_SHORT; }
    }
    for (const StageOut& o : so)
        if (o.c.NA > o.out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    q.SK = (uint64_t)b.S * b.K;
    const uint64_t nt1 = (q.M + m.tl.tile - 1) / m.tl.tile;
    uint64_t grid2 = 0;                                      // the second stage's workgroups, all stages
    for (StageOut& o : so) { o.c.nt = (o.c.NA + o.st->na - 1) / o.st->na; grid2 += o.c.nt * q.SK; }
    if (nt1 > (1u << 30) || b.S > 65535u || grid2 > 0x7FFFFFFFull) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }
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

// A bank's config as plain values, and the bank's own names and limits in the refusal texts.
struct StageConfig { uint32_t capture_rate, block, R, shift, pilot_min; };
struct StageLimits { uint32_t rate_floor; const char* decim; const char* taps; const char* shift; uint32_t max_shift; };

inline int stage_refuse(const char* text) { fmd_internal_set_err(text); return FMD_ERR_UNSUPPORTED; }

// The checks of a *_new whose `cfg` is not null, in the order they refuse: what every handle over the multiplex takes (mpx_args;
// `have_taps`: no second-stage tap pointer is null), then each second stage's own (stage_limits; *gsum = sum |g|).
template <class H>
inline int mpx_args(uint32_t rate_floor, const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc,
                    uint32_t n_stations, bool have_taps, uint32_t capture_rate, uint32_t block, const fmd_device_config* dev, H** out)
{
    if (!taps || !phase_inc || !have_taps || !dev || !out || dev->n_channels == 0) { fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG; }
    *out = nullptr;
    if (const int rc = fmd_ddc_front_args(taps, n_taps, decim, shift, n_stations, dev)) return rc;
    char m[160];
    snprintf(m, sizeof m, "need capture_rate >= %u * decim", rate_floor);
    if ((uint64_t)capture_rate < (uint64_t)rate_floor * decim) return stage_refuse(m);
    if (block < 1024u || block > 16384u || (block & (block - 1u)) != 0) return stage_refuse("block must be a power of two in [1024, 16384]");
    return FMD_OK;
}
inline int stage_limits(const StageLimits& lim, const int16_t* g, uint32_t Ta, uint32_t R, uint32_t shift, uint32_t pilot_min, uint64_t* gsum)
{
    char m[160];
    snprintf(m, sizeof m, "need 1 <= %s <= 32, 1 <= n_%s <= 256, %s <= %u, pilot_min <= 16384", lim.decim, lim.taps, lim.shift, lim.max_shift);
    if (R < 1u || R > 32u || Ta < 1u || Ta > 256u || shift > lim.max_shift || pilot_min > 16384u) return stage_refuse(m);
    *gsum = 0;
    for (uint32_t t = 0; t < Ta; ++t) *gsum += (uint64_t)(g[t] < 0 ? -(int)g[t] : g[t]);
    snprintf(m, sizeof m, "sum |%s| > 16383", lim.taps);
    if (*gsum > 16383u) return stage_refuse(m);              // both FIR sums fit 24-bit operands and 32-bit accumulators
    return FMD_OK;
}
template <class H>
inline int stage_args(const StageLimits& lim, const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc,
                      uint32_t n_stations, const int16_t* g, uint32_t Ta, const StageConfig& c, const fmd_device_config* dev, H** out,
                      uint64_t* gsum)
{
    if (const int rc = mpx_args(lim.rate_floor, taps, n_taps, decim, shift, phase_inc, n_stations, g != nullptr, c.capture_rate, c.block, dev, out)) return rc;
    return stage_limits(lim, g, Ta, c.R, c.shift, c.pilot_min, gsum);
}

// In a *_new, after mpx_init: a second stage's derived fields, its history pair and its taps.  `room` is the pairs a tile may
// stage beyond the Ta (or 2 Ta) that the stage's side of the kernel sets aside: R na <= room.
inline void stage_add(FmdDdcBank& b, MpxStage& s, uint32_t R, uint32_t shift, const int16_t* g, uint32_t Ta, uint32_t room)
{
    s.Ta = Ta; s.R = R; s.shift = shift;
    s.HX = Ta - 1u; s.HXS = s.HX ? s.HX : 1u;
    s.na = room / R < kStageTile ? room / R : kStageTile;
    fmd_ddc_add_pair(b.core, s.ph, (size_t)b.S * b.K * s.HXS * 8);
    fmd_ddc_add_owned(b.core, s.d_g, g, 2u * Ta);
}

// A *_new from the handle on: the bank's front step, init(handle) -- mpx_init and a stage_add per second stage -- and the device
// step.  A device that refuses has allocated nothing and the handle is deleted; a failed upload goes through the bank's own *_free.
template <class H, class Init>
inline int mpx_new(const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc, uint32_t n_stations,
                   const fmd_device_config* dev, void (*free_h)(H*), H** out, Init init)
{
    H* h = new (std::nothrow) H();
    if (!h) return FMD_ERR_NOMEM;
    uint64_t bound;
    if (const int rc = fmd_ddc_bank_front(h->bank, taps, n_taps, decim, shift, phase_inc, n_stations, dev, &bound)) { delete h; return rc; }
    init(*h);
    const char* what;
    if (const int rc = fmd_ddc_bank_device(h->bank, dev, &what)) {
        if (!what) { delete h; return rc; }
        fmd_internal_set_err(what); free_h(h); return rc;
    }
    *out = h;
    return FMD_OK;
}
// ... of a handle with one second stage
template <class H>
inline int stage_new(const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc, uint32_t n_stations,
                     const int16_t* g, uint32_t Ta, const StageConfig& c, uint32_t room, const fmd_device_config* dev, void (*free_h)(H*), H** out)
{
    return mpx_new(taps, n_taps, decim, shift, phase_inc, n_stations, dev, free_h, out, [&](H& h) {
        mpx_init(h.bank, h.mpx, c.block, c.pilot_min, c.capture_rate);
        stage_add(h.bank, h.st, c.R, c.shift, g, Ta, room);
    });
}

// What both second passes read: a bank's launch struct is this and the fields of its carrier.
struct StageLaunch {
    const int16_t* x;          // [S K][M]
    uint32_t M;
    const int32_t* ph_in;      // [S K][HXS][2]: the pairs of the HX samples before the call
    int32_t* ph_out;
    uint32_t HX, HXS;          // Ta - 1, row stride (>= 1)
    const long long* sums;     // [nbc][S K][2]
    const long long* carry_in; // [S K][4]: I, Q of block jfirst - 1; partial I, Q of block jfirst from earlier calls
    long long* carry_out;
    uint32_t SK;
    uint64_t mS, mE, jfirst;   // MPX samples before / after the call, block of mS
    uint64_t nS;               // outputs before the call
    uint32_t NA, na, ntiles;   // outputs of the call, per tile, tiles per row
    uint32_t R, Ta, shift, pshift;
    const int16_t* g;
    const uint32_t* tab;
    uint32_t* out;             // [S K][out_stride] packed pairs of int16
    uint64_t out_stride;
};

inline void stage_fill(StageLaunch& B, const FmdDdcBank& b, const MpxState& m, const MpxCall& q, const StageOut& o)
{
    const MpxStage& s = *o.st;
    const int cur = b.core.cur;
    B.x = static_cast<const int16_t*>(m.d_x); B.M = (uint32_t)q.M;
    B.ph_in = s.ph.in<int32_t>(cur); B.ph_out = s.ph.out<int32_t>(cur);
    B.HX = s.HX; B.HXS = s.HXS;
    B.sums = static_cast<const long long*>(m.d_sums);
    B.carry_in = m.carry.in<long long>(cur); B.carry_out = m.carry.out<long long>(cur);
    B.SK = (uint32_t)q.SK;
    B.mS = q.mS; B.mE = q.mE; B.jfirst = q.jfirst; B.nS = o.c.nS;
    B.NA = (uint32_t)o.c.NA; B.na = s.na; B.ntiles = (uint32_t)o.c.nt;
    B.R = s.R; B.Ta = s.Ta; B.shift = s.shift; B.pshift = m.pshift;
    B.g = static_cast<const int16_t*>(s.d_g);
    B.tab = b.core.d_tab;
    B.out = static_cast<uint32_t*>(o.d_out); B.out_stride = o.out_cap;
}

// An enqueue of a handle with one second stage: the call's plan, both launch structs, the multiplex pass, then launch(B, grid) --
// the bank sets its carrier fields and launches its second pass on `grid` workgroups of kThreads -- and the commit.
template <class Launch, class Fn>
inline int stage_enqueue(MpxHandle& h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream,
                         Fn launch)
{
    MpxCall q;
    MpxLaunch A{};
    StageOut so[1] = {{&h.st, d_out, out_cap, {}}};
    if (const int rc = mpx_plan_call(h.bank, h.mpx, so, d_iq, nbytes, q, A)) return rc;
    Launch B{};
    stage_fill(B, h.bank, h.mpx, q, so[0]);
    if (const int rc = mpx_enqueue(h.bank, h.mpx, q, A, stream)) return rc;
    launch(B, (uint32_t)(so[0].c.nt * q.SK));
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(h.bank.core, stream, q.ns);
    if (out_len) *out_len = (size_t)so[0].c.NA;
    return FMD_OK;
}

// a stage's outputs per row since creation or reset
inline uint64_t stage_count(const FmdDdcBank& b, const MpxStage& s)
{
    return fmd_ddc_fir_outputs(s.Ta, s.R, fmd_ddc_outputs(b.T, b.D, b.core.pos));
}

// fmd_stereo_outputs / fmd_rds_outputs
inline int stage_outputs(const MpxHandle* h, uint64_t* outputs)
{
    if (!h || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *outputs = stage_count(h->bank, h->st);
    return FMD_OK;
}

// The pilot report of a handle over the multiplex: the last complete block of (stream, station).
inline int mpx_pilot(const FmdDdcBank& b, const MpxState& m, uint32_t stream, uint32_t station, int* present, uint32_t* level)
{
    if (stream >= b.S || station >= b.K) { fmd_internal_set_err("stream or station out of range"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(b.core.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    long long c[4];
    FMD_DDC_TRY(hipMemcpy(c, m.carry.in<long long>(b.core.cur) + 4ull * ((size_t)stream * b.K + station), sizeof c, hipMemcpyDeviceToHost));
    pilot_report(c[0], c[1], m.pilot_min, m.P, present, level);
    return FMD_OK;
}

// fmd_stereo_pilot / fmd_rds_pilot
inline int stage_pilot(const MpxHandle* h, uint32_t stream, uint32_t station, int* present, uint32_t* level)
{
    if (!h || !present || !level) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return mpx_pilot(h->bank, h->mpx, stream, station, present, level);
}

// ---- the second stage over the multiplex: device ----------------------------------------------------------------------------------

// I, Q of block j (>= jfirst - 1, every sample of it already in the sums)
__device__ __forceinline__ void block_iq(const StageLaunch& L, uint32_t row, int64_t j, long long& I, long long& Q)
{
    const int64_t jf = (int64_t)L.jfirst;
    if (j < 0) { I = 0; Q = 0; return; }
    if (j == jf - 1) { I = L.carry_in[4u * row]; Q = L.carry_in[4u * row + 1u]; return; }
    const long long* p = L.sums + ((uint64_t)(j - jf) * L.SK + row) * 2u;
    I = p[0]; Q = p[1];
    if (j == jf) { I += L.carry_in[4u * row + 2u]; Q += L.carry_in[4u * row + 3u]; }
}

// the next call's block carry of `row`: the sums of the last complete block, the partial sums of a block that straddles calls
__device__ __forceinline__ void write_block_carry(const StageLaunch& L, uint32_t row)
{
    const int64_t jn = (int64_t)(L.mE >> L.pshift);
    long long I = 0, Q = 0, Ip = 0, Qp = 0;
    if (jn >= 1) block_iq(L, row, jn - 1, I, Q);
    if (L.mE & ((1ull << L.pshift) - 1u)) block_iq(L, row, jn, Ip, Qp);
    long long* const c = L.carry_out + 4u * row;
    c[0] = I; c[1] = Q; c[2] = Ip; c[3] = Qp;
}

constexpr uint32_t kStageSlots = 2048;                    // pairs of a kernel's LDS pair buffer (16 KiB)

// One tile of a second pass: one workgroup = one (stream, station) row and up to L.na consecutive outputs of it; `block` is the
// tile's index in [0, L.SK L.ntiles), row-major.  The kernel owns the LDS and hands it in -- ps[kStageSlots] (16-byte aligned),
// gl[256], tab[1024] -- so that a kernel which runs either of two sides (fmd_receiver.hip) holds one set.  `Launch` is the bank's
// launch struct (a StageLaunch), `Pass` the bank's side:
//   kSlots                    LDS slots for the pairs (<= kStageSlots); the host keeps a tile's span within what they hold
//   kCarry                    whether this side writes the next call's block carry: exactly one side of a call does
//   slot(i)                   the slot of the tile's pair i
//   before(L, row, tid, vlo, vhi)   a step of its own before the staging (followed by a barrier)
//   pair(L, tab, m, x)        the pair of multiplex sample m (global index), x = x[m]
//   output(a, b, shift)       the packed output dword from the two FIR sums
//
// Virtual index v of a row: multiplex sample mS - HX + v, so v < HX is the carried history and HX <= v < HX + M the call's own.
// Output n reads the Ta pairs from R n on, hence the tile's first window starts at vlo = R (nS + na0) + HX - mS; the call completes
// that output, so vlo + Ta <= HX + M, i.e. vlo <= M - 1.  A tile stages [vlo, vhi): up to the end of its last window, and in the
// row's last tile up to HX + M, which is further -- the output after the call's last is incomplete, so HX + M < vlo + R cnt + Ta --
// and holds the next call's history, the virtual indices M ... M + HX - 1, all of them >= vlo.  That span is the one the host's
// capacity rule bounds: R na + Ta pairs.
template <class Launch, class Pass>
__device__ __forceinline__ void stage_tile(const Launch& L, Pass pass, uint32_t block, int2* ps, int32_t* gl, int16_t* tab)
{
    static_assert(Pass::kSlots <= kStageSlots, "the side's slots exceed the kernel's pair buffer");
    const uint32_t tid = threadIdx.x;
    const uint32_t row = block / L.ntiles, t = block - row * L.ntiles;
    if (row >= L.SK) return;

    const uint32_t na0 = t * L.na;                           // first output (of this call) of the tile
    const uint32_t cnt = L.NA - na0 < L.na ? L.NA - na0 : L.na;
    const bool last = t == L.ntiles - 1u;
    const uint32_t vlo = (uint32_t)(L.R * (L.nS + na0) + L.HX - L.mS);
    const uint32_t vhi = last ? L.HX + L.M : vlo + L.R * (cnt - 1u) + L.Ta;
    const uint32_t span = vhi - vlo;

    // ---- 1. the bank's own step, the NCO table, the taps ----------------------------------------------------------------------
    pass.before(L, row, tid, vlo, vhi);
    for (uint32_t i = tid; i < 512u; i += fmd_ddc::kThreads) reinterpret_cast<uint32_t*>(tab)[i] = L.tab[i];
    for (uint32_t i = tid; i < L.Ta; i += fmd_ddc::kThreads) gl[i] = L.g[i];
    __syncthreads();

    // ---- 2. the pairs of the tile's samples -------------------------------------------------------------------------------------
    const int16_t* const xr = L.x + (uint64_t)row * L.M;
    const int32_t* const hin = L.ph_in + (uint64_t)row * L.HXS * 2u;
    for (uint32_t i = tid; i < span; i += fmd_ddc::kThreads) {
        const uint32_t v = vlo + i;
        int2 p;
        if (v < L.HX) p = int2{hin[2u * v], hin[2u * v + 1u]};
        else p = pass.pair(L, tab, L.mS + (v - L.HX), (int)xr[v - L.HX]);
        ps[Pass::slot(i)] = p;
    }
    __syncthreads();
    if (last) {                                              // the next call's history
        int32_t* const hout = L.ph_out + (uint64_t)row * L.HXS * 2u;
        for (uint32_t i = tid; i < L.HX; i += fmd_ddc::kThreads) {
            const int2 p = ps[Pass::slot(L.M + i - vlo)];
            hout[2u * i] = p.x; hout[2u * i + 1u] = p.y;
        }
    }
    if (Pass::kCarry && t == 0u && tid == 0u) write_block_carry(L, row);   // the next call's block carry

    // ---- 3. one lane per output: both FIR sums with v_mad_i32_i24 (|g| <= 16383 and the pairs fit 24-bit operands) ------------
    uint32_t* const out = L.out + (uint64_t)row * L.out_stride + na0;
    for (uint32_t i = tid; i < cnt; i += fmd_ddc::kThreads) {
        const uint32_t p0 = L.R * i;
        int a = 0, b = 0;
        for (uint32_t k = 0; k < L.Ta; ++k) {
            const int2 p = ps[Pass::slot(p0 + k)];
            const int gk = gl[k];
            a = __mul24(gk, p.x) + a;
            b = __mul24(gk, p.y) + b;
        }
        out[i] = Pass::output(a, b, L.shift);
    }
}

}  // namespace fmd_sto
