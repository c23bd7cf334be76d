// fmd_chan_stage.h -- the second stage that the narrow-band bank (fmd_narrow.hip) and the band-plan bank (fmd_bandplan.hip) share:
// a complex decimating FIR over a first stage's y, one of four detectors, a block-wise squelch (include/fmd.h, "narrow-band
// bank").  The two banks keep their own pass-2 kernels, launch structs and packed tap layouts; this header holds what is the same
// around them: the constructor's checks and derived fields, the host state, the counts and refusals of a call, the launch fields
// both kernels read, the level report, and the two device helpers both kernels use.
#pragma once

#include "fmd_ddc.h"

namespace fmd_chan {

constexpr uint32_t kCarry = 6;                            // u64 per row: E part, A part, E last, u[n - 1], dc, open

// ---- device ---------------------------------------------------------------------------------------------------------------------

// floor(sqrt(x)), x <= 2^29: the f32 estimate is within 1 of it
__device__ __forceinline__ uint32_t isqrt29(uint32_t x)
{
    uint32_t r = (uint32_t)__builtin_amdgcn_sqrtf((float)x);
    r -= (r * r > x) ? 1u : 0u;
    r += ((r + 1u) * (r + 1u) <= x) ? 1u : 0u;
    return r;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- host state -----------------------------------------------------------------------------------------------------------------

// What a handle with this second stage holds for it, next to its FmdDdcBank.  `pitch` (the LDS row pitch of the polyphase staging)
// follows from the handle's own tile and tap layout: the handle sets it, and registers its packed taps as d_g.
struct ChanStage {
    uint32_t Ta = 0, R = 0, P = 0, pshift = 0, chan_shift = 0, mode = 0, squelch = 0, gain = 0, width = 1;
    uint32_t HX = 0, HXS = 0, pitch = 0, rinv = 0;        // Ta - 1, its row stride (>= 1), ..., ceil(2^32 / R) (R >= 2)
    bool cplx = false;
    void* d_g = nullptr;                                  // the packed taps
    FmdDdcPair yh;                                        // [S K][HXS] y history (packed dwords)
    FmdDdcPair carry;                                     // [S K][kCarry] (u64)
    void* d_y = nullptr; size_t d_y_cap = 0;              // the call's y
};

// ---- constructor ----------------------------------------------------------------------------------------------------------------

// The config and the channel taps, for a bank that takes chan_decim <= max_R and n_chan_taps <= max_Ta.
// *gsum = sum |gr| + |gi|, *cplx = some gi != 0.
inline int chan_args(const fmd_narrow_config* cfg, const int16_t* re, const int16_t* im, uint32_t Ta, uint32_t max_R, uint32_t max_Ta,
                     uint64_t* gsum, bool* cplx)
{
    const uint32_t R = cfg->chan_decim, P = cfg->block;
    if (cfg->mode > FMD_NARROW_SSB || R < 1u || R > max_R || Ta < 1u || Ta > max_Ta || cfg->chan_shift > 30u || cfg->squelch > 23170u ||
        cfg->gain < 1u || cfg->gain > 65535u) {
        char m[160];
        snprintf(m, sizeof m, "need mode <= 3, 1 <= chan_decim <= %u, 1 <= n_chan_taps <= %u, chan_shift <= 30, squelch <= 23170, 1 <= gain <= 65535",
                 max_R, max_Ta);
        fmd_internal_set_err(m);
        return FMD_ERR_UNSUPPORTED;
    }
    if (P < 16u || P > 4096u || (P & (P - 1u)) != 0) { fmd_internal_set_err("block must be a power of two in [16, 4096]"); return FMD_ERR_UNSUPPORTED; }
    *gsum = 0;
    *cplx = false;
    for (uint32_t t = 0; t < Ta; ++t) {
        const int gr = re[t], gi = im ? im[t] : 0;
        if (gr > 16383 || gr < -16383 || gi > 16383 || gi < -16383) { fmd_internal_set_err("|chan tap| > 16383"); return FMD_ERR_UNSUPPORTED; }
        *gsum += (uint64_t)(gr < 0 ? -gr : gr) + (uint64_t)(gi < 0 ? -gi : gi);
        if (gi) *cplx = true;
    }
    if (*gsum > 65535u) { fmd_internal_set_err("sum |gr| + |gi| > 65535"); return FMD_ERR_UNSUPPORTED; }
    return FMD_OK;
}

// |u| <= 16384 per component: `bound` is the first stage's B_y
inline int chan_gain_ok(uint64_t bound, uint64_t gsum, uint32_t chan_shift)
{
    if (((bound * gsum + ((1ull << chan_shift) - 1ull)) >> chan_shift) <= 16384ull) return FMD_OK;
    fmd_internal_set_err("channel filter gain too large: need ceil(B_y * sum(|gr| + |gi|) / 2^chan_shift) <= 16384");
    return FMD_ERR_UNSUPPORTED;
}

// In a *_new, once b.S and b.K are set and before the bank's device step: the derived fields, the two state pairs and the call's
// y buffer.
inline void chan_init(FmdDdcBank& b, ChanStage& c, const fmd_narrow_config* cfg, uint32_t Ta, bool cplx)
{
    const uint32_t R = cfg->chan_decim;
    c.Ta = Ta; c.R = R; c.P = cfg->block; c.chan_shift = cfg->chan_shift; c.mode = cfg->mode;
    c.squelch = cfg->squelch; c.gain = cfg->gain; c.width = cfg->mode == FMD_NARROW_IQ ? 2u : 1u; c.cplx = cplx;
    while ((1u << c.pshift) < c.P) ++c.pshift;
    c.HX = Ta - 1u; c.HXS = c.HX ? c.HX : 1u;
    c.rinv = R >= 2u ? (uint32_t)(((1ull << 32) + R - 1u) / R) : 0u;
    const size_t SK = (size_t)b.S * b.K;
    fmd_ddc_add_pair(b.core, c.yh, SK * c.HXS * 4);
    fmd_ddc_add_pair(b.core, c.carry, SK * kCarry * 8);
    fmd_ddc_add_owned(b.core, c.d_y);
}

// ---- calls ----------------------------------------------------------------------------------------------------------------------

// audio samples completed once `samples` samples per stream have arrived
inline uint64_t chan_audio(const FmdDdcBank& b, const ChanStage& c, uint64_t samples)
{
    return fmd_ddc_fir_outputs(c.Ta, c.R, fmd_ddc_outputs(b.T, b.D, samples));
}

// The counts of one call: samples per stream; y before the call, of the call; audio samples before the call, of the call; rows;
// dwords of a row of the call's y (a multiple of 4).
struct ChanCall { uint64_t ns, mS, M, nS, NA, SK, ystride; };

// The start of an enqueue: the call checks, the counts, the refusals, the call's y buffer.
inline int chan_plan_call(FmdDdcBank& b, ChanStage& c, size_t nbytes, const void* d_iq, const void* d_out, size_t out_cap, ChanCall& q)
{
    if (const int rc = fmd_ddc_check_call(nbytes, d_iq, d_out, 2u * c.width)) return rc;
    const uint64_t pos = b.core.pos;
    q.ns = nbytes / 2;
    q.mS = fmd_ddc_outputs(b.T, b.D, pos); q.M = fmd_ddc_outputs(b.T, b.D, pos + q.ns) - q.mS;
    q.nS = chan_audio(b, c, pos); q.NA = chan_audio(b, c, pos + q.ns) - q.nS;
    if (q.NA < 1) { fmd_internal_set_err("the call completes no audio sample"); return FMD_ERR_TOO_SHORT; }
    if (q.NA > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    q.SK = (uint64_t)b.S * b.K;
    q.ystride = (q.M + 3) & ~3ull;
    FMD_DDC_TRY(fmd_ddc_grow(c.d_y, c.d_y_cap, (size_t)(q.SK * q.ystride * 4)));
    return FMD_OK;
}

// The fields of a pass-2 launch struct that both kernels read (same names in both).  The tile count and the fields of the
// kernel's own tap layout are the caller's.
template <class Launch>
inline void chan_fill(Launch& B, const FmdDdcBank& b, const ChanStage& c, const ChanCall& q, void* d_out, size_t out_cap)
{
    const int cur = b.core.cur;
    B.y = static_cast<const uint32_t*>(c.d_y); B.ystride = (uint32_t)q.ystride; B.M = (uint32_t)q.M;
    B.yh_in = c.yh.in<uint32_t>(cur); B.yh_out = c.yh.out<uint32_t>(cur);
    B.HX = c.HX; B.HXS = c.HXS;
    B.carry_in = c.carry.in<unsigned long long>(cur); B.carry_out = c.carry.out<unsigned long long>(cur);
    B.SK = (uint32_t)q.SK;
    B.yoff0 = (int32_t)((int64_t)(c.R * q.nS) - (int64_t)q.mS);
    B.nS = q.nS; B.NA = (uint32_t)q.NA;
    B.R = c.R; B.rinv = c.rinv; B.pitch = c.pitch; B.Ta = c.Ta;
    B.chan_shift = c.chan_shift; B.pshift = c.pshift; B.mode = c.mode; B.gain = c.gain;
    B.thr = (uint64_t)c.squelch * c.squelch * c.P;
    B.g = static_cast<decltype(B.g)>(c.d_g);
    B.out = static_cast<int16_t*>(d_out); B.out_cap = out_cap;   // samples per row: int16 each, a dword each in IQ mode
}

// ---- the level report -----------------------------------------------------------------------------------------------------------

inline uint32_t isqrt_u64(uint64_t v)
{
    uint64_t r = (uint64_t)std::sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return (uint32_t)r;
}

// fmd_narrow_level / fmd_bandplan_levels: the squelch state and the RMS of |u| of the last completed block of the rows
// row0 ... row0 + n - 1; all zero while no block has completed.
template <class Open>
inline int chan_levels(const FmdDdcBank& b, const ChanStage& c, size_t row0, size_t n, Open* open, uint32_t* rms)
{
    FMD_DDC_ON_DEVICE(b.core.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    for (size_t r = 0; r < n; ++r) { open[r] = 0; rms[r] = 0; }
    if ((chan_audio(b, c, b.core.pos) >> c.pshift) == 0) return FMD_OK;
    std::vector<unsigned long long> v(n * kCarry);
    FMD_DDC_TRY(hipMemcpy(v.data(), c.carry.in<unsigned long long>(b.core.cur) + row0 * kCarry, v.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < n; ++r) {
        open[r] = (c.squelch == 0u || v[r * kCarry + 5]) ? 1 : 0;
        rms[r] = isqrt_u64(v[r * kCarry + 2] >> c.pshift);
    }
    return FMD_OK;
}

}  // namespace fmd_chan
