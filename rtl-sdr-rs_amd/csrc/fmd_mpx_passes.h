// fmd_mpx_passes.h -- the two sides of a second pass over the multiplex (fmd_stereo_mpx.h, stage_tile), with their launch structs,
// LDS capacities and limits: the stereo bank's audio side (fmd_sto::AudioPass) and the RDS bank's baseband side
// (fmd_rdsk::BasebandPass).  fmd_stereo.hip and fmd_rds.hip instantiate one each, fmd_receiver.hip both in one kernel.
#pragma once

#include "fmd_stereo_mpx.h"

namespace fmd_sto {

constexpr uint32_t kXCap = 2048;                          // (x, s) pairs a tile has room for: R tile + 2 Ta <= kXCap
constexpr uint32_t kMaxBlocks = 4;                        // blocks one tile touches (<= 3: kXCap / 1024 + 1)

// the audio stage's names and limits in the refusal texts, and the stereo bank's rate floor
constexpr StageLimits kAudioLimits{106000u, "audio_decim", "audio_taps", "audio_shift", 16u};
// pairs a tile may stage beyond the 2 Ta set aside: na >= 48, R na + 2 Ta <= kXCap
constexpr uint32_t audio_room(uint32_t Ta) { return kXCap - 2u * Ta; }

struct AudioLaunch : StageLaunch {                          // x: the multiplex, pairs (x, s), shift: audio_shift, out: (L, R)
    uint32_t inc_p;
    uint64_t thr;              // pilot_min P 8192 (0: every block absent)
};

// a^2 + b^2 >= thr^2 in 128 bits (|a|, |b| <= 2^43, thr <= 2^41)
__device__ __forceinline__ bool pilot_present(long long I, long long Q, uint64_t thr)
{
    if (thr == 0u) return false;
    const uint64_t ua = (uint64_t)(I < 0 ? -I : I), ub = (uint64_t)(Q < 0 ? -Q : Q);
    const uint64_t alo = ua * ua, ahi = __umul64hi(ua, ua), blo = ub * ub, bhi = __umul64hi(ub, ub);
    const uint64_t lo = alo + blo, hi = ahi + bhi + (lo < alo ? 1u : 0u);
    const uint64_t tlo = thr * thr, thi = __umul64hi(thr, thr);
    return hi > thi || (hi == thi && lo >= tlo);
}

// The audio pass's side of a second-pass tile (fmd_stereo_mpx.h, stage_tile).
struct AudioPass {
    static constexpr uint32_t kSlots = kXCap;
    static constexpr bool kCarry = true;
    int32_t (*est)[3];                                       // LDS: present, c2, s2 of block jA - 1 + i
    uint64_t jA;                                             // block of the first of the call's own samples the tile stages

    static __device__ __forceinline__ uint32_t slot(uint32_t i) { return i; }

    // the estimate of each block the tile's own samples need, one lane per block (i64 / 128-bit arithmetic)
    __device__ __forceinline__ void before(const AudioLaunch& L, uint32_t row, uint32_t tid, uint32_t vlo, uint32_t vhi)
    {
        const uint32_t va = vlo > L.HX ? vlo : L.HX;         // first virtual index of the call's own samples
        jA = (L.mS + (va - L.HX)) >> L.pshift;
        if (va >= vhi || tid >= kMaxBlocks) return;
        const uint64_t jB = (L.mS + (vhi - 1u - L.HX)) >> L.pshift;
        if (jA + tid > jB) return;
        long long I, Q;
        block_iq(L, row, (int64_t)(jA + tid) - 1, I, Q);
        int present = pilot_present(I, Q, L.thr) ? 1 : 0, c2 = 0, s2 = 0;
        if (present) {
            const uint64_t mx = (uint64_t)(I < 0 ? -I : I) | (uint64_t)(Q < 0 ? -Q : Q);   // same bit length as the max
            const int bl = 64 - __builtin_clzll(mx);
            const int e = bl > 23 ? bl - 23 : 0;
            const long long a = I >> e, b = Q >> e;
            const long long E = a * a + b * b;
            c2 = (int)((b * b - a * a) * 16384 / E);
            s2 = (int)((2 * a * b) * 16384 / E);
        }
        est[tid][0] = present; est[tid][1] = c2; est[tid][2] = s2;
    }

    // (x, s): s = (x kc) >> 14 with kc from 2 theta and the block's estimate, 0 while the pilot is absent
    __device__ __forceinline__ int2 pair(const AudioLaunch& L, const int16_t* tab, uint64_t m, int xv) const
    {
        const uint32_t jj = (uint32_t)((m >> L.pshift) - jA);
        int sv = 0;
        if (est[jj][0]) {
            const uint32_t ix = (((uint32_t)m * L.inc_p) << 1) >> 22;                      // 2 theta
            const int kc = (tab[(ix - 256u) & 1023u] * est[jj][1] + tab[ix] * est[jj][2]) >> 13;
            sv = (xv * kc) >> 14;
        }
        return int2{xv, sv};
    }

    // the matrix step and the saturation: a = sum g x, b = sum g s
    static __device__ __forceinline__ uint32_t output(int a, int b, uint32_t shift)
    {
        int l = (a + b) >> (shift + 1u), r = (a - b) >> (shift + 1u);
        l = l > 32767 ? 32767 : (l < -32768 ? -32768 : l);
        r = r > 32767 ? 32767 : (r < -32768 ? -32768 : r);
        return ((uint32_t)l & 0xFFFFu) | ((uint32_t)r << 16);
    }
};

}  // namespace fmd_sto

namespace fmd_rdsk {

constexpr uint32_t kQCap = 1984;                          // pairs a tile stages: R tile + Ta <= kQCap
constexpr uint32_t kQSlots = 2048;                        // LDS slots: kQCap + kQCap / 32 = 2046 padded positions (16 KiB, the stereo pass's xs)

struct BasebandLaunch : fmd_sto::StageLaunch {            // pairs (qr, qi), shift: rds_shift, out: (ur, ui)
    uint32_t inc3;             // carrier step 3 inc_p mod 2^32
};

// The baseband pass's side of a second-pass tile (fmd_stereo_mpx.h, stage_tile).
struct BasebandPass {
    static constexpr uint32_t kSlots = kQSlots;
    static constexpr bool kCarry = true;

    // lanes read at stride R, and without the padding an even R puts them on few banks (R = 32: all 64 lanes on one pair of banks)
    static __device__ __forceinline__ uint32_t slot(uint32_t i) { return i + (i >> 5); }

    __device__ __forceinline__ void before(const BasebandLaunch&, uint32_t, uint32_t, uint32_t, uint32_t) {}

    // q[m] = (x cosq(phi), -x sinq(phi)) >> 14, phi = 3 m inc_p mod 2^32 (|x tab| <= 2^29)
    __device__ __forceinline__ int2 pair(const BasebandLaunch& L, const int16_t* tab, uint64_t m, int xv) const
    {
        const uint32_t ix = ((uint32_t)m * L.inc3) >> 22;
        return int2{(xv * (int)tab[ix]) >> 14, (-xv * (int)tab[(ix - 256u) & 1023u]) >> 14};
    }

    // the normalising shift; the host's store check makes the wrap to 16 bits exact (|v| < 2^29)
    static __device__ __forceinline__ uint32_t output(int a, int b, uint32_t shift)
    {
        return ((uint32_t)(a >> shift) & 0xFFFFu) | ((uint32_t)(b >> shift) << 16);
    }
};

// the baseband stage's names and limits in the refusal texts, and the RDS bank's rate floor
constexpr fmd_sto::StageLimits kBasebandLimits{120000u, "out_decim", "rds_taps", "rds_shift", 24u};
// pairs a tile may stage beyond the Ta set aside: na >= 54, R na + Ta <= kQCap
constexpr uint32_t baseband_room(uint32_t Ta) { return kQCap - Ta; }

// the exact-store check on rds_shift: with |q| <= 32768 every |v| <= 32768 sum |g|, and the shifted value must fit int16
inline int store_check(uint64_t gsum, uint32_t shift)
{
    if (((32768ull * gsum + ((1ull << shift) - 1ull)) >> shift) > 32767ull)
        return fmd_sto::stage_refuse("rds_shift too small: need ceil(32768 * sum |rds_taps| / 2^rds_shift) <= 32767");
    return FMD_OK;
}

}  // namespace fmd_rdsk
