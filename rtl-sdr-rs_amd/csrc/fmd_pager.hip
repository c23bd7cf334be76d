// fmd_pager.hip -- the page bank: the POCSAG batch decoder of every row on the device.  The soft decisions and the sync-word records
// the FSK front end (fmd_fsk.hip) leaves for every NFM row go through the search window, the batch's bit positions, the codeword
// correction and the message assembly in ONE gfx950 kernel, one lane per row, and only the messages come back.  No new arithmetic:
// row r behaves as an fmd_pocsag_decoder (fmd_pocsag_decode.cpp, tests/pocsag_ref.py) of its own would that is pushed exactly row
// r's samples and records of each call, with room for every message.
//
// The decoder acts only where something is due -- a record, a search window closing, a bit, slot 16 -- so a lane does not walk its
// row's samples: it steps from one due sample to the next (the smaller of the next record's k and k1 + r, p(nb) or p544 + r / 2),
// takes that sample's records, and then runs the definition's `advance` one step per turn of a loop that is uniform across the wave
// (`while (__any(busy))`); what differs between lanes is predicates and addresses.  A locked row takes about n / r turns per call.
//     p(n)   = k0 + Q(n), Q(n) = (2 n mod + step) / (2 step), formed without a division: with qd = mod / step and rd = 2 (mod % step),
//              Q(n + 1) = Q(n) + qd + c and R(n + 1) = R(n) + rd - 2 step c, where c = (R(n) + rd >= 2 step) and R is the division's
//              remainder; Q(1) = r, R(1) and Q(544) come from the host.  The lane keeps p(nb) and R(nb); k0 itself is not needed.
//     word   the remainder of bits 31 ... 1 by 0x769 (21 conditional XORs) and the parity of all 32 index a table of 2048 flip masks
//              in LDS, built on the host for the handle's max_errors from the definition: a word within max_errors bits of a
//              codeword has the syndrome of its error pattern, and two patterns of at most two bits with one syndrome would differ by
//              a codeword of weight <= 4 < 6.  0xFFFFFFFF: no codeword that near.
//     bits   the open message's bits live in device memory, 320 bytes per row, written in place: a message word starts on a byte or
//              on a nibble (20 bits each), so it is two whole bytes and a nibble, and the byte a nibble completes is read back from
//              the lane's own store.  With n_bits = 0 nothing of it is read before it is written.
// A message that closes is copied by the whole wave -- 88 dwords, zero behind its bytes -- from the header the lane snapshots and the
// row's open bits into the row's next record, before the next turn can write the bits of the message that follows.
//
// One workgroup = one wave = 64 consecutive rows for the whole call.  Every wave first carries its rows' last 64 soft decisions
// forward (eight lanes per row; 16-byte loads of the pieces that lie whole inside, element loads at the unaligned ends), since the
// caller's buffer may be gone by the next call and a bit may lie up to r / 2 samples behind the sample that makes it due.  Lanes
// whose row has no record and is neither locked nor searching are finished then; a wave without a busy lane loads no table.
// Carried per row: 32 dwords in a pair of the handle (all-zero is the reset state: nb - 1 is stored), the tail of 64 samples in the
// rows layer's history pair, and the open bits in place.  The counts and records go to a pair of their own, read behind the call.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_rows.h"

namespace fmd_pg {

constexpr int kThreads = 64;                              // one wave: a lane per row
constexpr uint32_t kRows = 64;
constexpr uint32_t kTail = 64;                            // soft decisions carried per row (the host decoder's ring)
constexpr uint32_t kState = 32;                           // dwords per row in the handle's pair
constexpr uint32_t kOpen = 320;                           // bytes per row of the open message's bits
constexpr uint32_t kMaxBits = 2560;
constexpr uint32_t kTable = 2048;                         // flip masks: index = remainder << 1 | parity
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kIdle = 0x7A89C197u, kPoly = 0x769u;
constexpr uint32_t kMsgDwords = 88;                       // sizeof(fmd_pocsag_msg) / 4

typedef int i4 __attribute__((ext_vector_type(4)));

// State words of a row: 0: bit 0 window, 1 locked, 2 inv, 3 the candidate's polarity, 4 best, 5 open, 6 the open message's
// polarity; bits 8-17 nb - 1.  1: word.  2-3: k1 while searching, p544 while locked.  4-5, 6, 7: k, thr, corr of the candidate
// (searching) or of the best record at slot 16 (locked).  8: thr.  9: R(nb).  10-11: p(nb).  12-15: the open message's address,
// function, n_bits, corrected.  16-17: its end_sample.  18-19: 0.  20-21 messages, 22-23 batches, 24-25 bad_codewords, 26-27
// orphans (low dword first).  28-31: 0.
enum : uint32_t { kWindow = 1u, kLocked = 2u, kInv = 4u, kXInv = 8u, kBest = 16u, kOpenMsg = 32u, kCurInv = 64u };

struct PagerLaunch {
    const int16_t* in;         // [n_rows][in_cap]
    uint64_t in_cap;
    uint32_t n_in;             // valid samples per row, >= 1
    uint32_t n_rows;
    const int16_t* tail_in;    // [n_rows][kTail]: the samples pos - 64 ... pos - 1
    int16_t* tail_out;
    const uint32_t* st_in;     // [n_rows][kState]
    uint32_t* st_out;
    uint8_t* open;             // [n_rows][kOpen], in place
    const uint32_t* table;     // [kTable]
    const uint32_t* hcnt;      // [n_rows]: the call's records per row, as the front end counted them
    const uint32_t* hrec;      // [n_rows][hit_cap] fmd_fsk_hit
    uint32_t* cnt_out;         // [n_rows]: the messages that closed in this call
    uint8_t* rec_out;          // [n_rows][msg_cap] fmd_pocsag_msg
    uint64_t pos;              // core.pos: samples per row before the call
    uint32_t hit_cap, msg_cap;
    uint32_t r, half;          // soft samples per bit, r / 2
    uint32_t q544;             // Q(544)
    uint32_t qd, rd, rem1;     // mod / step, 2 (mod % step), R(1)
    uint32_t two_step;         // 2 step <= mod < 2^32
};

__device__ __forceinline__ uint32_t mag(int c) { return c < 0 ? 0u - (uint32_t)c : (uint32_t)c; }

__global__ void __launch_bounds__(kThreads) fmd_pager_kernel(const PagerLaunch A)
{
    typedef const FMD_DDC_GLOBAL int16_t* gsrc;
    typedef FMD_DDC_GLOBAL int16_t* gdst;
    typedef const FMD_DDC_GLOBAL uint32_t* gw;
    __shared__ uint32_t tabL[kTable];

    const uint32_t l = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * kRows, row = row0 + l;
    const bool live = row < A.n_rows;
    const uint32_t n_in = A.n_in;
    const uint64_t n0 = A.pos;

    // ---- the last 64 soft decisions of every row of the wave, forward: eight lanes per row, eight rows per pass -----------------------
    {
        const uint32_t keep = n_in < kTail ? n_in : kTail;   // of them, the call's
        for (uint32_t pass = 0; pass < 8u; ++pass) {
            const uint32_t rr = pass * 8u + (l >> 3), p = l & 7u;
            const uint64_t grow = row0 + rr;
            if (grow >= A.n_rows) continue;
            const gsrc tin = (gsrc)(uintptr_t)(A.tail_in + grow * kTail);
            const gdst tout = (gdst)(uintptr_t)(A.tail_out + grow * kTail);
            for (uint32_t t = p; t + keep < kTail; t += 8u) tout[t] = tin[t + keep];
            const uintptr_t R = (uintptr_t)(A.in + grow * A.in_cap);
            const uintptr_t a1 = R + 2u * (uintptr_t)n_in, a0 = a1 - 2u * (uintptr_t)keep;
            for (uintptr_t ca = ((a0 >> 4) + p) << 4; ca < a1; ca += 8u * 16u) {
                if (ca >= a0 && ca + 16u <= a1) {            // a piece whole inside
                    const i4 v = *(const FMD_DDC_GLOBAL i4*)ca;
                    const uint32_t t0 = kTail - (uint32_t)((a1 - ca) >> 1);
                    if ((a1 & 15u) == 0u) {
                        *(FMD_DDC_GLOBAL i4*)(tout + t0) = v;
                    } else {
                        const uint32_t d[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
#pragma unroll
                        for (uint32_t e = 0; e < 8u; ++e) tout[t0 + e] = (int16_t)(d[e >> 1] >> (16u * (e & 1u)));
                    }
                } else {                                     // the unaligned head or tail: exactly the samples kept
                    for (uint32_t e = 0; e < 8u; ++e) {
                        const uintptr_t a = ca + 2u * e;
                        if (a < a0 || a >= a1) continue;
                        tout[kTail - (uint32_t)((a1 - a) >> 1)] = *(gsrc)a;
                    }
                }
            }
        }
    }

    // ---- the row's state ------------------------------------------------------------------------------------------------------------
    const uint64_t lrow = live ? row : 0;
    uint32_t cnt = 0;
    i4 s0 = i4{0, 0, 0, 0}, s1 = s0, s2 = s0, s3 = s0, s4 = s0, s5 = s0, s6 = s0;
    if (live) {
        const FMD_DDC_GLOBAL i4* const s = (const FMD_DDC_GLOBAL i4*)(uintptr_t)(A.st_in + row * kState);
        s0 = s[0]; s1 = s[1]; s2 = s[2]; s3 = s[3]; s4 = s[4]; s5 = s[5]; s6 = s[6];
        cnt = ((gw)(uintptr_t)A.hcnt)[row];
        cnt = cnt < A.hit_cap ? cnt : A.hit_cap;
    }
    uint32_t fl = (uint32_t)s0.x & 0x7Fu, nbm1 = ((uint32_t)s0.x >> 8) & 0x3FFu, word = (uint32_t)s0.y;
    uint64_t kp = (uint32_t)s0.z | (uint64_t)(uint32_t)s0.w << 32;
    uint64_t xk = (uint32_t)s1.x | (uint64_t)(uint32_t)s1.y << 32;
    int xthr = s1.z, xcorr = s1.w, thr = s2.x;
    uint32_t rem = (uint32_t)s2.y;
    uint64_t pnext = (uint32_t)s2.z | (uint64_t)(uint32_t)s2.w << 32;
    uint32_t c_addr = (uint32_t)s3.x, c_func = (uint32_t)s3.y, c_nbits = (uint32_t)s3.z, c_corr = (uint32_t)s3.w;
    uint64_t c_end = (uint32_t)s4.x | (uint64_t)(uint32_t)s4.y << 32;
    uint32_t d_msgs = 0, d_batches = 0, d_bad = 0, d_orph = 0, count = 0;

    bool busy = live && (cnt != 0u || (fl & (kWindow | kLocked)) != 0u);
    if (__any(busy)) {                                       // wave-uniform
        for (uint32_t e = l; e < kTable; e += kThreads) tabL[e] = ((gw)(uintptr_t)A.table)[e];
        __syncthreads();

        const gsrc in = (gsrc)(uintptr_t)(A.in + lrow * A.in_cap);
        const gsrc tail = (gsrc)(uintptr_t)(A.tail_in + lrow * kTail);
        const FMD_DDC_GLOBAL i4* const recs = (const FMD_DDC_GLOBAL i4*)(uintptr_t)(A.hrec + lrow * A.hit_cap * 4u);
        FMD_DDC_GLOBAL uint8_t* const open = (FMD_DDC_GLOBAL uint8_t*)(uintptr_t)(A.open + lrow * kOpen);
        const uint32_t r = A.r, half = A.half;

        uint32_t i = 0, hi = 0, hk = kNone;                  // the sample the lane is at or will look from; the next record and its k
        i4 hrec = i4{0, 0, 0, 0};
        bool at = false;                                     // sample i has been entered: its records are taken
        if (cnt) { hrec = recs[0]; hk = (uint32_t)hrec.x; }

        while (__any(busy)) {
            bool closed = false;
            uint32_t m_addr = 0, m_func = 0, m_nbits = 0, m_corr = 0, m_inv = 0, m_elo = 0, m_ehi = 0;
            // the open message closes: counted, and its header kept for the wave's copy
#define FMD_PG_CLOSE()                                                                                                             \
    do {                                                                                                                           \
        if (fl & kOpenMsg) {                                                                                                       \
            fl &= ~kOpenMsg; ++d_msgs; closed = true;                                                                              \
            m_addr = c_addr; m_func = c_func; m_nbits = c_nbits; m_corr = c_corr; m_inv = (fl & kCurInv) ? 1u : 0u;                \
            m_elo = (uint32_t)c_end; m_ehi = (uint32_t)(c_end >> 32);                                                              \
        }                                                                                                                          \
    } while (0)
            // a new batch behind the sync word whose last bit is sample k_
#define FMD_PG_ANCHOR(k_, t_)                                                                                                      \
    do {                                                                                                                           \
        thr = (t_); nbm1 = 0u; word = 0u; fl &= ~kBest;                                                                            \
        kp = (k_) + A.q544; pnext = (k_) + r; rem = A.rem1;                                                                        \
        ++d_batches;                                                                                                               \
    } while (0)
            if (busy && !at) {
                while (hk < i) {                             // records out of order: passed over
                    ++hi;
                    if (hi < cnt) { hrec = recs[hi]; hk = (uint32_t)hrec.x; } else hk = kNone;
                }
                uint32_t dr = kNone;                         // the pending event, as an index into this call
                if (fl & (kWindow | kLocked)) {
                    const uint64_t due = (fl & kLocked) ? (nbm1 < 512u ? pnext : kp + half) : kp + r;
                    if (due <= n0 + i) dr = i;
                    else if (due - n0 < (uint64_t)n_in) dr = (uint32_t)(due - n0);
                }
                const uint32_t nx = dr < hk ? dr : hk;
                if (nx >= n_in) busy = false;                // nothing more is due in this call
                else {
                    i = nx; at = true;
                    const uint64_t n = n0 + i;
                    while (hk <= i) {                        // the sample's records
                        if (hk == i) {
                            const uint32_t hinv = (uint32_t)hrec.y >> 31;
                            const int hcorr = hrec.z, hthr = hrec.w;
                            if (!(fl & kLocked)) {
                                if (!(fl & kWindow)) {
                                    fl = (fl & ~kXInv) | kWindow | (hinv ? kXInv : 0u);
                                    kp = n; xk = n; xthr = hthr; xcorr = hcorr;
                                } else if (n <= kp + r && mag(hcorr) > mag(xcorr)) {
                                    fl = (fl & ~kXInv) | (hinv ? kXInv : 0u);
                                    xk = n; xthr = hthr; xcorr = hcorr;
                                }
                            } else {
                                const uint64_t dist = n > kp ? n - kp : kp - n;
                                if (dist <= half && hinv == ((fl & kInv) ? 1u : 0u) && (!(fl & kBest) || mag(hcorr) > mag(xcorr))) {
                                    fl |= kBest; xk = n; xthr = hthr; xcorr = hcorr;
                                }
                            }
                        }
                        ++hi;
                        if (hi < cnt) { hrec = recs[hi]; hk = (uint32_t)hrec.x; } else hk = kNone;
                    }
                    if ((fl & (kLocked | kWindow)) == kWindow && n >= kp + r) {      // the search window closes: lock on the candidate
                        fl = (fl & ~(kWindow | kInv)) | kLocked | ((fl & kXInv) ? kInv : 0u);
                        FMD_PG_ANCHOR(xk, xthr);
                    }
                }
            }
            if (busy && at) {                                // one step of `advance` at sample n
                const uint64_t n = n0 + i;
                bool leave = false;
                if (!(fl & kLocked)) leave = true;
                else if (nbm1 < 512u) {
                    if (pnext > n) leave = true;
                    else {
                        // the bit at p(nb) <= n: of this call, or of the tail in front of it
                        const int v = pnext >= n0 ? (int)in[pnext - n0] : (int)tail[(kTail - (uint32_t)(n0 - pnext)) & (kTail - 1u)];
                        const uint32_t bit = ((32 * v > thr) ? 1u : 0u) ^ ((fl & kInv) ? 1u : 0u);
                        word = word << 1 | bit;
                        const uint32_t nb = nbm1 + 1u;
                        if ((nb & 31u) == 0u) {              // a codeword
                            uint32_t c = word >> 1;
#pragma unroll
                            for (int b = 30; b >= 10; --b) c ^= ((c >> b) & 1u) ? kPoly << (b - 10) : 0u;
                            const uint32_t m = tabL[(c & 0x3FFu) << 1 | ((uint32_t)__builtin_popcount(word) & 1u)];
                            const uint32_t cw = word ^ m, nfix = (uint32_t)__builtin_popcount(m);
                            if (m == kNone) { ++d_bad; FMD_PG_CLOSE(); }
                            else if (cw == kIdle) FMD_PG_CLOSE();
                            else if (!(cw >> 31)) {          // an address word: closes, and opens
                                FMD_PG_CLOSE();
                                c_addr = ((cw >> 13) & 0x3FFFFu) << 3 | ((nb / 32u - 1u) >> 1);
                                c_func = (cw >> 11) & 3u;
                                c_nbits = 0u; c_corr = nfix; c_end = pnext;
                                fl = (fl & ~kCurInv) | kOpenMsg | ((fl & kInv) ? kCurInv : 0u);
                            } else if (!(fl & kOpenMsg)) ++d_orph;
                            else {                           // a message word: 20 bits behind the c_nbits there are
                                const uint32_t data = (cw >> 11) & 0xFFFFFu;
                                if (c_nbits < kMaxBits) {    // (a multiple of 20: all 20 fit, the last byte is 319)
                                    const uint32_t b = c_nbits >> 3;
                                    if ((c_nbits & 7u) == 0u) {
                                        open[b] = (uint8_t)(data >> 12); open[b + 1u] = (uint8_t)(data >> 4); open[b + 2u] = (uint8_t)(data << 4);
                                    } else {
                                        open[b] = (uint8_t)(open[b] | (data >> 16)); open[b + 1u] = (uint8_t)(data >> 8); open[b + 2u] = (uint8_t)data;
                                    }
                                }
                                c_nbits += 20u; c_corr += nfix; c_end = pnext;
                            }
                            word = 0u;
                        }
                        nbm1 = nb;
                        const uint64_t t = (uint64_t)rem + A.rd;
                        const bool carry = t >= (uint64_t)A.two_step;
                        rem = (uint32_t)(carry ? t - A.two_step : t);
                        pnext += A.qd + (carry ? 1u : 0u);
                        if (nbm1 < 512u && pnext > n) leave = true;
                    }
                } else if (n < kp + half) leave = true;      // slot 16 is not due yet
                else if (fl & kBest) FMD_PG_ANCHOR(xk, xthr);
                else {                                       // no sync word where one was due
                    fl &= ~kLocked;
                    FMD_PG_CLOSE();
                    leave = true;
                }
                if (leave) {
                    at = false; ++i;
                    if (i >= n_in) busy = false;
                }
            }
#undef FMD_PG_CLOSE
#undef FMD_PG_ANCHOR
            // ---- the messages that closed in this turn: the whole wave copies them, lane after lane -------------------------------------
            unsigned long long mask = __ballot(closed);      // nearly always zero: one scalar branch
            if (mask) {
                __threadfence();                             // the lanes' byte stores, before other lanes read them
                while (mask) {
                    const int j = __builtin_ctzll(mask);
                    mask &= mask - 1ull;
                    const uint32_t slot = (uint32_t)__shfl((int)count, j);
                    const uint32_t ja = (uint32_t)__shfl((int)m_addr, j), jf = (uint32_t)__shfl((int)m_func, j);
                    const uint32_t jn = (uint32_t)__shfl((int)m_nbits, j), jc = (uint32_t)__shfl((int)m_corr, j);
                    const uint32_t jv = (uint32_t)__shfl((int)m_inv, j);
                    const uint32_t jl = (uint32_t)__shfl((int)m_elo, j), jh = (uint32_t)__shfl((int)m_ehi, j);
                    if (slot >= A.msg_cap) continue;         // counted, not delivered
                    const uint64_t jrow = row0 + (uint32_t)j;
                    const uint32_t len = ((jn < kMaxBits ? jn : kMaxBits) + 7u) >> 3;
                    const gw ow = (gw)(uintptr_t)(A.open + jrow * kOpen);
                    FMD_DDC_GLOBAL uint32_t* const rec =
                        (FMD_DDC_GLOBAL uint32_t*)(uintptr_t)(A.rec_out + (jrow * A.msg_cap + slot) * sizeof(fmd_pocsag_msg));
                    for (uint32_t d = l; d < kMsgDwords; d += kThreads) {
                        uint32_t v = 0u;
                        if (d >= 3u && d < 83u) {
                            const uint32_t b0 = 4u * (d - 3u);
                            if (b0 < len) {
                                v = ow[d - 3u];
                                if (len - b0 < 4u) v &= (1u << (8u * (len - b0))) - 1u;
                            }
                        }
                        else if (d == 0u) v = ja;
                        else if (d == 1u) v = jf;
                        else if (d == 2u) v = jn;
                        else if (d == 83u) v = jc;
                        else if (d == 84u) v = jv;
                        else if (d == 86u) v = jl;
                        else if (d == 87u) v = jh;
                        rec[d] = v;
                    }
                }
                __threadfence();                             // the copies' loads, before the rows' next byte stores
            }
            count += closed ? 1u : 0u;
        }
    }

    if (!live) return;
    uint64_t msgs = (uint32_t)s5.x | (uint64_t)(uint32_t)s5.y << 32, batches = (uint32_t)s5.z | (uint64_t)(uint32_t)s5.w << 32;
    uint64_t bad = (uint32_t)s6.x | (uint64_t)(uint32_t)s6.y << 32, orph = (uint32_t)s6.z | (uint64_t)(uint32_t)s6.w << 32;
    msgs += d_msgs; batches += d_batches; bad += d_bad; orph += d_orph;
    FMD_DDC_GLOBAL i4* const s = (FMD_DDC_GLOBAL i4*)(uintptr_t)(A.st_out + row * kState);
    s[0] = i4{(int)(fl | nbm1 << 8), (int)word, (int)(uint32_t)kp, (int)(uint32_t)(kp >> 32)};
    s[1] = i4{(int)(uint32_t)xk, (int)(uint32_t)(xk >> 32), xthr, xcorr};
    s[2] = i4{thr, (int)rem, (int)(uint32_t)pnext, (int)(uint32_t)(pnext >> 32)};
    s[3] = i4{(int)c_addr, (int)c_func, (int)c_nbits, (int)c_corr};
    s[4] = i4{(int)(uint32_t)c_end, (int)(uint32_t)(c_end >> 32), 0, 0};
    s[5] = i4{(int)(uint32_t)msgs, (int)(uint32_t)(msgs >> 32), (int)(uint32_t)batches, (int)(uint32_t)(batches >> 32)};
    s[6] = i4{(int)(uint32_t)bad, (int)(uint32_t)(bad >> 32), (int)(uint32_t)orph, (int)(uint32_t)(orph >> 32)};
    s[7] = i4{0, 0, 0, 0};
    ((FMD_DDC_GLOBAL uint32_t*)(uintptr_t)A.cnt_out)[row] = count;
}

}  // namespace fmd_pg

static_assert(sizeof(fmd_pocsag_msg) == 352 && offsetof(fmd_pocsag_msg, bits) == 12 && offsetof(fmd_pocsag_msg, corrected) == 332 &&
                  offsetof(fmd_pocsag_msg, inverted) == 336 && offsetof(fmd_pocsag_msg, end_sample) == 344,
              "the kernel writes fmd_pocsag_msg as 88 dwords");
static_assert(sizeof(fmd_fsk_hit) == 16, "the kernel reads fmd_fsk_hit as four dwords");

struct fmd_pager {
    FmdRows rows;                                         // width 1; its history pair is the tail: hcap = 64
    FmdDdcPair state;                                     // [n_rows][kState] uint32
    FmdRowRecords recs;                                   // fmd_pocsag_msg, msg_cap per row
    void* d_open = nullptr;                               // [n_rows][kOpen] bytes, in place (reset need not clear it: with n_bits = 0
                                                          // nothing of it is read before it is written)
    void* d_table = nullptr;                              // [kTable] uint32
    uint64_t mod = 0, step = 0;
    uint32_t max_errors = 0;
};

namespace {

// the remainder and the parity an error pattern leaves on any codeword: the table's index
uint32_t pg_key(uint32_t e)
{
    uint32_t c = e >> 1;
    for (int i = 30; i >= 10; --i)
        if ((c >> i) & 1u) c ^= fmd_pg::kPoly << (i - 10);
    return (c & 0x3FFu) << 1 | ((uint32_t)__builtin_popcount(e) & 1u);
}

int pg_domain(uint32_t rate_num, uint32_t rate_den, uint32_t baud, uint32_t max_errors)
{
    const uint64_t mod = rate_num, step = (uint64_t)baud * rate_den;
    // the host decoder's tests, in its order: `step > mod / 2` comes first and bounds step by 2^31, so that 32 * step cannot wrap
    if (step < 1 || step > mod / 2 || mod > 32 * step) { fmd_internal_set_err("need 2 <= rate / baud <= 32"); return FMD_ERR_UNSUPPORTED; }
    if (max_errors > 2) { fmd_internal_set_err("need max_errors <= 2"); return FMD_ERR_UNSUPPORTED; }
    return FMD_OK;
}

int pg_enqueue(fmd_pager* h, const void* d_in, size_t n_in, size_t in_cap, const void* d_counts, const void* d_hits, uint32_t hit_cap,
               hipStream_t stream)
{
    FmdRows& r = h->rows;
    if (hit_cap < 1 || hit_cap > 64) { fmd_internal_set_err("need 1 <= hit_cap <= 64"); return FMD_ERR_UNSUPPORTED; }
    if (((uintptr_t)d_counts & 3u) != 0 || ((uintptr_t)d_hits & 15u) != 0) { fmd_internal_set_err("misaligned device buffer"); return FMD_ERR_INVALID_ARG; }
    if (const int rc = fmd_rows_check_call(r, d_in, n_in, in_cap, nullptr)) return rc;
    if (n_in == 0) return FMD_OK;                            // nothing to take: no launch, the last call's results stay
    const uint64_t mod = h->mod, step = h->step;
    fmd_pg::PagerLaunch A{};
    A.in = static_cast<const int16_t*>(d_in); A.in_cap = in_cap; A.n_in = (uint32_t)n_in; A.n_rows = r.n_rows;
    A.tail_in = r.hist.in<int16_t>(r.core.cur); A.tail_out = r.hist.out<int16_t>(r.core.cur);
    A.st_in = h->state.in<uint32_t>(r.core.cur); A.st_out = h->state.out<uint32_t>(r.core.cur);
    A.open = static_cast<uint8_t*>(h->d_open);
    A.table = static_cast<const uint32_t*>(h->d_table);
    A.hcnt = static_cast<const uint32_t*>(d_counts); A.hrec = static_cast<const uint32_t*>(d_hits);
    A.cnt_out = h->recs.cnt_out(r.core.cur);
    A.rec_out = h->recs.rec_out(r.core.cur);
    A.pos = r.core.pos;
    A.hit_cap = hit_cap; A.msg_cap = h->recs.cap;
    A.r = (uint32_t)((2 * mod + step) / (2 * step)); A.half = A.r / 2;
    A.q544 = (uint32_t)((2 * 544 * mod + step) / (2 * step));
    A.qd = (uint32_t)(mod / step); A.rd = (uint32_t)(2 * (mod % step)); A.rem1 = (uint32_t)((2 * mod + step) % (2 * step));
    A.two_step = (uint32_t)(2 * step);
    const uint32_t grid = (r.n_rows + fmd_pg::kRows - 1u) / fmd_pg::kRows;
    return fmd_rows_launch(r, fmd_pg::fmd_pager_kernel, fmd_pg::fmd_pager_kernel, grid, fmd_pg::kThreads, A, stream, n_in, 0, nullptr);
}

}  // namespace

extern "C" {

size_t fmd_pager_max_messages(uint32_t rate_num, uint32_t rate_den, uint32_t baud, size_t n)
{
    const uint64_t mod = rate_num, step = (uint64_t)baud * rate_den;
    if (step < 1 || step > mod / 2) return 0;
    const uint64_t q = mod / step, B = ((uint64_t)n + q - 1) / q;
    return (size_t)((B + 31) / 32 + 1 + B / 512);
}

int fmd_pager_table(uint32_t max_errors, uint32_t* table)
{
    if (!table) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (max_errors > 2) { fmd_internal_set_err("need max_errors <= 2"); return FMD_ERR_UNSUPPORTED; }
    // the error patterns in the definition's order -- none, one bit, two bits -- each at the syndrome it leaves on any codeword
    for (uint32_t k = 0; k < fmd_pg::kTable; ++k) table[k] = fmd_pg::kNone;
    table[pg_key(0u)] = 0u;
    if (max_errors >= 1)
        for (uint32_t a = 0; a < 32; ++a)
            if (table[pg_key(1u << a)] == fmd_pg::kNone) table[pg_key(1u << a)] = 1u << a;
    if (max_errors >= 2)
        for (uint32_t a = 0; a < 32; ++a)
            for (uint32_t b = a + 1; b < 32; ++b) {
                const uint32_t e = 1u << a | 1u << b;
                if (table[pg_key(e)] == fmd_pg::kNone) table[pg_key(e)] = e;
            }
    return FMD_OK;
}

int fmd_pager_new(uint32_t rate_num, uint32_t rate_den, uint32_t baud, uint32_t max_errors, uint32_t msg_cap, const fmd_device_config* dev,
                  fmd_pager** out)
{
    if (const int rc = fmd_rows_new_args(dev, dev, out, 1)) return rc;       // (the pointers)
    if (const int rc = pg_domain(rate_num, rate_den, baud, max_errors)) return rc;
    if (msg_cap < 1 || msg_cap > 16) { fmd_internal_set_err("need 1 <= msg_cap <= 16"); return FMD_ERR_UNSUPPORTED; }
    if (const int rc = fmd_rows_count_arg(dev)) return rc;
    fmd_pager* h = new (std::nothrow) fmd_pager();
    if (!h) return FMD_ERR_NOMEM;
    h->mod = rate_num; h->step = (uint64_t)baud * rate_den; h->max_errors = max_errors;
    h->rows.width = 1; h->rows.n_rows = dev->n_channels; h->rows.hcap = fmd_pg::kTail;
    h->rows.lds = 0;                                         // the table is static
    const size_t n = dev->n_channels;
    std::vector<uint32_t> table(fmd_pg::kTable);
    (void)fmd_pager_table(max_errors, table.data());
    fmd_ddc_add_pair(h->rows.core, h->state, n * fmd_pg::kState * sizeof(uint32_t));
    fmd_rows_add_records(h->rows, h->recs, msg_cap, sizeof(fmd_pocsag_msg));
    fmd_ddc_add_owned(h->rows.core, h->d_table, table.data(), table.size() * sizeof(uint32_t));
    fmd_ddc_add_owned(h->rows.core, h->d_open, nullptr, n * fmd_pg::kOpen);
    return fmd_rows_device(h, dev, fmd_pager_free, out);
}

void fmd_pager_free(fmd_pager* h) { fmd_rows_free(h); }
int fmd_pager_reset(fmd_pager* h) { return fmd_rows_reset(h); }
int fmd_pager_check(fmd_pager* h) { return fmd_rows_check(h); }
int fmd_pager_inputs(const fmd_pager* h, uint64_t* inputs) { return fmd_rows_inputs(h, inputs); }
int fmd_pager_counts(fmd_pager* h, uint32_t* counts) { return fmd_rows_counts(h, counts); }
int fmd_pager_msgs(fmd_pager* h, const uint32_t* rows, size_t n_sel, fmd_pocsag_msg* msgs) { return fmd_rows_records(h, rows, n_sel, msgs); }

int fmd_pager_info(fmd_pager* h, fmd_pocsag_info* info)
{
    if (!h || !info) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    std::vector<uint32_t> st;
    if (const int rc = fmd_rows_read_state(h->rows, h->state, fmd_pg::kState, st)) return rc;
    for (size_t r = 0; r < h->rows.n_rows; ++r) {
        const uint32_t* const s = &st[r * fmd_pg::kState];
        memset(&info[r], 0, sizeof info[r]);
        info[r].messages = s[20] | (uint64_t)s[21] << 32;
        info[r].batches = s[22] | (uint64_t)s[23] << 32;
        info[r].bad_codewords = s[24] | (uint64_t)s[25] << 32;
        info[r].orphans = s[26] | (uint64_t)s[27] << 32;
        info[r].locked = (s[0] & fmd_pg::kLocked) ? 1 : 0;
        info[r].searching = !(s[0] & fmd_pg::kLocked) && (s[0] & fmd_pg::kWindow) ? 1 : 0;
    }
    return FMD_OK;
}

int fmd_pager_run_device(fmd_pager* h, const void* d_soft, size_t n_in, size_t in_cap, const void* d_counts, const void* d_hits,
                         uint32_t hit_cap, void* stream)
{
    if (!d_counts) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_run_device(h ? &h->rows.core : nullptr, d_soft, d_hits,
                              [&] { return pg_enqueue(h, d_soft, n_in, in_cap, d_counts, d_hits, hit_cap, static_cast<hipStream_t>(stream)); });
}

// Host rows, counts and records in, nothing out: the front end's counts and records are staged into core.d_out, laid out as an
// FmdRowRecords is.
int fmd_pager_run_batch(fmd_pager* h, const int16_t* soft, size_t n_in, size_t in_cap, const uint32_t* counts, const fmd_fsk_hit* hits,
                        uint32_t hit_cap)
{
    if (!h || !soft || !counts || !hits) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (hit_cap < 1 || hit_cap > 64) { fmd_internal_set_err("need 1 <= hit_cap <= 64"); return FMD_ERR_UNSUPPORTED; }
    const size_t n = h->rows.n_rows, cnt_bytes = fmd_rows_counts_bytes(n), hit_bytes = n * hit_cap * sizeof(fmd_fsk_hit);
    const auto stage = [&](FmdDdcCore& c) -> int {
        FMD_DDC_TRY(fmd_ddc_grow(c.d_out, c.d_out_cap, cnt_bytes + hit_bytes));
        uint8_t* const d_rec = static_cast<uint8_t*>(c.d_out);
        FMD_DDC_TRY(hipMemcpyAsync(d_rec, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
        FMD_DDC_TRY(hipMemcpyAsync(d_rec + cnt_bytes, hits, hit_bytes, hipMemcpyHostToDevice, c.stream));
        return FMD_OK;
    };
    return fmd_rows_feed_batch(h, soft, n_in, in_cap, stage, [&](const void* d_in, hipStream_t s) {
        const uint8_t* const d_rec = static_cast<const uint8_t*>(h->rows.core.d_out);
        return pg_enqueue(h, d_in, n_in, in_cap, d_rec, d_rec + cnt_bytes, hit_cap, s);
    });
}

int fmd_pager_kernel_name(const fmd_pager* h, char* name, size_t cap) { return fmd_rows_kernel_name(h, name, cap, "fmd_pg::fmd_pager_kernel"); }

}  // extern "C"
