// fmd_dcs.hip -- code squelch: every int16 row a bank leaves on the device is searched, decimated sample by decimated sample, for
// one of up to 128 23-bit words (DCS, the digital-coded squelch: a Golay word at 134.4 bit/s under the voice band), and gated by
// the code the blocks before decided on, in ONE gfx950 kernel.  Width 1 is mono audio, width 2 interleaved (L, R) whose mean is
// searched and whose two components share the gate.  No clock recovery: every k forms its own word from samples one bit apart.
//
// Definition (include/fmd.h, "code squelch"; tests/dcs_ref.py), per row, with P = block, r = i mod P:
//     m[i] = x[i][0] or (x[i][0] + x[i][1]) >> 1;   b[k] = (sum_{r<B} m[k B + r]) >> log2 B
//     soft[k] = sat16((sum_{t<T} lp[t] b[k - (T-1) + t]) >> lshift)
//     bit j of w[k] = 23 soft[k - tap[j]] > sum_j' soft[k - tap[j']];   d_f = popcount(w[k] ^ u_f);  f(k) = the first smallest
//     k is a hit on f(k) if d <= tol;  per block: hits_f, f* = the first largest, a hit on f* if hits_f* >= min_hits
//     (t, cand, cnt, h) step once per block;  s_j = 256 or 0
//     g[i] = s_{j-2} + (((s_{j-1} - s_{j-2}) (min(r, Q - 1) + 1)) >> log2 Q),  out[i][c] = (x[i][c] g[i]) >> 8
// n_out = n_in.  Per row the handle carries the open box's partial sum, the last T - 1 b, the last tap[22] soft, the F hit counters
// of the open block and the small state.
//
// One workgroup = one tile of kRows = 16 rows for the whole call.  All rows of a call share core.pos, hence every box end and every
// block end inside the call.  The call's samples are walked in chunks of kChunk = 64 stream samples, aligned to the stream (P is a
// multiple of 64 and B divides 64, so a chunk crosses neither a block end nor a box; the first and the last chunk of a call may be
// partial, and only they can leave a box open).  Per chunk, with one barrier (the staging buffers are doubled):
//   1. the samples: 16-byte loads of the pieces of each row that lie whole inside the chunk, element loads at the unaligned head
//      and tail; the sample as it is into rawL, m into mL (a partial chunk leaves zeros where the call has no sample: they add 0);
//   2. the gate of the current block (s_{j-2}, s_{j-1} of the row, from LDS) on rawL, stored with 16-byte stores where the OUTPUT
//      row is aligned, element stores at its head and tail; and the boxes: one lane per (row, box of the chunk) sums its B values
//      of m, adds the carried partial sum where the call began inside the box, and puts b[k] into the row's ring of 128 b
//      (index k mod 128) -- or, where the call ends inside the box, the partial sum into the state.
// The search runs over the boxes that wait, once the next chunk could make them more than 64 (every B chunks), at a block's end and
// at the call's end, so that its lanes are full whatever B is -- 16 rows x up to 64 k, one lane per (row, k), a wave per row:
//   3. soft[k]: T multiply-adds over the b ring against lp in LDS (read by broadcast), into the row's ring of soft (index k mod
//      the ring's size, the power of two that holds tap[22] back and 64 new; dynamic LDS, 16 KB at the designed tap[22] <= 347);
//   4. the word and the match: 23 LDS reads of soft, the mean threshold, then F times XOR, v_bcnt_u32_b32 and compare against the
//      table in LDS (broadcast), and one LDS atomic on hits[row][f(k)] when k hits.
// At a block end (inside the workgroup, so a later block of the same call is gated by it): 16 lanes per row reduce (hits, f) to the
// first largest with shuffles, lane 0 of the row steps the state, and the counters go back to zero.  The rings, the counters and
// the state come from the handle's pairs at entry and go back at exit.
// HBM traffic: the input once, the output once, and per row and call 2 (tap[22] + T - 1) + 4 F + 32 bytes each way for what is carried.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_rows.h"

namespace fmd_dc {

constexpr int kThreads = 256;
constexpr uint32_t kRows = 16;                            // rows per tile
constexpr uint32_t kLanes = kThreads / kRows;             // lanes per row in staging, gate and block end
constexpr uint32_t kChunk = 64;                           // samples per chunk
constexpr uint32_t kBRing = 128;                          // b per row in LDS: 63 back and 64 new
constexpr uint32_t kBCarry = 64;                          // b per row in the handle's pair (index k mod 64)
constexpr uint32_t kSRing = 1024;                         // soft per row in LDS at most: 511 back and 64 new (a launch has the power
                                                          // of two that holds its tap[22] + 64, as dynamic LDS)
constexpr uint32_t kSCarry = 512;                         // soft per row in the handle's pair (index k mod 512)
constexpr uint32_t kWords = 128;                          // F at most
constexpr uint32_t kState = 8;                            // int32 per row: t + 1, cand + 1, cnt, h, s_prev, s_cur, hits of f*, open box's sum

typedef int i4 __attribute__((ext_vector_type(4)));

// The handle's constant, as it lies on the device.
struct DcsConst {
    uint32_t words[kWords];
    int16_t lp[64];
    uint32_t tap[23];
    uint32_t F, T, lshift, tol, min_hits, confirm, hang, pad;
    uint64_t accept[2];
};

struct DcsLaunch {
    const int16_t* in;         // [n_rows][in_cap][W]
    uint64_t in_cap;
    uint32_t n_in;             // valid samples per row
    uint32_t n_rows;
    const int16_t* hist_in;    // (the rows layer's history: unused)
    int16_t* hist_out;
    uint32_t hcap;
    const int32_t* st_in;      // [n_rows][kState] (all-zero: the state at creation and after reset)
    int32_t* st_out;
    const int16_t* b_in;       // [n_rows][kBCarry]: b[k] at k mod 64
    int16_t* b_out;
    const int16_t* s_in;       // [n_rows][kSCarry]: soft[k] at k mod 512
    int16_t* s_out;
    const uint32_t* hits_in;   // [n_rows][F]: the counters of the block the stream stands in
    uint32_t* hits_out;
    const DcsConst* K;
    uint32_t pos_r;            // core.pos mod P: r of the call's first sample
    uint32_t kbase;            // (index of the first box of the block the call starts in) mod 1024
    uint32_t P, lgB, lgQ;
    uint32_t sring;            // soft per row in LDS: a power of two >= tap[22] + 64
    int16_t* out;              // [n_rows][out_cap][W]
    uint64_t out_cap;
};

template <int W> struct Sample;
template <> struct Sample<1> { typedef uint16_t type; };
template <> struct Sample<2> { typedef uint32_t type; };   // (c0, c1) of one sample

// m of one sample
template <int W>
__device__ __forceinline__ int16_t mix(uint32_t s)
{
    const int a = (int)(s << 16) >> 16;
    if (W == 1) return (int16_t)a;
    return (int16_t)((a + ((int)s >> 16)) >> 1);
}

// (x[c] g) >> 8 of one sample, packed as the sample is
template <int W>
__device__ __forceinline__ uint32_t gate(uint32_t s, int g)
{
    const int a = (int)(s << 16) >> 16;
    uint32_t y = (uint32_t)((a * g) >> 8) & 0xFFFFu;
    if (W == 2) y |= (uint32_t)((((int)s >> 16) * g) >> 8) << 16;
    return y;
}

template <int W>
__global__ void __launch_bounds__(kThreads) fmd_dcs_kernel(const DcsLaunch A)
{
    typedef typename Sample<W>::type sample_t;
    typedef const FMD_DDC_GLOBAL sample_t* gsrc;
    typedef FMD_DDC_GLOBAL sample_t* gdst;
    constexpr uint32_t EB = 2u * W;                          // bytes per sample
    constexpr uint32_t E = 16u / EB;                         // samples per 16-byte piece
    constexpr uint32_t NP = kChunk * EB / 16u + 1u;          // 16-byte pieces a chunk of one row touches at most
    extern __shared__ int16_t softL[];                       // [kRows][A.sring]
    __shared__ int16_t bL[kRows * kBRing];
    __shared__ __attribute__((aligned(16))) int16_t mL2[2 * kRows * kChunk];       // (two chunks: one barrier per chunk)
    __shared__ __attribute__((aligned(16))) sample_t rawL2[2 * kRows * kChunk];
    __shared__ uint32_t hitsL[kRows * kWords];
    __shared__ int32_t stL[kRows * kState];
    __shared__ int32_t carryL[kRows];
    __shared__ DcsConst KL;

    const uint32_t tid = threadIdx.x;
    const uint32_t row0 = blockIdx.x * kRows;
    if (row0 >= A.n_rows) return;
    const uint32_t nrow = A.n_rows - row0 < kRows ? A.n_rows - row0 : kRows;
    const uint32_t P = A.P, lgB = A.lgB, B = 1u << lgB, qm = (1u << A.lgQ) - 1u;
    const uint32_t lgNB = 6u - lgB, NB = 1u << lgNB;         // boxes per chunk
    const uint32_t SR = A.sring, sm = SR - 1u;

    for (uint32_t i = tid; i < sizeof(DcsConst) / 4u; i += kThreads)
        reinterpret_cast<uint32_t*>(&KL)[i] = reinterpret_cast<const uint32_t*>(A.K)[i];
    __syncthreads();
    const uint32_t F = KL.F, T = KL.T, tapmax = KL.tap[22];
    const uint32_t o_end = A.pos_r + A.n_in;                 // stream offsets [pos_r, o_end) from the start of the first block
    const uint32_t k0 = A.kbase + (A.pos_r >> lgB), k1 = A.kbase + (o_end >> lgB);    // boxes complete before and after the call

    if (tid < kRows * kState) stL[tid] = (tid >> 3) < nrow ? A.st_in[(uint64_t)row0 * kState + tid] : 0;
    for (uint32_t i = tid; i < kRows * kWords; i += kThreads) {
        const uint32_t tr = i >> 7, f = i & (kWords - 1u);
        hitsL[i] = tr < nrow && f < F ? A.hits_in[(uint64_t)(row0 + tr) * F + f] : 0u;
    }
    for (uint32_t i = tid; i < kRows * kSCarry; i += kThreads) {                    // soft[k0 - tap[22] ... k0)
        const uint32_t tr = i >> 9, e = i & (kSCarry - 1u);
        if (e < tapmax) {
            const uint32_t k = k0 - tapmax + e;
            softL[tr * SR + (k & sm)] = tr < nrow ? A.s_in[(uint64_t)(row0 + tr) * kSCarry + (k & (kSCarry - 1u))] : (int16_t)0;
        }
    }
    for (uint32_t i = tid; i < kRows * kBCarry; i += kThreads) {                    // b[k0 - (T - 1) ... k0)
        const uint32_t tr = i >> 6, e = i & (kBCarry - 1u);
        if (e + 1u < T) {
            const uint32_t k = k0 - (T - 1u) + e;
            bL[tr * kBRing + (k & (kBRing - 1u))] = tr < nrow ? A.b_in[(uint64_t)(row0 + tr) * kBCarry + (k & (kBCarry - 1u))] : (int16_t)0;
        }
    }
    for (uint32_t i = tid; i < kRows * kChunk; i += kThreads) reinterpret_cast<uint32_t*>(mL2)[i] = 0u;
    __syncthreads();
    if (tid < kRows) {                                       // the open box's sum: taken by the call's first chunk alone
        carryL[tid] = stL[tid * kState + 7u];
        stL[tid * kState + 7u] = 0;
    }
    __syncthreads();

    // staging and gate: thread (row = tid >> 4, pl = tid & 15) takes the pieces pl, pl + 16, ... of its row of every chunk
    const uint32_t row = tid / kLanes, pl = tid & (kLanes - 1u);
    const bool live = row < nrow;
    const uintptr_t R = live ? (uintptr_t)(A.in + (uint64_t)(row0 + row) * A.in_cap * W) : 0;       // the row's samples of this call
    const uintptr_t O = live ? (uintptr_t)(A.out + (uint64_t)(row0 + row) * A.out_cap * W) : 0;
    uint32_t cr = (A.pos_r >> 6) << 6;                       // the chunk's first sample, counted from its block's start
    uint32_t kdone = k0;                                     // the boxes [kdone, ...) are complete but not searched yet
    for (uint32_t c = A.pos_r >> 6; c <= (o_end - 1u) >> 6; ++c) {                 // block-uniform
        const uint32_t oa = c << 6 > A.pos_r ? c << 6 : A.pos_r, ob = (c + 1u) << 6 < o_end ? (c + 1u) << 6 : o_end;
        const uint32_t ja = oa - A.pos_r, jb = ob - A.pos_r;                       // call samples [ja, jb)
        int16_t* const mL = mL2 + (c & 1u) * (kRows * kChunk);
        sample_t* const rawL = rawL2 + (c & 1u) * (kRows * kChunk);
        if (ob - oa != kChunk) {                             // a partial chunk: zeros where the call has no sample
            for (uint32_t i = tid; i < kRows * kChunk / 2u; i += kThreads) reinterpret_cast<uint32_t*>(mL)[i] = 0u;
            __syncthreads();
        }
        // ---- 1. the samples -----------------------------------------------------------------------------------------------------
        for (uint32_t idx = pl; idx < NP; idx += kLanes) {   // lane pl of the row's 16 takes every 16th piece
            const uintptr_t a0 = R + (uintptr_t)ja * EB, a1 = R + (uintptr_t)jb * EB;
            const uintptr_t ca = ((a0 >> 4) + idx) << 4;
            if (!live || ca >= a1) continue;
            if (ca >= a0 && ca + 16u <= a1) {                // whole inside the chunk
                const i4 v = *(const FMD_DDC_GLOBAL i4*)ca;
                const uint32_t e0 = (A.pos_r + (uint32_t)((ca - R) / EB)) & 63u;
                const uint32_t d[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
#pragma unroll
                for (uint32_t e = 0; e < E; ++e) {
                    const uint32_t s = W == 2 ? d[e] : (d[e >> 1] >> (16u * (e & 1u))) & 0xFFFFu;
                    rawL[row * kChunk + e0 + e] = (sample_t)s;
                    mL[row * kChunk + e0 + e] = mix<W>(s);
                }
            } else {                                         // the unaligned head or tail: exactly the samples of the chunk
                for (uint32_t e = 0; e < E; ++e) {
                    const uintptr_t a = ca + e * EB;
                    if (a < a0 || a >= a1) continue;
                    const uint32_t eo = (A.pos_r + (uint32_t)((a - R) / EB)) & 63u;
                    const uint32_t s = *(gsrc)a;
                    rawL[row * kChunk + eo] = (sample_t)s;
                    mL[row * kChunk + eo] = mix<W>(s);
                }
            }
        }
        __syncthreads();

        // ---- 2. the gate of the current block -------------------------------------------------------------------------------------
        for (uint32_t idx = pl; idx < NP; idx += kLanes) {
            const uintptr_t o0 = O + (uintptr_t)ja * EB, o1 = O + (uintptr_t)jb * EB;
            const uintptr_t ca = ((o0 >> 4) + idx) << 4;
            if (!live || ca >= o1) continue;
            const int sp = stL[row * kState + 4u], ds = stL[row * kState + 5u] - sp;
            if (ca >= o0 && ca + 16u <= o1) {                // a whole piece of the output row
                const uint32_t o = A.pos_r + (uint32_t)((ca - O) / EB);
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (uint32_t e = 0; e < E; ++e) {
                    const uint32_t r = cr + ((o + e) & 63u), k = (r < qm ? r : qm) + 1u;
                    const uint32_t y = gate<W>(rawL[row * kChunk + ((o + e) & 63u)], sp + ((ds * (int)k) >> A.lgQ));
                    if (W == 2) w[e] = y; else w[e >> 1] |= y << (16u * (e & 1u));
                }
                *(FMD_DDC_GLOBAL i4*)ca = i4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
            } else {                                         // the unaligned head or tail
                for (uint32_t e = 0; e < E; ++e) {
                    const uintptr_t a = ca + e * EB;
                    if (a < o0 || a >= o1) continue;
                    const uint32_t o = A.pos_r + (uint32_t)((a - O) / EB);
                    const uint32_t r = cr + (o & 63u), k = (r < qm ? r : qm) + 1u;
                    *(gdst)a = (sample_t)gate<W>(rawL[row * kChunk + (o & 63u)], sp + ((ds * (int)k) >> A.lgQ));
                }
            }
        }

        // ---- 2b. the boxes --------------------------------------------------------------------------------------------------------
        const uint32_t ea = oa & 63u, eb = ob - (c << 6);    // the chunk's samples [ea, eb) of 64
        for (uint32_t i = tid; i < kRows << lgNB; i += kThreads) {
            const uint32_t tr = i >> lgNB, q = i & (NB - 1u), lo = q << lgB, hi = lo + B;
            if (hi <= ea || lo >= eb) continue;              // complete before the call, or not begun
            int s = lo < ea ? carryL[tr] : 0;                // (only the call's first chunk starts inside a box)
            for (uint32_t e = lo; e < hi; ++e) s += mL[tr * kChunk + e];
            if (hi <= eb) bL[tr * kBRing + ((A.kbase + (c << lgNB) + q) & (kBRing - 1u))] = (int16_t)(s >> lgB);
            else stL[tr * kState + 7u] = s;
        }

        // ---- the search: once 64 boxes wait, at a block's end and at the call's end -------------------------------------------------
        const uint32_t kcur = A.kbase + (c << lgNB) + (eb >> lgB);                 // boxes complete behind this chunk
        const bool block_end = eb == kChunk && cr + kChunk == P;
        if (block_end || ob == o_end || kcur - kdone + NB > kChunk) {              // block-uniform
            const uint32_t np = kcur - kdone;                // <= 64: the b ring holds them and 63 before them
            __syncthreads();                                 // the boxes are written
            if (np) {
                // ---- 3. soft ------------------------------------------------------------------------------------------------------
                for (uint32_t i = tid; i < kRows * kChunk; i += kThreads) {
                    const uint32_t tr = i >> 6, q = i & 63u;
                    if (q >= np) continue;
                    const uint32_t k = kdone + q;
                    const int16_t* const br = bL + tr * kBRing;
                    int acc = 0;
                    for (uint32_t t = 0; t < T; ++t) acc += (int)KL.lp[t] * (int)br[(k - (T - 1u) + t) & (kBRing - 1u)];
                    acc >>= KL.lshift;
                    acc = acc > 32767 ? 32767 : (acc < -32768 ? -32768 : acc);
                    softL[tr * SR + (k & sm)] = (int16_t)acc;
                }
                __syncthreads();
                // ---- 4. the word and the match ------------------------------------------------------------------------------------
                for (uint32_t i = tid; i < kRows * kChunk; i += kThreads) {
                    const uint32_t tr = i >> 6, q = i & 63u;
                    if (q >= np || tr >= nrow) continue;
                    const uint32_t k = kdone + q;
                    const int16_t* const sr = softL + tr * SR;
                    int v[23], sum = 0;
#pragma unroll
                    for (uint32_t j = 0; j < 23u; ++j) {
                        v[j] = sr[(k - KL.tap[j]) & sm];
                        sum += v[j];
                    }
                    uint32_t w = 0;
#pragma unroll
                    for (uint32_t j = 0; j < 23u; ++j) w |= (uint32_t)(23 * v[j] > sum) << j;
                    uint32_t best = 32u, bf = 0;
                    for (uint32_t f = 0; f < F; ++f) {
                        const uint32_t d = (uint32_t)__builtin_popcount(w ^ KL.words[f]);
                        if (d < best) { best = d; bf = f; }
                    }
                    if (best <= KL.tol) atomicAdd(&hitsL[tr * kWords + bf], 1u);
                }
                kdone = kcur;
            }
        }

        // ---- the block's end: f*, the decision, the state ---------------------------------------------------------------------------
        if (block_end) {                                     // block-uniform
            __syncthreads();                                 // the counters are complete
            uint32_t bh = 0, bf = 0xFFFFu;                   // no index yet
            for (uint32_t f = pl; f < F; f += kLanes) {
                const uint32_t n = hitsL[row * kWords + f];
                if (bf == 0xFFFFu || n > bh) { bh = n; bf = f; }
            }
            for (int off = 1; off < (int)kLanes; off <<= 1) {                      // the first largest of the row's 16 lanes
                const uint32_t oh = (uint32_t)__shfl_xor((int)bh, off), of = (uint32_t)__shfl_xor((int)bf, off);
                if (of != 0xFFFFu && (bf == 0xFFFFu || oh > bh || (oh == bh && of < bf))) { bh = oh; bf = of; }
            }
            for (uint32_t f = pl; f < kWords; f += kLanes) hitsL[row * kWords + f] = 0u;     // (each lane the counters it read)
            if (pl == 0u) {
                int32_t* const st = stL + row * kState;
                uint32_t t1 = (uint32_t)st[0], cand1 = (uint32_t)st[1], cnt = (uint32_t)st[2], h = (uint32_t)st[3];
                if (bh >= KL.min_hits) {
                    if (bf + 1u == cand1) cnt = cnt < 65535u ? cnt + 1u : 65535u;
                    else { cand1 = bf + 1u; cnt = 1u; }
                } else { cand1 = 0u; cnt = 0u; }
                if (cnt >= KL.confirm) { t1 = cand1; h = KL.hang; }
                else if (h > 0u) --h;
                else t1 = 0u;
                st[0] = (int32_t)t1; st[1] = (int32_t)cand1; st[2] = (int32_t)cnt; st[3] = (int32_t)h;
                st[4] = st[5];
                st[5] = t1 && ((KL.accept[(t1 - 1u) >> 6] >> ((t1 - 1u) & 63u)) & 1ull) ? 256 : 0;
                st[6] = (int32_t)bh;
            }
            __syncthreads();                                 // the next chunk's gate reads the state
        }
        cr = cr + kChunk == P ? 0u : cr + kChunk;
    }
    __syncthreads();                                         // the last search's counters, the last boxes

    if (tid < kRows * kState && (tid >> 3) < nrow) A.st_out[(uint64_t)row0 * kState + tid] = stL[tid];
    for (uint32_t i = tid; i < kRows * kWords; i += kThreads) {
        const uint32_t tr = i >> 7, f = i & (kWords - 1u);
        if (tr < nrow && f < F) A.hits_out[(uint64_t)(row0 + tr) * F + f] = hitsL[i];
    }
    for (uint32_t i = tid; i < kRows * kSCarry; i += kThreads) {                    // soft[k1 - tap[22] ... k1)
        const uint32_t tr = i >> 9, e = i & (kSCarry - 1u);
        if (e < tapmax && tr < nrow) {
            const uint32_t k = k1 - tapmax + e;
            A.s_out[(uint64_t)(row0 + tr) * kSCarry + (k & (kSCarry - 1u))] = softL[tr * SR + (k & sm)];
        }
    }
    for (uint32_t i = tid; i < kRows * kBCarry; i += kThreads) {                    // b[k1 - (T - 1) ... k1)
        const uint32_t tr = i >> 6, e = i & (kBCarry - 1u);
        if (e + 1u < T && tr < nrow) {
            const uint32_t k = k1 - (T - 1u) + e;
            A.b_out[(uint64_t)(row0 + tr) * kBCarry + (k & (kBCarry - 1u))] = bL[tr * kBRing + (k & (kBRing - 1u))];
        }
    }
}

}  // namespace fmd_dc

struct fmd_dcs {
    FmdRows rows;                                         // (its history is unused: hcap = 1, the smallest the layer takes)
    FmdDdcPair state;                                     // [n_rows][kState] int32
    FmdDdcPair rings;                                     // [n_rows][kSCarry] int16 of soft, then [n_rows][kBCarry] int16 of b
    FmdDdcPair hits;                                      // [n_rows][F] uint32
    void* d_const = nullptr;                              // one DcsConst
    fmd_dc::DcsConst konst{};                             // the same
    fmd_dcs_config cfg{};
    uint32_t F = 0, lgQ = 0, lgB = 0, sring = 128;
};

namespace {

int dcs_enqueue(fmd_dcs* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, hipStream_t stream)
{
    FmdRows& r = h->rows;
    if (const int rc = fmd_rows_check_call(r, d_in, n_in, in_cap, d_out)) return rc;
    if (out_cap < n_in) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    if (n_in == 0) {                                         // nothing to take: no launch
        if (n_out) *n_out = 0;
        return FMD_OK;
    }
    fmd_dc::DcsLaunch A{};
    fmd_rows_fill(A, r, d_in, n_in, in_cap, d_out, out_cap);
    A.st_in = h->state.in<int32_t>(r.core.cur); A.st_out = h->state.out<int32_t>(r.core.cur);
    A.s_in = h->rings.in<int16_t>(r.core.cur); A.s_out = h->rings.out<int16_t>(r.core.cur);
    A.b_in = A.s_in + (size_t)r.n_rows * fmd_dc::kSCarry; A.b_out = A.s_out + (size_t)r.n_rows * fmd_dc::kSCarry;
    A.hits_in = h->hits.in<uint32_t>(r.core.cur); A.hits_out = h->hits.out<uint32_t>(r.core.cur);
    A.K = static_cast<const fmd_dc::DcsConst*>(h->d_const);
    A.pos_r = (uint32_t)(r.core.pos % h->cfg.block);
    A.kbase = (uint32_t)(((r.core.pos - A.pos_r) >> h->lgB) & (fmd_dc::kSRing - 1u));
    A.P = h->cfg.block; A.lgB = h->lgB; A.lgQ = h->lgQ; A.sring = h->sring;
    const uint32_t grid = (r.n_rows + fmd_dc::kRows - 1u) / fmd_dc::kRows;
    return fmd_rows_launch(r, fmd_dc::fmd_dcs_kernel<1>, fmd_dc::fmd_dcs_kernel<2>, grid, fmd_dc::kThreads, A, stream, n_in, n_in, n_out);
}

bool pow2(uint32_t v) { return v && (v & (v - 1u)) == 0; }

}  // namespace

extern "C" {

size_t fmd_dcs_out_cap(size_t n_in) { return n_in; }

int fmd_dcs_new(const fmd_dcs_config* cfg, const uint32_t* words, uint32_t n_words, uint32_t width, const fmd_device_config* dev, fmd_dcs** out)
{
    if (const int rc = fmd_rows_new_args(cfg, dev, out, width)) return rc;
    if (!words) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    const uint32_t P = cfg->block, F = n_words;
    if (P < 64 || P > 32768 || (P & 63u)) { fmd_internal_set_err("need block a multiple of 64 in [64, 32768]"); return FMD_ERR_UNSUPPORTED; }
    if (!pow2(cfg->box) || cfg->box > 64) { fmd_internal_set_err("need box a power of two in [1, 64]"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->n_taps < 1 || cfg->n_taps > 64) { fmd_internal_set_err("need 1 <= n_taps <= 64"); return FMD_ERR_UNSUPPORTED; }
    for (uint32_t t = 0; t < cfg->n_taps; ++t)
        if (cfg->lp[t] > 1023 || cfg->lp[t] < -1023) { fmd_internal_set_err("|lp entry| > 1023"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->lshift > 31) { fmd_internal_set_err("need lshift <= 31"); return FMD_ERR_UNSUPPORTED; }
    bool taps_ok = cfg->tap[0] == 0 && cfg->tap[22] <= 511;
    for (uint32_t j = 1; j < 23; ++j) taps_ok = taps_ok && cfg->tap[j] >= cfg->tap[j - 1];
    if (!taps_ok) { fmd_internal_set_err("need tap[0] = 0, tap non-decreasing, tap[22] <= 511"); return FMD_ERR_UNSUPPORTED; }
    if (F < 1 || F > 128) { fmd_internal_set_err("need 1 <= n_words <= 128"); return FMD_ERR_UNSUPPORTED; }
    for (uint32_t f = 0; f < F; ++f)
        if (words[f] >> 23) { fmd_internal_set_err("need every word below 2^23"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->tol > 23) { fmd_internal_set_err("need tol <= 23"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->min_hits < 1) { fmd_internal_set_err("need min_hits >= 1"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->confirm < 1 || cfg->confirm > 255) { fmd_internal_set_err("need 1 <= confirm <= 255"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->hang > 65535) { fmd_internal_set_err("need hang <= 65535"); return FMD_ERR_UNSUPPORTED; }
    if (!pow2(cfg->ramp) || cfg->ramp > P) { fmd_internal_set_err("need ramp a power of two in [1, block]"); return FMD_ERR_UNSUPPORTED; }
    if (const int rc = fmd_rows_count_arg(dev)) return rc;
    fmd_dcs* h = new (std::nothrow) fmd_dcs();
    if (!h) return FMD_ERR_NOMEM;
    h->cfg = *cfg; h->F = F;
    while ((1u << h->lgQ) < cfg->ramp) ++h->lgQ;
    while ((1u << h->lgB) < cfg->box) ++h->lgB;
    fmd_dc::DcsConst& K = h->konst;
    for (uint32_t f = 0; f < F; ++f) K.words[f] = words[f];
    for (uint32_t t = 0; t < cfg->n_taps; ++t) K.lp[t] = cfg->lp[t];
    for (uint32_t j = 0; j < 23; ++j) K.tap[j] = cfg->tap[j];
    K.F = F; K.T = cfg->n_taps; K.lshift = cfg->lshift; K.tol = cfg->tol; K.min_hits = cfg->min_hits;
    K.confirm = cfg->confirm; K.hang = cfg->hang;
    K.accept[0] = cfg->accept[0]; K.accept[1] = cfg->accept[1];
    while (h->sring < cfg->tap[22] + fmd_dc::kChunk) h->sring <<= 1;          // <= kSRing
    h->rows.lds = (size_t)fmd_dc::kRows * h->sring * sizeof(int16_t);          // the soft rings; the rest of the kernel's LDS is static
    h->rows.width = width; h->rows.n_rows = dev->n_channels; h->rows.hcap = 1u;
    const size_t n = dev->n_channels;
    fmd_ddc_add_pair(h->rows.core, h->state, n * fmd_dc::kState * sizeof(int32_t));
    fmd_ddc_add_pair(h->rows.core, h->rings, n * (fmd_dc::kSCarry + fmd_dc::kBCarry) * sizeof(int16_t));
    fmd_ddc_add_pair(h->rows.core, h->hits, n * F * sizeof(uint32_t));
    fmd_ddc_add_owned(h->rows.core, h->d_const, &h->konst, sizeof h->konst);
    return fmd_rows_device(h, dev, fmd_dcs_free, out);
}

void fmd_dcs_free(fmd_dcs* h) { fmd_rows_free(h); }
int fmd_dcs_reset(fmd_dcs* h) { return fmd_rows_reset(h); }
int fmd_dcs_check(fmd_dcs* h) { return fmd_rows_check(h); }

int fmd_dcs_outputs(const fmd_dcs* h, uint64_t* inputs, uint64_t* outputs)
{
    return fmd_rows_outputs(h, inputs, outputs, [](const fmd_dcs*, uint64_t n) { return n; });
}

int fmd_dcs_status(fmd_dcs* h, int32_t* code, uint32_t* hits, uint8_t* open)
{
    if (!h || !code || !hits || !open) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    std::vector<int32_t> st;
    if (const int rc = fmd_rows_read_state(h->rows, h->state, fmd_dc::kState, st)) return rc;
    for (size_t r = 0; r < h->rows.n_rows; ++r) {
        const int32_t* s = &st[r * fmd_dc::kState];
        code[r] = s[0] - 1;
        hits[r] = (uint32_t)s[6];
        open[r] = s[5] != 0;
    }
    return FMD_OK;
}

int fmd_dcs_run_device(fmd_dcs* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, void* stream)
{
    return fmd_ddc_run_device(h ? &h->rows.core : nullptr, d_in, d_out,
                              [&] { return dcs_enqueue(h, d_in, n_in, in_cap, d_out, out_cap, n_out, static_cast<hipStream_t>(stream)); });
}

// (a call of no samples has nothing to take: it does not touch the device)
int fmd_dcs_run_batch(fmd_dcs* h, const int16_t* in, size_t n_in, size_t in_cap, int16_t* out, size_t out_cap, size_t* n_out)
{
    return fmd_rows_run_batch(h, dcs_enqueue, in, n_in, in_cap, out, out_cap, n_out, [](size_t n) { return n == 0; });
}

int fmd_dcs_kernel_name(const fmd_dcs* h, char* name, size_t cap)
{
    return fmd_rows_kernel_name(h, name, cap, "fmd_dc::fmd_dcs_kernel<%u>");
}

}  // extern "C"
