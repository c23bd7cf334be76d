// fmd_modes.hip -- the Mode S bank: the ADS-B messages of many 2 Msample/s u8 IQ streams, decoded on the device.
//
// Definition: include/fmd.h, "Mode S bank"; tests/modes_ref.py.  Per stream the call's n samples stand behind the m of the 240
// samples carried from the calls before: v[j], j < 240 + n, with v[240 + c] the call's sample c.  Position u < n of the call is the
// absolute position p = pos - 239 + u (decided here when p >= 0): its a_j is v[u + 1 + j], and the last one read, a_239, is the
// call's sample u.  Carrying 240 samples where 239 would do keeps v's index and the call's sample index equal mod 8, so that the
// 16-byte pieces of the staging are aligned in the call and in LDS at once.
//
// Pass 0, one workgroup of four waves per (stream, tile of kTile positions):
//   staging   the tile's v as a u16 plane in LDS: 16 bytes of IQ -> eight m -> one 16-byte LDS store per lane and piece; the
//             first 30 pieces of a stream's first tile are the carried samples as they lie;
//   preamble  a lane takes eight consecutive positions out of registers (three 16-byte LDS reads: 24 samples, 22 used); the eight
//             verdicts are a byte, and a wave scan of its popcounts puts the passing positions into an LDS queue in increasing p;
//   decode    a whole wave per queued candidate: lane l decides the bits l and l + 64, two ballots give the 112 bits as wave-uniform
//             words, every lane XORs in T[l] / T[l + 64] where its bit is set, an XOR reduction gives the syndrome, and the single-bit
//             fix is one compare against the lane's own two entries followed by a ballot.  The verdict goes into the queue entry;
//   keep      wave 0 ranks the accepted entries (ballot and popcount, in queue order) and leaves the tile's first min(count,
//             msg_cap) positions as u16 and the tile's three counts in scratch.  A stream's first msg_cap records, restricted to one
//             tile, are among that tile's first msg_cap.
// Pass 1, one wave per stream: walks the tiles' counts in tile order, decodes the stream's first msg_cap kept positions again --
// from global memory this time, with the same wave routine -- into the records, sums the counters, and carries the last 240 samples
// forward.  Nothing depends on scheduling: there is no atomic anywhere.
// Scratch per call: 16 bytes + 2 msg_cap bytes per tile; at 4096 streams x 32 tiles (262144 bytes each) and msg_cap 32 that is
// 10 MiB, at msg_cap 256 it is 66 MiB.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_rows.h"

namespace fmd_ms {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kTile = 4096;                          // positions per workgroup: two rounds of 256 lanes x 8
constexpr uint32_t kTail = 240;                           // samples carried per stream (as m, u16)
constexpr uint32_t kPieces = kTile / 8 + kTail / 8;       // 16-byte pieces of a tile's plane
constexpr uint32_t kRounds = kTile / (8 * kThreads);
constexpr uint32_t kAccepted = 0x8000u, kFixed = 0x4000u, kPosMask = 0x3FFFu;   // a queue entry: position in the tile and verdict
constexpr uint32_t kStats = 4;                            // dwords per tile: acceptances, candidates, fixes, 0
constexpr uint32_t kState = 8;                            // dwords per stream: samples, candidates, messages, fixed (u64 each)
static_assert(kTile <= kPosMask + 1u && kTile % (8 * kThreads) == 0 && kTail % 8 == 0, "tile geometry");

typedef int i4 __attribute__((ext_vector_type(4)));

struct ModesLaunch {
    const uint8_t* iq;         // [n_streams][cap_bytes]
    uint64_t cap_bytes;
    uint32_t n;                // samples per stream in this call, >= 1
    uint32_t n_streams, n_tiles;
    uint32_t skip;             // positions u < skip lie in front of the stream's sample 0
    uint32_t aligned;          // every stream's bytes start 16-byte aligned
    uint32_t min_power, fix_errors, df11, msg_cap;
    const uint16_t* tail_in;   // [n_streams][kTail]
    uint16_t* tail_out;
    const uint32_t* table;     // T_112
    uint32_t* stats;           // [n_streams][n_tiles][kStats]
    uint16_t* kept;            // [n_streams][n_tiles][msg_cap]
    const uint32_t* st_in;     // [n_streams][kState]
    uint32_t* st_out;
    uint32_t* cnt_out;         // [n_streams]
    uint8_t* rec_out;          // [n_streams][msg_cap] fmd_modes_msg
};

// m of the samples in one dword of IQ (I0 Q0 I1 Q1), packed low | high << 16
__device__ __forceinline__ uint32_t mag2(uint32_t d)
{
    const int i0 = 2 * (int)(d & 255u) - 255, q0 = 2 * (int)((d >> 8) & 255u) - 255;
    const int i1 = 2 * (int)((d >> 16) & 255u) - 255, q1 = 2 * (int)(d >> 24) - 255;
    return (uint32_t)(i0 * i0 + q0 * q0) >> 1 | ((uint32_t)(i1 * i1 + q1 * q1) >> 1) << 16;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v ^= (uint32_t)__shfl_xor((int)v, m);
    return v;
}

// What a wave makes of the candidate whose a_j is a(j): wave-uniform.
struct Verdict {
    bool accepted;
    uint32_t power, meta;      // S; n_bytes | fixed_bit << 8 | df << 16
    uint64_t hi, lo;           // the bits 0 ... 63 and 64 ... 127 as big-endian numbers, after the fix, zero behind the message
};

// tl, th: T_112[lane] and T_112[lane + 64] (0 from lane 48 on); ts: T_56[lane] (0 from lane 56 on)
template <class Fetch>
__device__ __forceinline__ Verdict decode(Fetch a, uint32_t lane, uint32_t tl, uint32_t th, uint32_t ts, uint32_t fix_errors, uint32_t df11)
{
    const bool b0 = a(16u + 2u * lane) > a(17u + 2u * lane);
    const bool b1 = lane < 48u && a(144u + 2u * lane) > a(145u + 2u * lane);
    uint64_t w0 = __ballot(b0), w1 = __ballot(b1);           // bit t of the message at bit t (w0) and t - 64 (w1)
    const bool is_long = (w0 & 1ull) != 0ull;
    const uint32_t df = (uint32_t)(__brevll(w0) >> 59);
    const uint32_t syn = wave_xor(is_long ? (b0 ? tl : 0u) ^ (b1 ? th : 0u) : (b0 ? ts : 0u));
    Verdict v;
    v.power = a(0u) + a(2u) + a(7u) + a(9u);
    uint32_t fixed = 0xFFu;
    if (df == 17u || df == 18u) {
        v.accepted = syn == 0u;
        if (!v.accepted && fix_errors) {
            const uint64_t f0 = __ballot(lane >= 5u && tl == syn), f1 = __ballot(lane < 48u && th == syn);
            if (f0 | f1) {                                   // (the entries are distinct: one bit at most)
                v.accepted = true;
                fixed = f0 ? (uint32_t)__builtin_ctzll(f0) : 64u + (uint32_t)__builtin_ctzll(f1);
                w0 ^= f0; w1 ^= f1;
            }
        }
    } else {
        v.accepted = df == 11u && df11 && (syn & 0xFFFF80u) == 0u;
    }
    if (!is_long) { w0 &= (1ull << 56) - 1ull; w1 = 0ull; }
    v.hi = __brevll(w0); v.lo = __brevll(w1);
    v.meta = (is_long ? 14u : 7u) | fixed << 8 | df << 16;
    return v;
}

__device__ __forceinline__ void lane_table(const ModesLaunch& L, uint32_t lane, uint32_t& tl, uint32_t& th, uint32_t& ts)
{
    typedef const FMD_DDC_GLOBAL uint32_t* gw;
    const gw T = (gw)(uintptr_t)L.table;
    tl = T[lane];
    th = lane < 48u ? T[lane + 64u] : 0u;
    ts = lane < 56u ? T[lane + 56u] : 0u;
}

__global__ void __launch_bounds__(kThreads) fmd_modes_tile_kernel(const ModesLaunch L)
{
    __shared__ __attribute__((aligned(16))) uint16_t plane[kPieces * 8u];     // v[tile * kTile + x]
    __shared__ uint16_t queue[kTile];
    __shared__ uint32_t wsum[kRounds][kWaves];

    typedef const FMD_DDC_GLOBAL uint32_t* gw;
    typedef const FMD_DDC_GLOBAL i4* gq;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t s = blockIdx.x / L.n_tiles, tile = blockIdx.x - s * L.n_tiles;
    const uint32_t u0 = tile * kTile;                        // the tile's first position; its plane starts at v[u0]
    const uint8_t* const row = L.iq + (uint64_t)s * L.cap_bytes;

    // ---- staging ------------------------------------------------------------------------------------------------------------------
    for (uint32_t k = tid; k < kPieces; k += kThreads) {
        const uint32_t j0 = u0 + 8u * k;                     // v index of the piece's first sample
        i4 piece = i4{0, 0, 0, 0};
        if (j0 < kTail) {
            piece = *(gq)(uintptr_t)(L.tail_in + (uint64_t)s * kTail + j0);
        } else {
            const uint32_t c0 = j0 - kTail;                  // the call's sample, a multiple of 8
            if (c0 < L.n) {
                uint32_t d[4] = {0u, 0u, 0u, 0u};
                if (L.aligned && c0 + 8u <= L.n) {
                    const i4 q = *(gq)(uintptr_t)(row + 2ull * c0);
                    d[0] = (uint32_t)q.x; d[1] = (uint32_t)q.y; d[2] = (uint32_t)q.z; d[3] = (uint32_t)q.w;
                } else {
                    const gw p = (gw)(uintptr_t)(row + 2ull * c0);
#pragma unroll
                    for (uint32_t e = 0; e < 4u; ++e)
                        if (c0 + 2u * e < L.n) d[e] = p[e];   // (n is even: a dword lies whole inside or outside; what lies
                }                                             // outside is read by no position that is decided)
                piece = i4{(int)mag2(d[0]), (int)mag2(d[1]), (int)mag2(d[2]), (int)mag2(d[3])};
            }
        }
        reinterpret_cast<i4*>(plane)[k] = piece;
    }
    __syncthreads();

    // ---- the preamble test: position w of the tile reads plane[w + 1 ...] ------------------------------------------------------------
    uint32_t mask8[kRounds], excl[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t g = r * kThreads + tid;
        uint32_t R[24];
#pragma unroll
        for (uint32_t q = 0; q < 3u; ++q) {
            const i4 v = reinterpret_cast<const i4*>(plane)[g + q];
            const uint32_t d[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e) { R[8u * q + 2u * e] = d[e] & 0xFFFFu; R[8u * q + 2u * e + 1u] = d[e] >> 16; }
        }
        uint32_t m = 0u;
#pragma unroll
        for (uint32_t e = 0; e < 8u; ++e) {
            const uint32_t* const a = &R[e + 1u];
            const uint32_t S = a[0] + a[2] + a[7] + a[9];
            bool ok = a[0] > a[1] && a[1] < a[2] && a[2] > a[3] && a[3] < a[0] && a[4] < a[0] && a[5] < a[0] && a[6] < a[0] &&
                      a[7] > a[8] && a[8] < a[9] && a[9] > a[6];
            ok = ok && 6u * a[4] < S && 6u * a[5] < S && 6u * a[11] < S && 6u * a[12] < S && 6u * a[13] < S && 6u * a[14] < S;
            ok = ok && S >= L.min_power;
            const uint32_t u = u0 + 8u * g + e;
            ok = ok && u < L.n && u >= L.skip;
            m |= ok ? 1u << e : 0u;
        }
        mask8[r] = m;
        uint32_t inc = (uint32_t)__builtin_popcount(m);      // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
            if (lane >= (uint32_t)o) inc += t;
        }
        excl[r] = inc - (uint32_t)__builtin_popcount(m);
        if (lane == 63u) wsum[r][wave] = inc;
    }
    __syncthreads();
    uint32_t qn = 0u;                                        // every thread ends with the queue's length
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        uint32_t at = qn + excl[r];
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            if (w < wave) at += wsum[r][w];
            qn += wsum[r][w];
        }
        const uint32_t g = r * kThreads + tid;
#pragma unroll
        for (uint32_t e = 0; e < 8u; ++e)
            if (mask8[r] >> e & 1u) queue[at++] = (uint16_t)(8u * g + e);
    }
    __syncthreads();

    // ---- a wave per candidate --------------------------------------------------------------------------------------------------------
    if (qn) {                                                // block-uniform
        uint32_t tl, th, ts;
        lane_table(L, lane, tl, th, ts);
        for (uint32_t i = wave; i < qn; i += kWaves) {
            const uint32_t w = queue[i];
            const uint16_t* const a0 = &plane[w + 1u];
            const Verdict v = decode([a0](uint32_t j) { return (uint32_t)a0[j]; }, lane, tl, th, ts, L.fix_errors, L.df11);
            if (lane == 0u && v.accepted) queue[i] = (uint16_t)(w | kAccepted | (((v.meta >> 8) & 0xFFu) != 0xFFu ? kFixed : 0u));
        }
    }
    __syncthreads();

    // ---- the tile's first msg_cap acceptances, in order, and its counts -----------------------------------------------------------------
    if (wave == 0u) {
        typedef FMD_DDC_GLOBAL uint16_t* gk;
        const uint64_t t_at = (uint64_t)s * L.n_tiles + tile;
        const gk kept = (gk)(uintptr_t)(L.kept + t_at * L.msg_cap);
        uint32_t n_acc = 0u, n_fix = 0u;
        for (uint32_t base = 0; base < qn; base += 64u) {
            const uint32_t i = base + lane, e = i < qn ? queue[i] : 0u;
            const uint64_t acc = __ballot((e & kAccepted) != 0u);
            const uint32_t rank = n_acc + (uint32_t)__builtin_popcountll(acc & ((1ull << lane) - 1ull));
            if ((e & kAccepted) && rank < L.msg_cap) kept[rank] = (uint16_t)(e & kPosMask);
            n_acc += (uint32_t)__builtin_popcountll(acc);
            n_fix += (uint32_t)__builtin_popcountll(__ballot((e & kFixed) != 0u));
        }
        if (lane == 0u)
            *(FMD_DDC_GLOBAL i4*)(uintptr_t)(L.stats + t_at * kStats) = i4{(int)n_acc, (int)qn, (int)n_fix, 0};
    }
}

// v[j] of stream s, from global memory: the carried samples, then the call's
__device__ __forceinline__ uint32_t sample_at(const ModesLaunch& L, uint32_t s, uint32_t j)
{
    if (j < kTail) return ((const FMD_DDC_GLOBAL uint16_t*)(uintptr_t)(L.tail_in + (uint64_t)s * kTail))[j];
    const FMD_DDC_GLOBAL uint8_t* const b = (const FMD_DDC_GLOBAL uint8_t*)(uintptr_t)(L.iq + (uint64_t)s * L.cap_bytes + 2ull * (j - kTail));
    const int i = 2 * (int)b[0] - 255, q = 2 * (int)b[1] - 255;
    return (uint32_t)(i * i + q * q) >> 1;
}

__global__ void __launch_bounds__(64) fmd_modes_gather_kernel(const ModesLaunch L)
{
    typedef const FMD_DDC_GLOBAL uint32_t* gw;
    typedef const FMD_DDC_GLOBAL uint16_t* gk;
    const uint32_t lane = threadIdx.x, s = blockIdx.x;
    const gw stats = (gw)(uintptr_t)(L.stats + (uint64_t)s * L.n_tiles * kStats);
    uint32_t tl = 0u, th = 0u, ts = 0u;
    bool have_table = false;
    uint64_t total = 0ull, cand = 0ull, fixd = 0ull;         // total is wave-uniform; cand and fixd are per lane until the end
    for (uint32_t tb = 0; tb < L.n_tiles; tb += 64u) {
        const uint32_t t = tb + lane;
        uint32_t c = 0u;
        if (t < L.n_tiles) { c = stats[t * kStats]; cand += stats[t * kStats + 1u]; fixd += stats[t * kStats + 2u]; }
        uint64_t busy = __ballot(c != 0u);
        while (busy) {                                       // the tiles with acceptances, in order
            const int tj = __builtin_ctzll(busy);
            busy &= busy - 1ull;
            const uint32_t ct = (uint32_t)__shfl((int)c, tj), tile = tb + (uint32_t)tj;
            const uint32_t have = ct < L.msg_cap ? ct : L.msg_cap;
            const gk kept = (gk)(uintptr_t)(L.kept + ((uint64_t)s * L.n_tiles + tile) * L.msg_cap);
            for (uint32_t k = 0; k < have && total + k < L.msg_cap; ++k) {
                if (!have_table) { lane_table(L, lane, tl, th, ts); have_table = true; }
                const uint32_t u = tile * kTile + kept[k];
                const Verdict v = decode([&L, s, u](uint32_t j) { return sample_at(L, s, u + 1u + j); }, lane, tl, th, ts, L.fix_errors, L.df11);
                if (lane == 0u) {
                    FMD_DDC_GLOBAL i4* const rec =
                        (FMD_DDC_GLOBAL i4*)(uintptr_t)(L.rec_out + ((uint64_t)s * L.msg_cap + total + k) * sizeof(fmd_modes_msg));
                    rec[0] = i4{(int)u - 239, (int)v.power, (int)v.meta, (int)__builtin_bswap32((uint32_t)(v.hi >> 32))};
                    rec[1] = i4{(int)__builtin_bswap32((uint32_t)v.hi), (int)__builtin_bswap32((uint32_t)(v.lo >> 32)),
                                (int)(__builtin_bswap32((uint32_t)v.lo) & 0xFFFFu), 0};
                }
            }
            total += ct;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { cand += __shfl_xor(cand, m); fixd += __shfl_xor(fixd, m); }

    // the last 240 samples, forward
    FMD_DDC_GLOBAL uint16_t* const tout = (FMD_DDC_GLOBAL uint16_t*)(uintptr_t)(L.tail_out + (uint64_t)s * kTail);
    for (uint32_t j = lane; j < kTail; j += 64u) tout[j] = (uint16_t)sample_at(L, s, L.n + j);

    if (lane == 0u) {
        const gw si = (gw)(uintptr_t)(L.st_in + (uint64_t)s * kState);
        FMD_DDC_GLOBAL uint32_t* const so = (FMD_DDC_GLOBAL uint32_t*)(uintptr_t)(L.st_out + (uint64_t)s * kState);
        const uint64_t add[4] = {L.n, cand, total, fixd};
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint64_t v = (si[2u * i] | (uint64_t)si[2u * i + 1u] << 32) + add[i];
            so[2u * i] = (uint32_t)v; so[2u * i + 1u] = (uint32_t)(v >> 32);
        }
        ((FMD_DDC_GLOBAL uint32_t*)(uintptr_t)L.cnt_out)[s] = (uint32_t)total;
    }
}

}  // namespace fmd_ms

static_assert(sizeof(fmd_modes_msg) == 32 && offsetof(fmd_modes_msg, n_bytes) == 8 && offsetof(fmd_modes_msg, bytes) == 12,
              "the kernel writes fmd_modes_msg as eight dwords");

struct fmd_modes {
    FmdRows rows;                                         // width 1; its history pair is the carried m: hcap = 240 u16 per stream
    FmdDdcPair state;                                     // [n_streams][kState] uint32
    FmdRowRecords recs;                                   // fmd_modes_msg, msg_cap per stream
    void* d_table = nullptr;                              // T_112
    void* d_scratch = nullptr; size_t scratch_cap = 0;    // the tiles' counts and kept positions of a call
    fmd_modes_config cfg{};
};

namespace {

int ms_enqueue(fmd_modes* h, const void* d_iq, size_t nbytes, size_t cap_bytes, hipStream_t stream)
{
    using namespace fmd_ms;
    FmdRows& r = h->rows;
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    if (nbytes > cap_bytes) { fmd_internal_set_err("nbytes > cap_bytes"); return FMD_ERR_CAPACITY; }
    if (((uintptr_t)d_iq & 3u) != 0 || cap_bytes % 4 != 0) { fmd_internal_set_err("misaligned device buffer"); return FMD_ERR_INVALID_ARG; }
    if (nbytes > (1ull << 31)) { fmd_internal_set_err("nbytes out of range"); return FMD_ERR_UNSUPPORTED; }
    if (nbytes == 0) return FMD_OK;                          // nothing to take: no launch, the last call's results stay
    const uint64_t n = nbytes / 2, n_tiles = (n + kTile - 1) / kTile;
    if (n_tiles * r.n_rows >= (1ull << 31)) { fmd_internal_set_err("call too large: more than 2^31 tiles"); return FMD_ERR_UNSUPPORTED; }
    const size_t stats_bytes = (size_t)r.n_rows * n_tiles * kStats * sizeof(uint32_t);
    FMD_DDC_TRY(r.core.order.before(stream));
    // (a scratch that grows is freed behind the calls that used it: hipFree synchronises the device)
    FMD_DDC_TRY(fmd_ddc_grow(h->d_scratch, h->scratch_cap, stats_bytes + (size_t)r.n_rows * n_tiles * h->cfg.msg_cap * sizeof(uint16_t)));
    ModesLaunch L{};
    L.iq = static_cast<const uint8_t*>(d_iq); L.cap_bytes = cap_bytes;
    L.n = (uint32_t)n; L.n_streams = r.n_rows; L.n_tiles = (uint32_t)n_tiles;
    L.skip = r.core.pos < 239 ? (uint32_t)(239 - r.core.pos) : 0u;
    L.aligned = ((uintptr_t)d_iq & 15u) == 0 && cap_bytes % 16 == 0 ? 1u : 0u;
    L.min_power = h->cfg.min_power; L.fix_errors = h->cfg.fix_errors; L.df11 = h->cfg.df11; L.msg_cap = h->cfg.msg_cap;
    L.tail_in = r.hist.in<uint16_t>(r.core.cur); L.tail_out = r.hist.out<uint16_t>(r.core.cur);
    L.table = static_cast<const uint32_t*>(h->d_table);
    L.stats = static_cast<uint32_t*>(h->d_scratch);
    L.kept = reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(h->d_scratch) + stats_bytes);
    L.st_in = h->state.in<uint32_t>(r.core.cur); L.st_out = h->state.out<uint32_t>(r.core.cur);
    L.cnt_out = h->recs.cnt_out(r.core.cur); L.rec_out = h->recs.rec_out(r.core.cur);
    hipLaunchKernelGGL(fmd_modes_tile_kernel, dim3((uint32_t)(n_tiles * r.n_rows)), dim3(kThreads), 0, stream, L);
    FMD_DDC_TRY(hipGetLastError());
    hipLaunchKernelGGL(fmd_modes_gather_kernel, dim3(r.n_rows), dim3(64), 0, stream, L);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(r.core, stream, n);
    return FMD_OK;
}

}  // namespace

extern "C" {

uint32_t fmd_modes_tile(void) { return fmd_ms::kTile; }

int fmd_modes_new(const fmd_modes_config* cfg, const fmd_device_config* dev, fmd_modes** out)
{
    if (const int rc = fmd_rows_new_args(cfg, dev, out, 1)) return rc;       // (the pointers)
    if (dev->n_channels == 0) { fmd_internal_set_err("need n_streams >= 1"); return FMD_ERR_INVALID_ARG; }
    if (cfg->min_power > 262144u) { fmd_internal_set_err("need min_power <= 262144"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->fix_errors > 1u || cfg->df11 > 1u) { fmd_internal_set_err("need fix_errors and df11 0 or 1"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->msg_cap < 1u || cfg->msg_cap > 256u) { fmd_internal_set_err("need 1 <= msg_cap <= 256"); return FMD_ERR_UNSUPPORTED; }
    fmd_modes* h = new (std::nothrow) fmd_modes();
    if (!h) return FMD_ERR_NOMEM;
    h->cfg = *cfg;
    h->rows.width = 1; h->rows.n_rows = dev->n_channels; h->rows.hcap = fmd_ms::kTail;
    uint32_t table[112];
    (void)fmd_modes_table(112, table);
    fmd_ddc_add_pair(h->rows.core, h->state, (size_t)dev->n_channels * fmd_ms::kState * sizeof(uint32_t));
    fmd_rows_add_records(h->rows, h->recs, cfg->msg_cap, sizeof(fmd_modes_msg));
    fmd_ddc_add_owned(h->rows.core, h->d_table, table, sizeof table);
    fmd_ddc_add_owned(h->rows.core, h->d_scratch);
    return fmd_rows_device(h, dev, fmd_modes_free, out);
}

void fmd_modes_free(fmd_modes* h) { fmd_rows_free(h); }
int fmd_modes_reset(fmd_modes* h) { return fmd_rows_reset(h); }
int fmd_modes_check(fmd_modes* h) { return fmd_rows_check(h); }
int fmd_modes_counts(fmd_modes* h, uint32_t* counts) { return fmd_rows_counts(h, counts); }
int fmd_modes_msgs(fmd_modes* h, const uint32_t* streams, size_t n_sel, fmd_modes_msg* msgs) { return fmd_rows_records(h, streams, n_sel, msgs); }

int fmd_modes_info(fmd_modes* h, fmd_modes_totals* info)
{
    if (!h || !info) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    std::vector<uint64_t> st;
    if (const int rc = fmd_rows_read_state(h->rows, h->state, fmd_ms::kState / 2, st)) return rc;
    for (size_t s = 0; s < h->rows.n_rows; ++s)
        info[s] = fmd_modes_totals{st[4 * s], st[4 * s + 1], st[4 * s + 2], st[4 * s + 3]};
    return FMD_OK;
}

int fmd_modes_run_device(fmd_modes* h, const void* d_iq, size_t nbytes, size_t cap_bytes, void* stream)
{
    return fmd_ddc_run_device(h ? &h->rows.core : nullptr, d_iq, d_iq,
                              [&] { return ms_enqueue(h, d_iq, nbytes, cap_bytes, static_cast<hipStream_t>(stream)); });
}

int fmd_modes_run_batch(fmd_modes* h, const uint8_t* iq, size_t nbytes, size_t cap_bytes)
{
    if (!h || !iq) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    if (nbytes > cap_bytes) { fmd_internal_set_err("nbytes > cap_bytes"); return FMD_ERR_CAPACITY; }
    if (cap_bytes % 4 != 0) { fmd_internal_set_err("cap_bytes % 4 != 0"); return FMD_ERR_INVALID_ARG; }
    if (nbytes == 0) return FMD_OK;
    FmdDdcCore& c = h->rows.core;
    FMD_DDC_ON_DEVICE(c.device);
    const size_t in_bytes = (size_t)h->rows.n_rows * cap_bytes;
    FMD_DDC_TRY(fmd_ddc_grow(c.d_iq, c.d_iq_cap, in_bytes));
    FMD_DDC_TRY(hipMemcpyAsync(c.d_iq, iq, in_bytes, hipMemcpyHostToDevice, c.stream));
    const int rc = ms_enqueue(h, c.d_iq, nbytes, cap_bytes, c.stream);
    const hipError_t e = hipStreamSynchronize(c.stream);
    if (rc) return rc;                                       // (the enqueue's status wins over the synchronise's)
    FMD_DDC_TRY(e);
    return FMD_OK;
}

int fmd_modes_kernel_name(const fmd_modes* h, uint32_t pass, char* name, size_t cap)
{
    if (!h || !name || cap == 0 || pass > 1) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, "%s", pass ? "fmd_ms::fmd_modes_gather_kernel" : "fmd_ms::fmd_modes_tile_kernel"), cap);
}

}  // extern "C"
