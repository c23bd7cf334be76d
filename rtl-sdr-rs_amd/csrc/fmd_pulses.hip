// fmd_pulses.hip -- the pulse bank: the on-off-keyed pulses of many u8 IQ streams, as width / gap / level records per stream.
//
// Definition: include/fmd.h, "Pulse bank"; tests/pulses_ref.py.  Per stream the call's n samples stand behind the m of the 64 samples
// carried from the calls before: v[j], j < 64 + n, with v[64 + c] the call's sample c (64 = the largest box; the carried samples, the
// call's samples and the 16-byte pieces of the staging lie on one 8-sample grid, as in fmd_modes.hip).  Position u < n of the call is
// the absolute sample pos + u; its box is e = v[64 + u - W + 1] + ... + v[64 + u].
//
// Pass 0, one workgroup of four waves per (stream, tile of kTile positions).  The tile does not know the state s it is entered with:
//   prefix    16 bytes of IQ -> eight m in registers; a shuffle scan of the pieces' sums and twelve wave totals give every piece its
//             base, and the lanes leave Q[x] = v[u0] + ... + v[u0 + x - 1] in LDS (no plane of m is kept: m is a difference of Q).
//             (kTile + 64) * 65025 < 2^32.  Position w of the tile has e = Q[65 + w] - Q[65 + w - W]: two reads, whatever W is;
//   classify  a lane takes eight consecutive positions: set (e >= hi), clear (e < lo) or keep, as two bytes.  Two ballots -- "has a
//             definite position" and "its last definite value" -- give every lane the state it is entered with: the nearest set bit
//             below it; the same over the eight wave chunks through LDS.  A lane that nothing definite precedes in the tile is
//             "unknown" and marks no edge until its first definite position;
//   queue     the known edges -- a definite position whose value differs from the known state in front of it -- go into an LDS queue
//             in increasing position by a scan of popcounts.  Edges alternate, so the queue needs no polarity: its first entry is a
//             rise iff the tile's first definite value is 0, fall j stands at index 2 j + (that), and its rise is the entry before it;
//   keep      the tile's first min(falls, pulse_cap) falls as (position, position of the rise or 0xFFFF, level), and a summary of four
//             dwords: first definite position and its value, the level in front of it, the number of known edges, the last two edges.
// Pass 1, one wave per stream: reads the summaries 64 at a time and walks the tiles in order with the stream's state in scalars.  A
// tile owes one more edge at its first definite position when the state it is entered with differs from that value; widths and gaps
// that cross tiles or calls are sums over the carried run.  It writes the stream's first pulse_cap records (a lane per record),
// sums the counters, and leaves s, the run, the open pulse's gap and the last 64 samples.  Nothing depends on scheduling: there is
// no atomic anywhere, and which records survive an overflow is fixed by position alone.
// Scratch per call: 16 bytes + 8 pulse_cap bytes per tile -- bounded by pulse_cap, not by the tile: with lo == hi noise puts an edge on
// most samples.  At 4096 streams x 32 tiles (262144 bytes each) and pulse_cap 64 that is 66 MiB.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_rows.h"

namespace fmd_pl {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kTile = 4096;                          // positions per workgroup: two rounds of 256 lanes x 8
constexpr uint32_t kTail = 64;                            // samples carried per stream (as m, u16): the largest box
constexpr uint32_t kPieces = kTile / 8 + kTail / 8;       // 16-byte pieces of a tile's samples, the halo in front included
constexpr uint32_t kRounds = kTile / (8 * kThreads);      // rounds of the classification
constexpr uint32_t kPRounds = (kPieces + kThreads - 1) / kThreads;     // rounds of the prefix
constexpr uint32_t kChunks = kRounds * kWaves;            // wave chunks of 512 positions, in position order
constexpr uint32_t kNone = 0xFFFFu;                       // no position
constexpr uint32_t kSum = 4;                              // dwords of a tile's summary
constexpr uint32_t kState = 12;                           // dwords per stream: samples, pulses, rises, run (u64 each), s, gap, 0, 0
constexpr uint64_t kSat = 0xFFFFFFFFull;
static_assert(kTile < kNone && kTile % (8 * kThreads) == 0 && kTail % 8 == 0, "tile geometry");
static_assert((uint64_t)(kTile + kTail) * 65025ull < (1ull << 32), "the prefix of a tile fits a dword");

typedef int i4 __attribute__((ext_vector_type(4)));
typedef int i2 __attribute__((ext_vector_type(2)));

struct PulsesLaunch {
    const uint8_t* iq;         // [n_streams][cap_bytes]
    uint64_t cap_bytes;
    uint32_t n;                // samples per stream in this call, >= 1
    uint32_t n_streams, n_tiles;
    uint32_t aligned;          // every stream's bytes start 16-byte aligned
    uint32_t W, lo, hi, pulse_cap;
    const uint16_t* tail_in;   // [n_streams][kTail]
    uint16_t* tail_out;
    uint32_t* sums;            // [n_streams][n_tiles][kSum]
    uint32_t* kept;            // [n_streams][n_tiles][pulse_cap][2]: position | rise << 16, level
    const uint32_t* st_in;     // [n_streams][kState]
    uint32_t* st_out;
    uint32_t* cnt_out;         // [n_streams]
    uint8_t* rec_out;          // [n_streams][pulse_cap] fmd_pulses_rec
};

// m of the samples in one dword of IQ (I0 Q0 I1 Q1), packed low | high << 16
__device__ __forceinline__ uint32_t mag2(uint32_t d)
{
    const int i0 = 2 * (int)(d & 255u) - 255, q0 = 2 * (int)((d >> 8) & 255u) - 255;
    const int i1 = 2 * (int)((d >> 16) & 255u) - 255, q1 = 2 * (int)(d >> 24) - 255;
    return (uint32_t)(i0 * i0 + q0 * q0) >> 1 | ((uint32_t)(i1 * i1 + q1 * q1) >> 1) << 16;
}

__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane)    // inclusive
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, o);
        if (lane >= (uint32_t)o) v += t;
    }
    return v;
}

__global__ void __launch_bounds__(kThreads) fmd_pulses_tile_kernel(const PulsesLaunch L)
{
    __shared__ __attribute__((aligned(16))) uint32_t Q[kTile + kTail + 8u];   // Q[x]: the sum of the x samples from v[u0] on
    __shared__ uint16_t queue[kTile];                                          // the known edges, in increasing position
    __shared__ uint32_t psum[kPRounds][kWaves];                                // the prefix's wave totals
    __shared__ uint32_t wsum[kRounds][kWaves];                                 // the queue's wave totals
    __shared__ uint32_t c_def[kChunks], c_val[kChunks], c_first[kChunks];      // per wave chunk: any definite, the last one's value,
                                                                               // the first one's position | value << 16 (kNone)
    typedef const FMD_DDC_GLOBAL uint32_t* gw;
    typedef const FMD_DDC_GLOBAL i4* gq;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t s = blockIdx.x / L.n_tiles, tile = blockIdx.x - s * L.n_tiles;
    const uint32_t u0 = tile * kTile;                        // the tile's first position; Q starts at v[u0]
    const uint8_t* const row = L.iq + (uint64_t)s * L.cap_bytes;

    // ---- the prefix ---------------------------------------------------------------------------------------------------------------
    uint32_t mp[kPRounds][4], pexcl[kPRounds];
#pragma unroll
    for (uint32_t r = 0; r < kPRounds; ++r) {
        const uint32_t k = r * kThreads + tid, j0 = u0 + 8u * k;      // v index of the piece's first sample
        i4 piece = i4{0, 0, 0, 0};
        if (k < kPieces) {
            if (j0 < kTail) {
                piece = *(gq)(uintptr_t)(L.tail_in + (uint64_t)s * kTail + j0);
            } else {
                const uint32_t c0 = j0 - kTail;              // the call's sample, a multiple of 8
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
        }
        mp[r][0] = (uint32_t)piece.x; mp[r][1] = (uint32_t)piece.y; mp[r][2] = (uint32_t)piece.z; mp[r][3] = (uint32_t)piece.w;
        uint32_t sum = 0u;
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) sum += (mp[r][e] & 0xFFFFu) + (mp[r][e] >> 16);
        const uint32_t inc = wave_scan(sum, lane);
        pexcl[r] = inc - sum;
        if (lane == 63u) psum[r][wave] = inc;
    }
    if (tid == 0u) Q[0] = 0u;
    __syncthreads();
    {
        uint32_t before = 0u;                                // the pieces of the rounds and waves in front
#pragma unroll
        for (uint32_t r = 0; r < kPRounds; ++r) {
            uint32_t run = before + pexcl[r];
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) {
                if (w < wave) run += psum[r][w];
                before += psum[r][w];
            }
            const uint32_t k = r * kThreads + tid;
            if (k < kPieces) {
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) {
                    run += mp[r][e] & 0xFFFFu; Q[8u * k + 2u * e + 1u] = run;
                    run += mp[r][e] >> 16;     Q[8u * k + 2u * e + 2u] = run;
                }
            }
        }
    }
    __syncthreads();

    // ---- classification: position w of the tile has e = Q[65 + w] - Q[65 + w - W] -------------------------------------------------------
    uint32_t def8[kRounds], val8[kRounds], st_in[kRounds], known_in[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t g = r * kThreads + tid, w0 = 8u * g;
        const uint32_t* const qa = &Q[kTail + 1u + w0];
        const uint32_t* const qb = qa - L.W;
        uint32_t d8 = 0u, v8 = 0u;
#pragma unroll
        for (uint32_t e = 0; e < 8u; ++e) {
            const uint32_t ev = qa[e] - qb[e];
            const bool valid = u0 + w0 + e < L.n, set = ev >= L.hi, clear = ev < L.lo;
            d8 |= valid && (set || clear) ? 1u << e : 0u;
            v8 |= valid && set ? 1u << e : 0u;
        }
        def8[r] = d8; val8[r] = v8;
        const bool has = d8 != 0u;
        const bool last = has && ((v8 >> (31u - (uint32_t)__builtin_clz(d8 | 1u))) & 1u) != 0u;
        const uint64_t D = __ballot(has), V = __ballot(last);
        const uint64_t below = D & ((1ull << lane) - 1ull);
        known_in[r] = below != 0ull ? 1u : 0u;
        st_in[r] = below != 0ull ? (uint32_t)(V >> (63u - (uint32_t)__builtin_clzll(below))) & 1u : 0u;
        const uint32_t c = r * kWaves + wave;
        if (D == 0ull) {
            if (lane == 0u) { c_def[c] = 0u; c_val[c] = 0u; c_first[c] = kNone; }
        } else {
            if (lane == 0u) { c_def[c] = 1u; c_val[c] = (uint32_t)(V >> (63u - (uint32_t)__builtin_clzll(D))) & 1u; }
            if (lane == (uint32_t)__builtin_ctzll(D)) {
                const uint32_t e0 = (uint32_t)__builtin_ctz(d8);
                c_first[c] = (w0 + e0) | ((v8 >> e0) & 1u) << 16;
            }
        }
    }
    __syncthreads();

    // ---- the known edges, and their places in the queue -----------------------------------------------------------------------------
    uint32_t edge8[kRounds], excl[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t c = r * kWaves + wave;
        uint32_t ck = 0u, cs = 0u;                           // the state the chunk is entered with, if a chunk in front knows it
        for (uint32_t cc = 0; cc < c; ++cc)
            if (c_def[cc]) { ck = 1u; cs = c_val[cc]; }
        uint32_t known = known_in[r] ? 1u : ck, st = known_in[r] ? st_in[r] : cs;
        uint32_t m = 0u;
#pragma unroll
        for (uint32_t e = 0; e < 8u; ++e) {
            if (def8[r] >> e & 1u) {
                const uint32_t v = val8[r] >> e & 1u;
                if (known && v != st) m |= 1u << e;
                st = v; known = 1u;
            }
        }
        edge8[r] = m;
        const uint32_t inc = wave_scan((uint32_t)__builtin_popcount(m), lane);
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
            if (edge8[r] >> e & 1u) queue[at++] = (uint16_t)(8u * g + e);
    }
    __syncthreads();

    // ---- the tile's first pulse_cap falls and its summary -------------------------------------------------------------------------------
    uint32_t first = kNone;                                  // the tile's first definite position | value << 16
    for (uint32_t c = 0; c < kChunks; ++c)
        if (first == kNone) first = c_first[c];
    const uint32_t vd = first >> 16 & 1u;
    const uint32_t n_falls = vd ? (qn + 1u) / 2u : qn / 2u, lead = vd ? 0u : 1u;
    const uint64_t t_at = (uint64_t)s * L.n_tiles + tile;
    FMD_DDC_GLOBAL i2* const kept = (FMD_DDC_GLOBAL i2*)(uintptr_t)(L.kept + t_at * L.pulse_cap * 2u);
    const uint32_t n_keep = n_falls < L.pulse_cap ? n_falls : L.pulse_cap;
    for (uint32_t j = tid; j < n_keep; j += kThreads) {
        const uint32_t idx = 2u * j + lead, f = queue[idx], rise = idx ? (uint32_t)queue[idx - 1u] : kNone;
        kept[j] = i2{(int)(f | rise << 16), (int)(Q[kTail + f] - Q[kTail + f - L.W])};
    }
    if (tid == 0u) {
        const uint32_t fd = first & 0xFFFFu;
        const uint32_t level = first == kNone ? 0u : Q[kTail + fd] - Q[kTail + fd - L.W];
        const uint32_t last2 = (qn >= 1u ? (uint32_t)queue[qn - 1u] : kNone) | (qn >= 2u ? (uint32_t)queue[qn - 2u] : kNone) << 16;
        *(FMD_DDC_GLOBAL i4*)(uintptr_t)(L.sums + t_at * kSum) = i4{(int)first, (int)level, (int)qn, (int)last2};
    }
}

// v[j] of stream s, from global memory: the carried samples, then the call's
__device__ __forceinline__ uint32_t sample_at(const PulsesLaunch& L, uint32_t s, uint32_t j)
{
    if (j < kTail) return ((const FMD_DDC_GLOBAL uint16_t*)(uintptr_t)(L.tail_in + (uint64_t)s * kTail))[j];
    const FMD_DDC_GLOBAL uint8_t* const b = (const FMD_DDC_GLOBAL uint8_t*)(uintptr_t)(L.iq + (uint64_t)s * L.cap_bytes + 2ull * (j - kTail));
    const int i = 2 * (int)b[0] - 255, q = 2 * (int)b[1] - 255;
    return (uint32_t)(i * i + q * q) >> 1;
}

__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t from)
{
    return (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)v, (int)from));
}

__device__ __forceinline__ uint32_t sat32(uint64_t v) { return v > kSat ? (uint32_t)kSat : (uint32_t)v; }

__global__ void __launch_bounds__(64) fmd_pulses_gather_kernel(const PulsesLaunch L)
{
    typedef const FMD_DDC_GLOBAL uint32_t* gw;
    typedef const FMD_DDC_GLOBAL i4* gq;
    typedef const FMD_DDC_GLOBAL i2* gk;
    const uint32_t lane = threadIdx.x, s = blockIdx.x;
    const gw si = (gw)(uintptr_t)(L.st_in + (uint64_t)s * kState);
    const gq sums = (gq)(uintptr_t)(L.sums + (uint64_t)s * L.n_tiles * kSum);
    // the stream's state, wave-uniform: s, the samples since the last edge, the open pulse's gap, whether a fall has been seen
    uint32_t st = si[8] & 1u, gap_open = si[9];
    uint64_t run = si[6] | (uint64_t)si[7] << 32;
    bool have_fall = (si[2] | si[3]) != 0u;
    uint32_t count = 0u, rises = 0u;                         // of this call
    FMD_DDC_GLOBAL i4* const recs = (FMD_DDC_GLOBAL i4*)(uintptr_t)(L.rec_out + (uint64_t)s * L.pulse_cap * sizeof(fmd_pulses_rec));

    for (uint32_t tb = 0; tb < L.n_tiles; tb += 64u) {
        i4 mine = i4{(int)kNone, 0, 0, 0};
        if (tb + lane < L.n_tiles) mine = sums[tb + lane];
        const uint32_t here = L.n_tiles - tb < 64u ? L.n_tiles - tb : 64u;
        for (uint32_t tj = 0; tj < here; ++tj) {
            const uint32_t first = bcast((uint32_t)mine.x, tj);
            const uint32_t tile0 = (tb + tj) * kTile, len = L.n - tile0 < kTile ? L.n - tile0 : kTile;
            if (first == kNone) { run += len; continue; }    // nothing definite: the tile keeps what it is entered with
            const uint32_t level = bcast((uint32_t)mine.y, tj), qn = bcast((uint32_t)mine.z, tj), last2 = bcast((uint32_t)mine.w, tj);
            const uint32_t fd = first & 0xFFFFu, vd = first >> 16 & 1u;
            const uint32_t n_falls = vd ? (qn + 1u) / 2u : qn / 2u;
            const bool owed = st != vd, had_fall = have_fall;
            const uint64_t run_in = run;
            if (owed && vd) {                                // a rise at fd
                gap_open = have_fall ? sat32(run_in + fd) : 0u;
                ++rises;
            } else if (owed) {                               // a fall at fd
                if (lane == 0u && count < L.pulse_cap)
                    recs[count] = i4{(int)(tile0 + fd), (int)sat32(run_in + fd), (int)gap_open, (int)level};
                ++count;
                have_fall = true;
            }
            // the known falls: entry j has its rise in the tile unless it is the tile's first known edge
            const uint32_t room = count < L.pulse_cap ? L.pulse_cap - count : 0u, n_write = n_falls < room ? n_falls : room;
            const gk kept = (gk)(uintptr_t)(L.kept + ((uint64_t)s * L.n_tiles + tb + tj) * L.pulse_cap * 2u);
            for (uint32_t jb = 0; jb < n_write; jb += 64u) {
                const uint32_t j = jb + lane;
                if (j < n_write) {
                    const i2 k = kept[j];
                    const uint32_t f = (uint32_t)k.x & 0xFFFFu, rise = (uint32_t)k.x >> 16;
                    uint32_t width, gap;
                    if (j) {
                        width = f - rise; gap = rise - ((uint32_t)kept[j - 1u].x & 0xFFFFu);
                    } else if (rise != kNone) {              // the tile's first known edge is this fall's rise
                        width = f - rise; gap = owed ? rise - fd : had_fall ? sat32(run_in + rise) : 0u;
                    } else {                                 // the pulse began at fd or in front of the tile
                        width = owed ? f - fd : sat32(run_in + f); gap = gap_open;
                    }
                    recs[count + j] = i4{(int)(tile0 + f), (int)width, (int)gap, (int)k.y};
                }
            }
            count += n_falls; rises += qn - n_falls;
            if (n_falls) have_fall = true;
            if (qn) {
                const uint32_t e_last = last2 & 0xFFFFu, e_prev = last2 >> 16;
                st = (qn & 1u) ^ vd;
                run = len - e_last;
                if (st) gap_open = qn >= 2u ? e_last - e_prev : owed ? e_last - fd : had_fall ? sat32(run_in + e_last) : 0u;
            } else {
                st = vd;
                run = owed ? (uint64_t)(len - fd) : run_in + len;
            }
        }
    }

    // the last 64 samples, forward
    FMD_DDC_GLOBAL uint16_t* const tout = (FMD_DDC_GLOBAL uint16_t*)(uintptr_t)(L.tail_out + (uint64_t)s * kTail);
    tout[lane] = (uint16_t)sample_at(L, s, L.n + lane);

    if (lane == 0u) {
        FMD_DDC_GLOBAL uint32_t* const so = (FMD_DDC_GLOBAL uint32_t*)(uintptr_t)(L.st_out + (uint64_t)s * kState);
        const uint64_t add[3] = {L.n, count, rises};
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            const uint64_t v = (si[2u * i] | (uint64_t)si[2u * i + 1u] << 32) + add[i];
            so[2u * i] = (uint32_t)v; so[2u * i + 1u] = (uint32_t)(v >> 32);
        }
        so[6] = (uint32_t)run; so[7] = (uint32_t)(run >> 32);
        so[8] = st; so[9] = gap_open; so[10] = 0u; so[11] = 0u;
        ((FMD_DDC_GLOBAL uint32_t*)(uintptr_t)L.cnt_out)[s] = count;
    }
}

}  // namespace fmd_pl

static_assert(sizeof(fmd_pulses_rec) == 16 && offsetof(fmd_pulses_rec, width) == 4 && offsetof(fmd_pulses_rec, level) == 12,
              "the kernel writes fmd_pulses_rec as four dwords");

struct fmd_pulses {
    FmdRows rows;                                         // width 1; its history pair is the carried m: hcap = 64 u16 per stream
    FmdDdcPair state;                                     // [n_streams][kState] uint32
    FmdRowRecords recs;                                   // fmd_pulses_rec, pulse_cap per stream
    void* d_scratch = nullptr; size_t scratch_cap = 0;    // the tiles' summaries and kept falls of a call
    fmd_pulses_config cfg{};
    uint32_t last_n = 0;                                  // samples per stream of the last call that launched
};

namespace {

int pl_enqueue(fmd_pulses* h, const void* d_iq, size_t nbytes, size_t cap_bytes, hipStream_t stream)
{
    using namespace fmd_pl;
    FmdRows& r = h->rows;
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    if (nbytes > cap_bytes) { fmd_internal_set_err("nbytes > cap_bytes"); return FMD_ERR_CAPACITY; }
    if (((uintptr_t)d_iq & 3u) != 0 || cap_bytes % 4 != 0) { fmd_internal_set_err("misaligned device buffer"); return FMD_ERR_INVALID_ARG; }
    if (nbytes > (1ull << 31)) { fmd_internal_set_err("nbytes out of range"); return FMD_ERR_UNSUPPORTED; }
    if (nbytes == 0) return FMD_OK;                          // nothing to take: no launch, the last call's results stay
    const uint64_t n = nbytes / 2, n_tiles = (n + kTile - 1) / kTile;
    if (n_tiles * r.n_rows >= (1ull << 31)) { fmd_internal_set_err("call too large: more than 2^31 tiles"); return FMD_ERR_UNSUPPORTED; }
    const size_t sums_bytes = (size_t)r.n_rows * n_tiles * kSum * sizeof(uint32_t);
    FMD_DDC_TRY(r.core.order.before(stream));
    // (a scratch that grows is freed behind the calls that used it: hipFree synchronises the device)
    FMD_DDC_TRY(fmd_ddc_grow(h->d_scratch, h->scratch_cap, sums_bytes + (size_t)r.n_rows * n_tiles * h->cfg.pulse_cap * 2 * sizeof(uint32_t)));
    PulsesLaunch L{};
    L.iq = static_cast<const uint8_t*>(d_iq); L.cap_bytes = cap_bytes;
    L.n = (uint32_t)n; L.n_streams = r.n_rows; L.n_tiles = (uint32_t)n_tiles;
    L.aligned = ((uintptr_t)d_iq & 15u) == 0 && cap_bytes % 16 == 0 ? 1u : 0u;
    L.W = h->cfg.W; L.lo = h->cfg.lo; L.hi = h->cfg.hi; L.pulse_cap = h->cfg.pulse_cap;
    L.tail_in = r.hist.in<uint16_t>(r.core.cur); L.tail_out = r.hist.out<uint16_t>(r.core.cur);
    L.sums = static_cast<uint32_t*>(h->d_scratch);
    L.kept = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(h->d_scratch) + sums_bytes);
    L.st_in = h->state.in<uint32_t>(r.core.cur); L.st_out = h->state.out<uint32_t>(r.core.cur);
    L.cnt_out = h->recs.cnt_out(r.core.cur); L.rec_out = h->recs.rec_out(r.core.cur);
    hipLaunchKernelGGL(fmd_pulses_tile_kernel, dim3((uint32_t)(n_tiles * r.n_rows)), dim3(kThreads), 0, stream, L);
    FMD_DDC_TRY(hipGetLastError());
    hipLaunchKernelGGL(fmd_pulses_gather_kernel, dim3(r.n_rows), dim3(64), 0, stream, L);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(r.core, stream, n);
    h->last_n = (uint32_t)n;
    return FMD_OK;
}

}  // namespace

// (fmd_rows.h: what fmd_packages_run_bank reads; every call that launches takes samples, so pos == 0 is "none since reset")
void fmd_pulses_last(fmd_pulses* h, FmdPulsesLast* out)
{
    const FmdDdcCore& c = h->rows.core;
    out->device = c.device; out->n_streams = h->rows.n_rows; out->pulse_cap = h->cfg.pulse_cap;
    out->launched = c.pos != 0; out->n_samples = h->last_n;
    out->d_counts = reinterpret_cast<const uint32_t*>(h->recs.counts(c.cur)); out->d_recs = h->recs.records(c.cur);
    out->d_state = h->state.in<uint32_t>(c.cur); out->state_dwords = fmd_pl::kState;
    out->order = &h->rows.core.order;
}

extern "C" {

uint32_t fmd_pulses_tile(void) { return fmd_pl::kTile; }

int fmd_pulses_new(const fmd_pulses_config* cfg, const fmd_device_config* dev, fmd_pulses** out)
{
    if (const int rc = fmd_rows_new_args(cfg, dev, out, 1)) return rc;       // (the pointers)
    if (cfg->W < 1u || cfg->W > 64u) { fmd_internal_set_err("need 1 <= W <= 64"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->lo < 1u || cfg->lo > cfg->hi || cfg->hi > 64u * 65025u) { fmd_internal_set_err("need 1 <= lo <= hi <= 64 * 65025"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->pulse_cap < 1u || cfg->pulse_cap > 1024u) { fmd_internal_set_err("need 1 <= pulse_cap <= 1024"); return FMD_ERR_UNSUPPORTED; }
    if (dev->n_channels < 1u) { fmd_internal_set_err("need n_streams >= 1"); return FMD_ERR_UNSUPPORTED; }
    fmd_pulses* h = new (std::nothrow) fmd_pulses();
    if (!h) return FMD_ERR_NOMEM;
    h->cfg = *cfg;
    h->rows.width = 1; h->rows.n_rows = dev->n_channels; h->rows.hcap = fmd_pl::kTail;
    fmd_ddc_add_pair(h->rows.core, h->state, (size_t)dev->n_channels * fmd_pl::kState * sizeof(uint32_t));
    fmd_rows_add_records(h->rows, h->recs, cfg->pulse_cap, sizeof(fmd_pulses_rec));
    fmd_ddc_add_owned(h->rows.core, h->d_scratch);
    return fmd_rows_device(h, dev, fmd_pulses_free, out);
}

void fmd_pulses_free(fmd_pulses* h) { fmd_rows_free(h); }
int fmd_pulses_reset(fmd_pulses* h) { return fmd_rows_reset(h); }
int fmd_pulses_check(fmd_pulses* h) { return fmd_rows_check(h); }
int fmd_pulses_counts(fmd_pulses* h, uint32_t* counts) { return fmd_rows_counts(h, counts); }
int fmd_pulses_recs(fmd_pulses* h, const uint32_t* streams, size_t n_sel, fmd_pulses_rec* recs) { return fmd_rows_records(h, streams, n_sel, recs); }

int fmd_pulses_info(fmd_pulses* h, fmd_pulses_totals* info)
{
    if (!h || !info) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    std::vector<uint32_t> st;
    if (const int rc = fmd_rows_read_state(h->rows, h->state, fmd_pl::kState, st)) return rc;
    for (size_t s = 0; s < h->rows.n_rows; ++s) {
        const uint32_t* const p = &st[s * fmd_pl::kState];
        const auto u64 = [p](int i) { return p[2 * i] | (uint64_t)p[2 * i + 1] << 32; };
        info[s] = fmd_pulses_totals{u64(0), u64(1), u64(2), p[8], 0u, u64(3)};
    }
    return FMD_OK;
}

int fmd_pulses_run_device(fmd_pulses* h, const void* d_iq, size_t nbytes, size_t cap_bytes, void* stream)
{
    return fmd_ddc_run_device(h ? &h->rows.core : nullptr, d_iq, d_iq,
                              [&] { return pl_enqueue(h, d_iq, nbytes, cap_bytes, static_cast<hipStream_t>(stream)); });
}

int fmd_pulses_run_batch(fmd_pulses* h, const uint8_t* iq, size_t nbytes, size_t cap_bytes)
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
    const int rc = pl_enqueue(h, c.d_iq, nbytes, cap_bytes, c.stream);
    const hipError_t e = hipStreamSynchronize(c.stream);
    if (rc) return rc;                                       // (the enqueue's status wins over the synchronise's)
    FMD_DDC_TRY(e);
    return FMD_OK;
}

int fmd_pulses_kernel_name(const fmd_pulses* h, uint32_t pass, char* name, size_t cap)
{
    if (!h || !name || cap == 0 || pass > 1) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, "%s", pass ? "fmd_pl::fmd_pulses_gather_kernel" : "fmd_pl::fmd_pulses_tile_kernel"), cap);
}

}  // extern "C"
