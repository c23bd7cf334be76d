// fmd_fsk.hip -- direct-FSK front end of the pager decoder: every mono int16 row a bank leaves on the device goes through a box
// matched filter one bit long and comes out as soft decisions, a few per bit, and every soft decision is tested for a 32-bit sync
// word (POCSAG: 0x7CD215D8) that ends there, in ONE gfx950 kernel.  No clock recovery: every k forms its own word from 32 soft
// samples one bit apart, sliced at their mean.  What hits is reported per row as records (where, how many bits differ, polarity,
// correlation, slicer level); the host decoder (fmd_pocsag_decode.cpp) takes bit timing, level and polarity from them.
//
// Definition (include/fmd.h, "pager decoder"; tests/fsk_ref.py), per row:
//     b[k] = sum_{r<D} x[k D + r];   soft[k] = (sum_{t<W} b[k - t]) >> shift = out[k]
//     thr[k] = sum_{j<32} soft[k - tap[j]];   bit j of w[k] = 32 soft[k - tap[j]] > thr[k]
//     d = popcount(w ^ sync);   C = sum_j (bit j of sync ? +1 : -1) soft[k - tap[j]]
//     normal hit: d <= tol and C >= min_corr;   inverted hit: d >= 32 - tol and -C >= min_corr
// Per row the handle carries the open box's partial sum, the last W - 1 b and the last tap[31] soft.
//
// One workgroup = one tile of kRows = 4 rows for the whole call, ONE WAVE PER ROW.  All rows of a call share core.pos, hence every
// box end.  The call is walked in chunks of kChunk = 64 boxes (64 D samples per row), counted from the box the call starts in; the
// first and the last box of a call may be partial, and only the last can stay open.  Per chunk, three barriers:
//   1. the samples: 16-byte loads of the pieces of the row that lie whole inside the chunk, element loads at the unaligned head
//      and tail, into the row's staging buffer (dynamic LDS, 64 D int16 per row);
//   2. the boxes: lane q of the row's wave sums the samples of box q that the call brought, adds the carried partial sum to the
//      call's first box, and puts b[k] into the row's ring of 128 b -- or, where the call ends inside the box, keeps the sum;
//   3. soft[k]: W adds over the b ring, the shift, into the row's ring of 512 soft and, lane after lane, to consecutive addresses
//      of the output row;
//   4. the word and the match: 32 ring reads (the lanes of a wave read consecutive entries), the sum, 32 compares, one XOR,
//      v_bcnt_u32_b32, the signed sum, the two tests.  A ballot over the wave and the count of the lower lanes' hits give each hit
//      its slot behind the row's count so far, which the wave keeps in a register: the records come out in increasing k with no
//      atomic and no sort, because a wave owns its row and the chunks go in order.
// HBM traffic: the input once, 2 / D of it out, and per row and call 2 tap[31] + 4 W bytes each way for what is carried, plus the
// count and the records.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_rows.h"

namespace fmd_fk {

constexpr int kThreads = 256;
constexpr uint32_t kRows = 4;                             // rows per tile: a wave each
constexpr uint32_t kChunk = 64;                           // boxes per chunk: a lane each
constexpr uint32_t kBRing = 128;                          // b per row in LDS: 15 back and 64 new
constexpr uint32_t kBCarry = 16;                          // b per row in the handle's pair (index k mod 16), then the open box's sum
constexpr uint32_t kBState = 32;                          // int32 per row in that pair
constexpr uint32_t kSRing = 512;                          // soft per row in LDS: 255 back and 64 new
constexpr uint32_t kSCarry = 256;                         // soft per row in the handle's pair (index k mod 256)

typedef int i4 __attribute__((ext_vector_type(4)));

struct FskLaunch {
    const int16_t* in;         // [n_rows][in_cap]
    uint64_t in_cap;
    uint32_t n_in;             // valid samples per row
    uint32_t n_rows;
    const int16_t* hist_in;    // (the rows layer's history: unused)
    int16_t* hist_out;
    uint32_t hcap;
    const int32_t* b_in;       // [n_rows][kBState]: b[k] at k mod 16, the open box's sum at 16 (all-zero: nothing carried)
    int32_t* b_out;
    const int16_t* s_in;       // [n_rows][kSCarry]: soft[k] at k mod 256
    int16_t* s_out;
    uint32_t* cnt_out;         // [n_rows]: the call's hits
    i4* rec_out;               // [n_rows][hit_cap] records
    uint32_t pos_r;            // core.pos mod D: samples of the open box that earlier calls brought
    uint32_t k0;               // (core.pos / D) mod 2^16: the box the call starts in
    uint32_t n_out;            // boxes the call completes
    uint32_t D, W, shift, sync, tol, hit_cap;
    int32_t min_corr;
    uint8_t tap[32];
    int16_t* out;              // [n_rows][out_cap]
    uint64_t out_cap;
};

__global__ void __launch_bounds__(kThreads) fmd_fsk_kernel(const FskLaunch A)
{
    typedef const FMD_DDC_GLOBAL int16_t* gsrc;
    extern __shared__ __attribute__((aligned(16))) int16_t rawL[];   // [kRows][kChunk * D]
    __shared__ int32_t bL[kRows * kBRing];
    __shared__ int16_t softL[kRows * kSRing];
    __shared__ int32_t carryInL[kRows], carryOutL[kRows];
    __shared__ int32_t tapL[32], signL[32];                  // tap[j] and +-1 by bit j of sync (uniform values: from LDS by broadcast,
                                                             // where 64 SGPRs and their selects would spill)

    const uint32_t tid = threadIdx.x;
    const uint32_t row = tid >> 6, q = tid & 63u;            // the wave's row of the tile, the lane's box of the chunk
    const uint32_t row0 = blockIdx.x * kRows;
    if (row0 >= A.n_rows) return;
    const bool live = row0 + row < A.n_rows;
    const uint32_t D = A.D, W = A.W, tapmax = A.tap[31];
    const uint32_t span = kChunk * D;                        // samples per chunk and row
    const uint32_t o_end = A.pos_r + A.n_in;                 // the call's samples are [pos_r, o_end), counted from the start of box k0
    const uint32_t k0 = A.k0, k1 = k0 + A.n_out;
    const uint32_t nbox = (o_end + D - 1u) / D;              // boxes the call touches
    const uint64_t grow = (uint64_t)(row0 + row);

    // what the handle carries: soft[k0 - tap[31] ... k0), b[k0 - (W - 1) ... k0), the open box's sum
    for (uint32_t e = q; e < tapmax; e += 64u) {
        const uint32_t k = k0 - tapmax + e;
        softL[row * kSRing + (k & (kSRing - 1u))] = live ? A.s_in[grow * kSCarry + (k & (kSCarry - 1u))] : (int16_t)0;
    }
    if (q + 1u < W) {
        const uint32_t k = k0 - (W - 1u) + q;
        bL[row * kBRing + (k & (kBRing - 1u))] = live ? A.b_in[grow * kBState + (k & (kBCarry - 1u))] : 0;
    }
    if (tid < 32u) {
        tapL[tid] = A.tap[tid];
        signL[tid] = (A.sync >> tid) & 1u ? 1 : -1;
    }
    if (q == 0u) {
        carryInL[row] = live ? A.b_in[grow * kBState + kBCarry] : 0;
        carryOutL[row] = 0;
    }
    __syncthreads();

    const uintptr_t R = live ? (uintptr_t)(A.in + grow * A.in_cap) : 0;         // the row's samples of this call
    int16_t* const raw = rawL + row * span;
    uint32_t count = 0;                                      // the row's hits so far: the same in every lane of the wave
    for (uint32_t c = 0; c * kChunk < nbox; ++c) {           // block-uniform
        const uint32_t cs = c * span;
        const uint32_t oa = cs > A.pos_r ? cs : A.pos_r, ob = cs + span < o_end ? cs + span : o_end;    // the chunk's samples
        // ---- 1. the samples -----------------------------------------------------------------------------------------------------
        if (live) {
            const uintptr_t a0 = R + 2u * (uintptr_t)(oa - A.pos_r), a1 = R + 2u * (uintptr_t)(ob - A.pos_r);
            for (uintptr_t ca = ((a0 >> 4) + q) << 4; ca < a1; ca += 64u * 16u) {
                if (ca >= a0 && ca + 16u <= a1) {            // a piece whole inside the chunk
                    const i4 v = *(const FMD_DDC_GLOBAL i4*)ca;
                    const uint32_t e0 = A.pos_r + (uint32_t)((ca - R) >> 1) - cs;
                    const uint32_t d[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
#pragma unroll
                    for (uint32_t e = 0; e < 8u; ++e) raw[e0 + e] = (int16_t)(d[e >> 1] >> (16u * (e & 1u)));
                } else {                                     // the unaligned head or tail: exactly the samples of the chunk
                    for (uint32_t e = 0; e < 8u; ++e) {
                        const uintptr_t a = ca + 2u * e;
                        if (a < a0 || a >= a1) continue;
                        raw[A.pos_r + (uint32_t)((a - R) >> 1) - cs] = *(gsrc)a;
                    }
                }
            }
        }
        __syncthreads();

        // ---- 2. the boxes ---------------------------------------------------------------------------------------------------------
        const uint32_t Q = c * kChunk + q;                   // the lane's box, counted from k0
        {
            const uint32_t lo = Q * D, hi = lo + D;
            if (lo < o_end) {
                const uint32_t ea = lo > oa ? lo : oa, eb = hi < ob ? hi : ob;
                int s = Q == 0u ? carryInL[row] : 0;         // (only the call's first box began before the call)
                for (uint32_t e = ea; e < eb; ++e) s += raw[e - cs];
                if (hi <= o_end) bL[row * kBRing + ((k0 + Q) & (kBRing - 1u))] = s;
                else carryOutL[row] = s;                     // the call ends inside the box
            }
        }
        __syncthreads();

        // ---- 3. soft --------------------------------------------------------------------------------------------------------------
        const uint32_t k = k0 + Q;
        const bool has = Q < A.n_out;
        if (has) {
            int acc = 0;
            for (uint32_t t = 0; t < W; ++t) acc += bL[row * kBRing + ((k - t) & (kBRing - 1u))];
            const int16_t s = (int16_t)(acc >> A.shift);     // |acc| <= D W 2^15 <= 2^(shift + 15)
            softL[row * kSRing + (k & (kSRing - 1u))] = s;
            if (live) ((FMD_DDC_GLOBAL int16_t*)(uintptr_t)(A.out + grow * A.out_cap))[Q] = s;
        }
        __syncthreads();

        // ---- 4. the word and the match --------------------------------------------------------------------------------------------
        int thr = 0, corr = 0;
        uint32_t dist = 16u;
        if (has) {
            const int16_t* const sr = softL + row * kSRing;
            int v[32];
#pragma unroll
            for (uint32_t j = 0; j < 32u; ++j) {
                v[j] = sr[(k - (uint32_t)tapL[j]) & (kSRing - 1u)];
                thr += v[j];
            }
            uint32_t w = 0;
#pragma unroll
            for (uint32_t j = 0; j < 32u; ++j) {
                w |= (uint32_t)(32 * v[j] > thr) << j;
                corr += signL[j] * v[j];
            }
            dist = (uint32_t)__builtin_popcount(w ^ A.sync);
        }
        const bool normal = has && dist <= A.tol && corr >= A.min_corr;
        const bool inverted = has && dist >= 32u - A.tol && -corr >= A.min_corr;
        const bool hit = live && (normal || inverted);
        const unsigned long long mask = __ballot(hit);       // the wave's hits: its row's, in increasing k
        if (hit) {
            const uint32_t slot = count + (uint32_t)__builtin_popcountll(mask & ((1ull << q) - 1ull));
            if (slot < A.hit_cap)
                ((FMD_DDC_GLOBAL i4*)(uintptr_t)(A.rec_out + grow * A.hit_cap))[slot] =
                    i4{(int)Q, (int)(dist | (inverted ? 0x80000000u : 0u)), corr, thr};
        }
        count += (uint32_t)__builtin_popcountll(mask);
    }
    __syncthreads();                                         // (a call of fewer samples than a chunk: the rings are complete)

    if (!live) return;
    if (q == 0u) {
        A.cnt_out[grow] = count;
        A.b_out[grow * kBState + kBCarry] = carryOutL[row];
    }
    for (uint32_t e = q; e < tapmax; e += 64u) {             // soft[k1 - tap[31] ... k1)
        const uint32_t k = k1 - tapmax + e;
        A.s_out[grow * kSCarry + (k & (kSCarry - 1u))] = softL[row * kSRing + (k & (kSRing - 1u))];
    }
    if (q + 1u < W) {                                        // b[k1 - (W - 1) ... k1)
        const uint32_t k = k1 - (W - 1u) + q;
        A.b_out[grow * kBState + (k & (kBCarry - 1u))] = bL[row * kBRing + (k & (kBRing - 1u))];
    }
}

}  // namespace fmd_fk

struct fmd_fsk {
    FmdRows rows;                                         // width 1 (its history is unused: hcap = 1, the smallest the layer takes)
    FmdDdcPair bsum;                                      // [n_rows][kBState] int32
    FmdDdcPair soft;                                      // [n_rows][kSCarry] int16
    FmdRowRecords recs;                                   // fmd_fsk_hit, hit_cap per row
    fmd_fsk_config cfg{};
};

namespace {

int fk_enqueue(fmd_fsk* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, hipStream_t stream)
{
    FmdRows& r = h->rows;
    if (const int rc = fmd_rows_check_call(r, d_in, n_in, in_cap, d_out)) return rc;
    const uint32_t D = h->cfg.D;
    const uint64_t pos_r = r.core.pos % D, cnt = (pos_r + n_in) / D;
    if (cnt > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    if (n_in == 0) {                                         // nothing to take: no launch
        if (n_out) *n_out = 0;
        return FMD_OK;
    }
    fmd_fk::FskLaunch A{};
    fmd_rows_fill(A, r, d_in, n_in, in_cap, d_out, out_cap);
    A.b_in = h->bsum.in<int32_t>(r.core.cur); A.b_out = h->bsum.out<int32_t>(r.core.cur);
    A.s_in = h->soft.in<int16_t>(r.core.cur); A.s_out = h->soft.out<int16_t>(r.core.cur);
    A.cnt_out = h->recs.cnt_out(r.core.cur);
    A.rec_out = reinterpret_cast<fmd_fk::i4*>(h->recs.rec_out(r.core.cur));
    A.pos_r = (uint32_t)pos_r;
    A.k0 = (uint32_t)((r.core.pos / D) & 0xFFFFu);
    A.n_out = (uint32_t)cnt;
    A.D = D; A.W = h->cfg.W; A.shift = h->cfg.shift; A.sync = h->cfg.sync; A.tol = h->cfg.tol; A.hit_cap = h->cfg.hit_cap;
    A.min_corr = h->cfg.min_corr;
    for (uint32_t j = 0; j < 32; ++j) A.tap[j] = (uint8_t)h->cfg.tap[j];
    const uint32_t grid = (r.n_rows + fmd_fk::kRows - 1u) / fmd_fk::kRows;
    return fmd_rows_launch(r, fmd_fk::fmd_fsk_kernel, fmd_fk::fmd_fsk_kernel, grid, fmd_fk::kThreads, A, stream, n_in, cnt, n_out);
}

}  // namespace

extern "C" {

size_t fmd_fsk_out_cap(uint32_t D, size_t n_in)
{
    if (!D) return 0;
    return (size_t)(((uint64_t)n_in + D - 1) / D) + 1;      // floor((p + n) / D) - floor(p / D) <= ceil(n / D) for every p
}

int fmd_fsk_new(const fmd_fsk_config* cfg, uint32_t width, const fmd_device_config* dev, fmd_fsk** out)
{
    if (const int rc = fmd_rows_new_args(cfg, dev, out, 1)) return rc;       // (the pointers)
    if (width != 1) { fmd_internal_set_err("need width 1"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->D < 1 || cfg->D > 64) { fmd_internal_set_err("need 1 <= D <= 64"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->W < 1 || cfg->W > 16) { fmd_internal_set_err("need 1 <= W <= 16"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->shift > 10 || cfg->D * cfg->W > (1u << cfg->shift)) { fmd_internal_set_err("need shift <= 10 and D W <= 2^shift"); return FMD_ERR_UNSUPPORTED; }
    bool taps_ok = cfg->tap[0] == 0 && cfg->tap[31] <= 255;
    for (uint32_t j = 1; j < 32; ++j) taps_ok = taps_ok && cfg->tap[j] >= cfg->tap[j - 1];
    if (!taps_ok) { fmd_internal_set_err("need tap[0] = 0, tap non-decreasing, tap[31] <= 255"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->tol > 15) { fmd_internal_set_err("need tol <= 15"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->min_corr < 0 || cfg->min_corr > (1 << 20)) { fmd_internal_set_err("need 0 <= min_corr <= 2^20"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->hit_cap < 1 || cfg->hit_cap > 64) { fmd_internal_set_err("need 1 <= hit_cap <= 64"); return FMD_ERR_UNSUPPORTED; }
    if (const int rc = fmd_rows_count_arg(dev)) return rc;
    fmd_fsk* h = new (std::nothrow) fmd_fsk();
    if (!h) return FMD_ERR_NOMEM;
    h->cfg = *cfg;
    h->rows.width = 1; h->rows.n_rows = dev->n_channels; h->rows.hcap = 1u;
    h->rows.lds = (size_t)fmd_fk::kRows * fmd_fk::kChunk * cfg->D * sizeof(int16_t);    // the staging buffers; the rings are static
    const size_t n = dev->n_channels;
    fmd_ddc_add_pair(h->rows.core, h->bsum, n * fmd_fk::kBState * sizeof(int32_t));
    fmd_ddc_add_pair(h->rows.core, h->soft, n * fmd_fk::kSCarry * sizeof(int16_t));
    fmd_rows_add_records(h->rows, h->recs, cfg->hit_cap, sizeof(fmd_fsk_hit));
    return fmd_rows_device(h, dev, fmd_fsk_free, out);
}

void fmd_fsk_free(fmd_fsk* h) { fmd_rows_free(h); }
int fmd_fsk_reset(fmd_fsk* h) { return fmd_rows_reset(h); }
int fmd_fsk_check(fmd_fsk* h) { return fmd_rows_check(h); }

int fmd_fsk_outputs(const fmd_fsk* h, uint64_t* inputs, uint64_t* outputs)
{
    return fmd_rows_outputs(h, inputs, outputs, [](const fmd_fsk* f, uint64_t n) { return n / f->cfg.D; });
}

int fmd_fsk_hits(fmd_fsk* h, uint32_t* counts, fmd_fsk_hit* hits)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->rows.core.device);
    const size_t n = h->rows.n_rows, cap = h->recs.cap;
    std::vector<uint32_t> cnt(n);
    if (const int rc = fmd_rows_read_counts(h->rows, h->recs, cnt.data())) return rc;
    if (counts) memcpy(counts, cnt.data(), n * sizeof(uint32_t));
    if (!hits) return FMD_OK;
    FMD_DDC_TRY(hipMemcpy(hits, h->recs.records(h->rows.core.cur), n * cap * sizeof(fmd_fsk_hit), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < n; ++r) fmd_rows_zero_behind(h->recs, cnt[r], hits + r * cap);
    return FMD_OK;
}

// where fmd_fsk_hits reads from (no synchronisation: a kernel behind the call that wrote them reads them in stream order)
int fmd_pager_fsk_hits(fmd_fsk* h, const void** d_counts, const void** d_hits)
{
    if (!h || !d_counts || !d_hits) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *d_counts = h->recs.counts(h->rows.core.cur);
    *d_hits = h->recs.records(h->rows.core.cur);
    return FMD_OK;
}

int fmd_fsk_run_device(fmd_fsk* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, void* stream)
{
    return fmd_ddc_run_device(h ? &h->rows.core : nullptr, d_in, d_out,
                              [&] { return fk_enqueue(h, d_in, n_in, in_cap, d_out, out_cap, n_out, static_cast<hipStream_t>(stream)); });
}

// (a call of no samples has nothing to take: it does not touch the device)
int fmd_fsk_run_batch(fmd_fsk* h, const int16_t* in, size_t n_in, size_t in_cap, int16_t* out, size_t out_cap, size_t* n_out)
{
    return fmd_rows_run_batch(h, fk_enqueue, in, n_in, in_cap, out, out_cap, n_out, [](size_t n) { return n == 0; });
}

int fmd_fsk_kernel_name(const fmd_fsk* h, char* name, size_t cap) { return fmd_rows_kernel_name(h, name, cap, "fmd_fk::fmd_fsk_kernel"); }

}  // extern "C"
