// fmd_tonesq.hip -- tone squelch: every int16 row a bank leaves on the device is correlated, block by block, against a table of up
// to 64 windowed reference tones (CTCSS), and gated by the tone the blocks before decided on, in ONE gfx950 kernel.  Width 1 is
// mono audio, width 2 interleaved (L, R) whose mean is correlated and whose two components share the gate.
//
// Definition (include/fmd.h, "tone squelch"; tests/tonesq_ref.py), per row, with P = block and r = i mod P:
//     m[i] = x[i][0] or (x[i][0] + x[i][1]) >> 1;   Re_f(j), Im_f(j) = sum over block j of c_f[r] m[i], s_f[r] m[i]    (exact)
//     W_f = (Re_f >> 14)^2 + (Im_f >> 14)^2;  f* = the first largest;  rest = max W_f over |f - f*| > guard
//     hit_j = f* if W_f* >= min_power and (W_f* >> dom_shift) >= rest;  (t, cand, cnt, h) step once per block;  s_j = 256 or 0
//     g[i] = s_{j-2} + (((s_{j-1} - s_{j-2}) (min(r, Q - 1) + 1)) >> log2 Q),  out[i][c] = (x[i][c] g[i]) >> 8
// n_out = n_in: the handle carries no samples, only the 2 F partial sums (i64) and the small state per row.
//
// One workgroup = one tile of kRows = 32 rows for the whole call.  All rows of a call share core.pos, hence the table window and
// every block end inside the call.  The call's samples are walked in chunks of kChunk = 64 stream samples, aligned to the stream
// (P is a multiple of 64, so a chunk never crosses a block end; the first and the last chunk of a call may be partial).  Per chunk:
//   1. the chunk of the table -- 2 F tone rows (q = 2 f: cosine, 2 f + 1: sine) of 64 int16, which the host packed chunk-major so
//      that it is one contiguous piece -- into LDS, once for the 32 rows of the tile (rows q >= 2 F are zeros);
//   2. the samples: 16-byte loads of the pieces of each row that lie whole inside the chunk, element loads at the unaligned head
//      and tail; the sample as it is into rawL, m into mL (a partial chunk leaves zeros where the call has no sample: they add 0);
//   3. the gate of the current block (s_{j-2}, s_{j-1} of the row, from LDS) on rawL, stored with 16-byte stores where the OUTPUT
//      row is aligned (its alignment is its own: out_cap need not be in_cap), element stores at its head and tail;
//   4. the products, register-blocked: thread (qg = tid >> 3, rg = tid & 7) owns tone rows qg + 32 j and tile rows rg + 8 jj
//      (j, jj < 4): per 8 samples 4 + 4 ds_read_b128 feed 64 v_dot2_i32_i16.  64 samples sum in i32 (64 * 32768 * 1023 < 2^31),
//      then into the thread's 16 i64 accumulators.  Staged rows are 144 bytes apart, so the 8 rows a wave reads at once lie in
//      8 distinct groups of 4 banks.  A wave whose tone rows all lie beyond 2 F skips the phase; the j it runs are wave-uniform.
// At a block end (inside the workgroup, so a later block of the same call is gated by it): the accumulators >> 14 go to LDS (over
// the table chunk, which is dead by then), 8 lanes per row form W_f, reduce (W, f) to f* with shuffles, then `rest`, and lane 0
// of the row steps the state in LDS.  The sums and the state come from the handle's pairs at entry and go back at exit.
// HBM traffic: the input once, the output once, 16 F + 32 bytes per row and call for the sums and the state; the table chunk
// (128 * 2 F bytes) comes from L2 once per 32 rows x 64 samples: F / 8 table bytes per input sample.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_rows.h"

namespace fmd_tq {

constexpr int kThreads = 256;
constexpr uint32_t kRows = 32;                            // rows per tile
constexpr uint32_t kChunk = 64;                           // samples per chunk: the i32 grouping bound
constexpr uint32_t kStride = 72;                          // int16 per staged row (144 bytes)
constexpr uint32_t kQ = 128;                              // tone rows at most: 2 F
constexpr uint32_t kState = 8;                            // int32 per row: t + 1, cand + 1, cnt, h, s_prev, s_cur, power lo, hi

typedef int i4 __attribute__((ext_vector_type(4)));
typedef short s2 __attribute__((ext_vector_type(2)));

struct TsqLaunch {
    const int16_t* in;         // [n_rows][in_cap][W]
    uint64_t in_cap;
    uint32_t n_in;             // valid samples per row
    uint32_t n_rows;
    const int16_t* hist_in;    // (the rows layer's history: unused)
    int16_t* hist_out;
    uint32_t hcap;
    const int32_t* st_in;      // [n_rows][kState] (all-zero: the state at creation and after reset)
    int32_t* st_out;
    const int64_t* sum_in;     // [n_rows][nq]: the partial sums of the block the stream stands in
    int64_t* sum_out;
    const int16_t* tab;        // [P / 64][nq][64], and behind it one TsqDecide
    uint32_t pos_r;            // core.pos mod P: r of the call's first sample
    uint32_t P, nq;            // nq = 2 F
    uint32_t lgQ;              // log2 ramp
    int16_t* out;              // [n_rows][out_cap][W]
    uint64_t out_cap;
};

// What only a block's end reads: behind the table in its device buffer, so that it costs no scalar registers in between.
struct TsqDecide {
    uint64_t min_power, accept;
    uint32_t guard, dom_shift, confirm, hang;
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

__device__ __forceinline__ int dot2(int a, int b, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s2, a), __builtin_bit_cast(s2, b), acc, false);
}

// One chunk of the thread's NJ x 4 (tone row, tile row) sums: 64 samples in i32, then into the i64 accumulators.
template <int NJ>
__device__ __forceinline__ void accumulate(const int16_t* tabL, const int16_t* mL, uint32_t qg, uint32_t rg, int64_t (&acc)[4][4])
{
    int s[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) s[j][jj] = 0;
#pragma unroll 2
    for (uint32_t kk = 0; kk < kChunk / 8u; ++kk) {
        i4 t[NJ], x[4];
#pragma unroll
        for (int j = 0; j < NJ; ++j) t[j] = *reinterpret_cast<const i4*>(tabL + (qg + 32u * j) * kStride + 8u * kk);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) x[jj] = *reinterpret_cast<const i4*>(mL + (rg + 8u * jj) * kStride + 8u * kk);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                s[j][jj] = dot2(t[j].x, x[jj].x, s[j][jj]);
                s[j][jj] = dot2(t[j].y, x[jj].y, s[j][jj]);
                s[j][jj] = dot2(t[j].z, x[jj].z, s[j][jj]);
                s[j][jj] = dot2(t[j].w, x[jj].w, s[j][jj]);
            }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[j][jj] += (int64_t)s[j][jj];
}

__device__ __forceinline__ uint64_t power_of(const int32_t* ab, uint32_t f)
{
    const int64_t a = ab[2u * f], b = ab[2u * f + 1u];
    return (uint64_t)(a * a) + (uint64_t)(b * b);
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int off)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
    return ((uint64_t)hi << 32) | lo;
}

template <int W>
__global__ void __launch_bounds__(kThreads) fmd_tonesq_kernel(const TsqLaunch A)
{
    typedef typename Sample<W>::type sample_t;
    typedef const FMD_DDC_GLOBAL sample_t* gsrc;
    typedef FMD_DDC_GLOBAL sample_t* gdst;
    constexpr uint32_t EB = 2u * W;                          // bytes per sample
    constexpr uint32_t E = 16u / EB;                         // samples per 16-byte piece
    constexpr uint32_t NP = kChunk * EB / 16u + 1u;          // 16-byte pieces a chunk of one row touches at most
    __shared__ __attribute__((aligned(16))) int16_t tabL[kQ * kStride];            // the table chunk; at a block end AB [kRows][kQ]
    __shared__ __attribute__((aligned(16))) int16_t mL[kRows * kStride];
    __shared__ __attribute__((aligned(16))) sample_t rawL[kRows * kChunk];
    __shared__ int32_t stL[kRows * kState];
    int32_t* const AB = reinterpret_cast<int32_t*>(tabL);

    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t row0 = blockIdx.x * kRows;
    if (row0 >= A.n_rows) return;
    const uint32_t nrow = A.n_rows - row0 < kRows ? A.n_rows - row0 : kRows;
    const uint32_t rg = tid & 7u, qg = tid >> 3;
    const uint32_t nq = A.nq, P = A.P, qm = (1u << A.lgQ) - 1u;
    // tone rows qg + 32 j: the j this wave runs (its smallest qg is 8 wave)
    uint32_t nj = nq > 8u * wave ? (nq - 8u * wave + 31u) >> 5 : 0u;
    nj = (uint32_t)__builtin_amdgcn_readfirstlane((int)(nj < 4u ? nj : 4u));

    int64_t acc[4][4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j)
#pragma unroll
        for (uint32_t jj = 0; jj < 4u; ++jj) {
            const uint32_t q = qg + 32u * j, tr = rg + 8u * jj;
            acc[j][jj] = q < nq && tr < nrow ? A.sum_in[(uint64_t)(row0 + tr) * nq + q] : 0;
        }
    stL[tid] = (tid >> 3) < nrow ? A.st_in[(uint64_t)row0 * kState + tid] : 0;     // kRows kState == kThreads
    for (uint32_t i = tid; i < kRows * kStride / 2u; i += kThreads) reinterpret_cast<uint32_t*>(mL)[i] = 0u;
    __syncthreads();

    // staging and gate: thread (row = tid >> 3, pl = tid & 7) takes the pieces pl, pl + 8, ... of its row of every chunk
    const uint32_t row = tid >> 3, pl = tid & 7u;
    const bool live = row < nrow;
    const uintptr_t R = live ? (uintptr_t)(A.in + (uint64_t)(row0 + row) * A.in_cap * W) : 0;       // the row's samples of this call
    const uintptr_t O = live ? (uintptr_t)(A.out + (uint64_t)(row0 + row) * A.out_cap * W) : 0;
    const uint32_t o_end = A.pos_r + A.n_in;                 // stream offsets [pos_r, o_end) from the start of the first block
    for (uint32_t c = A.pos_r >> 6; c <= (o_end - 1u) >> 6; ++c) {                 // block-uniform
        const uint32_t oa = c << 6 > A.pos_r ? c << 6 : A.pos_r, ob = (c + 1u) << 6 < o_end ? (c + 1u) << 6 : o_end;
        const uint32_t ja = oa - A.pos_r, jb = ob - A.pos_r;                       // call samples [ja, jb)
        if (ob - oa != kChunk) {                             // a partial chunk: zeros where the call has no sample
            for (uint32_t i = tid; i < kRows * kStride / 2u; i += kThreads) reinterpret_cast<uint32_t*>(mL)[i] = 0u;
            __syncthreads();
        }
        // ---- 1. the table chunk -------------------------------------------------------------------------------------------------
        {
            const FMD_DDC_GLOBAL i4* const src = (const FMD_DDC_GLOBAL i4*)(uintptr_t)(A.tab + (uint64_t)(c & ((P >> 6) - 1u)) * nq * kChunk);
            for (uint32_t p = tid; p < kQ * 8u; p += kThreads) {
                const uint32_t q = p >> 3, part = p & 7u;
                *reinterpret_cast<i4*>(tabL + q * kStride + 8u * part) = q < nq ? src[p] : i4{0, 0, 0, 0};
            }
        }
        // ---- 2. the samples -----------------------------------------------------------------------------------------------------
        for (uint32_t idx = pl; idx < NP; idx += 8u) {       // lane pl of the row's 8 takes every 8th piece
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
                    mL[row * kStride + e0 + e] = mix<W>(s);
                }
            } else {                                         // the unaligned head or tail: exactly the samples of the chunk
                for (uint32_t e = 0; e < E; ++e) {
                    const uintptr_t a = ca + e * EB;
                    if (a < a0 || a >= a1) continue;
                    const uint32_t eo = (A.pos_r + (uint32_t)((a - R) / EB)) & 63u;
                    const uint32_t s = *(gsrc)a;
                    rawL[row * kChunk + eo] = (sample_t)s;
                    mL[row * kStride + eo] = mix<W>(s);
                }
            }
        }
        __syncthreads();

        // ---- 3. the gate of the current block -------------------------------------------------------------------------------------
        for (uint32_t idx = pl; idx < NP; idx += 8u) {
            const uintptr_t o0 = O + (uintptr_t)ja * EB, o1 = O + (uintptr_t)jb * EB;
            const uintptr_t ca = ((o0 >> 4) + idx) << 4;
            if (!live || ca >= o1) continue;
            const int sp = stL[row * kState + 4u], ds = stL[row * kState + 5u] - sp;
            if (ca >= o0 && ca + 16u <= o1) {                // a whole piece of the output row
                const uint32_t o = A.pos_r + (uint32_t)((ca - O) / EB);
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (uint32_t e = 0; e < E; ++e) {
                    const uint32_t r = (o + e) & (P - 1u), k = (r < qm ? r : qm) + 1u;
                    const uint32_t y = gate<W>(rawL[row * kChunk + ((o + e) & 63u)], sp + ((ds * (int)k) >> A.lgQ));
                    if (W == 2) w[e] = y; else w[e >> 1] |= y << (16u * (e & 1u));
                }
                *(FMD_DDC_GLOBAL i4*)ca = i4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
            } else {                                         // the unaligned head or tail
                for (uint32_t e = 0; e < E; ++e) {
                    const uintptr_t a = ca + e * EB;
                    if (a < o0 || a >= o1) continue;
                    const uint32_t o = A.pos_r + (uint32_t)((a - O) / EB);
                    const uint32_t r = o & (P - 1u), k = (r < qm ? r : qm) + 1u;
                    *(gdst)a = (sample_t)gate<W>(rawL[row * kChunk + (o & 63u)], sp + ((ds * (int)k) >> A.lgQ));
                }
            }
        }

        // ---- 4. the products ----------------------------------------------------------------------------------------------------
        switch (nj) {                                        // wave-uniform
        case 1: accumulate<1>(tabL, mL, qg, rg, acc); break;
        case 2: accumulate<2>(tabL, mL, qg, rg, acc); break;
        case 3: accumulate<3>(tabL, mL, qg, rg, acc); break;
        case 4: accumulate<4>(tabL, mL, qg, rg, acc); break;
        default: break;
        }
        __syncthreads();                                     // the table chunk and the samples are dead

        // ---- the block's end: W_f, the decision, the state ------------------------------------------------------------------------
        if ((ob & (P - 1u)) == 0u) {                         // block-uniform
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j)
#pragma unroll
                for (uint32_t jj = 0; jj < 4u; ++jj) {
                    AB[(rg + 8u * jj) * kQ + qg + 32u * j] = (int32_t)(acc[j][jj] >> 14);      // |Re|, |Im| <= 2^38
                    acc[j][jj] = 0;
                }
            __syncthreads();
            {
                const uint32_t l = pl;
                const int32_t* const ab = AB + row * kQ;
                const FMD_DDC_GLOBAL TsqDecide* const D = (const FMD_DDC_GLOBAL TsqDecide*)(uintptr_t)(A.tab + (uint64_t)nq * P);
                const uint32_t guard = D->guard;
                uint64_t bw = 0;
                uint32_t bf = 0xFFFFu;                       // no tone yet
                for (uint32_t f = l; f < (nq >> 1); f += 8u) {
                    const uint64_t w = power_of(ab, f);
                    if (bf == 0xFFFFu || w > bw) { bw = w; bf = f; }
                }
                for (int off = 1; off < 8; off <<= 1) {      // the first largest of the row's 8 lanes
                    const uint64_t ow = shfl_xor_u64(bw, off);
                    const uint32_t of = (uint32_t)__shfl_xor((int)bf, off);
                    if (ow > bw || (ow == bw && of < bf)) { bw = ow; bf = of; }
                }
                uint64_t rest = 0;
                for (uint32_t f = l; f < (nq >> 1); f += 8u) {
                    const uint32_t d = f > bf ? f - bf : bf - f;
                    if (d > guard) {
                        const uint64_t w = power_of(ab, f);
                        rest = w > rest ? w : rest;
                    }
                }
                for (int off = 1; off < 8; off <<= 1) {
                    const uint64_t o = shfl_xor_u64(rest, off);
                    rest = o > rest ? o : rest;
                }
                if (l == 0u) {
                    int32_t* const st = stL + row * kState;
                    uint32_t t1 = (uint32_t)st[0], cand1 = (uint32_t)st[1], cnt = (uint32_t)st[2], h = (uint32_t)st[3];
                    if (bw >= D->min_power && (bw >> D->dom_shift) >= rest) {
                        if (bf + 1u == cand1) cnt = cnt < 65535u ? cnt + 1u : 65535u;
                        else { cand1 = bf + 1u; cnt = 1u; }
                    } else { cand1 = 0u; cnt = 0u; }
                    if (cnt >= D->confirm) { t1 = cand1; h = D->hang; }
                    else if (h > 0u) --h;
                    else t1 = 0u;
                    st[0] = (int32_t)t1; st[1] = (int32_t)cand1; st[2] = (int32_t)cnt; st[3] = (int32_t)h;
                    st[4] = st[5];
                    st[5] = t1 && ((D->accept >> (t1 - 1u)) & 1ull) ? 256 : 0;
                    st[6] = (int32_t)(uint32_t)bw; st[7] = (int32_t)(uint32_t)(bw >> 32);
                }
            }
            __syncthreads();                                 // the next chunk's table goes over AB, its gate reads the state
        }
    }

#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j)
#pragma unroll
        for (uint32_t jj = 0; jj < 4u; ++jj) {
            const uint32_t q = qg + 32u * j, tr = rg + 8u * jj;
            if (q < nq && tr < nrow) A.sum_out[(uint64_t)(row0 + tr) * nq + q] = acc[j][jj];
        }
    if ((tid >> 3) < nrow) A.st_out[(uint64_t)row0 * kState + tid] = stL[tid];
}

}  // namespace fmd_tq

struct fmd_tonesq {
    FmdRows rows;                                         // (its history is unused: hcap = 1, the smallest the layer takes)
    FmdDdcPair state;                                     // [n_rows][kState] int32
    FmdDdcPair sums;                                      // [n_rows][2 F] int64
    void* d_tab = nullptr;                                // [P / 64][2 F][64] int16, then one TsqDecide
    std::vector<int16_t> packed;                          // the same, until the device step
    fmd_tonesq_config cfg{};
    uint32_t F = 0, lgQ = 0;
};

namespace {

int tonesq_enqueue(fmd_tonesq* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, hipStream_t stream)
{
    FmdRows& r = h->rows;
    if (const int rc = fmd_rows_check_call(r, d_in, n_in, in_cap, d_out)) return rc;
    if (out_cap < n_in) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    if (n_in == 0) {                                         // nothing to take: no launch
        if (n_out) *n_out = 0;
        return FMD_OK;
    }
    fmd_tq::TsqLaunch A{};
    fmd_rows_fill(A, r, d_in, n_in, in_cap, d_out, out_cap);
    A.st_in = h->state.in<int32_t>(r.core.cur); A.st_out = h->state.out<int32_t>(r.core.cur);
    A.sum_in = h->sums.in<int64_t>(r.core.cur); A.sum_out = h->sums.out<int64_t>(r.core.cur);
    A.tab = static_cast<const int16_t*>(h->d_tab);
    A.pos_r = (uint32_t)(r.core.pos & (h->cfg.block - 1u));
    A.P = h->cfg.block; A.nq = 2u * h->F;
    A.lgQ = h->lgQ;
    const uint32_t grid = (r.n_rows + fmd_tq::kRows - 1u) / fmd_tq::kRows;
    return fmd_rows_launch(r, fmd_tq::fmd_tonesq_kernel<1>, fmd_tq::fmd_tonesq_kernel<2>, grid, fmd_tq::kThreads, A, stream, n_in, n_in, n_out);
}

bool pow2(uint32_t v) { return v && (v & (v - 1u)) == 0; }

}  // namespace

extern "C" {

size_t fmd_tonesq_out_cap(size_t n_in) { return n_in; }

int fmd_tonesq_new(const fmd_tonesq_config* cfg, const int16_t* table, uint32_t n_tones, uint32_t width, const fmd_device_config* dev,
                   fmd_tonesq** out)
{
    if (const int rc = fmd_rows_new_args(cfg, dev, out, width)) return rc;
    if (!table) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    const uint32_t P = cfg->block, F = n_tones;
    if (!pow2(P) || P < 64 || P > 8192) { fmd_internal_set_err("need block a power of two in [64, 8192]"); return FMD_ERR_UNSUPPORTED; }
    if (F < 1 || F > 64) { fmd_internal_set_err("need 1 <= n_tones <= 64"); return FMD_ERR_UNSUPPORTED; }
    if ((uint64_t)F * P > 262144) { fmd_internal_set_err("need n_tones * block <= 262144"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->guard > 63) { fmd_internal_set_err("need guard <= 63"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->dom_shift > 32) { fmd_internal_set_err("need dom_shift <= 32"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->min_power < 1) { fmd_internal_set_err("need min_power >= 1"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->confirm < 1 || cfg->confirm > 255) { fmd_internal_set_err("need 1 <= confirm <= 255"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->hang > 65535) { fmd_internal_set_err("need hang <= 65535"); return FMD_ERR_UNSUPPORTED; }
    if (!pow2(cfg->ramp) || cfg->ramp > P) { fmd_internal_set_err("need ramp a power of two in [1, block]"); return FMD_ERR_UNSUPPORTED; }
    for (size_t i = 0; i < (size_t)F * P * 2; ++i)
        if (table[i] > 1023 || table[i] < -1023) { fmd_internal_set_err("|table entry| > 1023"); return FMD_ERR_UNSUPPORTED; }
    if (const int rc = fmd_rows_count_arg(dev)) return rc;
    fmd_tonesq* h = new (std::nothrow) fmd_tonesq();
    if (!h) return FMD_ERR_NOMEM;
    h->cfg = *cfg; h->F = F;
    while ((1u << h->lgQ) < cfg->ramp) ++h->lgQ;
    // chunk-major: [P / 64][q = 2 f + (0: c_f, 1: s_f)][64]
    const uint32_t nq = 2u * F;
    h->packed.resize((size_t)nq * P + sizeof(fmd_tq::TsqDecide) / sizeof(int16_t));      // (2 nq P bytes: a multiple of 8)
    const fmd_tq::TsqDecide dec{cfg->min_power, cfg->accept, cfg->guard, cfg->dom_shift, cfg->confirm, cfg->hang};
    memcpy(&h->packed[(size_t)nq * P], &dec, sizeof dec);
    for (uint32_t f = 0; f < F; ++f)
        for (uint32_t r = 0; r < P; ++r)
            for (uint32_t k = 0; k < 2u; ++k)
                h->packed[((size_t)(r >> 6) * nq + 2u * f + k) * fmd_tq::kChunk + (r & 63u)] = table[((size_t)f * P + r) * 2u + k];
    h->rows.lds = 0;                                         // (the kernel's LDS is static)
    h->rows.width = width; h->rows.n_rows = dev->n_channels; h->rows.hcap = 1u;
    fmd_ddc_add_pair(h->rows.core, h->state, (size_t)dev->n_channels * fmd_tq::kState * sizeof(int32_t));
    fmd_ddc_add_pair(h->rows.core, h->sums, (size_t)dev->n_channels * nq * sizeof(int64_t));
    fmd_ddc_add_owned(h->rows.core, h->d_tab, h->packed.data(), h->packed.size() * sizeof(int16_t));
    const int rc = fmd_rows_device(h, dev, fmd_tonesq_free, out);
    if (rc == FMD_OK) std::vector<int16_t>().swap(h->packed);
    return rc;
}

void fmd_tonesq_free(fmd_tonesq* h) { fmd_rows_free(h); }
int fmd_tonesq_reset(fmd_tonesq* h) { return fmd_rows_reset(h); }
int fmd_tonesq_check(fmd_tonesq* h) { return fmd_rows_check(h); }

int fmd_tonesq_outputs(const fmd_tonesq* h, uint64_t* inputs, uint64_t* outputs)
{
    return fmd_rows_outputs(h, inputs, outputs, [](const fmd_tonesq*, uint64_t n) { return n; });
}

int fmd_tonesq_status(fmd_tonesq* h, int32_t* tone, uint64_t* power, uint8_t* open)
{
    if (!h || !tone || !power || !open) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    std::vector<int32_t> st;
    if (const int rc = fmd_rows_read_state(h->rows, h->state, fmd_tq::kState, st)) return rc;
    for (size_t r = 0; r < h->rows.n_rows; ++r) {
        const int32_t* s = &st[r * fmd_tq::kState];
        tone[r] = s[0] - 1;
        power[r] = ((uint64_t)(uint32_t)s[7] << 32) | (uint32_t)s[6];
        open[r] = s[5] != 0;
    }
    return FMD_OK;
}

int fmd_tonesq_run_device(fmd_tonesq* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, void* stream)
{
    return fmd_ddc_run_device(h ? &h->rows.core : nullptr, d_in, d_out,
                              [&] { return tonesq_enqueue(h, d_in, n_in, in_cap, d_out, out_cap, n_out, static_cast<hipStream_t>(stream)); });
}

// (a call of no samples has nothing to take: it does not touch the device)
int fmd_tonesq_run_batch(fmd_tonesq* h, const int16_t* in, size_t n_in, size_t in_cap, int16_t* out, size_t out_cap, size_t* n_out)
{
    return fmd_rows_run_batch(h, tonesq_enqueue, in, n_in, in_cap, out, out_cap, n_out, [](size_t n) { return n == 0; });
}

int fmd_tonesq_kernel_name(const fmd_tonesq* h, char* name, size_t cap)
{
    return fmd_rows_kernel_name(h, name, cap, "fmd_tq::fmd_tonesq_kernel<%u>");
}

}  // extern "C"
