// fmd_agc.hip -- automatic gain control: a block-peak AGC with one block of look-ahead over the int16 rows a bank leaves on the
// device, in ONE gfx950 kernel.  Width 1 is mono audio, width 2 interleaved (L, R) or (I, Q) under one common gain; a row is one
// (stream, station) or (stream, channel).
//
// Definition (include/fmd.h, "automatic gain control"; tests/agc_ref.py), per row:
//     m[i] = max_c |x[i][c]|,  p_j = max of m over block j (P samples),  e_j = max(p_j, p_{j+1})
//     d_j  = min(gain_max, floor(1024 target / e_j))                                          (Q10, for e_j > 0)
//     (G, h) from (gain_max, 0), per block: e_j == 0 holds; d_j <= G attacks (G = d_j, h = hang); h > 0 counts down; otherwise
//                                          G = min(d_j, G + max(1, ((d_j - G) decay) >> 8))
//     g[i] = G_{j-1} + (((G_j - G_{j-1}) (r + 1)) >> log2 P),  out[i][c] = (x[i][c] g[i]) >> 10
// Block j comes with the call that completes block j + 1; the handle carries the samples not yet emitted (they start on a block
// boundary, at most 2 P - 1 of them) and (G, h) per row.
//
// One workgroup = one row.  Virtual sample v of a call is sample v of (carried history ++ the call's samples); v = 0 is the call's
// first output.  The call's nb blocks are walked in segments of sb = ring / P - 1 blocks, through a ring of ring = sb + 1 blocks of
// samples in LDS (sample v at ring position (v + sh) mod ring): the segment plan depends on nb only.  Per segment:
//   1. stage the segment's blocks and its look-ahead block: 16-byte loads of the chunks of the row that lie whole inside the
//      needed samples, each to one aligned 16-byte LDS store (sh shifts the ring so that a 16-byte chunk of the row lands on a
//      16-byte boundary), element loads for the unaligned head and tail and for the carried history.  The look-ahead block of one
//      segment is the first block of the next and stays where it is, so every sample of the call is read once;
//   2. block peaks: the waves take the blocks in turn (64 / P blocks per wave and turn for P < 64), a shuffle reduction per block;
//   3. d_j, one lane per block (a 32-bit integer division);
//   4. one thread steps (G, h) over the segment's blocks and leaves G_{j-1}, G_j in LDS;
//   5. all lanes apply g[i]: whole 16-byte chunks of the output row in one store, element stores at the unaligned head and tail.
// The workgroup also writes the next call's history (from the samples' source, they are not all staged) and (G, h).
// HBM traffic: the input once, the output once, the history (at most 2 P - 1 samples per row) written once and read twice.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>

#include "fmd_rows.h"

namespace fmd_ag {

constexpr int kThreads = 256;
constexpr uint32_t kRingBytes = 16384;                    // the ring of samples: this, or two blocks where they are larger

typedef int i4 __attribute__((ext_vector_type(4)));

struct AgcLaunch {
    const int16_t* in;         // [n_rows][in_cap][W]
    uint64_t in_cap;
    uint32_t n_in;             // valid samples per row
    uint32_t n_rows;
    const int16_t* hist_in;    // [n_rows][hcap][W]: the first h are the samples in front of the call
    int16_t* hist_out;
    uint32_t hcap, h, h_next;
    const int32_t* st_in;      // [n_rows][2]: gain_max - G, h (all-zero: the state at creation and after reset)
    int32_t* st_out;
    uint32_t nb;               // blocks this call emits
    uint32_t first;            // 1: the call's first block is block 0 of the stream (G_{-1} := G_0)
    uint32_t P, lgP;
    uint32_t ring;             // samples in the ring: a power of two, >= 2 P
    uint32_t sb;               // blocks per segment: ring / P - 1
    uint32_t num;              // 1024 target
    int32_t gain_max;
    uint32_t hang, decay;
    int16_t* out;              // [n_rows][out_cap][W]
    uint64_t out_cap;
};

template <int W> struct Sample;
template <> struct Sample<1> { typedef uint16_t type; };
template <> struct Sample<2> { typedef uint32_t type; };   // (c0, c1) of one sample

// max_c |x[c]| of one sample: 0 ... 32768
template <int W>
__device__ __forceinline__ uint32_t peak_of(uint32_t s)
{
    const int a = (int)(s << 16) >> 16;
    uint32_t m = (uint32_t)(a < 0 ? -a : a);
    if (W == 2) {
        const int b = (int)s >> 16;
        const uint32_t mb = (uint32_t)(b < 0 ? -b : b);
        m = m > mb ? m : mb;
    }
    return m;
}

// (x[c] g) >> 10 of one sample, packed as the sample is
template <int W>
__device__ __forceinline__ uint32_t scale(uint32_t s, int g)
{
    const int a = (int)(s << 16) >> 16;
    uint32_t y = (uint32_t)((a * g) >> 10) & 0xFFFFu;
    if (W == 2) {
        const int b = (int)s >> 16;
        y |= (uint32_t)((b * g) >> 10) << 16;
    }
    return y;
}

template <int W>
__global__ void __launch_bounds__(kThreads) fmd_agc_kernel(const AgcLaunch A)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    typedef typename Sample<W>::type sample_t;
    typedef const FMD_DDC_GLOBAL sample_t* gsrc;
    typedef FMD_DDC_GLOBAL sample_t* gdst;
    constexpr uint32_t EB = 2u * W;                          // bytes per sample
    constexpr uint32_t E = 16u / EB;                         // samples per 16-byte chunk
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t row = blockIdx.x;
    if (row >= A.n_rows) return;
    sample_t* const ring = reinterpret_cast<sample_t*>(lds);                       // [ring]
    uint32_t* const pk = lds + ((A.ring * EB) >> 2);                               // [sb + 1]: peaks of the segment's blocks
    int* const gs = reinterpret_cast<int*>(pk + (A.ring >> A.lgP));                // [sb + 2]: G_{b0 - 1}, then G of every block
    const uint32_t P = A.P, lgP = A.lgP, mask = A.ring - 1u;

    const uintptr_t R = (uintptr_t)(A.in + (uint64_t)row * A.in_cap * W);          // the row's samples of this call
    const gsrc cin = (gsrc)R;
    const gsrc hin = (gsrc)(uintptr_t)(A.hist_in + (uint64_t)row * A.hcap * W);
    const uintptr_t O = (uintptr_t)(A.out + (uint64_t)row * A.out_cap * W);
    // call sample j sits at ring position (h + j + sh) & mask, which is (R / EB + j) mod E: a 16-byte chunk of the row is one of the ring
    const uint32_t sh = ((uint32_t)(R & 15u) / EB + E - A.h % E) % E;

    // the next call's history: the virtual samples from block nb on
    {
        const gdst hout = (gdst)(uintptr_t)(A.hist_out + (uint64_t)row * A.hcap * W);
        const uint32_t v0 = A.nb << lgP;
        for (uint32_t i = tid; i < A.h_next; i += kThreads) {
            const uint32_t v = v0 + i;
            hout[i] = v < A.h ? hin[v] : cin[v - A.h];
        }
    }

    int G = 0, hg = 0;                                       // thread 0: the state after the last block
    if (tid == 0) { G = A.gain_max - A.st_in[2u * row]; hg = A.st_in[2u * row + 1u]; }

    for (uint32_t b0 = 0; b0 < A.nb; b0 += A.sb) {           // block-uniform
        const uint32_t nk = A.nb - b0 < A.sb ? A.nb - b0 : A.sb;   // blocks b0 ... b0 + nk - 1 are emitted, block b0 + nk is the look-ahead
        const uint32_t kf = b0 ? 1u : 0u;                    // block b0 is the look-ahead of the segment before
        // ---- 1. staging: virtual samples [va, vb) -----------------------------------------------------------------------------
        const uint32_t va = (b0 + kf) << lgP, vb = (b0 + nk + 1u) << lgP;
        {
            const uint32_t he = vb < A.h ? vb : A.h;
            for (uint32_t v = va + tid; v < he; v += kThreads) ring[(v + sh) & mask] = hin[v];
        }
        if (vb > A.h) {
            const uint32_t ja = va > A.h ? va - A.h : 0u, jb = vb - A.h;           // call samples [ja, jb), jb <= n_in
            const uintptr_t a0 = R + (uintptr_t)ja * EB, a1 = R + (uintptr_t)jb * EB;
            const uintptr_t c_lo = a0 >> 4, c_hi = (a1 + 15u) >> 4;
            for (uint32_t i = tid; i < (uint32_t)(c_hi - c_lo); i += kThreads) {
                const uintptr_t ca = (c_lo + i) << 4;
                if (ca >= a0 && ca + 16u <= a1) {            // whole inside the needed samples
                    const uint32_t j = (uint32_t)((ca - R) / EB);
                    *reinterpret_cast<i4*>(ring + ((A.h + j + sh) & mask)) = *(const FMD_DDC_GLOBAL i4*)ca;
                } else {                                     // the unaligned head or tail: exactly the samples needed
                    for (uint32_t e = 0; e < E; ++e) {
                        const uintptr_t a = ca + e * EB;
                        if (a < a0 || a >= a1) continue;
                        const uint32_t j = (uint32_t)((a - R) / EB);
                        ring[(A.h + j + sh) & mask] = *(gsrc)a;
                    }
                }
            }
        }
        __syncthreads();

        // ---- 2. block peaks: LP lanes per block -------------------------------------------------------------------------------
        {
            const uint32_t lgLP = lgP < 6u ? lgP : 6u, LP = 1u << lgLP, per = 64u >> lgLP;
            const uint32_t sub = lane >> lgLP, l0 = lane & (LP - 1u);
            for (uint32_t kb = kf + wave * per; kb <= nk; kb += 4u * per) {        // wave-uniform
                const uint32_t k = kb + sub;
                uint32_t m = 0u;
                if (k <= nk) {
                    const uint32_t base = ((b0 + k) << lgP) + sh;
                    for (uint32_t i = l0; i < P; i += LP) {
                        const uint32_t pm = peak_of<W>(ring[(base + i) & mask]);
                        m = m > pm ? m : pm;
                    }
                }
                for (uint32_t off = LP >> 1; off; off >>= 1) {
                    const uint32_t o = (uint32_t)__shfl_xor((int)m, (int)off);
                    m = m > o ? m : o;
                }
                if (k <= nk && l0 == 0u) pk[k] = m;
            }
        }
        __syncthreads();

        // ---- 3. desired gains, one lane per block; -1: a silent block ------------------------------------------------------------
        for (uint32_t k = tid; k < nk; k += kThreads) {
            const uint32_t pa = pk[k], pb = pk[k + 1u], e = pa > pb ? pa : pb;
            int d = -1;
            if (e) {
                const uint32_t q = A.num / e;                // exact: 32-bit integer division
                d = q < (uint32_t)A.gain_max ? (int)q : A.gain_max;
            }
            gs[k + 1u] = d;
        }
        __syncthreads();

        // ---- 4. the recursion ---------------------------------------------------------------------------------------------------
        if (tid == 0) {
            const int Gp = G;
            for (uint32_t k = 0; k < nk; ++k) {
                const int d = gs[k + 1u];
                if (d >= 0) {
                    if (d <= G) { G = d; hg = (int)A.hang; }
                    else if (hg > 0) --hg;
                    else {
                        int inc = ((d - G) * (int)A.decay) >> 8;
                        if (inc < 1) inc = 1;
                        G = G + inc < d ? G + inc : d;
                    }
                }
                gs[k + 1u] = G;
            }
            gs[0] = (A.first && b0 == 0u) ? gs[1] : Gp;
            pk[0] = pk[nk];                                  // the look-ahead block is the next segment's first
        }
        __syncthreads();

        // ---- 5. apply: virtual samples [b0 P, (b0 + nk) P) are this call's outputs of the same index ------------------------------
        {
            const uintptr_t o0 = O + ((uintptr_t)b0 << lgP) * EB, o1 = O + ((uintptr_t)(b0 + nk) << lgP) * EB;
            const uintptr_t c_lo = o0 >> 4, c_hi = (o1 + 15u) >> 4;
            for (uint32_t i = tid; i < (uint32_t)(c_hi - c_lo); i += kThreads) {
                const uintptr_t ca = (c_lo + i) << 4;
                if (ca >= o0 && ca + 16u <= o1) {            // a whole chunk of the output row
                    const uint32_t v = (uint32_t)((ca - O) / EB);
                    uint32_t k = (v >> lgP) - b0, r = v & (P - 1u);
                    int ga = gs[k], dg = gs[k + 1u] - ga;
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (uint32_t e = 0; e < E; ++e) {
                        if (r == P) { r = 0u; ++k; ga = gs[k]; dg = gs[k + 1u] - ga; }
                        const int g = ga + ((dg * (int)(r + 1u)) >> lgP);
                        const uint32_t y = scale<W>(ring[(v + e + sh) & mask], g);
                        if (W == 2) w[e] = y; else w[e >> 1] |= y << (16u * (e & 1u));
                        ++r;
                    }
                    *(FMD_DDC_GLOBAL i4*)ca = i4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
                } else {                                     // the unaligned head or tail
                    for (uint32_t e = 0; e < E; ++e) {
                        const uintptr_t a = ca + e * EB;
                        if (a < o0 || a >= o1) continue;
                        const uint32_t v = (uint32_t)((a - O) / EB);
                        const uint32_t k = (v >> lgP) - b0, r = v & (P - 1u);
                        const int ga = gs[k], g = ga + (((gs[k + 1u] - ga) * (int)(r + 1u)) >> lgP);
                        *(gdst)a = (sample_t)scale<W>(ring[(v + sh) & mask], g);
                    }
                }
            }
        }
        __syncthreads();                                     // the next segment's staging overwrites the ring
    }

    if (tid == 0) { A.st_out[2u * row] = A.gain_max - G; A.st_out[2u * row + 1u] = hg; }
}

}  // namespace fmd_ag

struct fmd_agc {
    FmdRows rows;                                         // the history: the samples not yet emitted, hcap = 2 P
    FmdDdcPair state;                                     // [n_rows][2] int32: gain_max - G, h
    uint32_t P = 0, lgP = 0, target = 0, gain_max = 0, hang = 0, decay = 0;
    uint32_t ring = 0;
};

namespace {

// blocks emitted once `n` samples per row have arrived: block j comes with block j + 1
uint64_t agc_blocks(const fmd_agc* h, uint64_t n)
{
    const uint64_t full = n >> h->lgP;
    return full > 1 ? full - 1 : 0;
}

int agc_enqueue(fmd_agc* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, hipStream_t stream)
{
    FmdRows& r = h->rows;
    if (const int rc = fmd_rows_check_call(r, d_in, n_in, in_cap, d_out)) return rc;
    if (r.n_rows >= (1ull << 31)) { fmd_internal_set_err("too many rows for the grid"); return FMD_ERR_UNSUPPORTED; }
    const uint64_t N0 = r.core.pos, N1 = N0 + n_in;
    const uint64_t B0 = agc_blocks(h, N0), B1 = agc_blocks(h, N1), cnt = (B1 - B0) << h->lgP;
    if (cnt > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    if (n_in == 0) {                                         // nothing to take: no launch
        if (n_out) *n_out = 0;
        return FMD_OK;
    }
    fmd_ag::AgcLaunch A{};
    fmd_rows_fill(A, r, d_in, n_in, in_cap, d_out, out_cap);
    A.h = (uint32_t)(N0 - (B0 << h->lgP));                  // <= 2 P - 1
    A.h_next = (uint32_t)(N1 - (B1 << h->lgP));             // <= 2 P - 1
    A.st_in = h->state.in<int32_t>(r.core.cur); A.st_out = h->state.out<int32_t>(r.core.cur);
    A.nb = (uint32_t)(B1 - B0);
    A.first = B0 == 0 ? 1u : 0u;
    A.P = h->P; A.lgP = h->lgP; A.ring = h->ring; A.sb = (h->ring >> h->lgP) - 1u;
    A.num = 1024u * h->target; A.gain_max = (int32_t)h->gain_max; A.hang = h->hang; A.decay = h->decay;
    if (A.h >= r.hcap || A.h_next >= r.hcap) { fmd_internal_set_err("internal: history out of range"); return FMD_ERR_BAD_STATE; }
    return fmd_rows_launch(r, fmd_ag::fmd_agc_kernel<1>, fmd_ag::fmd_agc_kernel<2>, r.n_rows, fmd_ag::kThreads, A, stream, n_in, cnt, n_out);
}

}  // namespace

extern "C" {

size_t fmd_agc_out_cap(uint32_t block, size_t n_in)
{
    if (!block) return 0;
    return (size_t)(((uint64_t)n_in + block - 1) / block) * block;   // blocks(N + n) - blocks(N) <= ceil(n / P) for every N
}

int fmd_agc_new(const fmd_agc_config* cfg, uint32_t width, const fmd_device_config* dev, fmd_agc** out)
{
    if (const int rc = fmd_rows_new_args(cfg, dev, out, width)) return rc;
    if (cfg->block < 16 || cfg->block > 4096 || (cfg->block & (cfg->block - 1u)) != 0) {
        fmd_internal_set_err("need block a power of two in [16, 4096]"); return FMD_ERR_UNSUPPORTED;
    }
    if (cfg->target < 1 || cfg->target > 32767) { fmd_internal_set_err("need 1 <= target <= 32767"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->gain_max < 1 || cfg->gain_max > 262144) { fmd_internal_set_err("need 1 <= gain_max <= 262144"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->hang > 65535) { fmd_internal_set_err("need hang <= 65535"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->decay < 1 || cfg->decay > 256) { fmd_internal_set_err("need 1 <= decay <= 256"); return FMD_ERR_UNSUPPORTED; }
    if (const int rc = fmd_rows_count_arg(dev)) return rc;
    fmd_agc* h = new (std::nothrow) fmd_agc();
    if (!h) return FMD_ERR_NOMEM;
    h->P = cfg->block; h->target = cfg->target; h->gain_max = cfg->gain_max; h->hang = cfg->hang; h->decay = cfg->decay;
    while ((1u << h->lgP) < h->P) ++h->lgP;
    const uint32_t eb = 2u * width;
    h->ring = fmd_ag::kRingBytes / eb > 2u * h->P ? fmd_ag::kRingBytes / eb : 2u * h->P;
    const uint32_t slots = h->ring >> h->lgP;                // sb + 1
    h->rows.lds = (size_t)h->ring * eb + 4ull * slots + 4ull * (slots + 1u);
    h->rows.width = width; h->rows.n_rows = dev->n_channels; h->rows.hcap = 2u * h->P;   // (at most 2 P - 1 are carried; rows stay 16-byte aligned)
    fmd_ddc_add_pair(h->rows.core, h->state, (size_t)dev->n_channels * 2 * sizeof(int32_t));
    return fmd_rows_device(h, dev, fmd_agc_free, out);
}

void fmd_agc_free(fmd_agc* h) { fmd_rows_free(h); }
int fmd_agc_reset(fmd_agc* h) { return fmd_rows_reset(h); }
int fmd_agc_check(fmd_agc* h) { return fmd_rows_check(h); }

int fmd_agc_outputs(const fmd_agc* h, uint64_t* inputs, uint64_t* outputs)
{
    return fmd_rows_outputs(h, inputs, outputs, [](const fmd_agc* a, uint64_t n) { return agc_blocks(a, n) << a->lgP; });
}

int fmd_agc_gain(fmd_agc* h, uint32_t row, uint32_t* gain, uint32_t* hang)
{
    if (!h || !gain || !hang) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (row >= h->rows.n_rows) { fmd_internal_set_err("row out of range"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->rows.core.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    int32_t st[2] = {0, 0};
    FMD_DDC_TRY(hipMemcpy(st, h->state.in<int32_t>(h->rows.core.cur) + 2 * (size_t)row, sizeof st, hipMemcpyDeviceToHost));
    *gain = h->gain_max - (uint32_t)st[0];
    *hang = (uint32_t)st[1];
    return FMD_OK;
}

int fmd_agc_run_device(fmd_agc* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, void* stream)
{
    return fmd_ddc_run_device(h ? &h->rows.core : nullptr, d_in, d_out,
                              [&] { return agc_enqueue(h, d_in, n_in, in_cap, d_out, out_cap, n_out, static_cast<hipStream_t>(stream)); });
}

// (a call of no samples has nothing to take: it does not touch the device)
int fmd_agc_run_batch(fmd_agc* h, const int16_t* in, size_t n_in, size_t in_cap, int16_t* out, size_t out_cap, size_t* n_out)
{
    return fmd_rows_run_batch(h, agc_enqueue, in, n_in, in_cap, out, out_cap, n_out, [](size_t n) { return n == 0; });
}

int fmd_agc_kernel_name(const fmd_agc* h, char* name, size_t cap) { return fmd_rows_kernel_name(h, name, cap, "fmd_ag::fmd_agc_kernel<%u>"); }

}  // extern "C"
