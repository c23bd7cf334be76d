// fmd_narrow.hip -- narrow-band bank: K narrow channels per wideband IQ stream, each through a second, complex decimating FIR and
// one of four detectors (IQ, NFM, AM, SSB) with a block-wise squelch, in two gfx950 kernels per call.  The project's own operator
// (like the stereo bank), not the reference's chain.
//
// Definition (include/fmd.h, "narrow-band bank"; tests/narrow_ref.py): the channelizer's y, v[n] = sum_t g[t] y[R n + t] with
// complex taps g, u = v >> chan_shift per component, a = isqrt(|u|^2), the block sums E_j = sum |u|^2 and A_j = sum a over blocks
// of P audio samples, and per sample the detector's value, the gain and the squelch decided by block j - 1.
//
// Pass 1 (fmd_narrow_ddc_kernel): the channelizer's tile -- the fmd_ddc.h front end (staging, contraction on
//   v_mfma_i32_16x16x64_i8, rotation into LDS rows) over all K stations of one stream; y leaves as packed re | im << 16 dwords
//   into a buffer the handle owns, rows padded to 16 bytes so that every store is a dwordx4.
// Pass 2 (fmd_narrow_chan_kernel<complex taps>): one workgroup = one (stream, station) row; it walks the row's tiles of up to 256
//   audio samples IN ORDER, so the sums of block j - 1 are always complete when a sample of block j is written: no third pass,
//   no atomics, no intermediate u buffer.  Per tile:
//   1. y (history first) into LDS, unpacked to (yr, yi) and in POLYPHASE order: sample i of the tile at [i % R][i / R].  Lane l
//      (audio sample l of the tile) then reads, for tap t = R q + r, the cell [r][l + q]: consecutive lanes read consecutive
//      8-byte cells for every R, which is free of bank conflicts (a stride-R layout is not, for even R);
//   2. the FIR with v_mad_i32_i24, the taps in the same polyphase order ([R][Q], Q = ceil(Ta / R) rounded up to a multiple of
//      4, zero padded) read through the scalar cache (their address is wave-uniform; four taps per s_load_dwordx8), so a tap
//      step is ONE ds_read_b64 and two (real taps) or four multiply-adds;
//      the shift, the exact integer square root (v_sqrt_f32 estimate, integer correction);
//   3. the tile's block sums, one wave per block, wave reduction; thread 0 then steps the (at most 17) blocks of the tile through
//      the squelch state;
//   4. the detector, the gain, the squelch; int16 stores (a dword per sample in IQ mode).
//   After the last tile: the next call's y history and the row's carry (partial sums, last block's estimates, u[n - 1]).
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_chan_stage.h"
#include "fmd_ddc.h"
#include "fmd_device.h"
#include "fmd_internal.h"

namespace fmd_nb {

using fmd_ddc::kThreads;
using fmd_ddc::kTableBytes;
using fmd_chan::kCarry;                                   // u64 per row: E part, A part, E last, u[n - 1], dc, open
using fmd_chan::isqrt29;
using fmd_chan::wave_sum64;

constexpr uint32_t kTile = 256;                           // audio samples per pass-2 tile (at most)
constexpr uint32_t kYCap = 6144;                          // (yr, yi) cells a pass-2 tile stages: R pitch <= kYCap
constexpr uint32_t kMaxBlk = kTile / 16 + 2;              // blocks one tile touches (<= 17: P >= 16)

struct DdcLaunch {
    const uint8_t* iq;         // [S][nbytes]
    uint64_t nbytes;
    const uint8_t* hist_in;    // [S][HB]
    uint8_t* hist_out;
    uint32_t HB;
    uint32_t vb_first;         // virtual byte (history ++ call) of the window of the call's first output
    uint32_t m0_lo;            // global index of the call's first output, mod 2^32
    uint32_t M;                // outputs of this call per (stream, station)
    uint32_t D, T, K, S, shift;
    uint32_t nrt, nkc, digits;
    uint32_t tile, ntiles, raw_bytes;
    const uint32_t* amat;
    const int32_t* kconst;
    const uint32_t* dinc;
    const uint32_t* tab;
    uint32_t* y;               // [S K][ystride] packed (yr, yi); ystride % 4 == 0, 16-byte aligned
    uint32_t ystride;
};

__global__ void __launch_bounds__(kThreads) fmd_narrow_ddc_kernel(const DdcLaunch L)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t s = blockIdx.y, t = blockIdx.x;
    if (s >= L.S || t >= L.ntiles) return;

    const uint32_t o0 = t * L.tile;                          // first output (of this call) of the tile
    const uint32_t no = L.M - o0 < L.tile ? L.M - o0 : L.tile;
    const uint32_t vb = L.vb_first + 2u * L.D * o0;
    const uint32_t base = vb & ~15u, d0 = vb - base;
    const uint32_t nq = (d0 + 2u * L.D * (no - 1u) + 2u * L.T + 15u) >> 4;   // <= raw_bytes / 16: host plan
    int16_t* const tab = reinterpret_cast<int16_t*>(lds + (L.raw_bytes >> 2));
    uint32_t* const ypk = lds + ((L.raw_bytes + kTableBytes) >> 2);          // [K][tile]

    fmd_ddc::stage(L, s, base, nq, lds, tab, tid, wave);
    if (t == L.ntiles - 1u) fmd_ddc::write_history(L, s, tid);
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0): the LDS-DMAs have landed
    __syncthreads();

    fmd_ddc::contract(L, s, wave, lane, d0, no, L.m0_lo + o0, lds, tab, ypk, L.tile, 0u);
    __syncthreads();

    // whole dwordx4 stores: o0 % 4 == 0 and the rows are padded to a multiple of 4 (the padding takes whatever the LDS row holds)
    typedef FMD_DDC_GLOBAL fmd_ddc::i4* gqo;
    const uint32_t n4 = (no + 3u) >> 2;
    for (uint32_t idx = tid; idx < L.K * n4; idx += kThreads) {
        const uint32_t k = idx / n4, i = idx - k * n4;
        ((gqo)(uintptr_t)(L.y + ((uint64_t)s * L.K + k) * L.ystride + o0))[i] = reinterpret_cast<const fmd_ddc::i4*>(ypk + k * L.tile)[i];
    }
}

struct ChanLaunch {
    const uint32_t* y;         // [S K][ystride]: the call's y
    uint32_t ystride, M;
    const uint32_t* yh_in;     // [S K][HXS]: y of the HX samples before the call
    uint32_t* yh_out;
    uint32_t HX, HXS;          // Ta - 1, row stride (>= 1)
    const unsigned long long* carry_in;   // [S K][kCarry]
    unsigned long long* carry_out;
    uint32_t SK;
    int32_t yoff0;             // R nS - mS: the first window of the call, relative to the call's first y (> -Ta)
    uint64_t nS;               // audio samples before the call
    uint32_t NA, na, ntiles;   // audio samples of the call, per tile, tiles per row
    uint32_t R, Q, rinv, pitch, Ta;   // Q = ceil(Ta / R) rounded up to a multiple of 4; rinv = ceil(2^32 / R) (R >= 2); LDS row pitch (odd)
    uint32_t chan_shift, pshift, mode, gain;
    uint64_t thr;              // squelch^2 P (0: always open)
    const int2* g;             // [R][Q] (gr, gi), polyphase order, zero padded (32-byte aligned rows)
    int16_t* out;              // [S K][out_cap][width]
    uint64_t out_cap;
};

// acc + g y with 24-bit operands; the tap g is wave-uniform (an SGPR)
__device__ __forceinline__ int mad24(int g, int y, int acc)
{
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "s"(g), "v"(y), "v"(acc));
    return r;
}

// one tap (gr + j gi) on one sample: four real multiply-adds, two when the taps are real
template <bool CPLX>
__device__ __forceinline__ void fir_step(int gr, int gi, int2 y, int& vr, int& vi)
{
    vr = mad24(gr, y.x, vr);
    vi = mad24(gr, y.y, vi);
    if (CPLX) {
        vr = mad24(-gi, y.y, vr);                            // (the negation is scalar)
        vi = mad24(gi, y.x, vi);
    }
}

typedef int tap4 __attribute__((ext_vector_type(8)));       // four (gr, gi) taps
typedef const __attribute__((address_space(4))) tap4* ctap4;

template <bool CPLX>
__global__ void __launch_bounds__(kThreads) fmd_narrow_chan_kernel(const ChanLaunch L)
{
    __shared__ __attribute__((aligned(16))) int2 ys[kYCap];
    __shared__ uint32_t ub[kTile + 1];                       // u packed; ub[0] = u of the sample before the tile
    __shared__ uint32_t ab[kTile];                           // a
    __shared__ unsigned long long bE[kMaxBlk];               // the tile's share of each block's sums
    __shared__ uint32_t bA[kMaxBlk];
    __shared__ uint32_t est[kMaxBlk][2];                     // open, dc of the block BEFORE block jlo + i
    __shared__ unsigned long long st[kCarry];                // the row's running carry
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t row = blockIdx.x;
    if (row >= L.SK) return;

    typedef const __attribute__((address_space(4))) int2* ctaps;             // wave-uniform reads: the scalar cache
    const ctaps g = (ctaps)(uintptr_t)L.g;
    const uint32_t* const yrow = L.y + (uint64_t)row * L.ystride;
    const uint32_t* const hin = L.yh_in + (uint64_t)row * L.HXS;
    if (tid < kCarry) st[tid] = L.carry_in[(uint64_t)row * kCarry + tid];
    __syncthreads();
    if (tid == 0u) ub[0] = (uint32_t)st[3];

    for (uint32_t t = 0; t < L.ntiles; ++t) {
        const uint32_t na0 = t * L.na;                       // first audio sample (of this call) of the tile
        const uint32_t cnt = L.NA - na0 < L.na ? L.NA - na0 : L.na;
        const int rel0 = L.yoff0 + (int)(L.R * na0);         // the tile's first y, relative to the call's first
        const uint32_t nsamp = L.R * (cnt - 1u) + L.Ta;      // <= R pitch: host plan

        // ---- 1. y into LDS, polyphase ---------------------------------------------------------------------------------------
        for (uint32_t i = tid; i < nsamp; i += kThreads) {
            const int rel = rel0 + (int)i;
            const uint32_t p = rel < 0 ? hin[(int)L.HX + rel] : yrow[rel];
            const uint32_t c = L.R == 1u ? i : __umulhi(i, L.rinv);
            const uint32_t r = i - c * L.R;
            ys[r * L.pitch + c] = int2{(int)(int16_t)(p & 0xFFFFu), (int)p >> 16};
        }
        __syncthreads();

        // ---- 2. FIR, shift, magnitude ---------------------------------------------------------------------------------------
        if (tid < cnt) {
            int vr = 0, vi = 0;
            const int2* w = ys + tid;
            ctaps gp = g;
            for (uint32_t r = 0; r < L.R; ++r) {
#pragma unroll 2
                for (uint32_t q = 0; q < L.Q; q += 4u) {     // Q % 4 == 0: four taps per s_load_dwordx8
                    const tap4 gv = *reinterpret_cast<ctap4>(gp + q);
                    const int2 y0 = w[q], y1 = w[q + 1u], y2 = w[q + 2u], y3 = w[q + 3u];
                    fir_step<CPLX>(gv.s0, gv.s1, y0, vr, vi);
                    fir_step<CPLX>(gv.s2, gv.s3, y1, vr, vi);
                    fir_step<CPLX>(gv.s4, gv.s5, y2, vr, vi);
                    fir_step<CPLX>(gv.s6, gv.s7, y3, vr, vi);
                }
                w += L.pitch;
                gp += L.Q;
            }
            const int ur = vr >> L.chan_shift, ui = vi >> L.chan_shift;
            ub[tid + 1u] = ((uint32_t)ur & 0xFFFFu) | ((uint32_t)ui << 16);
            ab[tid] = isqrt29((uint32_t)(ur * ur + ui * ui));
        }
        __syncthreads();

        // ---- 3. block sums and the squelch state ----------------------------------------------------------------------------
        const uint64_t N0 = L.nS + na0;
        const uint64_t jlo = N0 >> L.pshift;
        const uint32_t nblk = (uint32_t)(((N0 + cnt - 1u) >> L.pshift) - jlo) + 1u;   // <= kMaxBlk
        for (uint32_t b = wave; b < nblk; b += 4u) {
            const uint64_t bs = (jlo + b) << L.pshift, be = bs + (1ull << L.pshift);
            const uint32_t i0 = bs > N0 ? (uint32_t)(bs - N0) : 0u;
            const uint32_t i1 = be < N0 + cnt ? (uint32_t)(be - N0) : cnt;
            unsigned long long se = 0;
            uint32_t sa = 0;
            for (uint32_t i = i0 + lane; i < i1; i += 64u) {
                const uint32_t p = ub[i + 1u];
                const int ur = (int16_t)(p & 0xFFFFu), ui = (int)p >> 16;
                se += (uint32_t)(ur * ur + ui * ui);
                sa += ab[i];
            }
            se = wave_sum64(se);
            sa = (uint32_t)wave_sum64(sa);
            if (lane == 0u) { bE[b] = se; bA[b] = sa; }
        }
        __syncthreads();
        if (tid == 0u) {
            unsigned long long E = st[0], A = st[1], Elast = st[2], dc = st[4], open = st[5];
            for (uint32_t b = 0; b < nblk; ++b) {
                est[b][0] = (L.thr == 0u || open) ? 1u : 0u;
                est[b][1] = (uint32_t)dc;
                E += bE[b]; A += bA[b];
                if (((jlo + b + 1u) << L.pshift) <= N0 + cnt) {              // the block is complete
                    open = E >= L.thr ? 1u : 0u;
                    dc = A >> L.pshift;
                    Elast = E;
                    E = 0; A = 0;
                }
            }
            st[0] = E; st[1] = A; st[2] = Elast; st[4] = dc; st[5] = open;
        }
        __syncthreads();

        // ---- 4. detector, gain, squelch -------------------------------------------------------------------------------------
        if (tid < cnt) {
            const uint32_t b = (uint32_t)(((N0 + tid) >> L.pshift) - jlo);
            const bool open = est[b][0] != 0u;
            const uint32_t cur = ub[tid + 1u];
            const uint64_t o = (uint64_t)row * L.out_cap + na0 + tid;
            if (L.mode == FMD_NARROW_IQ) {
                reinterpret_cast<uint32_t*>(L.out)[o] = open ? cur : 0u;
            } else {
                int wv;
                if (L.mode == FMD_NARROW_FM) wv = (int)(int16_t)fmd_dev::disc_nosel(cur, ub[tid]);
                else if (L.mode == FMD_NARROW_AM) wv = (int)ab[tid] - (int)est[b][1];
                else wv = (int)(int16_t)(cur & 0xFFFFu);
                int v = (wv * (int)L.gain) >> 8;
                v = v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
                L.out[o] = open ? (int16_t)v : (int16_t)0;
            }
        }
        __syncthreads();
        if (tid == 0u) ub[0] = ub[cnt];
    }

    // ---- the next call's state ----------------------------------------------------------------------------------------------
    uint32_t* const hout = L.yh_out + (uint64_t)row * L.HXS;
    for (uint32_t i = tid; i < L.HX; i += kThreads) {        // y of the call's last HX samples: virtual index over history ++ call
        const uint32_t v = L.M + i;
        hout[i] = v < L.HX ? hin[v] : yrow[v - L.HX];
    }
    if (tid == 0u) {
        unsigned long long* const c = L.carry_out + (uint64_t)row * kCarry;
        c[0] = st[0]; c[1] = st[1]; c[2] = st[2]; c[3] = ub[0]; c[4] = st[4]; c[5] = st[5];
    }
}

}  // namespace fmd_nb

struct fmd_narrow {
    FmdDdcBank bank;
    FmdDdcTiling tl;
    fmd_chan::ChanStage cs;                               // d_g: [R][Q] polyphase taps (int2)
    uint32_t Q = 0, na = 0;                               // taps per polyphase row (a multiple of 4), audio samples per pass-2 tile
};

namespace {

int nb_enqueue(fmd_narrow* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream)
{
    FmdDdcBank& b = h->bank;
    FmdDdcCore& c = h->bank.core;
    fmd_chan::ChanCall q;
    if (const int rc = fmd_chan::chan_plan_call(b, h->cs, nbytes, d_iq, d_out, out_cap, q)) return rc;
    const uint64_t nt1 = (q.M + h->tl.tile - 1) / h->tl.tile, nt2 = (q.NA + h->na - 1) / h->na;
    // (cannot happen: the constructor refuses S > 65535 and the call checks bound M)
    if (nt1 > (1u << 30) || b.S > 65535u) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }

    fmd_nb::DdcLaunch A{};
    fmd_ddc_fill_front(A, b, d_iq, nbytes, q.mS);
    A.m0_lo = (uint32_t)q.mS; A.M = (uint32_t)q.M;
    A.tile = h->tl.tile; A.ntiles = (uint32_t)nt1; A.raw_bytes = h->tl.raw_bytes;
    A.y = static_cast<uint32_t*>(h->cs.d_y); A.ystride = (uint32_t)q.ystride;

    fmd_nb::ChanLaunch B{};
    fmd_chan::chan_fill(B, b, h->cs, q, d_out, out_cap);
    B.na = h->na; B.ntiles = (uint32_t)nt2; B.Q = h->Q;

    FMD_DDC_TRY(c.order.before(stream));
    hipLaunchKernelGGL(fmd_nb::fmd_narrow_ddc_kernel, dim3(A.ntiles, b.S), dim3(fmd_nb::kThreads), h->tl.lds, stream, A);
    FMD_DDC_TRY(hipGetLastError());
    if (h->cs.cplx) hipLaunchKernelGGL(fmd_nb::fmd_narrow_chan_kernel<true>, dim3(B.SK), dim3(fmd_nb::kThreads), 0, stream, B);
    else hipLaunchKernelGGL(fmd_nb::fmd_narrow_chan_kernel<false>, dim3(B.SK), dim3(fmd_nb::kThreads), 0, stream, B);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(c, stream, q.ns);
    if (out_len) *out_len = (size_t)q.NA;
    return FMD_OK;
}

}  // namespace

extern "C" {

size_t fmd_narrow_out_cap(uint32_t decim, uint32_t chan_decim, size_t nbytes) { return fmd_ddc_fir_out_cap(decim, chan_decim, nbytes); }

uint32_t fmd_narrow_out_width(uint32_t mode) { return mode == FMD_NARROW_IQ ? 2u : 1u; }

int fmd_narrow_new(const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc,
                   uint32_t n_stations, const int16_t* chan_taps_re, const int16_t* chan_taps_im, uint32_t n_chan_taps,
                   const fmd_narrow_config* cfg, const fmd_device_config* dev, fmd_narrow** out)
{
    if (!taps || !phase_inc || !chan_taps_re || !cfg || !dev || !out || dev->n_channels == 0) {
        fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    if (const int rc = fmd_ddc_front_args(taps, n_taps, decim, shift, n_stations, dev)) return rc;
    const uint32_t R = cfg->chan_decim, Ta = n_chan_taps;
    uint64_t gsum = 0;
    bool cplx = false;
    if (const int rc = fmd_chan::chan_args(cfg, chan_taps_re, chan_taps_im, Ta, 32u, 256u, &gsum, &cplx)) return rc;
    fmd_narrow* h = new (std::nothrow) fmd_narrow();
    if (!h) return FMD_ERR_NOMEM;
    uint64_t bound;
    if (const int rc = fmd_ddc_bank_front(h->bank, taps, n_taps, decim, shift, phase_inc, n_stations, dev, &bound)) { delete h; return rc; }
    if (const int rc = fmd_chan::chan_gain_ok(bound, gsum, cfg->chan_shift)) { delete h; return rc; }
    h->tl = fmd_ddc_tiling(decim, h->bank.plan.nkc, n_taps, n_stations);
    fmd_chan::chan_init(h->bank, h->cs, cfg, Ta, cplx);
    h->Q = ((Ta + R - 1u) / R + 3u) & ~3u;
    const uint32_t pmax = (fmd_nb::kYCap / R - 1u) | 1u;  // the largest odd pitch with R pitch <= kYCap (>= 191)
    const uint32_t na = pmax - h->Q;                      // >= 183
    h->na = na < fmd_nb::kTile ? na : fmd_nb::kTile;
    h->cs.pitch = (h->na + h->Q) | 1u;                    // <= pmax

    std::vector<int2> gp((size_t)R * h->Q, int2{0, 0});
    for (uint32_t t = 0; t < Ta; ++t) gp[(size_t)(t % R) * h->Q + t / R] = int2{chan_taps_re[t], chan_taps_im ? chan_taps_im[t] : 0};
    fmd_ddc_add_owned(h->bank.core, h->cs.d_g, gp.data(), gp.size() * sizeof(int2));
    const char* what;
    if (const int rc = fmd_ddc_bank_device(h->bank, dev, &what)) {
        if (!what) { delete h; return rc; }
        fmd_internal_set_err(what); fmd_narrow_free(h); return rc;
    }
    *out = h;
    return FMD_OK;
}

void fmd_narrow_free(fmd_narrow* h)
{
    if (!h) return;
    fmd_ddc_free(h->bank.core);
    delete h;
}

int fmd_narrow_reset(fmd_narrow* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_reset(h->bank.core);
}

int fmd_narrow_run_device(fmd_narrow* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, void* stream)
{
    return fmd_ddc_run_device(h ? &h->bank.core : nullptr, d_iq, d_out,
                              [&] { return nb_enqueue(h, d_iq, nbytes, d_out, out_cap, out_len, static_cast<hipStream_t>(stream)); });
}

int fmd_narrow_check(fmd_narrow* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_check(h->bank.core);
}

int fmd_narrow_run_batch(fmd_narrow* h, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!h || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    const size_t out_bytes = out_cap * h->bank.S * h->bank.K * h->cs.width * sizeof(int16_t);
    return fmd_ddc_run_batch(h->bank, iq, nbytes, out, out_bytes, out_cap, out_len, [h](auto... a) { return nb_enqueue(h, a...); });
}

int fmd_narrow_outputs(const fmd_narrow* h, uint64_t* outputs)
{
    if (!h || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *outputs = fmd_chan::chan_audio(h->bank, h->cs, h->bank.core.pos);
    return FMD_OK;
}

int fmd_narrow_level(fmd_narrow* h, uint32_t stream, uint32_t station, int* open, uint32_t* rms)
{
    if (!h || !open || !rms) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (stream >= h->bank.S || station >= h->bank.K) { fmd_internal_set_err("stream or station out of range"); return FMD_ERR_INVALID_ARG; }
    return fmd_chan::chan_levels(h->bank, h->cs, (size_t)stream * h->bank.K + station, 1, open, rms);
}

int fmd_narrow_kernel_name(const fmd_narrow* h, uint32_t pass, char* name, size_t cap)
{
    if (!h || !name || cap == 0 || pass > 1) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, pass == 0 ? "fmd_nb::fmd_narrow_ddc_kernel" :
                                    (h->cs.cplx ? "fmd_nb::fmd_narrow_chan_kernel<true>" : "fmd_nb::fmd_narrow_chan_kernel<false>")), cap);
}

}  // extern "C"
