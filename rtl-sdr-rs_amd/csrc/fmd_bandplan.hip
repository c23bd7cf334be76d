// fmd_bandplan.hip -- band-plan bank: the audio (AM, NFM, SSB) or the narrowed IQ of EVERY channel of a band plan, with a block-wise
// squelch and an activity map, in two gfx950 kernels per call.  The project's own operator: the composition of the uniform
// channelizer (fmd_uniform.hip) and the narrow-band bank's second stage (fmd_narrow.hip), with no new arithmetic.
//
// Definition (include/fmd.h, "band-plan bank"; tests/bandplan_ref.py): y[k][m] exactly the uniform channelizer's, then exactly the
// narrow-band bank's v, u, a, E_j, A_j, open_j, dc_j, w and out over that y.
//
// Pass 1: the uniform channelizer's kernel, unchanged -- the handle owns an fmd_uniform and enqueues it through
//   fmd_uniform_run_device on the caller's stream, into a y buffer of packed re | im << 16 dwords that the handle owns.
// Pass 2 (fmd_bp::fmd_bandplan_chan_kernel<complex taps>): ONE WAVE = one (stream, channel) row (a workgroup is one wave).  A band
//   plan has 10^4 ... 10^5 rows of a few hundred audio samples each, so the rows alone fill the chip; a row's tiles have to be walked
//   in order (sample n of block j needs the sums of block j - 1), and a wave that owns its row does that without one s_barrier:
//   every hand-over through LDS is wave-local.  Per tile of up to kTile = 256 audio samples, FOUR per lane (l, l + 64, l + 128,
//   l + 192):
//   1. y (history first) into LDS as it is -- the packed dword IS the v_dot2 operand -- in POLYPHASE order: sample i of the tile at
//      [i % R][i / R].  For tap t = R q + r the lane reads the cells [r][l + 64 j + q]: consecutive lanes read consecutive dwords
//      for every R in 1 ... 8, which is free of bank conflicts;
//   2. the FIR with v_dot2c_i32_i16 on the packed (yr, yi): the host packs every tap as the pair of operands (gr, -gi) and
//      (gi, gr), so vr += dot2(y, A) and vi += dot2(y, B) -- two instructions per complex tap.  Real taps take the same two
//      instructions with A = (g, 0) and B = (0, g) = A << 16, one dword per tap in memory.  The taps come through the scalar cache
//      (their address is wave-uniform), eight dwords per load -- four complex taps or eight real ones -- and the NEXT chunk's load
//      is issued before the current chunk's multiply-adds; a loaded tap serves the lane's four samples;
//      then the shift, the exact integer square root, |u|^2;
//   3. the tile's blocks in order, the sums from the lanes' registers (a lane's four samples, then one wave reduction of the pair
//      (E, A) packed into 64 bits), the squelch state stepped in registers;
//   4. the detector, the gain, the squelch.  IQ mode stores a dword per sample.  The other modes put their int16 into LDS at the
//      parity of their global address and leave as dwords; only a row's odd first or last sample is a 2-byte store.
//   After the last tile: the next call's y history and the row's carry (partial sums, last block's estimates, u[n - 1]), both
//   double-buffered through FmdDdcCore.
//
// Host side: the second stage's checks, state, call plan, launch fields and level report are fmd_chan_stage.h's, shared with the
// narrow-band bank; stage one's domain and gain bound are decided by the uniform channelizer's own constructor steps
// (fmd_ddc.h).  This file keeps the kernel, its tap layout and the order of the two.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_chan_stage.h"
#include "fmd_ddc.h"
#include "fmd_device.h"
#include "fmd_internal.h"

namespace fmd_bp {

using fmd_chan::kCarry;                                   // u64 per row: E part, A part, E last, u[n - 1], dc, open
using fmd_chan::isqrt29;
using fmd_chan::wave_sum64;

constexpr uint32_t kWave = 64;                            // threads of a workgroup: one wave, one row
constexpr uint32_t kPer = 4;                              // audio samples per lane and tile
constexpr uint32_t kTile = kWave * kPer;                  // audio samples per tile (at most)
constexpr uint32_t kMaxR = 8, kMaxTa = 64;
constexpr uint32_t kYCap = 2176;                          // y dwords a tile stages: R pitch <= kYCap (fmd_bandplan_new)

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
    uint32_t NA, ntiles;       // audio samples of the call, tiles per row
    uint32_t R, cpr, rinv, pitch, Ta;   // cpr: eight-dword tap chunks per polyphase row; rinv = ceil(2^32 / R) (R >= 2); LDS row pitch (odd)
    uint32_t chan_shift, pshift, mode, gain;
    uint64_t thr;              // squelch^2 P (0: always open)
    const uint32_t* g;         // [R][cpr][8] tap operands, polyphase order, zero padded (32-byte aligned)
    int16_t* out;              // [S K][out_cap][width]
    uint64_t out_cap;
};

typedef short s2 __attribute__((ext_vector_type(2)));

// acc + y.lo g.lo + y.hi g.hi (v_dot2c_i32_i16): every operand fits 16 bits and every partial sum 31, so no clamp
__device__ __forceinline__ int dot2(uint32_t y, uint32_t g, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s2, y), __builtin_bit_cast(s2, g), acc, false);
}

typedef uint32_t tap8 __attribute__((ext_vector_type(8)));  // four complex taps (A, B pairs) or eight real ones (A)
typedef const __attribute__((address_space(4))) tap8* ctap8;

// one chunk of taps on the lane's kPer samples; w: the lane's cell of the chunk's first tap
template <bool CPLX>
__device__ __forceinline__ void fir_chunk(const tap8 g, const uint32_t* w, int (&vr)[kPer], int (&vi)[kPer])
{
    constexpr uint32_t n = CPLX ? 4u : 8u;
    uint32_t yv[n][kPer];
#pragma unroll
    for (uint32_t k = 0; k < n; ++k)
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) yv[k][j] = w[k + kWave * j];
#pragma unroll
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t A = CPLX ? g[2u * k] : g[k];
        const uint32_t B = CPLX ? g[2u * k + 1u] : g[k] << 16;   // (a scalar shift)
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            vr[j] = dot2(yv[k][j], A, vr[j]);
            vi[j] = dot2(yv[k][j], B, vi[j]);
        }
    }
}

template <bool CPLX>
__global__ void __launch_bounds__(kWave) fmd_bandplan_chan_kernel(const ChanLaunch L)
{
    __shared__ uint32_t ys[kYCap];
    __shared__ uint32_t ub[kTile + 1];                       // u packed; ub[0] = u of the sample before the tile
    __shared__ __attribute__((aligned(4))) int16_t ob[kTile + 2];   // the tile's int16 outputs, at the parity of their address
    const uint32_t lane = threadIdx.x;
    const uint32_t row = blockIdx.x;
    if (row >= L.SK) return;

    const ctap8 g = (ctap8)(uintptr_t)L.g;
    const uint32_t* const yrow = L.y + (uint64_t)row * L.ystride;
    const uint32_t* const hin = L.yh_in + (uint64_t)row * L.HXS;
    const unsigned long long* const cin = L.carry_in + (uint64_t)row * kCarry;
    unsigned long long E = cin[0], A = cin[1], Elast = cin[2], dc = cin[4], open = cin[5];   // the row's running carry, in every lane
    if (lane == 0u) ub[0] = (uint32_t)cin[3];
    const uint32_t nchunks = L.R * L.cpr;
    const uint32_t qp = L.cpr * (CPLX ? 4u : 8u);            // taps per polyphase row, padded

    for (uint32_t t = 0; t < L.ntiles; ++t) {
        const uint32_t na0 = t * kTile;                      // first audio sample (of this call) of the tile
        const uint32_t cnt = L.NA - na0 < kTile ? L.NA - na0 : kTile;
        const int rel0 = L.yoff0 + (int)(L.R * na0);         // the tile's first y, relative to the call's first
        const uint32_t nsamp = L.R * (cnt - 1u) + L.Ta;      // <= R pitch: host plan

        // ---- 1. y into LDS, polyphase -------------------------------------------------------------------------------------------
#pragma unroll 4
        for (uint32_t i = lane; i < nsamp; i += kWave) {
            const int rel = rel0 + (int)i;
            const uint32_t p = rel < 0 ? hin[(int)L.HX + rel] : yrow[rel];
            const uint32_t c = L.R == 1u ? i : __umulhi(i, L.rinv);
            const uint32_t r = i - c * L.R;
            ys[r * L.pitch + c] = p;
        }
        __syncthreads();                                     // (one wave: no s_barrier, the LDS writes are waited for)

        // ---- 2. FIR, shift, magnitude -------------------------------------------------------------------------------------------
        int vr[kPer], vi[kPer];
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) { vr[j] = 0; vi[j] = 0; }
        {
            const uint32_t* w = ys + lane;
            tap8 cur = g[0];
            uint32_t qc = 0;
            for (uint32_t c = 0; c < nchunks; ++c) {
                const tap8 nxt = g[c + 1u < nchunks ? c + 1u : c];   // ahead of this chunk's multiply-adds
                fir_chunk<CPLX>(cur, w, vr, vi);
                cur = nxt;
                w += CPLX ? 4u : 8u;
                if (++qc == L.cpr) { qc = 0; w += L.pitch - qp; }
            }
        }
        uint32_t up[kPer], av[kPer], ev[kPer];
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) {
            const int ur = vr[j] >> L.chan_shift, ui = vi[j] >> L.chan_shift;
            up[j] = ((uint32_t)ur & 0xFFFFu) | ((uint32_t)ui << 16);
            ev[j] = (uint32_t)(ur * ur + ui * ui);
            av[j] = isqrt29(ev[j]);
            ub[1u + lane + kWave * j] = up[j];               // (lanes past cnt write their own cell: never read)
        }
        __syncthreads();

        // ---- 3. block sums and the squelch state, block by block ----------------------------------------------------------------
        const uint64_t N0 = L.nS + na0;
        const uint64_t jlo = N0 >> L.pshift;
        const uint32_t nblk = (uint32_t)(((N0 + cnt - 1u) >> L.pshift) - jlo) + 1u;
        bool opn[kPer];
        int dcv[kPer];
#pragma unroll
        for (uint32_t j = 0; j < kPer; ++j) { opn[j] = false; dcv[j] = 0; }
        for (uint32_t b = 0; b < nblk; ++b) {
            const uint64_t bs = (jlo + b) << L.pshift, be = bs + (1ull << L.pshift);
            const uint32_t i0 = bs > N0 ? (uint32_t)(bs - N0) : 0u;
            const uint32_t i1 = be < N0 + cnt ? (uint32_t)(be - N0) : cnt;
            const bool open_now = L.thr == 0u || open != 0u;
            uint32_t se = 0, sa = 0;                          // <= 4 2^29 and 4 23170
#pragma unroll
            for (uint32_t j = 0; j < kPer; ++j) {
                const uint32_t n = lane + kWave * j;
                if (n >= i0 && n < i1) { se += ev[j]; sa += av[j]; opn[j] = open_now; dcv[j] = (int)dc; }
            }
            // (E, A) of the wave in one reduction: E < 2^37 below bit 40, A < 2^23 above it
            const unsigned long long s = wave_sum64((unsigned long long)se | ((unsigned long long)sa << 40));
            E += s & ((1ull << 40) - 1ull);
            A += s >> 40;
            if (((jlo + b + 1u) << L.pshift) <= N0 + cnt) {  // the block is complete
                open = E >= L.thr ? 1u : 0u;
                dc = A >> L.pshift;
                Elast = E;
                E = 0; A = 0;
            }
        }

        // ---- 4. detector, gain, squelch -----------------------------------------------------------------------------------------
        const uint64_t o0 = (uint64_t)row * L.out_cap + na0;     // the tile's first output of the row
        if (L.mode == FMD_NARROW_IQ) {
#pragma unroll
            for (uint32_t j = 0; j < kPer; ++j) {
                const uint32_t n = lane + kWave * j;
                if (n < cnt) reinterpret_cast<uint32_t*>(L.out)[o0 + n] = opn[j] ? up[j] : 0u;
            }
            __syncthreads();
        } else {
            const uint32_t par = (uint32_t)((uintptr_t)(L.out + o0) >> 1) & 1u;
#pragma unroll
            for (uint32_t j = 0; j < kPer; ++j) {
                const uint32_t n = lane + kWave * j;
                int wv;
                if (L.mode == FMD_NARROW_FM) wv = (int)(int16_t)fmd_dev::disc_nosel(up[j], ub[n]);
                else if (L.mode == FMD_NARROW_AM) wv = (int)av[j] - dcv[j];
                else wv = (int)(int16_t)(up[j] & 0xFFFFu);
                int v = (wv * (int)L.gain) >> 8;
                v = v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
                ob[par + n] = opn[j] ? (int16_t)v : (int16_t)0;
            }
            __syncthreads();
            // dword d holds the samples 2 d - par and 2 d - par + 1 of the tile
            const uint32_t nd = (par + cnt + 1u) >> 1;       // <= 129
            for (uint32_t d = lane; d < nd; d += kWave) {
                const int lo = (int)(2u * d) - (int)par;
                const uint32_t pair = reinterpret_cast<const uint32_t*>(ob)[d];
                if (lo >= 0 && (uint32_t)lo + 1u < cnt) *reinterpret_cast<uint32_t*>(L.out + o0 + lo) = pair;
                else if (lo < 0) L.out[o0] = (int16_t)(pair >> 16);                       // the row's odd first sample (cnt >= 1)
                else if ((uint32_t)lo < cnt) L.out[o0 + lo] = (int16_t)(pair & 0xFFFFu);  // ... and its odd last one
            }
        }
        if (lane == 0u) ub[0] = ub[cnt];
        __syncthreads();
    }

    // ---- the next call's state --------------------------------------------------------------------------------------------------
    uint32_t* const hout = L.yh_out + (uint64_t)row * L.HXS;
    for (uint32_t i = lane; i < L.HX; i += kWave) {          // y of the call's last HX samples: virtual index over history ++ call
        const uint32_t v = L.M + i;
        hout[i] = v < L.HX ? hin[v] : yrow[v - L.HX];
    }
    if (lane == 0u) {
        unsigned long long* const c = L.carry_out + (uint64_t)row * kCarry;
        c[0] = E; c[1] = A; c[2] = Elast; c[3] = ub[0]; c[4] = dc; c[5] = open;
    }
}

}  // namespace fmd_bp

struct fmd_bandplan {
    FmdDdcBank bank;                                      // T, D = hop, K = selected channels, S; the core holds pass 2's state
    fmd_uniform* uv = nullptr;                            // pass 1
    fmd_chan::ChanStage cs;                               // d_g: [R][cpr][8] tap operands
    uint32_t cpr = 0;                                     // eight-dword tap chunks per polyphase row
};

namespace {

int bp_enqueue(fmd_bandplan* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream)
{
    FmdDdcBank& b = h->bank;
    FmdDdcCore& c = h->bank.core;
    if (nbytes % (2ull * b.D) != 0) { fmd_internal_set_err("nbytes % (2 hop) != 0"); return FMD_ERR_BAD_LENGTH; }
    fmd_chan::ChanCall q;
    if (const int rc = fmd_chan::chan_plan_call(b, h->cs, nbytes, d_iq, d_out, out_cap, q)) return rc;   // (pass 1 not enqueued)

    fmd_bp::ChanLaunch B{};
    fmd_chan::chan_fill(B, b, h->cs, q, d_out, out_cap);
    B.ntiles = (uint32_t)((q.NA + fmd_bp::kTile - 1) / fmd_bp::kTile); B.cpr = h->cpr;

    FMD_DDC_TRY(c.order.before(stream));
    // pass 1 counts the same samples as this handle, so it completes exactly M outputs; a refusal leaves both handles as they were
    size_t m1 = 0;
    if (const int rc = fmd_uniform_run_device(h->uv, d_iq, nbytes, h->cs.d_y, (size_t)q.ystride, &m1, stream)) return rc;
    if (m1 != q.M) { fmd_internal_set_err("the two passes disagree on the call's outputs"); return FMD_ERR_BAD_STATE; }
    if (h->cs.cplx) hipLaunchKernelGGL(fmd_bp::fmd_bandplan_chan_kernel<true>, dim3(B.SK), dim3(fmd_bp::kWave), 0, stream, B);
    else hipLaunchKernelGGL(fmd_bp::fmd_bandplan_chan_kernel<false>, dim3(B.SK), dim3(fmd_bp::kWave), 0, stream, B);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(c, stream, q.ns);
    if (out_len) *out_len = (size_t)q.NA;
    return FMD_OK;
}

}  // namespace

extern "C" {

size_t fmd_bandplan_out_cap(uint32_t hop, uint32_t chan_decim, size_t nbytes) { return fmd_ddc_fir_out_cap(hop, chan_decim, nbytes); }

int fmd_bandplan_new(const int16_t* taps, uint32_t n_taps, uint32_t n_channels, uint32_t hop, uint32_t shift, const uint32_t* channels,
                     uint32_t n_selected, const int16_t* chan_taps_re, const int16_t* chan_taps_im, uint32_t n_chan_taps,
                     const fmd_narrow_config* cfg, const fmd_device_config* dev, fmd_bandplan** out)
{
    if (!taps || !chan_taps_re || !cfg || !dev || !out || dev->n_channels == 0) {
        fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    // the refusals in this order, all before a device is queried: stage one's domain, stage two's, stage one's gain, stage two's
    if (const int rc = fmd_uniform_args(taps, n_taps, n_channels, hop, shift, channels, n_selected, dev)) return rc;
    const uint32_t R = cfg->chan_decim, Ta = n_chan_taps;
    uint64_t gsum = 0, bound = 0;
    bool cplx = false;
    if (const int rc = fmd_chan::chan_args(cfg, chan_taps_re, chan_taps_im, Ta, fmd_bp::kMaxR, fmd_bp::kMaxTa, &gsum, &cplx)) return rc;
    fmd_bandplan* h = new (std::nothrow) fmd_bandplan();
    if (!h) return FMD_ERR_NOMEM;
    if (const int rc = fmd_uniform_host(taps, n_taps, n_channels, hop, shift, channels, n_selected, dev, &h->uv, &bound)) { delete h; return rc; }
    const auto refuse = [&](int rc) { fmd_uniform_discard(h->uv); delete h; return rc; };
    if (const int rc = fmd_chan::chan_gain_ok(bound, gsum, cfg->chan_shift)) return refuse(rc);

    FmdDdcBank& b = h->bank;                              // (its plan stays empty: the front end is pass 1's, in the uniform handle)
    b.T = n_taps; b.D = hop; b.K = channels ? n_selected : n_channels; b.S = dev->n_channels; b.shift = shift; b.HB = 0;
    fmd_chan::chan_init(b, h->cs, cfg, Ta, cplx);
    const uint32_t tpc = cplx ? 4u : 8u;                  // taps per eight-dword chunk
    h->cpr = ((Ta + R - 1u) / R + tpc - 1u) / tpc;
    // LDS row pitch: a tile's kTile cells and the padded taps' reach, odd (the staging writes of consecutive samples go to R rows)
    h->cs.pitch = (fmd_bp::kTile + h->cpr * tpc) | 1u;
    static_assert((fmd_bp::kMaxR * ((fmd_bp::kTile + 8u + 7u) | 1u)) <= fmd_bp::kYCap, "R = 8 with its 8 (padded: up to 15) taps per row");
    if ((uint64_t)R * h->cs.pitch > fmd_bp::kYCap) {      // (R qp <= Ta + 8 R - 1 < 128: cannot happen inside the domain)
        fmd_internal_set_err("second stage does not fit the tile"); return refuse(FMD_ERR_UNSUPPORTED);
    }

    // [R][cpr][8]: complex taps as the operand pairs A = (gr, -gi), B = (gi, gr); real taps as A = (g, 0) alone
    std::vector<uint32_t> gp((size_t)R * h->cpr * 8u, 0u);
    for (uint32_t t = 0; t < Ta; ++t) {
        const uint32_t r = t % R, q = t / R;
        const uint32_t gr = (uint32_t)(int32_t)chan_taps_re[t] & 0xFFFFu;
        if (cplx) {
            const int32_t gi = chan_taps_im[t];
            const size_t at = ((size_t)r * h->cpr + q / 4u) * 8u + 2u * (q % 4u);
            gp[at] = gr | (((uint32_t)(-gi) & 0xFFFFu) << 16);
            gp[at + 1] = ((uint32_t)gi & 0xFFFFu) | (gr << 16);
        } else {
            gp[((size_t)r * h->cpr + q / 8u) * 8u + q % 8u] = gr;
        }
    }
    fmd_ddc_add_owned(b.core, h->cs.d_g, gp.data(), gp.size() * sizeof(uint32_t));
    if (const int rc = fmd_uniform_device(h->uv, dev)) { delete h; return rc; }
    const char* what;
    if (const int rc = fmd_ddc_bank_device(b, dev, &what)) {
        if (!what) { fmd_uniform_free(h->uv); delete h; return rc; }
        fmd_internal_set_err(what); fmd_bandplan_free(h); return rc;
    }
    *out = h;
    return FMD_OK;
}

void fmd_bandplan_free(fmd_bandplan* h)
{
    if (!h) return;
    fmd_ddc_free(h->bank.core);
    fmd_uniform_free(h->uv);
    delete h;
}

int fmd_bandplan_reset(fmd_bandplan* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    if (const int rc = fmd_uniform_reset(h->uv)) return rc;
    return fmd_ddc_reset(h->bank.core);
}

int fmd_bandplan_run_device(fmd_bandplan* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, void* stream)
{
    return fmd_ddc_run_device(h ? &h->bank.core : nullptr, d_iq, d_out,
                              [&] { return bp_enqueue(h, d_iq, nbytes, d_out, out_cap, out_len, static_cast<hipStream_t>(stream)); });
}

int fmd_bandplan_check(fmd_bandplan* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_check(h->bank.core);                   // (pass 2 is the last launch of a call on its stream)
}

int fmd_bandplan_run_batch(fmd_bandplan* h, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!h || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (nbytes % (2ull * h->bank.D) != 0) { fmd_internal_set_err("nbytes % (2 hop) != 0"); return FMD_ERR_BAD_LENGTH; }
    const size_t out_bytes = out_cap * h->bank.S * h->bank.K * h->cs.width * sizeof(int16_t);
    return fmd_ddc_run_batch(h->bank, iq, nbytes, out, out_bytes, out_cap, out_len, [h](auto... a) { return bp_enqueue(h, a...); });
}

int fmd_bandplan_outputs(const fmd_bandplan* h, uint64_t* outputs)
{
    if (!h || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *outputs = fmd_chan::chan_audio(h->bank, h->cs, h->bank.core.pos);
    return FMD_OK;
}

int fmd_bandplan_levels(fmd_bandplan* h, uint8_t* open, uint32_t* rms)
{
    if (!h || !open || !rms) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_chan::chan_levels(h->bank, h->cs, 0, (size_t)h->bank.S * h->bank.K, open, rms);
}

int fmd_bandplan_kernel_name(const fmd_bandplan* h, uint32_t pass, char* name, size_t cap)
{
    if (!h || !name || cap == 0 || pass > 1) return FMD_ERR_INVALID_ARG;
    if (pass == 0) return fmd_uniform_kernel_name(h->uv, name, cap);
    return fmd_ddc_name_rc(snprintf(name, cap, h->cs.cplx ? "fmd_bp::fmd_bandplan_chan_kernel<true>" : "fmd_bp::fmd_bandplan_chan_kernel<false>"), cap);
}

}  // extern "C"
