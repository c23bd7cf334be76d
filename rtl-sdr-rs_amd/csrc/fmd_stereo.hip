// fmd_stereo.hip -- stereo station bank: pilot-locked L/R audio per FM station, K stations per wideband IQ stream, in two
// gfx950 kernels per call.
//
// Definition (include/fmd.h, "stereo station bank"; tests/stereo_ref.py): the channelizer's y, the reference's integer
// discriminator at the multiplex rate x[m] = (i16) polar_discriminant_fast(y[m], y[m-1]), the pilot's correlations I_j, Q_j per
// block of P samples, the subcarrier kc[m] = 2 sin(2 theta + 2 alpha) in Q14 from the estimate of block j - 1, s = x kc >> 14,
// and one FIR g (stride R) over the sum x and the difference s; L / R = (M +- S) >> (audio_shift + 1), saturated.
//
// Pass 1 (fmd_stereo_mpx_kernel): one workgroup = one tile of up to 64 G - 1 consecutive MPX samples of ONE stream, all K stations:
//   1. - 3. the channelizer's front end (fmd_ddc.h: staging, contraction on v_mfma_i32_16x16x64_i8, rotation into LDS rows), over
//      the tile's outputs AND the output before them (recomputed; the call's first tile takes it from the carried last y);
//   4. one wave per station row: the integer discriminator (fmd_device.h disc_nosel), the pilot products x cosq(theta),
//      x sinq(theta) summed per block (a tile touches at most two: P >= 1024), reduced across the wave and added into the call's
//      block sums with 64-bit integer atomics (exact in any order); x stored as i16.
// Pass 2 (fmd_stereo_audio_kernel): one workgroup = one (stream, station) row and one tile of up to 256 audio samples:
//   1. the estimate (present, c2, s2) of each block the tile's inputs need, one lane per block (i64 / 128-bit arithmetic);
//   2. (x, s) of every MPX sample the tile's FIR reads into LDS: the carried Ta - 1 samples of the previous call from the history,
//      the call's own with s = (x kc) >> 14, kc from the NCO table in LDS;
//   3. one lane per audio sample: both FIRs with v_mad_i32_i24 (|g| <= 16383, |x| <= 32768, |s| <= 65540 fit 24-bit operands), the
//      matrix step, saturation, one dword store of the (L, R) pair.
// The last tile of a row writes the next call's (x, s) history; tile 0 the next call's block carry (the sums of the last
// complete block, the partial sums of a block that straddles calls).
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>

#include "fmd_ddc.h"
#include "fmd_device.h"
#include "fmd_internal.h"
#include "fmd_stereo_mpx.h"

namespace fmd_sto {

using fmd_ddc::kThreads;
using fmd_ddc::kTableBytes;

constexpr uint32_t kAudioTile = 256;                      // audio samples per pass-2 tile (at most)
constexpr uint32_t kXCap = 2048;                          // (x, s) pairs a pass-2 tile stages: R tile + 2 Ta <= kXCap
constexpr uint32_t kMaxBlocks = 4;                        // blocks one pass-2 tile touches (<= 3: kXCap / 1024 + 1)

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(kThreads) fmd_stereo_mpx_kernel(const MpxLaunch L)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t s = blockIdx.y, t = blockIdx.x;
    if (s >= L.S || t >= L.ntiles) return;

    const uint32_t o0 = t * L.tile;                          // first output (of this call) of the tile
    const uint32_t no = L.M - o0 < L.tile ? L.M - o0 : L.tile;
    const uint32_t c0 = t ? o0 - 1u : o0;                    // first output contracted: the one before the tile, except in tile 0
    const uint32_t nc = t ? no + 1u : no;
    const uint32_t vb = L.vb_first + 2u * L.D * c0;
    const uint32_t base = vb & ~15u, d0 = vb - base;
    const uint32_t nq = (d0 + 2u * L.D * (nc - 1u) + 2u * L.T + 15u) >> 4;   // <= raw_bytes / 16: host plan
    int16_t* const tab = reinterpret_cast<int16_t*>(lds + (L.raw_bytes >> 2));
    uint32_t* const ypk = lds + ((L.raw_bytes + kTableBytes) >> 2);          // [K][cols]: y of output o0 - 1 + i at i

    // ---- 1. staging ---------------------------------------------------------------------------------------------------------
    fmd_ddc::stage(L, s, base, nq, lds, tab, tid, wave);
    if (t == L.ntiles - 1u) fmd_ddc::write_history(L, s, tid);
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0): the LDS-DMAs have landed
    __syncthreads();

    // ---- 2./3. contraction, rotation, packing -------------------------------------------------------------------------------
    fmd_ddc::contract(L, s, wave, lane, d0, nc, (uint32_t)L.m0 + c0, lds, tab, ypk, L.cols, t ? 0u : 1u);
    if (t == 0u)
        for (uint32_t k = tid; k < L.K; k += kThreads) ypk[k * L.cols] = L.ylast_in[s * L.K + k];
    __syncthreads();
    if (t == L.ntiles - 1u)
        for (uint32_t k = tid; k < L.K; k += kThreads) L.ylast_out[s * L.K + k] = ypk[k * L.cols + no];

    // ---- 4. discriminator, pilot sums, x --------------------------------------------------------------------------------------
    const uint64_t mt = L.m0 + o0;                           // global index of the tile's first output
    const uint64_t b0 = mt >> L.pshift;
    const uint64_t SK = (uint64_t)L.S * L.K;
    for (uint32_t k = wave; k < L.K; k += 4u) {
        const uint32_t* y = ypk + k * L.cols;
        const uint64_t row = (uint64_t)s * L.K + k;
        int16_t* const xo = L.x + row * L.M + o0;
        long long i0 = 0, q0 = 0, i1 = 0, q1 = 0;
        for (uint32_t o = lane; o < no; o += 64u) {
            const int xv = (int)(int16_t)fmd_dev::disc_nosel(y[o + 1u], y[o]);
            const uint64_t m = mt + o;
            const uint32_t ix = ((uint32_t)m * L.inc_p) >> 22;
            const int pc = xv * (int)tab[ix], ps = xv * (int)tab[(ix - 256u) & 1023u];   // |x tab| <= 2^29
            if ((m >> L.pshift) == b0) { i0 += pc; q0 += ps; } else { i1 += pc; q1 += ps; }
            xo[o] = (int16_t)xv;
        }
        i0 = wave_sum(i0); q0 = wave_sum(q0); i1 = wave_sum(i1); q1 = wave_sum(q1);
        if (lane == 0u) {
            unsigned long long* const p0 = L.sums + ((b0 - L.jfirst) * SK + row) * 2u;
            atomicAdd(p0, (unsigned long long)i0);
            atomicAdd(p0 + 1, (unsigned long long)q0);
            if (((mt + no - 1u) >> L.pshift) != b0) {        // the tile straddles a block edge
                unsigned long long* const p1 = p0 + 2u * SK;
                atomicAdd(p1, (unsigned long long)i1);
                atomicAdd(p1 + 1, (unsigned long long)q1);
            }
        }
    }
}

hipError_t launch_mpx(const MpxLaunch& A, size_t lds, hipStream_t stream)
{
    hipLaunchKernelGGL(fmd_stereo_mpx_kernel, dim3(A.ntiles, A.S), dim3(kThreads), lds, stream, A);
    return hipGetLastError();
}

struct AudioLaunch {
    const int16_t* x;          // [S K][M]
    uint32_t M;
    const int32_t* xh_in;      // [S K][HXS][2]: (x, s) of the HX samples before the call
    int32_t* xh_out;
    uint32_t HX, HXS;          // Ta - 1, row stride (>= 1)
    const long long* sums;     // [nbc][S K][2]
    const long long* carry_in; // [S K][4]: I, Q of block jfirst - 1; partial I, Q of block jfirst from earlier calls
    long long* carry_out;
    uint32_t SK;
    uint64_t mS, mE, jfirst;   // MPX samples before / after the call, block of mS
    uint64_t nS;               // audio samples before the call
    uint32_t NA, na, ntiles;   // audio samples of the call, per tile, tiles per row
    uint32_t R, Ta, audio_shift;
    uint32_t pshift, inc_p;
    uint64_t thr;              // pilot_min P 8192 (0: every block absent)
    const int16_t* g;
    const uint32_t* tab;
    uint32_t* out;             // [S K][out_stride] (L, R) pairs
    uint64_t out_stride;
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

__global__ void __launch_bounds__(kThreads) fmd_stereo_audio_kernel(const AudioLaunch L)
{
    __shared__ __attribute__((aligned(16))) int2 xs[kXCap];
    __shared__ int32_t gl[256];
    __shared__ int16_t tab[1024];
    __shared__ int32_t est[kMaxBlocks][3];                   // present, c2, s2 of block jA - 1 + i
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / L.ntiles, t = blockIdx.x - row * L.ntiles;
    if (row >= L.SK) return;

    const uint32_t na0 = t * L.na;                           // first audio sample (of this call) of the tile
    const uint32_t cnt = L.NA - na0 < L.na ? L.NA - na0 : L.na;
    const bool last = t == L.ntiles - 1u;
    // virtual index v: MPX sample mS - HX + v (v < HX: the carried history)
    const uint32_t vfir = (uint32_t)(L.R * (L.nS + na0) + L.HX - L.mS);      // the tile's first FIR window
    const uint32_t vtot = L.HX + L.M;
    uint32_t vlo = vfir, vhi = vfir + L.R * (cnt - 1u) + L.Ta;
    if (last) { vlo = vlo < L.M ? vlo : L.M; vhi = vtot; }   // the last tile also forms the next call's history
    const uint32_t span = vhi - vlo;                         // <= kXCap: host plan
    const uint32_t va = vlo > L.HX ? vlo : L.HX;             // first virtual index of the call's own samples
    const uint64_t jA = (L.mS + (va - L.HX)) >> L.pshift;

    // ---- 1. block estimates, the NCO table, the taps ------------------------------------------------------------------------
    if (va < vhi && tid < kMaxBlocks) {
        const uint64_t jB = (L.mS + (vhi - 1u - L.HX)) >> L.pshift;
        if (jA + tid <= jB) {
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
    }
    for (uint32_t i = tid; i < 512u; i += kThreads) reinterpret_cast<uint32_t*>(tab)[i] = L.tab[i];
    for (uint32_t i = tid; i < L.Ta; i += kThreads) gl[i] = L.g[i];
    __syncthreads();

    // ---- 2. (x, s) of the tile's samples ------------------------------------------------------------------------------------
    const int16_t* const xr = L.x + (uint64_t)row * L.M;
    const int32_t* const hin = L.xh_in + (uint64_t)row * L.HXS * 2u;
    for (uint32_t i = tid; i < span; i += kThreads) {
        const uint32_t v = vlo + i;
        int2 p;
        if (v < L.HX) {
            p = int2{hin[2u * v], hin[2u * v + 1u]};
        } else {
            const uint64_t m = L.mS + (v - L.HX);
            const int xv = xr[v - L.HX];
            const uint32_t jj = (uint32_t)((m >> L.pshift) - jA);
            int sv = 0;
            if (est[jj][0]) {
                const uint32_t ix = (((uint32_t)m * L.inc_p) << 1) >> 22;                  // 2 theta
                const int kc = (tab[(ix - 256u) & 1023u] * est[jj][1] + tab[ix] * est[jj][2]) >> 13;
                sv = (xv * kc) >> 14;
            }
            p = int2{xv, sv};
        }
        xs[i] = p;
    }
    __syncthreads();
    if (last) {                                              // the next call's history: virtual indices M ... M + HX - 1
        int32_t* const hout = L.xh_out + (uint64_t)row * L.HXS * 2u;
        for (uint32_t i = tid; i < L.HX; i += kThreads) {
            const int2 p = xs[L.M + i - vlo];
            hout[2u * i] = p.x; hout[2u * i + 1u] = p.y;
        }
    }
    if (t == 0u && tid == 0u) write_block_carry(L, row);     // the next call's block carry

    // ---- 3. FIRs, matrix, saturation ------------------------------------------------------------------------------------------
    uint32_t* const out = L.out + (uint64_t)row * L.out_stride + na0;
    const uint32_t sh = L.audio_shift + 1u;
    for (uint32_t i = tid; i < cnt; i += kThreads) {
        const int2* w = xs + (vfir - vlo) + L.R * i;
        int m = 0, sd = 0;
        for (uint32_t k = 0; k < L.Ta; ++k) {
            const int2 p = w[k];
            const int gk = gl[k];
            m = __mul24(gk, p.x) + m;
            sd = __mul24(gk, p.y) + sd;
        }
        int l = (m + sd) >> sh, r = (m - sd) >> sh;
        l = l > 32767 ? 32767 : (l < -32768 ? -32768 : l);
        r = r > 32767 ? 32767 : (r < -32768 ? -32768 : r);
        out[i] = ((uint32_t)l & 0xFFFFu) | ((uint32_t)r << 16);
    }
}

}  // namespace fmd_sto

struct fmd_stereo {
    FmdDdcBank bank;
    fmd_sto::MpxState mpx;
    uint32_t Ta = 0, R = 0, audio_shift = 0;
    uint32_t HX = 0, HXS = 0, na = 0;
    void* d_g = nullptr;                                  // int16 audio taps
    FmdDdcPair xh;                                        // [S K][HXS][2] (x, s) history (int32)
};

namespace {

int st_enqueue(fmd_stereo* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream)
{
    FmdDdcCore& c = h->bank.core;
    fmd_sto::MpxCall q;
    fmd_sto::MpxLaunch A{};
    if (const int rc = fmd_sto::mpx_plan_call(h->bank, h->mpx, h->Ta, h->R, h->na, d_iq, nbytes, d_out, out_cap, q, A)) return rc;

    fmd_sto::AudioLaunch B{};
    fmd_sto::mpx_fill_blocks(B, h->bank, h->mpx, q);
    B.xh_in = h->xh.in<int32_t>(c.cur); B.xh_out = h->xh.out<int32_t>(c.cur);
    B.HX = h->HX; B.HXS = h->HXS;
    B.na = h->na;
    B.R = h->R; B.Ta = h->Ta; B.audio_shift = h->audio_shift;
    B.inc_p = h->mpx.inc_p;
    B.thr = (uint64_t)h->mpx.pilot_min * h->mpx.P * 8192u;
    B.g = static_cast<const int16_t*>(h->d_g);
    B.out = static_cast<uint32_t*>(d_out); B.out_stride = out_cap;

    if (const int rc = fmd_sto::mpx_enqueue(h->bank, h->mpx, q, A, stream)) return rc;
    hipLaunchKernelGGL(fmd_sto::fmd_stereo_audio_kernel, dim3((uint32_t)(q.nt2 * q.SK)), dim3(fmd_sto::kThreads), 0, stream, B);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(c, stream, q.ns);
    if (out_len) *out_len = (size_t)q.NA;
    return FMD_OK;
}

}  // namespace

extern "C" {

size_t fmd_stereo_out_cap(uint32_t decim, uint32_t audio_decim, size_t nbytes)
{
    if (!decim || !audio_decim) return 0;
    const uint64_t d = 2ull * decim * audio_decim;
    return (size_t)((nbytes + d - 1) / d);
}

int fmd_stereo_pilot_inc(uint32_t capture_rate, uint32_t decim, uint32_t* inc)
{
    if (!inc || !capture_rate || !decim) { fmd_internal_set_err("null argument or zero rate"); return FMD_ERR_INVALID_ARG; }
    const unsigned __int128 num = ((unsigned __int128)19000u * decim << 32) + capture_rate / 2u;
    *inc = (uint32_t)(uint64_t)(num / capture_rate);
    return FMD_OK;
}

int fmd_stereo_new(const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc,
                   uint32_t n_stations, const int16_t* audio_taps, uint32_t n_audio_taps, const fmd_stereo_config* cfg,
                   const fmd_device_config* dev, fmd_stereo** out)
{
    if (!taps || !phase_inc || !audio_taps || !cfg || !dev || !out || dev->n_channels == 0) {
        fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    if (const int rc = fmd_ddc_front_args(taps, n_taps, decim, shift, n_stations, dev)) return rc;
    if ((uint64_t)cfg->capture_rate < 106000ull * decim) { fmd_internal_set_err("need capture_rate >= 106000 * decim"); return FMD_ERR_UNSUPPORTED; }
    const uint32_t P = cfg->block;
    if (P < 1024u || P > 16384u || (P & (P - 1u)) != 0) { fmd_internal_set_err("block must be a power of two in [1024, 16384]"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->audio_decim < 1u || cfg->audio_decim > 32u || n_audio_taps < 1u || n_audio_taps > 256u || cfg->audio_shift > 16u ||
        cfg->pilot_min > 16384u) {
        fmd_internal_set_err("need 1 <= audio_decim <= 32, 1 <= n_audio_taps <= 256, audio_shift <= 16, pilot_min <= 16384");
        return FMD_ERR_UNSUPPORTED;
    }
    uint64_t gsum = 0;
    for (uint32_t t = 0; t < n_audio_taps; ++t) gsum += (uint64_t)(audio_taps[t] < 0 ? -(int)audio_taps[t] : audio_taps[t]);
    if (gsum > 16383u) { fmd_internal_set_err("sum |audio_taps| > 16383"); return FMD_ERR_UNSUPPORTED; }
    fmd_stereo* h = new (std::nothrow) fmd_stereo();
    if (!h) return FMD_ERR_NOMEM;
    uint64_t bound;
    if (const int rc = fmd_ddc_bank_front(h->bank, taps, n_taps, decim, shift, phase_inc, n_stations, dev, &bound)) { delete h; return rc; }
    fmd_sto::mpx_init(h->bank, h->mpx, P, cfg->pilot_min, cfg->capture_rate);
    h->Ta = n_audio_taps; h->R = cfg->audio_decim; h->audio_shift = cfg->audio_shift;
    h->HX = n_audio_taps - 1u; h->HXS = h->HX ? h->HX : 1u;
    const uint32_t na = (fmd_sto::kXCap - 2u * h->Ta) / h->R;   // >= 48: R tile + 2 Ta <= kXCap
    h->na = na < fmd_sto::kAudioTile ? na : fmd_sto::kAudioTile;
    fmd_ddc_add_pair(h->bank.core, h->xh, (size_t)h->bank.S * h->bank.K * h->HXS * 8);
    fmd_ddc_add_owned(h->bank.core, h->d_g, audio_taps, 2u * n_audio_taps);

    const char* what;
    if (const int rc = fmd_ddc_bank_device(h->bank, dev, &what)) {
        if (!what) { delete h; return rc; }
        fmd_internal_set_err(what); fmd_stereo_free(h); return rc;
    }
    *out = h;
    return FMD_OK;
}

void fmd_stereo_free(fmd_stereo* h)
{
    if (!h) return;
    fmd_ddc_free(h->bank.core);
    delete h;
}

int fmd_stereo_reset(fmd_stereo* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_reset(h->bank.core);
}

int fmd_stereo_run_device(fmd_stereo* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, void* stream)
{
    return fmd_ddc_run_device(h ? &h->bank.core : nullptr, d_iq, d_out,
                              [&] { return st_enqueue(h, d_iq, nbytes, d_out, out_cap, out_len, static_cast<hipStream_t>(stream)); });
}

int fmd_stereo_check(fmd_stereo* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_check(h->bank.core);
}

int fmd_stereo_run_batch(fmd_stereo* h, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!h || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    const size_t out_bytes = out_cap * h->bank.S * h->bank.K * sizeof(uint32_t);   // (L, R) pairs
    return fmd_ddc_run_batch(h->bank, iq, nbytes, out, out_bytes, out_cap, out_len, [h](auto... a) { return st_enqueue(h, a...); });
}

int fmd_stereo_outputs(const fmd_stereo* h, uint64_t* outputs)
{
    if (!h || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *outputs = fmd_ddc_fir_outputs(h->Ta, h->R, fmd_ddc_outputs(h->bank.T, h->bank.D, h->bank.core.pos));
    return FMD_OK;
}

int fmd_stereo_pilot(fmd_stereo* h, uint32_t stream, uint32_t station, int* present, uint32_t* level)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_sto::mpx_pilot(h->bank, h->mpx, stream, station, present, level);
}

int fmd_stereo_kernel_name(const fmd_stereo* h, uint32_t pass, char* name, size_t cap)
{
    if (!h || !name || cap == 0 || pass > 1) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, pass == 0 ? "fmd_sto::fmd_stereo_mpx_kernel" : "fmd_sto::fmd_stereo_audio_kernel"), cap);
}

}  // extern "C"
