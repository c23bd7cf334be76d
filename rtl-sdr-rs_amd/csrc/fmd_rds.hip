// fmd_rds.hip -- RDS bank: each FM station's 57 kHz subcarrier as a complex baseband of a few kHz, K stations per wideband IQ
// stream, in two gfx950 kernels per call.  The sequential part of RDS (carrier, symbol timing, block synchronisation, groups) runs on
// this low-rate stream on the host: fmd_rds_decode.cpp.
//
// Definition (include/fmd.h, "RDS bank"; tests/rds_ref.py): the stereo bank's multiplex x[m] and pilot block sums, the free-running
// carrier phi_m = 3 m inc_p, q[m] = (x cosq(phi), -x sinq(phi)) >> 14, one real FIR g (stride R) over both components, and the
// normalising shift to int16.
//
// Pass 0 is the stereo bank's multiplex pass, fmd_sto::fmd_stereo_mpx_kernel -- the one compiled in fmd_stereo.hip, launched through
// fmd_stereo_mpx.h: front end, discriminator, pilot block sums, x as i16.
// Pass 1 (fmd_rds_baseband_kernel): one workgroup = one (stream, station) row and one tile of up to 256 outputs:
//   1. the NCO table and the taps into LDS;
//   2. (qr, qi) of every MPX sample the tile's FIR reads into LDS: the carried Ta - 1 pairs of the previous call from the history,
//      the call's own from x and the table.  Pair i sits in slot i + (i >> 5): lanes read at stride R, and without the padding an
//      even R puts them on few banks (R = 32: all 64 lanes on one pair of banks);
//   3. one lane per output: both FIR sums with v_mad_i32_i24 (|g| <= 16383, |q| <= 32768 fit 24-bit operands; |v| < 2^29), the
//      shift, one dword store of the (ur, ui) pair.
// The last tile of a row writes the next call's q history; tile 0 the next call's block carry, as the stereo bank's pass 2 does.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>

#include "fmd_ddc.h"
#include "fmd_internal.h"
#include "fmd_stereo_mpx.h"

namespace fmd_rdsk {

using fmd_ddc::kThreads;

constexpr uint32_t kTile = 256;                           // outputs per pass-1 tile (at most)
constexpr uint32_t kQCap = 1984;                          // pairs a tile stages: R tile + Ta <= kQCap
constexpr uint32_t kQSlots = 2048;                        // LDS slots: kQCap + kQCap / 32 = 2046 padded positions (16 KiB, the stereo pass's xs)

struct BasebandLaunch {
    const int16_t* x;          // [S K][M]
    uint32_t M;
    const int32_t* qh_in;      // [S K][HXS][2]: (qr, qi) of the HX samples before the call
    int32_t* qh_out;
    uint32_t HX, HXS;          // Ta - 1, row stride (>= 1)
    const long long* sums;     // [nbc][S K][2]
    const long long* carry_in; // [S K][4]: I, Q of block jfirst - 1; partial I, Q of block jfirst from earlier calls
    long long* carry_out;
    uint32_t SK;
    uint64_t mS, mE, jfirst;   // MPX samples before / after the call, block of mS
    uint64_t nS;               // outputs before the call
    uint32_t NA, na, ntiles;   // outputs of the call, per tile, tiles per row
    uint32_t R, Ta, rds_shift;
    uint32_t pshift, inc3;     // log2 P, carrier step 3 inc_p mod 2^32
    const int16_t* g;
    const uint32_t* tab;
    uint32_t* out;             // [S K][out_stride] (ur, ui) pairs
    uint64_t out_stride;
};

// I, Q of block j (>= jfirst - 1, every sample of it already in the sums)
__device__ __forceinline__ void block_iq(const BasebandLaunch& L, uint32_t row, int64_t j, long long& I, long long& Q)
{
    const int64_t jf = (int64_t)L.jfirst;
    if (j < 0) { I = 0; Q = 0; return; }
    if (j == jf - 1) { I = L.carry_in[4u * row]; Q = L.carry_in[4u * row + 1u]; return; }
    const long long* p = L.sums + ((uint64_t)(j - jf) * L.SK + row) * 2u;
    I = p[0]; Q = p[1];
    if (j == jf) { I += L.carry_in[4u * row + 2u]; Q += L.carry_in[4u * row + 3u]; }
}

__device__ __forceinline__ uint32_t slot(uint32_t i) { return i + (i >> 5); }

__global__ void __launch_bounds__(kThreads) fmd_rds_baseband_kernel(const BasebandLaunch L)
{
    __shared__ __attribute__((aligned(16))) int2 qs[kQSlots];
    __shared__ int32_t gl[256];
    __shared__ int16_t tab[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / L.ntiles, t = blockIdx.x - row * L.ntiles;
    if (row >= L.SK) return;

    const uint32_t na0 = t * L.na;                           // first output (of this call) of the tile
    const uint32_t cnt = L.NA - na0 < L.na ? L.NA - na0 : L.na;
    const bool last = t == L.ntiles - 1u;
    // virtual index v: MPX sample mS - HX + v (v < HX: the carried history)
    const uint32_t vlo = (uint32_t)(L.R * (L.nS + na0) + L.HX - L.mS);       // the tile's first FIR window (< M: the call completes it)
    // the last tile also forms the next call's history, virtual indices M ... M + HX - 1; the output after the call's last is
    // incomplete, so HX + M - vlo < R cnt + Ta
    const uint32_t vhi = last ? L.HX + L.M : vlo + L.R * (cnt - 1u) + L.Ta;
    const uint32_t span = vhi - vlo;                         // <= kQCap: host plan

    // ---- 1. the NCO table, the taps ---------------------------------------------------------------------------------------------
    for (uint32_t i = tid; i < 512u; i += kThreads) reinterpret_cast<uint32_t*>(tab)[i] = L.tab[i];
    for (uint32_t i = tid; i < L.Ta; i += kThreads) gl[i] = L.g[i];
    __syncthreads();

    // ---- 2. (qr, qi) of the tile's samples --------------------------------------------------------------------------------------
    const int16_t* const xr = L.x + (uint64_t)row * L.M;
    const int32_t* const hin = L.qh_in + (uint64_t)row * L.HXS * 2u;
    for (uint32_t i = tid; i < span; i += kThreads) {
        const uint32_t v = vlo + i;
        int2 p;
        if (v < L.HX) {
            p = int2{hin[2u * v], hin[2u * v + 1u]};
        } else {
            const uint32_t m = (uint32_t)L.mS + (v - L.HX);  // mod 2^32, as phi
            const int xv = xr[v - L.HX];
            const uint32_t ix = (m * L.inc3) >> 22;
            p = int2{(xv * (int)tab[ix]) >> 14, (-xv * (int)tab[(ix - 256u) & 1023u]) >> 14};   // |x tab| <= 2^29
        }
        qs[slot(i)] = p;
    }
    __syncthreads();
    if (last) {                                              // the next call's history
        int32_t* const hout = L.qh_out + (uint64_t)row * L.HXS * 2u;
        for (uint32_t i = tid; i < L.HX; i += kThreads) {
            const int2 p = qs[slot(L.M + i - vlo)];
            hout[2u * i] = p.x; hout[2u * i + 1u] = p.y;
        }
    }
    if (t == 0u && tid == 0u) {                              // the next call's block carry
        const int64_t jn = (int64_t)(L.mE >> L.pshift);
        long long I = 0, Q = 0, Ip = 0, Qp = 0;
        if (jn >= 1) block_iq(L, row, jn - 1, I, Q);
        if (L.mE & ((1ull << L.pshift) - 1u)) block_iq(L, row, jn, Ip, Qp);
        long long* const c = L.carry_out + 4u * row;
        c[0] = I; c[1] = Q; c[2] = Ip; c[3] = Qp;
    }

    // ---- 3. FIRs, shift -----------------------------------------------------------------------------------------------------------
    uint32_t* const out = L.out + (uint64_t)row * L.out_stride + na0;
    for (uint32_t i = tid; i < cnt; i += kThreads) {
        const uint32_t p0 = L.R * i;
        int vr = 0, vi = 0;
        for (uint32_t k = 0; k < L.Ta; ++k) {
            const int2 p = qs[slot(p0 + k)];
            const int gk = gl[k];
            vr = __mul24(gk, p.x) + vr;
            vi = __mul24(gk, p.y) + vi;
        }
        out[i] = ((uint32_t)(vr >> L.rds_shift) & 0xFFFFu) | ((uint32_t)(vi >> L.rds_shift) << 16);
    }
}

}  // namespace fmd_rdsk

struct fmd_rds {
    uint32_t T = 0, D = 0, K = 0, S = 0, shift = 0, HB = 0;
    fmd_sto::MpxTiling tl;
    uint32_t Ta = 0, R = 0, P = 0, pshift = 0, rds_shift = 0, pilot_min = 0, inc_p = 0;
    uint32_t HX = 0, HXS = 0, na = 0;
    FmdDdcPlan plan;
    FmdDdcCore core;
    int16_t* d_g = nullptr;
    uint32_t* d_ylast[2] = {nullptr, nullptr};            // [S K] packed y, read [core.cur], written [core.cur ^ 1]
    int32_t* d_qh[2] = {nullptr, nullptr};                // [S K][HXS][2] (qr, qi) history
    long long* d_carry[2] = {nullptr, nullptr};           // [S K][4] block carry
    void* d_x = nullptr; size_t d_x_cap = 0;              // the call's MPX samples
    void* d_sums = nullptr; size_t d_sums_cap = 0;        // the call's block sums
};

namespace {

uint64_t rd_mpx(const fmd_rds* h, uint64_t S) { return S >= h->T ? (S - h->T) / h->D + 1 : 0; }
uint64_t rd_out(const fmd_rds* h, uint64_t m) { return m >= h->Ta ? (m - h->Ta) / h->R + 1 : 0; }

int rd_enqueue(fmd_rds* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream)
{
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    if (nbytes > (1ull << 31) - (1ull << 20)) { fmd_internal_set_err("nbytes out of range"); return FMD_ERR_UNSUPPORTED; }
    if (((uintptr_t)d_iq & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0) { fmd_internal_set_err("misaligned device buffer"); return FMD_ERR_INVALID_ARG; }
    FmdDdcCore& c = h->core;
    const uint64_t ns = nbytes / 2;
    const uint64_t mS = rd_mpx(h, c.pos), mE = rd_mpx(h, c.pos + ns), M = mE - mS;
    const uint64_t nS = rd_out(h, mS), NA = rd_out(h, mE) - nS;
    if (NA < 1) { fmd_internal_set_err("the call completes no output"); return FMD_ERR_TOO_SHORT; }
    if (NA > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    const uint64_t SK = (uint64_t)h->S * h->K;
    const uint64_t nt1 = (M + h->tl.tile - 1) / h->tl.tile, nt2 = (NA + h->na - 1) / h->na;
    if (nt1 > (1u << 30) || h->S > 65535u || nt2 * SK > 0x7FFFFFFFull) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }
    const uint64_t jfirst = mS >> h->pshift, nbc = ((mE - 1) >> h->pshift) - jfirst + 1;
    const size_t sums_bytes = (size_t)(nbc * SK * 16);
    FMD_DDC_TRY(fmd_ddc_grow(h->d_x, h->d_x_cap, (size_t)(SK * M * 2)));
    FMD_DDC_TRY(fmd_ddc_grow(h->d_sums, h->d_sums_cap, sums_bytes));
    const int cur = c.cur;

    fmd_sto::MpxLaunch A{};
    A.iq = static_cast<const uint8_t*>(d_iq);
    A.nbytes = nbytes;
    A.hist_in = c.d_hist[cur]; A.hist_out = c.d_hist[cur ^ 1];
    A.HB = h->HB;
    A.vb_first = (uint32_t)(2ull * (h->D * mS + h->HB / 2 - c.pos));
    A.m0 = mS; A.M = (uint32_t)M;
    A.D = h->D; A.T = h->T; A.K = h->K; A.S = h->S; A.shift = h->shift;
    A.nrt = h->plan.nrt; A.nkc = h->plan.nkc; A.digits = h->plan.digits;
    A.tile = h->tl.tile; A.cols = h->tl.cols; A.ntiles = (uint32_t)nt1; A.raw_bytes = h->tl.raw_bytes;
    A.pshift = h->pshift; A.inc_p = h->inc_p; A.jfirst = jfirst;
    A.amat = c.d_amat; A.kconst = c.d_kconst; A.dinc = c.d_dinc; A.tab = c.d_tab;
    A.ylast_in = h->d_ylast[cur]; A.ylast_out = h->d_ylast[cur ^ 1];
    A.x = static_cast<int16_t*>(h->d_x);
    A.sums = static_cast<unsigned long long*>(h->d_sums);

    fmd_rdsk::BasebandLaunch B{};
    B.x = A.x; B.M = (uint32_t)M;
    B.qh_in = h->d_qh[cur]; B.qh_out = h->d_qh[cur ^ 1];
    B.HX = h->HX; B.HXS = h->HXS;
    B.sums = static_cast<const long long*>(h->d_sums);
    B.carry_in = h->d_carry[cur]; B.carry_out = h->d_carry[cur ^ 1];
    B.SK = (uint32_t)SK;
    B.mS = mS; B.mE = mE; B.jfirst = jfirst; B.nS = nS;
    B.NA = (uint32_t)NA; B.na = h->na; B.ntiles = (uint32_t)nt2;
    B.R = h->R; B.Ta = h->Ta; B.rds_shift = h->rds_shift;
    B.pshift = h->pshift; B.inc3 = 3u * h->inc_p;
    B.g = h->d_g; B.tab = c.d_tab;
    B.out = static_cast<uint32_t*>(d_out); B.out_stride = out_cap;

    FMD_DDC_TRY(c.order.before(stream));
    FMD_DDC_TRY(hipMemsetAsync(h->d_sums, 0, sums_bytes, stream));
    FMD_DDC_TRY(fmd_sto::launch_mpx(A, h->tl.lds, stream));
    hipLaunchKernelGGL(fmd_rdsk::fmd_rds_baseband_kernel, dim3((uint32_t)(nt2 * SK)), dim3(fmd_rdsk::kThreads), 0, stream, B);
    FMD_DDC_TRY(hipGetLastError());
    (void)c.order.after(stream);
    c.cur ^= 1;
    c.pos += ns;
    if (out_len) *out_len = (size_t)NA;
    return FMD_OK;
}

}  // namespace

extern "C" {

size_t fmd_rds_out_cap(uint32_t decim, uint32_t out_decim, size_t nbytes)
{
    if (!decim || !out_decim) return 0;
    const uint64_t d = 2ull * decim * out_decim;
    return (size_t)((nbytes + d - 1) / d);
}

int fmd_rds_new(const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc, uint32_t n_stations,
                const int16_t* rds_taps, uint32_t n_rds_taps, const fmd_rds_config* cfg, const fmd_device_config* dev, fmd_rds** out)
{
    if (!taps || !phase_inc || !rds_taps || !cfg || !dev || !out || dev->n_channels == 0) {
        fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    if (n_taps == 0 || n_taps > 256 || decim < 2 || decim % 2 != 0 || decim > 64 || shift > 24 || n_stations == 0 || n_stations > 32 ||
        dev->n_channels > 65535u) {
        fmd_internal_set_err("need 1 <= n_taps <= 256, an even 2 <= decim <= 64, shift <= 24, 1 <= n_stations <= 32, n_streams <= 65535");
        return FMD_ERR_UNSUPPORTED;
    }
    for (uint32_t t = 0; t < n_taps; ++t)
        if (taps[t] > 2047 || taps[t] < -2047) { fmd_internal_set_err("|tap| > 2047"); return FMD_ERR_UNSUPPORTED; }
    if ((uint64_t)cfg->capture_rate < 120000ull * decim) { fmd_internal_set_err("need capture_rate >= 120000 * decim"); return FMD_ERR_UNSUPPORTED; }
    const uint32_t P = cfg->block;
    if (P < 1024u || P > 16384u || (P & (P - 1u)) != 0) { fmd_internal_set_err("block must be a power of two in [1024, 16384]"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->out_decim < 1u || cfg->out_decim > 32u || n_rds_taps < 1u || n_rds_taps > 256u || cfg->rds_shift > 24u || cfg->pilot_min > 16384u) {
        fmd_internal_set_err("need 1 <= out_decim <= 32, 1 <= n_rds_taps <= 256, rds_shift <= 24, pilot_min <= 16384");
        return FMD_ERR_UNSUPPORTED;
    }
    uint64_t gsum = 0;
    for (uint32_t t = 0; t < n_rds_taps; ++t) gsum += (uint64_t)(rds_taps[t] < 0 ? -(int)rds_taps[t] : rds_taps[t]);
    if (gsum > 16383u) { fmd_internal_set_err("sum |rds_taps| > 16383"); return FMD_ERR_UNSUPPORTED; }
    if (((32768ull * gsum + ((1ull << cfg->rds_shift) - 1ull)) >> cfg->rds_shift) > 32767ull) {
        fmd_internal_set_err("rds_shift too small: need ceil(32768 * sum |rds_taps| / 2^rds_shift) <= 32767");
        return FMD_ERR_UNSUPPORTED;
    }
    fmd_rds* h = new (std::nothrow) fmd_rds();
    if (!h) return FMD_ERR_NOMEM;
    h->T = n_taps; h->D = decim; h->K = n_stations; h->S = dev->n_channels; h->shift = shift;
    fmd_st_build_plan(taps, n_taps, decim, phase_inc, h->S, h->K, h->plan);
    const uint64_t bound = (256ull * h->plan.max_gain + ((1ull << shift) - 1ull)) >> shift;
    if (bound > 16384ull) {
        delete h;
        fmd_internal_set_err("filter gain too large: need ceil(256 * max sum(|Wr| + |Wi|) / 2^shift) <= 16384");
        return FMD_ERR_UNSUPPORTED;
    }
    h->tl = fmd_sto::mpx_tiling(decim, h->plan.nkc, n_taps, n_stations);
    h->HB = 2u * ((n_taps - 1u + 7u) & ~7u);
    h->Ta = n_rds_taps; h->R = cfg->out_decim; h->P = P; h->rds_shift = cfg->rds_shift; h->pilot_min = cfg->pilot_min;
    while ((1u << h->pshift) < P) ++h->pshift;
    (void)fmd_stereo_pilot_inc(cfg->capture_rate, decim, &h->inc_p);
    h->HX = n_rds_taps - 1u; h->HXS = h->HX ? h->HX : 1u;
    const uint32_t na = (fmd_rdsk::kQCap - h->Ta) / h->R;   // >= 54: R tile + Ta <= kQCap
    h->na = na < fmd_rdsk::kTile ? na : fmd_rdsk::kTile;

    if (const int rc = fmd_ddc_open(h->core, dev)) { delete h; return rc; }
    auto fail = [&](const char* what) { fmd_internal_set_err(what); fmd_rds_free(h); return FMD_ERR_HIP; };
    FmdDeviceGuard guard(h->core.device);
    if (guard.error() != hipSuccess) return fail("hipSetDevice");
    if (const char* what = fmd_ddc_upload(h->core, h->plan, (size_t)h->S * (h->HB ? h->HB : 16))) return fail(what);
    const size_t SK = (size_t)h->S * h->K;
    if (hipMalloc(&h->d_g, 2u * n_rds_taps) != hipSuccess || hipMemcpy(h->d_g, rds_taps, 2u * n_rds_taps, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMalloc(RDS taps)");
    for (int i = 0; i < 2; ++i) {
        if (hipMalloc(&h->d_ylast[i], SK * 4) != hipSuccess || hipMemset(h->d_ylast[i], 0, SK * 4) != hipSuccess) return fail("hipMalloc(last y)");
        if (hipMalloc(&h->d_qh[i], SK * h->HXS * 8) != hipSuccess || hipMemset(h->d_qh[i], 0, SK * h->HXS * 8) != hipSuccess) return fail("hipMalloc(q history)");
        if (hipMalloc(&h->d_carry[i], SK * 32) != hipSuccess || hipMemset(h->d_carry[i], 0, SK * 32) != hipSuccess) return fail("hipMalloc(block carry)");
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    *out = h;
    return FMD_OK;
}

void fmd_rds_free(fmd_rds* h)
{
    if (!h) return;
    FmdDeviceGuard guard(h->core.device);
    (void)hipDeviceSynchronize();
    for (void* p : {(void*)h->d_g, (void*)h->d_ylast[0], (void*)h->d_ylast[1], (void*)h->d_qh[0], (void*)h->d_qh[1], (void*)h->d_carry[0],
                    (void*)h->d_carry[1], h->d_x, h->d_sums})
        if (p) (void)hipFree(p);
    fmd_ddc_release(h->core);
    delete h;
}

int fmd_rds_reset(fmd_rds* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    FMD_DDC_ON_DEVICE(h->core.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    const size_t SK = (size_t)h->S * h->K;
    for (int i = 0; i < 2; ++i) {
        FMD_DDC_TRY(hipMemset(h->d_ylast[i], 0, SK * 4));
        FMD_DDC_TRY(hipMemset(h->d_qh[i], 0, SK * h->HXS * 8));
        FMD_DDC_TRY(hipMemset(h->d_carry[i], 0, SK * 32));
    }
    FMD_DDC_TRY(fmd_ddc_zero_history(h->core));          // (ends with the device synchronised; position and buffer index to 0)
    return FMD_OK;
}

int fmd_rds_run_device(fmd_rds* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, void* stream)
{
    if (!h || !d_iq || !d_out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->core.device);
    return rd_enqueue(h, d_iq, nbytes, d_out, out_cap, out_len, static_cast<hipStream_t>(stream));
}

int fmd_rds_check(fmd_rds* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->core.device);
    if (h->core.order.have_last) FMD_DDC_TRY(hipStreamSynchronize(h->core.order.last));
    FMD_DDC_TRY(hipGetLastError());
    return FMD_OK;
}

int fmd_rds_run_batch(fmd_rds* h, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!h || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->core.device);
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    FmdDdcCore& c = h->core;
    const size_t rows = (size_t)h->S * h->K;
    const size_t in_bytes = nbytes * (size_t)h->S, out_bytes = out_cap * rows * sizeof(uint32_t);   // (ur, ui) pairs
    FMD_DDC_TRY(fmd_ddc_grow(c.d_iq, c.d_iq_cap, in_bytes));
    FMD_DDC_TRY(fmd_ddc_grow(c.d_out, c.d_out_cap, out_bytes));
    FMD_DDC_TRY(hipMemcpyAsync(c.d_iq, iq, in_bytes, hipMemcpyHostToDevice, c.stream));
    size_t n = 0;
    int rc = rd_enqueue(h, c.d_iq, nbytes, c.d_out, out_cap, &n, c.stream);
    if (rc) { (void)hipStreamSynchronize(c.stream); return rc; }
    FMD_DDC_TRY(hipMemcpyAsync(out, c.d_out, out_bytes, hipMemcpyDeviceToHost, c.stream));
    FMD_DDC_TRY(hipStreamSynchronize(c.stream));
    *out_len = n;
    return FMD_OK;
}

int fmd_rds_outputs(const fmd_rds* h, uint64_t* outputs)
{
    if (!h || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *outputs = rd_out(h, rd_mpx(h, h->core.pos));
    return FMD_OK;
}

int fmd_rds_pilot(fmd_rds* h, uint32_t stream, uint32_t station, int* present, uint32_t* level)
{
    if (!h || !present || !level) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (stream >= h->S || station >= h->K) { fmd_internal_set_err("stream or station out of range"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->core.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    long long c[4];
    FMD_DDC_TRY(hipMemcpy(c, h->d_carry[h->core.cur] + 4ull * ((size_t)stream * h->K + station), sizeof c, hipMemcpyDeviceToHost));
    fmd_sto::pilot_report(c[0], c[1], h->pilot_min, h->P, present, level);
    return FMD_OK;
}

int fmd_rds_kernel_name(const fmd_rds* h, uint32_t pass, char* name, size_t cap)
{
    if (!h || !name || cap == 0 || pass > 1) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, pass == 0 ? "fmd_sto::fmd_stereo_mpx_kernel" : "fmd_rdsk::fmd_rds_baseband_kernel"), cap);
}

}  // extern "C"
