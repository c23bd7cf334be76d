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
    if (t == 0u && tid == 0u) fmd_sto::write_block_carry(L, row);   // the next call's block carry

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
    FmdDdcBank bank;
    fmd_sto::MpxState mpx;
    uint32_t Ta = 0, R = 0, rds_shift = 0;
    uint32_t HX = 0, HXS = 0, na = 0;
    void* d_g = nullptr;                                  // int16 RDS taps
    FmdDdcPair qh;                                        // [S K][HXS][2] (qr, qi) history (int32)
};

namespace {

int rd_enqueue(fmd_rds* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream)
{
    FmdDdcCore& c = h->bank.core;
    fmd_sto::MpxCall q;
    fmd_sto::MpxLaunch A{};
    if (const int rc = fmd_sto::mpx_plan_call(h->bank, h->mpx, h->Ta, h->R, h->na, d_iq, nbytes, d_out, out_cap, q, A)) return rc;

    fmd_rdsk::BasebandLaunch B{};
    fmd_sto::mpx_fill_blocks(B, h->bank, h->mpx, q);
    B.qh_in = h->qh.in<int32_t>(c.cur); B.qh_out = h->qh.out<int32_t>(c.cur);
    B.HX = h->HX; B.HXS = h->HXS;
    B.na = h->na;
    B.R = h->R; B.Ta = h->Ta; B.rds_shift = h->rds_shift;
    B.inc3 = 3u * h->mpx.inc_p;
    B.g = static_cast<const int16_t*>(h->d_g);
    B.out = static_cast<uint32_t*>(d_out); B.out_stride = out_cap;

    if (const int rc = fmd_sto::mpx_enqueue(h->bank, h->mpx, q, A, stream)) return rc;
    hipLaunchKernelGGL(fmd_rdsk::fmd_rds_baseband_kernel, dim3((uint32_t)(q.nt2 * q.SK)), dim3(fmd_rdsk::kThreads), 0, stream, B);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(c, stream, q.ns);
    if (out_len) *out_len = (size_t)q.NA;
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
    if (const int rc = fmd_ddc_front_args(taps, n_taps, decim, shift, n_stations, dev)) return rc;
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
    uint64_t bound;
    if (const int rc = fmd_ddc_bank_front(h->bank, taps, n_taps, decim, shift, phase_inc, n_stations, dev, &bound)) { delete h; return rc; }
    fmd_sto::mpx_init(h->bank, h->mpx, P, cfg->pilot_min, cfg->capture_rate);
    h->Ta = n_rds_taps; h->R = cfg->out_decim; h->rds_shift = cfg->rds_shift;
    h->HX = n_rds_taps - 1u; h->HXS = h->HX ? h->HX : 1u;
    const uint32_t na = (fmd_rdsk::kQCap - h->Ta) / h->R;   // >= 54: R tile + Ta <= kQCap
    h->na = na < fmd_rdsk::kTile ? na : fmd_rdsk::kTile;
    fmd_ddc_add_pair(h->bank.core, h->qh, (size_t)h->bank.S * h->bank.K * h->HXS * 8);
    fmd_ddc_add_owned(h->bank.core, h->d_g, rds_taps, 2u * n_rds_taps);

    const char* what;
    if (const int rc = fmd_ddc_bank_device(h->bank, dev, &what)) {
        if (!what) { delete h; return rc; }
        fmd_internal_set_err(what); fmd_rds_free(h); return rc;
    }
    *out = h;
    return FMD_OK;
}

void fmd_rds_free(fmd_rds* h)
{
    if (!h) return;
    fmd_ddc_free(h->bank.core);
    delete h;
}

int fmd_rds_reset(fmd_rds* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_reset(h->bank.core);
}

int fmd_rds_run_device(fmd_rds* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, void* stream)
{
    return fmd_ddc_run_device(h ? &h->bank.core : nullptr, d_iq, d_out,
                              [&] { return rd_enqueue(h, d_iq, nbytes, d_out, out_cap, out_len, static_cast<hipStream_t>(stream)); });
}

int fmd_rds_check(fmd_rds* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_check(h->bank.core);
}

int fmd_rds_run_batch(fmd_rds* h, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!h || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    const size_t out_bytes = out_cap * h->bank.S * h->bank.K * sizeof(uint32_t);   // (ur, ui) pairs
    return fmd_ddc_run_batch(h->bank, iq, nbytes, out, out_bytes, out_cap, out_len, [h](auto... a) { return rd_enqueue(h, a...); });
}

int fmd_rds_outputs(const fmd_rds* h, uint64_t* outputs)
{
    if (!h || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *outputs = fmd_ddc_fir_outputs(h->Ta, h->R, fmd_ddc_outputs(h->bank.T, h->bank.D, h->bank.core.pos));
    return FMD_OK;
}

int fmd_rds_pilot(fmd_rds* h, uint32_t stream, uint32_t station, int* present, uint32_t* level)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_sto::mpx_pilot(h->bank, h->mpx, stream, station, present, level);
}

int fmd_rds_kernel_name(const fmd_rds* h, uint32_t pass, char* name, size_t cap)
{
    if (!h || !name || cap == 0 || pass > 1) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, pass == 0 ? "fmd_sto::fmd_stereo_mpx_kernel" : "fmd_rdsk::fmd_rds_baseband_kernel"), cap);
}

}  // extern "C"
