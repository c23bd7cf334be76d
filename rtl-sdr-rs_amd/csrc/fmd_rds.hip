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
// Pass 1 (fmd_rds_baseband_kernel) is the second-pass tile that this bank and the stereo bank share (fmd_stereo_mpx.h, stage_tile: one
// workgroup = one (stream, station) row and one tile of up to 256 outputs, the pairs of every MPX sample the tile's FIR reads in
// LDS, the last Ta - 1 of them carried from call to call, one lane per output) with this bank's side (BasebandPass):
//   - the pair (qr, qi) from x and the NCO table, in slot i + (i >> 5) of the LDS;
//   - from the two FIR sums (|g| <= 16383, |q| <= 32768 fit v_mad_i32_i24's 24-bit operands; |v| < 2^29) the shift and one dword
//     store of the (ur, ui) pair.
// The host side of the second stage -- handle, constructor, launch fields, enqueue -- is that header's as well; the exact-store check
// on rds_shift is this bank's own.  BasebandPass and its launch struct are in fmd_mpx_passes.h, where the receiver bank finds them too.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include "fmd_ddc.h"
#include "fmd_internal.h"
#include "fmd_mpx_passes.h"
#include "fmd_stereo_mpx.h"

namespace fmd_rdsk {

using fmd_ddc::kThreads;

__global__ void __launch_bounds__(kThreads) fmd_rds_baseband_kernel(const BasebandLaunch L)
{
    __shared__ __attribute__((aligned(16))) int2 ps[fmd_sto::kStageSlots];
    __shared__ int32_t gl[256];
    __shared__ int16_t tab[1024];
    fmd_sto::stage_tile(L, BasebandPass{}, blockIdx.x, ps, gl, tab);
}

}  // namespace fmd_rdsk

struct fmd_rds : fmd_sto::MpxHandle {};

namespace {

constexpr fmd_sto::StageLimits kLimits = fmd_rdsk::kBasebandLimits;

int rd_enqueue(fmd_rds* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream)
{
    return fmd_sto::stage_enqueue<fmd_rdsk::BasebandLaunch>(*h, d_iq, nbytes, d_out, out_cap, out_len, stream, [&](fmd_rdsk::BasebandLaunch& B, uint32_t grid) {
        B.inc3 = 3u * h->mpx.inc_p;
        hipLaunchKernelGGL(fmd_rdsk::fmd_rds_baseband_kernel, dim3(grid), dim3(fmd_rdsk::kThreads), 0, stream, B);
    });
}

}  // namespace

extern "C" {

size_t fmd_rds_out_cap(uint32_t decim, uint32_t out_decim, size_t nbytes) { return fmd_ddc_fir_out_cap(decim, out_decim, nbytes); }

int fmd_rds_new(const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc, uint32_t n_stations,
                const int16_t* rds_taps, uint32_t n_rds_taps, const fmd_rds_config* cfg, const fmd_device_config* dev, fmd_rds** out)
{
    if (!cfg) { fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG; }
    const fmd_sto::StageConfig c{cfg->capture_rate, cfg->block, cfg->out_decim, cfg->rds_shift, cfg->pilot_min};
    uint64_t gsum;
    if (const int rc = fmd_sto::stage_args(kLimits, taps, n_taps, decim, shift, phase_inc, n_stations, rds_taps, n_rds_taps, c, dev, out, &gsum)) return rc;
    if (const int rc = fmd_rdsk::store_check(gsum, c.shift)) return rc;
    return fmd_sto::stage_new(taps, n_taps, decim, shift, phase_inc, n_stations, rds_taps, n_rds_taps, c, fmd_rdsk::baseband_room(n_rds_taps), dev,
                              fmd_rds_free, out);
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

int fmd_rds_outputs(const fmd_rds* h, uint64_t* outputs) { return fmd_sto::stage_outputs(h, outputs); }

int fmd_rds_pilot(fmd_rds* h, uint32_t stream, uint32_t station, int* present, uint32_t* level)
{
    return fmd_sto::stage_pilot(h, stream, station, present, level);
}

int fmd_rds_kernel_name(const fmd_rds* h, uint32_t pass, char* name, size_t cap)
{
    if (!h || !name || cap == 0 || pass > 1) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, pass == 0 ? "fmd_sto::fmd_stereo_mpx_kernel" : "fmd_rdsk::fmd_rds_baseband_kernel"), cap);
}

}  // extern "C"
