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
// on rds_shift is this bank's own.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include "fmd_ddc.h"
#include "fmd_internal.h"
#include "fmd_stereo_mpx.h"

namespace fmd_rdsk {

using fmd_ddc::kThreads;

constexpr uint32_t kQCap = 1984;                          // pairs a tile stages: R tile + Ta <= kQCap
constexpr uint32_t kQSlots = 2048;                        // LDS slots: kQCap + kQCap / 32 = 2046 padded positions (16 KiB, the stereo pass's xs)

struct BasebandLaunch : fmd_sto::StageLaunch {            // pairs (qr, qi), shift: rds_shift, out: (ur, ui)
    uint32_t inc3;             // carrier step 3 inc_p mod 2^32
};

// The baseband pass's side of a second-pass tile (fmd_stereo_mpx.h, stage_tile).
struct BasebandPass {
    static constexpr uint32_t kSlots = kQSlots;

    // lanes read at stride R, and without the padding an even R puts them on few banks (R = 32: all 64 lanes on one pair of banks)
    static __device__ __forceinline__ uint32_t slot(uint32_t i) { return i + (i >> 5); }

    __device__ __forceinline__ void before(const BasebandLaunch&, uint32_t, uint32_t, uint32_t, uint32_t) {}

    // q[m] = (x cosq(phi), -x sinq(phi)) >> 14, phi = 3 m inc_p mod 2^32 (|x tab| <= 2^29)
    __device__ __forceinline__ int2 pair(const BasebandLaunch& L, const int16_t* tab, uint64_t m, int xv) const
    {
        const uint32_t ix = ((uint32_t)m * L.inc3) >> 22;
        return int2{(xv * (int)tab[ix]) >> 14, (-xv * (int)tab[(ix - 256u) & 1023u]) >> 14};
    }

    // the normalising shift; the host's store check makes the wrap to 16 bits exact (|v| < 2^29)
    static __device__ __forceinline__ uint32_t output(int a, int b, uint32_t shift)
    {
        return ((uint32_t)(a >> shift) & 0xFFFFu) | ((uint32_t)(b >> shift) << 16);
    }
};

__global__ void __launch_bounds__(kThreads) fmd_rds_baseband_kernel(const BasebandLaunch L)
{
    fmd_sto::stage_tile(L, BasebandPass{});
}

}  // namespace fmd_rdsk

struct fmd_rds : fmd_sto::MpxHandle {};

namespace {

constexpr fmd_sto::StageLimits kLimits{120000u, "out_decim", "rds_taps", "rds_shift", 24u};

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
    if (((32768ull * gsum + ((1ull << c.shift) - 1ull)) >> c.shift) > 32767ull) {
        fmd_internal_set_err("rds_shift too small: need ceil(32768 * sum |rds_taps| / 2^rds_shift) <= 32767");
        return FMD_ERR_UNSUPPORTED;
    }
    const uint32_t room = fmd_rdsk::kQCap - n_rds_taps;      // na >= 54: R na + Ta <= kQCap
    return fmd_sto::stage_new(taps, n_taps, decim, shift, phase_inc, n_stations, rds_taps, n_rds_taps, c, room, dev, fmd_rds_free, out);
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
