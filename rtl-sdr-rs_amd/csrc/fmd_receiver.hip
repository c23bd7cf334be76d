// fmd_receiver.hip -- FM receiver bank: each station's pilot-locked stereo audio AND its RDS baseband, K stations per wideband IQ
// stream, in two gfx950 kernels per call.  A stereo station bank and an RDS bank over the same bytes each run the multiplex pass;
// this handle runs it once and both second stages read its x[m] and block sums.
//
// Definition (include/fmd.h, "FM receiver bank"; tests/receiver_ref.py): the audio is the stereo bank's and the baseband the RDS
// bank's, bit for bit; a call must complete an output of each.
//
// Pass 0 is the stereo bank's multiplex pass, fmd_sto::fmd_stereo_mpx_kernel -- the one compiled in fmd_stereo.hip, launched through
// fmd_stereo_mpx.h.
// Pass 1 (fmd_receiver_second_kernel) holds the tiles of both second stages in one grid: a workgroup runs the second-pass tile
// (fmd_stereo_mpx.h, stage_tile) with the baseband side or the audio side (fmd_mpx_passes.h), chosen by its block index -- uniform
// over the workgroup -- on the kernel's one set of LDS (the 16 KiB pair buffer, the taps, the NCO table, the audio side's block
// estimates: 19504 B, what the stereo bank's pass holds).  The baseband tiles come first in the grid: a baseband tile keeps one lane
// per output busy through its whole tap loop and RDS filters are the long ones (at R = 32 with 255 taps a tile has 54 outputs, one
// wave of four, for 255 dependent rounds, against 256 outputs for 127 rounds of an audio tile), so they are the longer-running
// kind, and started last they would be the grid's tail with most of every CU idle.  The audio side writes the next call's block
// carry, as in the stereo bank; the baseband side does not (ReceiverBasebandPass), so one workgroup per row writes it.
// Both choices were measured: the one launch is 1 - 2 % faster per call than the two banks' second passes launched one
// after the other behind the one multiplex pass, and faster than the same grid with the audio tiles first.
// The host side is fmd_stereo_mpx.h's, with two MpxStage over the one MpxState.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include "fmd_ddc.h"
#include "fmd_internal.h"
#include "fmd_mpx_passes.h"
#include "fmd_stereo_mpx.h"

namespace fmd_rx {

using fmd_ddc::kThreads;

struct ReceiverLaunch {
    fmd_rdsk::BasebandLaunch r;
    fmd_sto::AudioLaunch a;
    uint32_t nb_r;             // baseband tiles of the grid, r.SK r.ntiles: blocks [0, nb_r); the audio tiles follow
};

// the RDS bank's side, except that the audio side of the same launch writes the block carry
struct ReceiverBasebandPass : fmd_rdsk::BasebandPass {
    static constexpr bool kCarry = false;
};

__global__ void __launch_bounds__(kThreads) fmd_receiver_second_kernel(const ReceiverLaunch L)
{
    __shared__ __attribute__((aligned(16))) int2 ps[fmd_sto::kStageSlots];
    __shared__ int32_t gl[256];
    __shared__ int16_t tab[1024];
    __shared__ int32_t est[fmd_sto::kMaxBlocks][3];
    if (blockIdx.x < L.nb_r) fmd_sto::stage_tile(L.r, ReceiverBasebandPass{}, blockIdx.x, ps, gl, tab);
    else fmd_sto::stage_tile(L.a, fmd_sto::AudioPass{est, 0}, blockIdx.x - L.nb_r, ps, gl, tab);
}

}  // namespace fmd_rx

struct fmd_receiver {
    FmdDdcBank bank;
    fmd_sto::MpxState mpx;
    fmd_sto::MpxStage audio, rds;
};

namespace {

int rx_enqueue(fmd_receiver* h, const void* d_iq, size_t nbytes, void* d_audio, size_t audio_cap, size_t* n_audio, void* d_rds,
               size_t rds_cap, size_t* n_rds, hipStream_t stream)
{
    using namespace fmd_sto;
    MpxCall q;
    MpxLaunch A{};
    StageOut so[2] = {{&h->audio, d_audio, audio_cap, {}}, {&h->rds, d_rds, rds_cap, {}}};
    if (const int rc = mpx_plan_call(h->bank, h->mpx, so, d_iq, nbytes, q, A)) return rc;
    fmd_rx::ReceiverLaunch B{};
    stage_fill(B.a, h->bank, h->mpx, q, so[0]);
    B.a.inc_p = h->mpx.inc_p;
    B.a.thr = (uint64_t)h->mpx.pilot_min * h->mpx.P * 8192u;
    stage_fill(B.r, h->bank, h->mpx, q, so[1]);
    B.r.inc3 = 3u * h->mpx.inc_p;
    B.nb_r = (uint32_t)(so[1].c.nt * q.SK);
    const uint32_t nb_a = (uint32_t)(so[0].c.nt * q.SK);
    if (const int rc = mpx_enqueue(h->bank, h->mpx, q, A, stream)) return rc;
    hipLaunchKernelGGL(fmd_rx::fmd_receiver_second_kernel, dim3(B.nb_r + nb_a), dim3(fmd_rx::kThreads), 0, stream, B);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(h->bank.core, stream, q.ns);
    if (n_audio) *n_audio = (size_t)so[0].c.NA;
    if (n_rds) *n_rds = (size_t)so[1].c.NA;
    return FMD_OK;
}

}  // namespace

extern "C" {

int fmd_receiver_new(const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc, uint32_t n_stations,
                     const int16_t* audio_taps, uint32_t n_audio_taps, const int16_t* rds_taps, uint32_t n_rds_taps,
                     const fmd_receiver_config* cfg, const fmd_device_config* dev, fmd_receiver** out)
{
    using namespace fmd_sto;
    if (!cfg) { fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG; }
    // the rate floor is the RDS bank's, the stricter of the two
    if (const int rc = mpx_args(fmd_rdsk::kBasebandLimits.rate_floor, taps, n_taps, decim, shift, phase_inc, n_stations,
                                audio_taps && rds_taps, cfg->capture_rate, cfg->block, dev, out)) return rc;
    uint64_t gsum;
    if (const int rc = stage_limits(kAudioLimits, audio_taps, n_audio_taps, cfg->audio_decim, cfg->audio_shift, cfg->pilot_min, &gsum)) return rc;
    if (const int rc = stage_limits(fmd_rdsk::kBasebandLimits, rds_taps, n_rds_taps, cfg->rds_decim, cfg->rds_shift, cfg->pilot_min, &gsum)) return rc;
    if (const int rc = fmd_rdsk::store_check(gsum, cfg->rds_shift)) return rc;
    return mpx_new(taps, n_taps, decim, shift, phase_inc, n_stations, dev, fmd_receiver_free, out, [&](fmd_receiver& h) {
        mpx_init(h.bank, h.mpx, cfg->block, cfg->pilot_min, cfg->capture_rate);
        stage_add(h.bank, h.audio, cfg->audio_decim, cfg->audio_shift, audio_taps, n_audio_taps, audio_room(n_audio_taps));
        stage_add(h.bank, h.rds, cfg->rds_decim, cfg->rds_shift, rds_taps, n_rds_taps, fmd_rdsk::baseband_room(n_rds_taps));
    });
}

void fmd_receiver_free(fmd_receiver* h)
{
    if (!h) return;
    fmd_ddc_free(h->bank.core);
    delete h;
}

int fmd_receiver_reset(fmd_receiver* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_reset(h->bank.core);
}

int fmd_receiver_run_device(fmd_receiver* h, const void* d_iq, size_t nbytes, void* d_audio, size_t audio_cap, size_t* n_audio, void* d_rds,
                            size_t rds_cap, size_t* n_rds, void* stream)
{
    if (!d_rds) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_run_device(h ? &h->bank.core : nullptr, d_iq, d_audio, [&] {
        return rx_enqueue(h, d_iq, nbytes, d_audio, audio_cap, n_audio, d_rds, rds_cap, n_rds, static_cast<hipStream_t>(stream));
    });
}

int fmd_receiver_check(fmd_receiver* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_check(h->bank.core);
}

// Both outputs in the core's one staging buffer, the baseband behind the audio at a 256-byte boundary, copied back separately.
int fmd_receiver_run_batch(fmd_receiver* h, const uint8_t* iq, size_t nbytes, int16_t* audio, size_t audio_cap, size_t* n_audio,
                           int16_t* rds, size_t rds_cap, size_t* n_rds)
{
    if (!h || !iq || !audio || !n_audio || !rds || !n_rds) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FmdDdcCore& c = h->bank.core;
    const size_t rows = (size_t)h->bank.S * h->bank.K;
    const size_t a_bytes = audio_cap * rows * sizeof(uint32_t), r_bytes = rds_cap * rows * sizeof(uint32_t);   // (L, R), (ur, ui) pairs
    const size_t r_off = (a_bytes + 255u) & ~(size_t)255u;
    FMD_DDC_ON_DEVICE(c.device);
    size_t na = 0, nr = 0;
    const int rc = fmd_ddc_batch_enqueue(h->bank, iq, nbytes, r_off + r_bytes, audio_cap, &na,
                                         [&](const void* d_iq, size_t nb, void* d_out, size_t cap, size_t* n, hipStream_t stream) {
        return rx_enqueue(h, d_iq, nb, d_out, cap, n, static_cast<char*>(d_out) + r_off, rds_cap, &nr, stream);
    });
    if (rc) {
        (void)hipStreamSynchronize(c.stream);
        return rc;
    }
    FMD_DDC_TRY(hipMemcpyAsync(audio, c.d_out, a_bytes, hipMemcpyDeviceToHost, c.stream));
    FMD_DDC_TRY(hipMemcpyAsync(rds, static_cast<char*>(c.d_out) + r_off, r_bytes, hipMemcpyDeviceToHost, c.stream));
    FMD_DDC_TRY(hipStreamSynchronize(c.stream));
    *n_audio = na; *n_rds = nr;
    return FMD_OK;
}

int fmd_receiver_outputs(const fmd_receiver* h, uint64_t* audio, uint64_t* rds)
{
    if (!h || !audio || !rds) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *audio = fmd_sto::stage_count(h->bank, h->audio);
    *rds = fmd_sto::stage_count(h->bank, h->rds);
    return FMD_OK;
}

int fmd_receiver_pilot(fmd_receiver* h, uint32_t stream, uint32_t station, int* present, uint32_t* level)
{
    if (!h || !present || !level) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_sto::mpx_pilot(h->bank, h->mpx, stream, station, present, level);
}

int fmd_receiver_kernel_name(const fmd_receiver* h, uint32_t pass, char* name, size_t cap)
{
    if (!h || !name || cap == 0 || pass > 1) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, pass == 0 ? "fmd_sto::fmd_stereo_mpx_kernel" : "fmd_rx::fmd_receiver_second_kernel"), cap);
}

}  // extern "C"
