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
// Pass 2 (fmd_stereo_audio_kernel) is the second-pass tile that this bank and the RDS bank share (fmd_stereo_mpx.h, stage_tile: one
// workgroup = one (stream, station) row and one tile of up to 256 audio samples, the pairs of every MPX sample the tile's FIR reads
// in LDS, the last Ta - 1 of them carried from call to call, one lane per audio sample) with this bank's side (AudioPass):
//   - before the staging, the estimate (present, c2, s2) of each block the tile's inputs need, one lane per block;
//   - the pair (x, s), s = (x kc) >> 14 with kc from the NCO table in LDS;
//   - from the two FIR sums (|g| <= 16383, |x| <= 32768, |s| <= 65540 fit v_mad_i32_i24's 24-bit operands) the matrix step, the
//     saturation, one dword store of the (L, R) pair.
// AudioPass and its launch struct are in fmd_mpx_passes.h, where the receiver bank finds them too.
// The host side of the second stage -- handle, constructor, launch fields, enqueue -- is that header's as well.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include "fmd_ddc.h"
#include "fmd_device.h"
#include "fmd_internal.h"
#include "fmd_mpx_passes.h"
#include "fmd_stereo_mpx.h"

namespace fmd_sto {

using fmd_ddc::kThreads;
using fmd_ddc::kTableBytes;

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

__global__ void __launch_bounds__(kThreads) fmd_stereo_audio_kernel(const AudioLaunch L)
{
    __shared__ __attribute__((aligned(16))) int2 ps[kStageSlots];
    __shared__ int32_t gl[256];
    __shared__ int16_t tab[1024];
    __shared__ int32_t est[kMaxBlocks][3];
    stage_tile(L, AudioPass{est, 0}, blockIdx.x, ps, gl, tab);
}

}  // namespace fmd_sto

struct fmd_stereo : fmd_sto::MpxHandle {};

namespace {

constexpr fmd_sto::StageLimits kLimits = fmd_sto::kAudioLimits;

int st_enqueue(fmd_stereo* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream)
{
    return fmd_sto::stage_enqueue<fmd_sto::AudioLaunch>(*h, d_iq, nbytes, d_out, out_cap, out_len, stream, [&](fmd_sto::AudioLaunch& B, uint32_t grid) {
        B.inc_p = h->mpx.inc_p;
        B.thr = (uint64_t)h->mpx.pilot_min * h->mpx.P * 8192u;
        hipLaunchKernelGGL(fmd_sto::fmd_stereo_audio_kernel, dim3(grid), dim3(fmd_sto::kThreads), 0, stream, B);
    });
}

}  // namespace

extern "C" {

size_t fmd_stereo_out_cap(uint32_t decim, uint32_t audio_decim, size_t nbytes) { return fmd_ddc_fir_out_cap(decim, audio_decim, nbytes); }

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
    if (!cfg) { fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG; }
    const fmd_sto::StageConfig c{cfg->capture_rate, cfg->block, cfg->audio_decim, cfg->audio_shift, cfg->pilot_min};
    uint64_t gsum;
    if (const int rc = fmd_sto::stage_args(kLimits, taps, n_taps, decim, shift, phase_inc, n_stations, audio_taps, n_audio_taps, c, dev, out, &gsum)) return rc;
    return fmd_sto::stage_new(taps, n_taps, decim, shift, phase_inc, n_stations, audio_taps, n_audio_taps, c, fmd_sto::audio_room(n_audio_taps), dev,
                              fmd_stereo_free, out);
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

int fmd_stereo_outputs(const fmd_stereo* h, uint64_t* outputs) { return fmd_sto::stage_outputs(h, outputs); }

int fmd_stereo_pilot(fmd_stereo* h, uint32_t stream, uint32_t station, int* present, uint32_t* level)
{
    return fmd_sto::stage_pilot(h, stream, station, present, level);
}

int fmd_stereo_kernel_name(const fmd_stereo* h, uint32_t pass, char* name, size_t cap)
{
    if (!h || !name || cap == 0 || pass > 1) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, pass == 0 ? "fmd_sto::fmd_stereo_mpx_kernel" : "fmd_sto::fmd_stereo_audio_kernel"), cap);
}

}  // extern "C"
