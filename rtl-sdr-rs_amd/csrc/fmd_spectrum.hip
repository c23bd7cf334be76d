// fmd_spectrum.hip -- power-spectrum scanner: the integrated power of N DFT bins of every IQ stream, in ONE gfx950 kernel.
//
// Definition (include/fmd.h, "power spectrum"; tests/spectrum_ref.py): per stream, frames of N samples on a hop of `hop` samples,
//     z[k][f] = sum_{t < N} W[k][t] c[f hop + t]      (W = window x NCO twiddles at inc_k = k 2^32 / N, c = raw bytes - 127)
//     P[k]    = sum_f (zr^2 + zi^2) >> shift          (u64, natural DFT order)
// A DFT bin is a station-bank filter whose decimation is the hop and which needs no back-rotation, so the tap matrix and its
// centring constants are the station bank's (fmd_ddc.h: fmd_st_complex_taps, the i8 digits, W = 128 hi + lo).
// Unlike the bank the tap matrix is the same for every stream and every frame starts 16-byte aligned, so this is a GEMM proper:
//   rows    = bin x {zr, zi} x i8 digit (a 16-row tile holds (zr_lo, zr_hi, zi_lo, zi_hi) of 4 bins, or (zr, zi) of 8),
//   K       = the frame's 2 N bytes, padded with zero A entries to whole 64-byte chunks,
//   columns = frames; one wave takes G groups of 16 consecutive frames of one stream at a time.
// v_mfma_i32_16x16x64_i8 with B = the frame bytes xor 0x80 (-> s8, c = B + 1).  Operand traffic: a wave loads its frames' bytes ONCE
// from global memory into registers (G x NKC fragments, each byte of a hop = N scan is read by exactly one lane) and keeps them for
// every row tile; the A fragments -- 1 KiB per (row tile, K chunk), the same for every wave -- stream from L2, one row tile ahead,
// and each serves G MFMAs.  No LDS staging: no byte is shared between waves (at hop < N the overlap between a wave's own frames is served by L1).
// Epilogue, lane-local thanks to the 16x16 output layout (lane (j, q) holds rows 4 q ... 4 q + 3 of column j): digits recombined,
// centring constants added, the 64-bit square shifted and summed over the lane's frames, then a 16-lane shuffle sum over the
// columns, one LDS u64 add per (wave, bin), and after the block one global 64-bit atomic add per (block, bin).  Integer adds keep
// the result bit-exact whatever the order.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_ddc.h"

namespace fmd_sp {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
typedef int sp_i4 __attribute__((ext_vector_type(4)));

struct SpLaunch {
    const uint8_t* iq;          // [S][nbytes]
    uint64_t nbytes;
    uint32_t hop, F, fpb;       // frame step (samples), frames per stream, frames per block
    uint32_t n_bins, nrt, digits, shift;
    uint32_t aligned;           // every frame start is 16-byte aligned in memory (row base and nbytes)
    const sp_i4* amat;          // [nrt][NKC][64 lanes]
    const int32_t* kconst;      // [n_bins][2]: the additive constants of zr, zi
    unsigned long long* power;  // [S][n_bins]
};

// G groups of 16 frames per wave: the B fragments of a batch take 4 G NKC VGPRs
template <int NKC> struct SpShape { static constexpr int G = NKC >= 8 ? 4 : 8; };

__device__ __forceinline__ unsigned long long sum16(unsigned long long v)     // over the 16 lanes of one q row
{
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, 16);
    return v;
}

__device__ __forceinline__ unsigned long long frame_power(int zr, int zi, uint32_t shift)
{
    return ((unsigned long long)((long long)zr * zr) + (unsigned long long)((long long)zi * zi)) >> shift;
}

template <int NKC>
__global__ void __launch_bounds__(kThreads) fmd_spectrum_power_kernel(const SpLaunch L)
{
    constexpr int G = SpShape<NKC>::G;
    extern __shared__ __attribute__((aligned(16))) unsigned long long sp_lds[];
    unsigned long long* const part = sp_lds;                                  // [n_bins] the block's sums
    int32_t* const kc = reinterpret_cast<int32_t*>(sp_lds + L.n_bins);        // [n_bins][2]
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t s = blockIdx.y;
    const uint32_t f_begin = blockIdx.x * L.fpb;
    const uint32_t f_end = L.F - f_begin < L.fpb ? L.F : f_begin + L.fpb;
    for (uint32_t i = tid; i < L.n_bins; i += kThreads) {
        part[i] = 0ull;
        kc[2u * i] = L.kconst[2u * i];
        kc[2u * i + 1u] = L.kconst[2u * i + 1u];
    }
    __syncthreads();

    const uint32_t j = lane & 15u, q = lane >> 4;
    const uint8_t* const row = L.iq + (uint64_t)s * L.nbytes;
    const uint32_t kbytes = 2u * L.n_bins;
    typedef const FMD_DDC_GLOBAL sp_i4* gq;
    typedef const FMD_DDC_GLOBAL uint32_t* gw;
    for (uint32_t fb = f_begin + 16u * G * wave; fb < f_end; fb += 16u * G * kWaves) {
        // ---- the batch's frame bytes, straight into registers ------------------------------------------------------------
        sp_i4 B[G][NKC];
        bool valid[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const uint32_t f = fb + 16u * g + j;
            valid[g] = f < f_end;
            const uint8_t* const fr = row + 2ull * L.hop * f;
#pragma unroll
            for (int c = 0; c < NKC; ++c) {
                const uint32_t off = 64u * c + 16u * q;
                sp_i4 v = sp_i4{0, 0, 0, 0};
                if (valid[g] && off < kbytes) {                  // (K padding and frames past the block are never read)
                    if (L.aligned) {
                        v = *(gq)(uintptr_t)(fr + off);
                    } else {
                        const gw p = (gw)(uintptr_t)(fr + off);
                        v = sp_i4{(int)p[0], (int)p[1], (int)p[2], (int)p[3]};
                    }
                    v = v ^ (int)0x80808080;                     // u8 -> s8
                }
                B[g][c] = v;
            }
        }
        // ---- every row tile against the batch, then the epilogue -----------------------------------------------------------
        const gq amat = (gq)(uintptr_t)L.amat + lane;
        sp_i4 A[NKC], An[NKC];                                   // this row tile's A fragments and the next one's (in flight)
#pragma unroll
        for (int c = 0; c < NKC; ++c) An[c] = amat[c * 64u];
        for (uint32_t rt = 0; rt < L.nrt; ++rt) {
#pragma unroll
            for (int c = 0; c < NKC; ++c) A[c] = An[c];
            if (rt + 1u < L.nrt) {
#pragma unroll
                for (int c = 0; c < NKC; ++c) An[c] = amat[((rt + 1u) * NKC + c) * 64u];
            }
            sp_i4 acc[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                acc[g] = sp_i4{0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < NKC; ++c) acc[g] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[c], B[g][c], acc[g], 0, 0, 0);
            }
            if (L.digits == 2u) {                                // rows (zr_lo, zr_hi, zi_lo, zi_hi) of bin 4 rt + q
                const uint32_t k = 4u * rt + q;
                const int cr = kc[2u * k], ci = kc[2u * k + 1u];
                unsigned long long p = 0ull;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int zr = (int)((uint32_t)acc[g].x + ((uint32_t)acc[g].y << 7)) + cr;
                    const int zi = (int)((uint32_t)acc[g].z + ((uint32_t)acc[g].w << 7)) + ci;
                    if (valid[g]) p += frame_power(zr, zi, L.shift);
                }
                p = sum16(p);
                if (j == 0u) atomicAdd(&part[k], p);
            } else {                                             // rows (zr, zi) of bins 8 rt + 2 q and 8 rt + 2 q + 1
                const uint32_t k = 8u * rt + 2u * q;
                const int cr0 = kc[2u * k], ci0 = kc[2u * k + 1u], cr1 = kc[2u * k + 2u], ci1 = kc[2u * k + 3u];
                unsigned long long p0 = 0ull, p1 = 0ull;
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (valid[g]) {
                        p0 += frame_power(acc[g].x + cr0, acc[g].y + ci0, L.shift);
                        p1 += frame_power(acc[g].z + cr1, acc[g].w + ci1, L.shift);
                    }
                p0 = sum16(p0);
                p1 = sum16(p1);
                if (j == 0u) { atomicAdd(&part[k], p0); atomicAdd(&part[k + 1u], p1); }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < L.n_bins; i += kThreads)
        if (part[i]) atomicAdd(L.power + (uint64_t)s * L.n_bins + i, part[i]);
}

}  // namespace fmd_sp

struct fmd_spectrum {
    uint32_t N = 0, hop = 0, shift = 0, S = 0;
    uint32_t digits = 2, nrt = 0, nkc = 0;
    FmdDdcCore core;                                      // core.d_out: the host entry point's power sums
};

namespace {

bool sp_valid_bins(uint32_t n) { return n == 16 || n == 32 || n == 64 || n == 128 || n == 256; }

// One tap row per bin, mixed by inc_k = k 2^32 / N; every frame starts 16-byte aligned (one delta, no slack in K).
void sp_build_plan(const int16_t* w, uint32_t N, FmdDdcPlan& P)
{
    std::vector<uint32_t> inc(N);
    for (uint32_t k = 0; k < N; ++k) inc[k] = k * (uint32_t)((1ull << 32) / N);
    fmd_ddc_build_plan(w, N, inc.data(), 1u, N, 1u, (2u * N + 63u) / 64u, P);
}

uint64_t sp_frames(uint32_t N, uint32_t hop, uint64_t nbytes)
{
    const uint64_t ns = nbytes / 2;
    return ns < N ? 0 : (ns - N) / hop + 1;
}

// Refusals that need no device: BAD_LENGTH, TOO_SHORT (nothing is written), the 32-bit frame range.
int sp_check_len(const fmd_spectrum* h, size_t nbytes, uint64_t* F)
{
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    *F = sp_frames(h->N, h->hop, nbytes);
    if (*F == 0) { fmd_internal_set_err("the call holds no complete frame (nbytes / 2 < n_bins)"); return FMD_ERR_TOO_SHORT; }
    if (*F > (1ull << 31)) { fmd_internal_set_err("call too large: more than 2^31 frames per stream"); return FMD_ERR_UNSUPPORTED; }
    return FMD_OK;
}

int sp_enqueue(fmd_spectrum* h, const void* d_iq, size_t nbytes, uint64_t F, void* d_power, bool accumulate, hipStream_t stream)
{
    using namespace fmd_sp;
    SpLaunch L{};
    L.iq = static_cast<const uint8_t*>(d_iq);
    L.nbytes = nbytes;
    L.hop = h->hop; L.F = (uint32_t)F;
    L.n_bins = h->N; L.nrt = h->nrt; L.digits = h->digits; L.shift = h->shift;
    L.aligned = ((uintptr_t)d_iq & 15u) == 0 && nbytes % 16 == 0 ? 1u : 0u;
    L.amat = reinterpret_cast<const sp_i4*>(h->core.d_amat);
    L.kconst = h->core.d_kconst;
    L.power = static_cast<unsigned long long*>(d_power);
    // blocks: about 2048 over the whole grid, each at least one batch of every wave
    const uint32_t batch = 16u * (h->nkc >= 8 ? 4u : 8u);
    const uint64_t per_block_min = (uint64_t)batch * kWaves;
    uint64_t bps = (2048u + h->S - 1u) / h->S;
    const uint64_t most = (F + per_block_min - 1) / per_block_min;
    if (bps > most) bps = most;
    if (bps < 1) bps = 1;
    uint64_t fpb = (F + bps - 1) / bps;
    fpb = (fpb + batch - 1) / batch * batch;
    bps = (F + fpb - 1) / fpb;
    L.fpb = (uint32_t)fpb;
    FMD_DDC_TRY(h->core.order.before(stream));
    if (!accumulate) FMD_DDC_TRY(hipMemsetAsync(d_power, 0, (size_t)h->S * h->N * sizeof(uint64_t), stream));
    const size_t lds = (size_t)h->N * 16u;
    const dim3 grid((uint32_t)bps, h->S), block(kThreads);
    switch (h->nkc) {
    case 1: hipLaunchKernelGGL(fmd_spectrum_power_kernel<1>, grid, block, lds, stream, L); break;
    case 2: hipLaunchKernelGGL(fmd_spectrum_power_kernel<2>, grid, block, lds, stream, L); break;
    case 4: hipLaunchKernelGGL(fmd_spectrum_power_kernel<4>, grid, block, lds, stream, L); break;
    default: hipLaunchKernelGGL(fmd_spectrum_power_kernel<8>, grid, block, lds, stream, L); break;
    }
    FMD_DDC_TRY(hipGetLastError());
    (void)h->core.order.after(stream);
    return FMD_OK;
}

}  // namespace

extern "C" {

int fmd_spectrum_hann(uint32_t n_bins, uint32_t amplitude, int16_t* window)
{
    if (!window) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (!sp_valid_bins(n_bins) || amplitude < 1 || amplitude > 2047) {
        fmd_internal_set_err("need n_bins in {16, 32, 64, 128, 256} and 1 <= amplitude <= 2047");
        return FMD_ERR_UNSUPPORTED;
    }
    int16_t tab[1024];
    fmd_st_nco_table(tab);
    for (uint32_t n = 0; n < n_bins; ++n)
        window[n] = (int16_t)(((int32_t)amplitude * (16384 - tab[(n * (1024u / n_bins)) & 1023u]) + 16384) >> 15);
    return FMD_OK;
}

int fmd_spectrum_bin_inc(uint32_t bin, uint32_t n_bins, uint32_t* inc)
{
    if (!inc) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (!sp_valid_bins(n_bins) || bin >= n_bins) { fmd_internal_set_err("need a valid n_bins and bin < n_bins"); return FMD_ERR_UNSUPPORTED; }
    *inc = bin * (uint32_t)((1ull << 32) / n_bins);
    return FMD_OK;
}

size_t fmd_spectrum_frames(uint32_t n_bins, uint32_t hop, size_t nbytes)
{
    if (!sp_valid_bins(n_bins) || hop < 8 || hop % 8 != 0 || hop > n_bins) return 0;
    return (size_t)sp_frames(n_bins, hop, nbytes);
}

int fmd_spectrum_new(const int16_t* window, uint32_t n_bins, uint32_t hop, uint32_t shift, const fmd_device_config* dev,
                     fmd_spectrum** out)
{
    if (!window || !dev || !out || dev->n_channels == 0) { fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!sp_valid_bins(n_bins) || hop < 8 || hop % 8 != 0 || hop > n_bins || shift > 63 || dev->n_channels > 65535u) {
        fmd_internal_set_err("need n_bins in {16, 32, 64, 128, 256}, hop a multiple of 8 in 8 ... n_bins, shift <= 63, n_streams <= 65535");
        return FMD_ERR_UNSUPPORTED;
    }
    for (uint32_t t = 0; t < n_bins; ++t)
        if (window[t] > 2047 || window[t] < -2047) { fmd_internal_set_err("|window| > 2047"); return FMD_ERR_UNSUPPORTED; }
    fmd_spectrum* h = new (std::nothrow) fmd_spectrum();
    if (!h) return FMD_ERR_NOMEM;
    h->N = n_bins; h->hop = hop; h->shift = shift; h->S = dev->n_channels;
    FmdDdcPlan P;
    sp_build_plan(window, n_bins, P);
    h->digits = P.digits; h->nrt = P.nrt; h->nkc = P.nkc;

    if (const int rc = fmd_ddc_open(h->core, dev)) { delete h; return rc; }
    auto fail = [&](const char* what) { fmd_internal_set_err(what); fmd_spectrum_free(h); return FMD_ERR_HIP; };
    FmdDeviceGuard guard(h->core.device);
    if (guard.error() != hipSuccess) return fail("hipSetDevice");
    if (const char* what = fmd_ddc_upload(h->core, P, 0)) return fail(what);
    if (fmd_ddc_grow(h->core.d_out, h->core.d_out_cap, (size_t)h->S * n_bins * sizeof(uint64_t)) != hipSuccess) return fail("hipMalloc(power)");
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    *out = h;
    return FMD_OK;
}

void fmd_spectrum_free(fmd_spectrum* h)
{
    if (!h) return;
    FmdDeviceGuard guard(h->core.device);
    fmd_ddc_release(h->core);
    delete h;
}

int fmd_spectrum_power_batch(fmd_spectrum* h, const uint8_t* iq, size_t nbytes, uint64_t* power)
{
    if (!h || !iq || !power) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    uint64_t F = 0;
    int rc = sp_check_len(h, nbytes, &F);
    if (rc) return rc;
    FMD_DDC_ON_DEVICE(h->core.device);
    FmdDdcCore& c = h->core;
    const size_t in_bytes = nbytes * (size_t)h->S;
    FMD_DDC_TRY(fmd_ddc_grow(c.d_iq, c.d_iq_cap, in_bytes));
    FMD_DDC_TRY(hipMemcpyAsync(c.d_iq, iq, in_bytes, hipMemcpyHostToDevice, c.stream));
    rc = sp_enqueue(h, c.d_iq, nbytes, F, c.d_out, false, c.stream);
    if (rc) return rc;
    FMD_DDC_TRY(hipMemcpyAsync(power, c.d_out, (size_t)h->S * h->N * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream));
    FMD_DDC_TRY(hipStreamSynchronize(c.stream));
    return FMD_OK;
}

int fmd_spectrum_power_device(fmd_spectrum* h, const void* d_iq, size_t nbytes, void* d_power, int accumulate, void* stream)
{
    if (!h || !d_iq || !d_power) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    uint64_t F = 0;
    int rc = sp_check_len(h, nbytes, &F);
    if (rc) return rc;
    if (((uintptr_t)d_iq & 3u) != 0 || ((uintptr_t)d_power & 7u) != 0) { fmd_internal_set_err("misaligned device buffer"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->core.device);
    return sp_enqueue(h, d_iq, nbytes, F, d_power, accumulate != 0, static_cast<hipStream_t>(stream));
}

int fmd_spectrum_check(fmd_spectrum* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_check(h->core);
}

int fmd_spectrum_tap_digits(const fmd_spectrum* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    return (int)h->digits;
}

int fmd_spectrum_kernel_name(const fmd_spectrum* h, char* name, size_t cap)
{
    if (!h || !name || cap == 0) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, "fmd_sp::fmd_spectrum_power_kernel<%u>", h->nkc), cap);
}

}  // extern "C"
