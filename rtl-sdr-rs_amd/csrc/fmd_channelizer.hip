// fmd_channelizer.hip -- channelizer: K digital down-converters per wideband IQ stream, each returning the station's decimated
// complex baseband, in ONE gfx950 kernel.
//
// Definition (include/fmd.h, "channelizer"; tests/channelizer_ref.py): the station bank's steps 1 - 5, nothing after them.  Per
// (stream, station k) the complex tapped FIR
//     z[k][m] = sum_t W[k][t] c[D m + t]      (W = the real prototype h mixed to the station's offset, c = raw bytes - 127)
// rotated back to baseband by the NCO and normalised by >> (14 + shift): y[k][m], stored as the int16 pair (yr, yi).
//
// One workgroup = one tile of `tile` consecutive filter outputs of ONE stream (tile = 64 G, G = 16-column groups per wave, 1 ... 4,
// fixed per handle by the LDS budget), for all K stations of it:
//   1. stage the raw bytes of the tile's filter windows in LDS (global_load_lds_dwordx4; through registers where the range touches
//      the stream's history or is not 16-byte aligned), and the NCO table;
//   2. the contraction on the matrix cores, v_mfma_i32_16x16x64_i8, with the station bank's A fragments (one or two i8 digits)
//      and B = window bytes (xor 0x80 -> s8), one column per filter output; wave w takes the outputs w + 4 i, whose windows
//      share one 16-byte offset delta that the host-built fragments absorb;
//   3. per (station, output): the additive centring constant, the rotation by the NCO (table in LDS, i64 products), the
//      normalising shift; packed re | im << 16 into LDS, one row of `tile` dwords per station;
//   4. the rows leave LDS as whole segments: each wave instruction stores 1 KiB of one station's row (dwordx4 per lane) when the
//      output rows are 16-byte aligned, 256 B (dword per lane) otherwise.
// Steps 1 - 3 are the station bank's own front end (fmd_ddc.h); only the tile geometry and step 4 are the channelizer's.
// HBM traffic: the u8 input once, the (L2-resident) tap fragments once per block, 4 bytes per (station, output).
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>

#include "fmd_ddc.h"
#include "fmd_internal.h"

namespace fmd_ch {

using fmd_ddc::kThreads;
using fmd_ddc::kTableBytes;

struct ChLaunch {
    const uint8_t* iq;         // [S][nbytes]
    uint64_t nbytes;
    const uint8_t* hist_in;    // [S][HB]: the last HB / 2 samples before the call
    uint8_t* hist_out;
    uint32_t HB;               // history bytes per stream (multiple of 16)
    uint32_t vb_first;         // virtual byte (history ++ call) of the window of the call's first output
    uint32_t m0_lo;            // global index of the call's first output, mod 2^32
    uint32_t M;                // outputs of this call per (stream, station)
    uint32_t D, T, K, S, shift;
    uint32_t nrt, nkc, digits;
    uint32_t groups, tile;     // 16-column groups per wave, outputs per tile (64 groups)
    uint32_t ntiles, raw_bytes;
    uint32_t vec4;             // output rows 16-byte aligned: dwordx4 stores
    const uint32_t* amat;      // [S][4][nrt][nkc][64][4]
    const int32_t* kconst;     // [S][K][2]
    const uint32_t* dinc;      // [S][K]
    const uint32_t* tab;       // NCO table, 512 dwords
    uint32_t* out;             // [S][K][out_stride] packed (yr, yi)
    uint64_t out_stride;
};

__global__ void __launch_bounds__(kThreads) fmd_channelizer_kernel(const ChLaunch L)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t s = blockIdx.y, t = blockIdx.x;
    if (s >= L.S || t >= L.ntiles) return;

    const uint32_t o0 = t * L.tile;                          // first output (of this call) of the tile
    const uint32_t no = L.M - o0 < L.tile ? L.M - o0 : L.tile;
    const uint32_t vb = L.vb_first + 2u * L.D * o0;          // virtual byte of output o0's window
    const uint32_t base = vb & ~15u, d0 = vb - base;
    const uint32_t nq = (d0 + 2u * L.D * (no - 1u) + 2u * L.T + 15u) >> 4;   // 16-byte chunks staged (<= raw_bytes / 16: host plan)
    int16_t* const tab = reinterpret_cast<int16_t*>(lds + (L.raw_bytes >> 2));
    uint32_t* const ypk = lds + ((L.raw_bytes + kTableBytes) >> 2);          // [K][tile]: y of output o0 + i at i

    // ---- 1. staging ---------------------------------------------------------------------------------------------------------
    fmd_ddc::stage(L, s, base, nq, lds, tab, tid, wave);
    if (t == L.ntiles - 1u) fmd_ddc::write_history(L, s, tid);   // the stream's last tile also writes the next call's history
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0): the LDS-DMAs have landed
    __syncthreads();

    // ---- 2./3. contraction on the matrix cores, rotation, packing -----------------------------------------------------------
    fmd_ddc::contract(L, s, wave, lane, d0, no, L.m0_lo + o0, lds, tab, ypk, L.tile, 0u);
    __syncthreads();

    // ---- 4. the stations' rows, whole segments ------------------------------------------------------------------------------
    typedef FMD_DDC_GLOBAL uint32_t* gwo;
    gwo const out = (gwo)(uintptr_t)(L.out + (uint64_t)s * L.K * L.out_stride + o0);
    if (L.vec4) {                                            // out_stride % 4 == 0, 16-byte aligned base, o0 % 4 == 0
        typedef FMD_DDC_GLOBAL fmd_ddc::i4* gqo;
        const uint32_t n4 = no >> 2, rem = no & 3u;
        for (uint32_t idx = tid; idx < L.K * n4; idx += kThreads) {
            const uint32_t k = idx / n4, i = idx - k * n4;
            ((gqo)(out + (uint64_t)k * L.out_stride))[i] = reinterpret_cast<const fmd_ddc::i4*>(ypk + k * L.tile)[i];
        }
        for (uint32_t idx = tid; idx < L.K * rem; idx += kThreads) {
            const uint32_t k = idx / rem, i = 4u * n4 + (idx - k * rem);
            out[(uint64_t)k * L.out_stride + i] = ypk[k * L.tile + i];
        }
    } else {
        for (uint32_t idx = tid; idx < L.K * no; idx += kThreads) {
            const uint32_t k = idx / no, i = idx - k * no;
            out[(uint64_t)k * L.out_stride + i] = ypk[k * L.tile + i];
        }
    }
}

}  // namespace fmd_ch

struct fmd_channelizer {
    uint32_t T = 0, D = 0, K = 0, S = 0, shift = 0, HB = 0;
    uint32_t groups = 0, tile = 0, raw_bytes = 0;
    size_t lds = 0;
    FmdDdcPlan plan;
    FmdDdcCore core;
};

namespace {

using fmd_ddc::kTableBytes;

constexpr size_t kLdsBudget = 40960;                      // 4 tiles per CU

// LDS of a tile of G groups per wave (64 G outputs): raw bytes the matrix phase may read + NCO table + one row per station
size_t ch_lds(uint32_t D, uint32_t nkc, uint32_t T, uint32_t K, uint32_t G, uint32_t* raw_bytes)
{
    const uint64_t cap = 64ull * G;
    const uint64_t reads = 12 + 6ull * D + 8ull * D * (16 * G - 1) + 64ull * nkc;
    const uint64_t staged = 12 + 2ull * D * (cap - 1) + 2ull * T + 15;
    const uint64_t raw = ((reads > staged ? reads : staged) + 15) & ~15ull;
    *raw_bytes = (uint32_t)raw;
    return (size_t)(raw + kTableBytes + 4ull * K * cap);
}

// outputs completed once `S` samples per stream have arrived
uint64_t ch_outputs(const fmd_channelizer* h, uint64_t S) { return S >= h->T ? (S - h->T) / h->D + 1 : 0; }

int ch_enqueue(fmd_channelizer* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream)
{
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    if (nbytes > (1ull << 31) - (1ull << 20)) { fmd_internal_set_err("nbytes out of range"); return FMD_ERR_UNSUPPORTED; }
    if (((uintptr_t)d_iq & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0) { fmd_internal_set_err("misaligned device buffer"); return FMD_ERR_INVALID_ARG; }
    const uint64_t ns = nbytes / 2;
    FmdDdcCore& c = h->core;
    const uint64_t m0 = ch_outputs(h, c.pos), m1 = ch_outputs(h, c.pos + ns);
    const uint64_t M = m1 - m0;
    if (M < 1) { fmd_internal_set_err("the call completes no filter output"); return FMD_ERR_TOO_SHORT; }
    if (M > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    const uint64_t ntiles = (M + h->tile - 1) / h->tile;
    if (ntiles > (1u << 30) || h->S > 65535u) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }
    fmd_ch::ChLaunch L{};
    L.iq = static_cast<const uint8_t*>(d_iq);
    L.nbytes = nbytes;
    L.hist_in = c.d_hist[c.cur]; L.hist_out = c.d_hist[c.cur ^ 1];
    L.HB = h->HB;
    L.vb_first = (uint32_t)(2ull * (h->D * m0 + h->HB / 2 - c.pos));   // >= 0: the window of output m0 starts at most n_taps - 1 samples back
    L.m0_lo = (uint32_t)m0;
    L.M = (uint32_t)M;
    L.D = h->D; L.T = h->T; L.K = h->K; L.S = h->S; L.shift = h->shift;
    L.nrt = h->plan.nrt; L.nkc = h->plan.nkc; L.digits = h->plan.digits;
    L.groups = h->groups; L.tile = h->tile; L.ntiles = (uint32_t)ntiles; L.raw_bytes = h->raw_bytes;
    L.vec4 = (((uintptr_t)d_out & 15u) == 0 && out_cap % 4 == 0) ? 1u : 0u;
    L.amat = c.d_amat; L.kconst = c.d_kconst; L.dinc = c.d_dinc; L.tab = c.d_tab;
    L.out = static_cast<uint32_t*>(d_out); L.out_stride = out_cap;
    FMD_DDC_TRY(c.order.before(stream));
    hipLaunchKernelGGL(fmd_ch::fmd_channelizer_kernel, dim3(L.ntiles, h->S), dim3(fmd_ch::kThreads), h->lds, stream, L);
    FMD_DDC_TRY(hipGetLastError());
    (void)c.order.after(stream);
    c.cur ^= 1;
    c.pos += ns;
    if (out_len) *out_len = (size_t)M;
    return FMD_OK;
}

}  // namespace

extern "C" {

size_t fmd_channelizer_out_cap(uint32_t decim, size_t nbytes)
{
    if (!decim) return 0;
    return (nbytes + 2ull * decim - 1) / (2ull * decim);
}

int fmd_channelizer_new(const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc,
                        uint32_t n_stations, const fmd_device_config* dev, fmd_channelizer** out)
{
    if (!taps || !phase_inc || !dev || !out || dev->n_channels == 0) { fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n_taps == 0 || n_taps > 256 || decim < 2 || decim % 2 != 0 || decim > 64 || shift > 24 || n_stations == 0 || n_stations > 32 ||
        dev->n_channels > 65535u) {
        fmd_internal_set_err("need 1 <= n_taps <= 256, an even 2 <= decim <= 64, shift <= 24, 1 <= n_stations <= 32, n_streams <= 65535");
        return FMD_ERR_UNSUPPORTED;
    }
    for (uint32_t t = 0; t < n_taps; ++t)
        if (taps[t] > 2047 || taps[t] < -2047) { fmd_internal_set_err("|tap| > 2047"); return FMD_ERR_UNSUPPORTED; }
    fmd_channelizer* h = new (std::nothrow) fmd_channelizer();
    if (!h) return FMD_ERR_NOMEM;
    h->T = n_taps; h->D = decim; h->K = n_stations; h->S = dev->n_channels; h->shift = shift;
    fmd_st_build_plan(taps, n_taps, decim, phase_inc, h->S, h->K, h->plan);
    // |y| <= 256 G / 2^shift (|z| <= 128 G per component, the rotation adds two of them): exact in int16 while <= 16384
    const uint64_t bound = (256ull * h->plan.max_gain + ((1ull << shift) - 1ull)) >> shift;
    if (bound > 16384ull) {
        delete h;
        fmd_internal_set_err("filter gain too large for int16 output: need ceil(256 * max sum(|Wr| + |Wi|) / 2^shift) <= 16384");
        return FMD_ERR_UNSUPPORTED;
    }
    for (uint32_t G = fmd_ddc::kGroups; G >= 1; --G) {     // the largest tile within the budget (G = 1 always fits: <= 19 KB)
        uint32_t rb;
        const size_t l = ch_lds(decim, h->plan.nkc, n_taps, n_stations, G, &rb);
        if (l <= kLdsBudget || G == 1) { h->groups = G; h->tile = 64u * G; h->raw_bytes = rb; h->lds = l; break; }
    }
    h->HB = 2u * ((n_taps - 1u + 7u) & ~7u);

    if (const int rc = fmd_ddc_open(h->core, dev)) { delete h; return rc; }
    auto fail = [&](const char* what) { fmd_internal_set_err(what); fmd_channelizer_free(h); return FMD_ERR_HIP; };
    FmdDeviceGuard guard(h->core.device);
    if (guard.error() != hipSuccess) return fail("hipSetDevice");
    if (const char* what = fmd_ddc_upload(h->core, h->plan, (size_t)h->S * (h->HB ? h->HB : 16))) return fail(what);
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    *out = h;
    return FMD_OK;
}

void fmd_channelizer_free(fmd_channelizer* h)
{
    if (!h) return;
    FmdDeviceGuard guard(h->core.device);
    fmd_ddc_release(h->core);
    delete h;
}

int fmd_channelizer_reset(fmd_channelizer* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    FMD_DDC_ON_DEVICE(h->core.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    FMD_DDC_TRY(fmd_ddc_zero_history(h->core));          // (ends with the device synchronised)
    return FMD_OK;
}

int fmd_channelizer_run_device(fmd_channelizer* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len,
                               void* stream)
{
    if (!h || !d_iq || !d_out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->core.device);
    return ch_enqueue(h, d_iq, nbytes, d_out, out_cap, out_len, static_cast<hipStream_t>(stream));
}

int fmd_channelizer_check(fmd_channelizer* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->core.device);
    if (h->core.order.have_last) FMD_DDC_TRY(hipStreamSynchronize(h->core.order.last));
    FMD_DDC_TRY(hipGetLastError());
    return FMD_OK;
}

int fmd_channelizer_run_batch(fmd_channelizer* h, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!h || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->core.device);
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    FmdDdcCore& c = h->core;
    const size_t rows = (size_t)h->S * h->K;
    const size_t in_bytes = nbytes * (size_t)h->S, out_bytes = out_cap * rows * sizeof(uint32_t);   // (yr, yi) pairs
    FMD_DDC_TRY(fmd_ddc_grow(c.d_iq, c.d_iq_cap, in_bytes));
    FMD_DDC_TRY(fmd_ddc_grow(c.d_out, c.d_out_cap, out_bytes));
    FMD_DDC_TRY(hipMemcpyAsync(c.d_iq, iq, in_bytes, hipMemcpyHostToDevice, c.stream));
    size_t n = 0;
    int rc = ch_enqueue(h, c.d_iq, nbytes, c.d_out, out_cap, &n, c.stream);
    if (rc) { (void)hipStreamSynchronize(c.stream); return rc; }
    FMD_DDC_TRY(hipMemcpyAsync(out, c.d_out, out_bytes, hipMemcpyDeviceToHost, c.stream));
    FMD_DDC_TRY(hipStreamSynchronize(c.stream));
    *out_len = n;
    return FMD_OK;
}

int fmd_channelizer_outputs(const fmd_channelizer* h, uint64_t* outputs)
{
    if (!h || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *outputs = ch_outputs(h, h->core.pos);
    return FMD_OK;
}

int fmd_channelizer_kernel_name(const fmd_channelizer* h, char* name, size_t cap)
{
    if (!h || !name || cap == 0) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, "fmd_ch::fmd_channelizer_kernel"), cap);
}

}  // extern "C"
