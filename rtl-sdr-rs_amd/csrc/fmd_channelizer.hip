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
    FmdDdcBank bank;
    FmdDdcTiling tl;
};

namespace {

int ch_enqueue(fmd_channelizer* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream)
{
    if (const int rc = fmd_ddc_check_call(nbytes, d_iq, d_out, 4u)) return rc;
    const FmdDdcBank& b = h->bank;
    FmdDdcCore& c = h->bank.core;
    const uint64_t ns = nbytes / 2;
    const uint64_t m0 = fmd_ddc_outputs(b.T, b.D, c.pos), M = fmd_ddc_outputs(b.T, b.D, c.pos + ns) - m0;
    if (M < 1) { fmd_internal_set_err("the call completes no filter output"); return FMD_ERR_TOO_SHORT; }
    if (M > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    const uint64_t ntiles = (M + h->tl.tile - 1) / h->tl.tile;
    if (ntiles > (1u << 30) || b.S > 65535u) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }
    fmd_ch::ChLaunch L{};
    fmd_ddc_fill_front(L, b, d_iq, nbytes, m0);
    L.m0_lo = (uint32_t)m0;
    L.M = (uint32_t)M;
    L.groups = h->tl.groups; L.tile = h->tl.tile; L.ntiles = (uint32_t)ntiles; L.raw_bytes = h->tl.raw_bytes;
    L.vec4 = (((uintptr_t)d_out & 15u) == 0 && out_cap % 4 == 0) ? 1u : 0u;
    L.out = static_cast<uint32_t*>(d_out); L.out_stride = out_cap;
    FMD_DDC_TRY(c.order.before(stream));
    hipLaunchKernelGGL(fmd_ch::fmd_channelizer_kernel, dim3(L.ntiles, b.S), dim3(fmd_ch::kThreads), h->tl.lds, stream, L);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(c, stream, ns);
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
    fmd_channelizer* h = new (std::nothrow) fmd_channelizer();
    if (!h) return FMD_ERR_NOMEM;
    uint64_t bound;
    if (const int rc = fmd_ddc_bank_front(h->bank, taps, n_taps, decim, shift, phase_inc, n_stations, dev, &bound)) { delete h; return rc; }
    h->tl = fmd_ddc_tiling(decim, h->bank.plan.nkc, n_taps, n_stations);

    const char* what;
    if (const int rc = fmd_ddc_bank_device(h->bank, dev, &what)) {
        if (!what) { delete h; return rc; }
        fmd_internal_set_err(what); fmd_channelizer_free(h); return rc;
    }
    *out = h;
    return FMD_OK;
}

void fmd_channelizer_free(fmd_channelizer* h)
{
    if (!h) return;
    fmd_ddc_free(h->bank.core);
    delete h;
}

int fmd_channelizer_reset(fmd_channelizer* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_reset(h->bank.core);
}

int fmd_channelizer_run_device(fmd_channelizer* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len,
                               void* stream)
{
    return fmd_ddc_run_device(h ? &h->bank.core : nullptr, d_iq, d_out,
                              [&] { return ch_enqueue(h, d_iq, nbytes, d_out, out_cap, out_len, static_cast<hipStream_t>(stream)); });
}

int fmd_channelizer_check(fmd_channelizer* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_check(h->bank.core);
}

int fmd_channelizer_run_batch(fmd_channelizer* h, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!h || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    const size_t out_bytes = out_cap * h->bank.S * h->bank.K * sizeof(uint32_t);   // (yr, yi) pairs
    return fmd_ddc_run_batch(h->bank, iq, nbytes, out, out_bytes, out_cap, out_len, [h](auto... a) { return ch_enqueue(h, a...); });
}

int fmd_channelizer_outputs(const fmd_channelizer* h, uint64_t* outputs)
{
    if (!h || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *outputs = fmd_ddc_outputs(h->bank.T, h->bank.D, h->bank.core.pos);
    return FMD_OK;
}

int fmd_channelizer_kernel_name(const fmd_channelizer* h, char* name, size_t cap)
{
    if (!h || !name || cap == 0) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, "fmd_ch::fmd_channelizer_kernel"), cap);
}

}  // extern "C"
