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
//      the stream's history or is not 16-byte aligned), and the NCO table -- as fmd_stations.hip;
//   2. the contraction on the matrix cores, v_mfma_i32_16x16x64_i8, with the station bank's A fragments (fmd_stations_common.h,
//      one or two i8 digits) and B = window bytes (xor 0x80 -> s8), one column per filter output; wave w takes the outputs
//      w + 4 i, whose windows share one 16-byte offset delta that the host-built fragments absorb;
//   3. per (station, output): the additive centring constant, the rotation by the NCO (table in LDS, i64 products), the
//      normalising shift; packed re | im << 16 into LDS, one row of `tile` dwords per station;
//   4. the rows leave LDS as whole segments: each wave instruction stores 1 KiB of one station's row (dwordx4 per lane) when the
//      output rows are 16-byte aligned, 256 B (dword per lane) otherwise.
// HBM traffic: the u8 input once, the (L2-resident) tap fragments once per block, 4 bytes per (station, output).
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>

#include "fmd_host.h"
#include "fmd_internal.h"
#include "fmd_stations_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define FMD_CH_GLOBAL __attribute__((address_space(1)))
#else
#define FMD_CH_GLOBAL
#endif

namespace fmd_ch {

constexpr int kThreads = 256;
constexpr uint32_t kMaxGroups = 4;                        // 16-column MFMA groups per wave: at most 4 waves x 4 x 16 = 256 outputs per tile
constexpr uint32_t kTableBytes = 2048;                    // 1024 x i16
typedef int ch_i4 __attribute__((ext_vector_type(4)));

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

__device__ __forceinline__ uint32_t virt_dword(const ChLaunch& L, uint32_t s, uint32_t v)   // v: virtual byte, multiple of 4
{
    typedef const FMD_CH_GLOBAL uint32_t* gw;
    if (v < L.HB) return ((gw)(uintptr_t)(L.hist_in + (uint64_t)s * L.HB + v))[0];
    const uint64_t b = (uint64_t)(v - L.HB);
    if (b >= L.nbytes) return 0u;                          // beyond the call: only outputs that are discarded read it
    return ((gw)(uintptr_t)(L.iq + (uint64_t)s * L.nbytes + b))[0];
}

__device__ __forceinline__ void dma16(const unsigned char* g, unsigned char* lds_wave_base)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 2 /* nt */);
}

// rotation back to baseband and the normalising shift (include/fmd.h step 5), packed re | im << 16
__device__ __forceinline__ uint32_t ch_rotate(const int16_t* tab, int zr, int zi, uint32_t psi, uint32_t sh)
{
    const uint32_t ix = psi >> 22;
    const int64_t C = tab[ix], S = tab[(ix - 256u) & 1023u];
    const int yr = (int)(((int64_t)zr * C + (int64_t)zi * S) >> sh);
    const int yi = (int)(((int64_t)zi * C - (int64_t)zr * S) >> sh);
    return ((uint32_t)yr & 0xFFFFu) | ((uint32_t)yi << 16);
}

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
    const uint8_t* const row = L.iq + (uint64_t)s * L.nbytes;
    const bool whole = base >= L.HB && (uint64_t)(base - L.HB) + 16ull * nq <= L.nbytes && (((uintptr_t)row + (base - L.HB)) & 15u) == 0u;
    if (whole) {
        const unsigned char* src = row + (base - L.HB) + 16u * tid;
        unsigned char* dst = reinterpret_cast<unsigned char*>(lds) + 1024u * wave;
        const uint32_t nfull = nq / kThreads, ntail = nq - nfull * kThreads;
        for (uint32_t l = 0; l < nfull; ++l) dma16(src + (16u * kThreads) * l, dst + (16u * kThreads) * l);
        if (tid < ntail) dma16(src + (16u * kThreads) * nfull, dst + (16u * kThreads) * nfull);
    } else {
        ch_i4* lq = reinterpret_cast<ch_i4*>(lds);
        for (uint32_t i = tid; i < nq; i += kThreads) {
            const uint32_t v = base + 16u * i;
            lq[i] = ch_i4{(int)virt_dword(L, s, v), (int)virt_dword(L, s, v + 4u), (int)virt_dword(L, s, v + 8u), (int)virt_dword(L, s, v + 12u)};
        }
    }
    {
        typedef const FMD_CH_GLOBAL uint32_t* gw;
        uint32_t* const tw = reinterpret_cast<uint32_t*>(tab);
        for (uint32_t i = tid; i < kTableBytes / 4u; i += kThreads) tw[i] = ((gw)(uintptr_t)L.tab)[i];
    }
    // the stream's last tile also writes the next call's history (virtual bytes nbytes ... nbytes + HB)
    if (t == L.ntiles - 1u) {
        typedef FMD_CH_GLOBAL uint32_t* gwo;
        for (uint32_t i = tid; i < L.HB / 4u; i += kThreads)
            ((gwo)(uintptr_t)(L.hist_out + (uint64_t)s * L.HB))[i] = virt_dword(L, s, (uint32_t)L.nbytes + 4u * i);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0): the LDS-DMAs have landed
    __syncthreads();

    // ---- 2./3. contraction on the matrix cores, rotation, packing -----------------------------------------------------------
    {
        const uint8_t* lb = reinterpret_cast<const uint8_t*>(lds);
        const uint32_t j = lane & 15u, q = lane >> 4;
        const uint32_t pw = d0 + 2u * L.D * wave;           // window of the wave's first output o0 + wave
        const uint32_t aw = pw & ~15u, dl = (pw & 15u) >> 2;
        const uint32_t nout_w = no > wave ? (no - wave + 3u) >> 2 : 0u;
        const uint32_t groups = (nout_w + 15u) >> 4;        // wave-uniform, <= L.groups
        typedef const FMD_CH_GLOBAL ch_i4* gq;
        const gq amat = (gq)(uintptr_t)L.amat + (((uint64_t)s * 4u + dl) * L.nrt) * L.nkc * 64u + lane;
        const uint32_t col = aw + 8u * L.D * j + 16u * q;   // this lane's B bytes of group 0, chunk 0
        const uint32_t sh = 14u + L.shift;
        const uint32_t m_base = L.m0_lo + o0 + wave;        // global index (mod 2^32) of the wave's first output
        for (uint32_t rt = 0; rt < L.nrt; ++rt) {
            ch_i4 acc[kMaxGroups];
#pragma unroll
            for (uint32_t g = 0; g < kMaxGroups; ++g) acc[g] = ch_i4{0, 0, 0, 0};
            for (uint32_t kc = 0; kc < L.nkc; ++kc) {
                const ch_i4 A = amat[(rt * L.nkc + kc) * 64u];
#pragma unroll
                for (uint32_t g = 0; g < kMaxGroups; ++g) {
                    if (g < groups) {
                        ch_i4 B = *reinterpret_cast<const ch_i4*>(lb + col + 128u * L.D * g + 64u * kc);
                        B = B ^ (int)0x80808080;                                               // u8 -> s8
                        acc[g] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B, acc[g], 0, 0, 0);
                    }
                }
            }
            // lane (j, q) holds rows 4 q ... 4 q + 3 of column j: two digits -> (zr_lo, zr_hi, zi_lo, zi_hi) of station 4 rt + q;
            // one digit -> (zr, zi) of stations 8 rt + 2 q and 8 rt + 2 q + 1
            const uint32_t ka = L.digits == 2u ? 4u * rt + q : 8u * rt + 2u * q;
            const uint32_t skb = s * L.K + ka;
            const bool has0 = ka < L.K, has1 = L.digits == 1u && ka + 1u < L.K;
            const int c0r = has0 ? L.kconst[2u * skb] : 0, c0i = has0 ? L.kconst[2u * skb + 1u] : 0;
            const uint32_t i0 = has0 ? L.dinc[skb] : 0u;
            const int c1r = has1 ? L.kconst[2u * skb + 2u] : 0, c1i = has1 ? L.kconst[2u * skb + 3u] : 0;
            const uint32_t i1 = has1 ? L.dinc[skb + 1u] : 0u;
#pragma unroll
            for (uint32_t g = 0; g < kMaxGroups; ++g) {
                const uint32_t o = wave + 4u * (16u * g + j);  // output o0 + o of the call
                if (g < groups && o < no) {
                    const uint32_t m = m_base + 4u * (16u * g + j);
                    if (L.digits == 2u) {
                        if (has0) {
                            const int zr = (int)((uint32_t)acc[g].x + ((uint32_t)acc[g].y << 7)) + c0r;
                            const int zi = (int)((uint32_t)acc[g].z + ((uint32_t)acc[g].w << 7)) + c0i;
                            ypk[ka * L.tile + o] = ch_rotate(tab, zr, zi, m * i0, sh);
                        }
                    } else {
                        if (has0) ypk[ka * L.tile + o] = ch_rotate(tab, acc[g].x + c0r, acc[g].y + c0i, m * i0, sh);
                        if (has1) ypk[(ka + 1u) * L.tile + o] = ch_rotate(tab, acc[g].z + c1r, acc[g].w + c1i, m * i1, sh);
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- 4. the stations' rows, whole segments ------------------------------------------------------------------------------
    typedef FMD_CH_GLOBAL uint32_t* gwo;
    gwo const out = (gwo)(uintptr_t)(L.out + (uint64_t)s * L.K * L.out_stride + o0);
    if (L.vec4) {                                            // out_stride % 4 == 0, 16-byte aligned base, o0 % 4 == 0
        typedef FMD_CH_GLOBAL ch_i4* gqo;
        const uint32_t n4 = no >> 2, rem = no & 3u;
        for (uint32_t idx = tid; idx < L.K * n4; idx += kThreads) {
            const uint32_t k = idx / n4, i = idx - k * n4;
            ((gqo)(out + (uint64_t)k * L.out_stride))[i] = reinterpret_cast<const ch_i4*>(ypk + k * L.tile)[i];
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

#define CH_TRY(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            char m_[256];                                                                   \
            snprintf(m_, sizeof m_, "%s failed: %s", #expr, hipGetErrorString(e_));         \
            fmd_internal_set_err(m_);                                                       \
            return e_ == hipErrorOutOfMemory ? FMD_ERR_NOMEM : FMD_ERR_HIP;                 \
        }                                                                                   \
    } while (0)

#define CH_ON_DEVICE(dev)                                                                   \
    FmdDeviceGuard dev_guard_(dev);                                                         \
    if (dev_guard_.error() != hipSuccess) { fmd_internal_set_err("hipSetDevice failed"); return FMD_ERR_HIP; }

}  // namespace fmd_ch

struct fmd_channelizer {
    uint32_t T = 0, D = 0, K = 0, S = 0, shift = 0, HB = 0;
    uint32_t groups = 0, tile = 0, raw_bytes = 0;
    size_t lds = 0;
    int device = 0;
    uint64_t pos = 0;                                     // samples consumed per stream
    FmdStationsPlan plan;
    uint32_t* d_amat = nullptr;
    int32_t* d_kconst = nullptr;
    uint32_t* d_dinc = nullptr;
    uint32_t* d_tab = nullptr;
    uint8_t* d_hist[2] = {nullptr, nullptr};
    int cur = 0;
    FmdStreamOrder order;
    hipStream_t stream = nullptr;
    uint8_t* d_iq = nullptr; size_t d_iq_cap = 0;
    uint32_t* d_out = nullptr; size_t d_out_cap = 0;
};

namespace {

using fmd_ch::kTableBytes;

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
    const uint64_t m0 = ch_outputs(h, h->pos), m1 = ch_outputs(h, h->pos + ns);
    const uint64_t M = m1 - m0;
    if (M < 1) { fmd_internal_set_err("the call completes no filter output"); return FMD_ERR_TOO_SHORT; }
    if (M > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    const uint64_t ntiles = (M + h->tile - 1) / h->tile;
    if (ntiles > (1u << 30) || h->S > 65535u) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }
    fmd_ch::ChLaunch L{};
    L.iq = static_cast<const uint8_t*>(d_iq);
    L.nbytes = nbytes;
    L.hist_in = h->d_hist[h->cur]; L.hist_out = h->d_hist[h->cur ^ 1];
    L.HB = h->HB;
    L.vb_first = (uint32_t)(2ull * (h->D * m0 + h->HB / 2 - h->pos));   // >= 0: the window of output m0 starts at most n_taps - 1 samples back
    L.m0_lo = (uint32_t)m0;
    L.M = (uint32_t)M;
    L.D = h->D; L.T = h->T; L.K = h->K; L.S = h->S; L.shift = h->shift;
    L.nrt = h->plan.nrt; L.nkc = h->plan.nkc; L.digits = h->plan.digits;
    L.groups = h->groups; L.tile = h->tile; L.ntiles = (uint32_t)ntiles; L.raw_bytes = h->raw_bytes;
    L.vec4 = (((uintptr_t)d_out & 15u) == 0 && out_cap % 4 == 0) ? 1u : 0u;
    L.amat = h->d_amat; L.kconst = h->d_kconst; L.dinc = h->d_dinc; L.tab = h->d_tab;
    L.out = static_cast<uint32_t*>(d_out); L.out_stride = out_cap;
    CH_TRY(h->order.before(stream));
    hipLaunchKernelGGL(fmd_ch::fmd_channelizer_kernel, dim3(L.ntiles, h->S), dim3(fmd_ch::kThreads), h->lds, stream, L);
    CH_TRY(hipGetLastError());
    (void)h->order.after(stream);
    h->cur ^= 1;
    h->pos += ns;
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
    for (uint32_t G = fmd_ch::kMaxGroups; G >= 1; --G) {     // the largest tile within the budget (G = 1 always fits: <= 19 KB)
        uint32_t rb;
        const size_t l = ch_lds(decim, h->plan.nkc, n_taps, n_stations, G, &rb);
        if (l <= kLdsBudget || G == 1) { h->groups = G; h->tile = 64u * G; h->raw_bytes = rb; h->lds = l; break; }
    }
    h->HB = 2u * ((n_taps - 1u + 7u) & ~7u);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { delete h; fmd_internal_set_err("no HIP device (this library has no CPU path)"); return FMD_ERR_NO_DEVICE; }
    int device = dev->device_id;
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    hipDeviceProp_t prop;
    if (device >= ndev || hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        delete h; fmd_internal_set_err("device is not a gfx950"); return FMD_ERR_NO_DEVICE;
    }
    h->device = device;
    auto fail = [&](const char* what) { fmd_internal_set_err(what); fmd_channelizer_free(h); return FMD_ERR_HIP; };
    FmdDeviceGuard guard(device);
    if (guard.error() != hipSuccess) return fail("hipSetDevice");
    const FmdStationsPlan& P = h->plan;
    if (hipMalloc(&h->d_amat, P.amat.size() * 4) != hipSuccess || hipMemcpy(h->d_amat, P.amat.data(), P.amat.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMalloc(tap matrix)");
    if (hipMalloc(&h->d_kconst, P.kconst.size() * 4) != hipSuccess || hipMemcpy(h->d_kconst, P.kconst.data(), P.kconst.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMalloc(constants)");
    if (hipMalloc(&h->d_dinc, P.dinc.size() * 4) != hipSuccess || hipMemcpy(h->d_dinc, P.dinc.data(), P.dinc.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMalloc(phase steps)");
    int16_t tab[1024];
    fmd_st_nco_table(tab);
    if (hipMalloc(&h->d_tab, sizeof tab) != hipSuccess || hipMemcpy(h->d_tab, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMalloc(NCO table)");
    const size_t hb = (size_t)h->S * (h->HB ? h->HB : 16);
    for (int i = 0; i < 2; ++i)
        if (hipMalloc(&h->d_hist[i], hb) != hipSuccess || hipMemset(h->d_hist[i], 0, hb) != hipSuccess) return fail("hipMalloc(history)");
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate");
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    *out = h;
    return FMD_OK;
}

void fmd_channelizer_free(fmd_channelizer* h)
{
    if (!h) return;
    FmdDeviceGuard guard(h->device);
    (void)hipDeviceSynchronize();
    h->order.destroy();
    if (h->d_amat) (void)hipFree(h->d_amat);
    if (h->d_kconst) (void)hipFree(h->d_kconst);
    if (h->d_dinc) (void)hipFree(h->d_dinc);
    if (h->d_tab) (void)hipFree(h->d_tab);
    for (int i = 0; i < 2; ++i) if (h->d_hist[i]) (void)hipFree(h->d_hist[i]);
    if (h->d_iq) (void)hipFree(h->d_iq);
    if (h->d_out) (void)hipFree(h->d_out);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int fmd_channelizer_reset(fmd_channelizer* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    CH_ON_DEVICE(h->device);
    CH_TRY(hipDeviceSynchronize());
    const size_t hb = (size_t)h->S * (h->HB ? h->HB : 16);
    for (int i = 0; i < 2; ++i) CH_TRY(hipMemset(h->d_hist[i], 0, hb));
    CH_TRY(hipDeviceSynchronize());
    h->pos = 0; h->cur = 0;
    h->order.reset();
    return FMD_OK;
}

int fmd_channelizer_run_device(fmd_channelizer* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len,
                               void* stream)
{
    if (!h || !d_iq || !d_out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    CH_ON_DEVICE(h->device);
    return ch_enqueue(h, d_iq, nbytes, d_out, out_cap, out_len, static_cast<hipStream_t>(stream));
}

int fmd_channelizer_check(fmd_channelizer* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    CH_ON_DEVICE(h->device);
    if (h->order.have_last) CH_TRY(hipStreamSynchronize(h->order.last));
    CH_TRY(hipGetLastError());
    return FMD_OK;
}

int fmd_channelizer_run_batch(fmd_channelizer* h, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!h || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    CH_ON_DEVICE(h->device);
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    const size_t rows = (size_t)h->S * h->K;
    const size_t in_bytes = nbytes * (size_t)h->S, out_elems = out_cap * rows;   // out_elems: (yr, yi) pairs
    if (in_bytes > h->d_iq_cap) {
        if (h->d_iq) { CH_TRY(hipFree(h->d_iq)); h->d_iq = nullptr; h->d_iq_cap = 0; }
        CH_TRY(hipMalloc(&h->d_iq, in_bytes ? in_bytes : 1));
        h->d_iq_cap = in_bytes;
    }
    if (out_elems > h->d_out_cap) {
        if (h->d_out) { CH_TRY(hipFree(h->d_out)); h->d_out = nullptr; h->d_out_cap = 0; }
        CH_TRY(hipMalloc(&h->d_out, (out_elems ? out_elems : 1) * sizeof(uint32_t)));
        h->d_out_cap = out_elems;
    }
    CH_TRY(hipMemcpyAsync(h->d_iq, iq, in_bytes, hipMemcpyHostToDevice, h->stream));
    size_t n = 0;
    int rc = ch_enqueue(h, h->d_iq, nbytes, h->d_out, out_cap, &n, h->stream);
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    CH_TRY(hipMemcpyAsync(out, h->d_out, out_elems * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    CH_TRY(hipStreamSynchronize(h->stream));
    *out_len = n;
    return FMD_OK;
}

int fmd_channelizer_outputs(const fmd_channelizer* h, uint64_t* outputs)
{
    if (!h || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *outputs = ch_outputs(h, h->pos);
    return FMD_OK;
}

int fmd_channelizer_kernel_name(const fmd_channelizer* h, char* name, size_t cap)
{
    if (!h || !name || cap == 0) return FMD_ERR_INVALID_ARG;
    const int n = snprintf(name, cap, "fmd_ch::fmd_channelizer_kernel");
    return n < 0 || (size_t)n >= cap ? FMD_ERR_CAPACITY : FMD_OK;
}

}  // extern "C"
