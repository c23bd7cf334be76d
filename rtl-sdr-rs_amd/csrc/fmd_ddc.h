// fmd_ddc.h -- what the matrix-core handles share: the five down-converter banks (fmd_stations.hip, fmd_channelizer.hip,
// fmd_stereo.hip, fmd_narrow.hip, fmd_rds.hip) and the power-spectrum scanner (fmd_spectrum.hip).  The handle core also carries the
// row processors (fmd_resample.hip, fmd_agc.hip, fmd_tonesq.hip, fmd_afsk.hip), whose own host layer on top of it is fmd_rows.h, and the FIR and
// the fused FIR-demod handle (fmd_fir.hip, fmd_firdemod.hip: raw dwords in d_hist, their own kernels, call checks and batch copies).
// Only the demod handle (fmd_api.cpp), with its ring of three settle and replay slots, keeps a host side of its own.
//   plan (host):        the NCO table, the complex taps of every row, the matrix-core A fragments and their centring constants;
//   front end (device): the banks' digital down-converter -- staging of the filter windows and the NCO table in LDS, the
//                       history write, the contraction on the matrix cores, the rotation back to baseband;
//   handle core (host): device, stream, uploaded plan, double-buffered history, per-row ping-pong state, batch staging buffers;
//   bank (host):        what a down-converter's entry points do around its own kernels -- the constructor's front-end checks and
//                       device step, the tile sizing, the output counters, the call checks, the launch fields the front end
//                       reads, the batch path, check, reset and free.
// Definitions: include/fmd.h, "station bank", "channelizer", "power spectrum".
#pragma once

#include "../../include/fmd.h"

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fmd_host.h"

// ---- plan ---------------------------------------------------------------------------------------------------------------------

// TAB[i] = round(16384 cos(2 pi i / 1024)); no entry lies near a rounding tie, so any libm gives the same table.
inline void fmd_st_nco_table(int16_t* tab)
{
    const double two_pi = 6.28318530717958647692528676655900577;
    for (int i = 0; i < 1024; ++i) tab[i] = (int16_t)std::lround(16384.0 * std::cos(two_pi * i / 1024.0));
}
inline int fmd_st_cosq(const int16_t* tab, uint32_t phi) { return tab[phi >> 22]; }
inline int fmd_st_sinq(const int16_t* tab, uint32_t phi) { return tab[((phi >> 22) - 256u) & 1023u]; }

// W[t] = rnd(h[t] cosq(t inc)) + j rnd(-h[t] sinq(t inc)), rnd(v) = (v + 8192) >> 14 (arithmetic shift): |W| <= 2047.
inline void fmd_st_complex_taps(const int16_t* h, uint32_t n_taps, uint32_t inc, const int16_t* tab, int32_t* wr, int32_t* wi)
{
    for (uint32_t t = 0; t < n_taps; ++t) {
        const uint32_t phi = t * inc;                                    // mod 2^32
        wr[t] = (h[t] * fmd_st_cosq(tab, phi) + 8192) >> 14;
        wi[t] = (-h[t] * fmd_st_sinq(tab, phi) + 8192) >> 14;
    }
}

// The tap matrix on the matrix cores (v_mfma_i32_16x16x64_i8, A = 16 rows x 64 bytes per K chunk).  Rows:
//   two digits (any |W| <= 2047): row 4 i + (zr_lo, zr_hi, zi_lo, zi_hi) of tap row 4 rt + i, W = 128 hi + lo (|lo| <= 64, |hi| <= 16);
//   one digit (every |W| <= 127): row 2 i + (zr, zi) of tap row 8 rt + i.
// K index = byte offset from a 16-byte aligned address; the window of the column's output starts `delta` bytes further, byte 2 t
// is I and 2 t + 1 is Q of sample t.  With B = b - 128 (the bytes xor 0x80, as s8) the sample is c = (B_I + 1) + j (B_Q + 1), so
//   zr = sum Wr cI - Wi cQ  -> I weight Wr, Q weight -Wi, constant sum (Wr - Wi)
//   zi = sum Wi cI + Wr cQ  -> I weight Wi, Q weight  Wr, constant sum (Wr + Wi).
// A tap row is a (stream, station) of the bank and the channelizer, a DFT bin of the scanner.
struct FmdDdcPlan {
    uint32_t K = 0, T = 0, S = 0;     // tap rows per stream, taps, streams
    uint32_t digits = 2;              // i8 digits per tap
    uint32_t spt = 4;                 // tap rows per row tile (4: two digits, 8: one)
    uint32_t nrt = 0, nkc = 0;        // row tiles, 64-byte K chunks
    std::vector<uint32_t> amat;       // [S][deltas][nrt][nkc][64 lanes][4 dwords]
    std::vector<int32_t> kconst;      // [S][K][2]: the additive constants of zr, zi
    std::vector<uint32_t> dinc;       // [S][K]: decim * inc mod 2^32 (output rotation step; down-converters only)
    uint64_t max_gain = 0;            // max over tap rows of sum_t |Wr| + |Wi|
};

inline int fmd_st_a_entry(const int32_t* wr, const int32_t* wi, uint32_t T, uint32_t comp, uint32_t kb, uint32_t delta)
{
    if (kb < delta || kb - delta >= 2u * T) return 0;
    const uint32_t u = kb - delta, t = u >> 1, q = u & 1u;
    return comp == 0u ? (q ? -wi[t] : wr[t]) : (q ? wr[t] : wi[t]);
}

// The A fragments of the K tap rows of one stream, for the window offsets delta = 4 dl, dl < ndelta:
// ab = [ndelta][nrt][nkc][64 lanes][16 bytes] (lane l: row l & 15, K bytes 16 (l >> 4) ... + 15 of the chunk).
inline void fmd_ddc_pack_a(const int32_t* wr, const int32_t* wi, uint32_t T, uint32_t K, uint32_t nrt, uint32_t nkc,
                           uint32_t ndelta, bool small, uint8_t* ab)
{
    for (uint32_t dl = 0; dl < ndelta; ++dl)
        for (uint32_t rt = 0; rt < nrt; ++rt)
            for (uint32_t kc = 0; kc < nkc; ++kc)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint32_t row = lane & 15u, q = lane >> 4;
                    uint32_t k, comp, dsel;
                    if (small) { k = 8u * rt + (row >> 1); comp = row & 1u; dsel = 0u; }
                    else { k = 4u * rt + (row >> 2); comp = (row >> 1) & 1u; dsel = 1u + (row & 1u); }
                    if (k >= K) continue;
                    const size_t base = ((((size_t)dl * nrt + rt) * nkc + kc) * 64 + lane) * 16;
                    for (uint32_t b = 0; b < 16; ++b) {
                        const int v = fmd_st_a_entry(&wr[(size_t)k * T], &wi[(size_t)k * T], T, comp, 64u * kc + 16u * q + b, 4u * dl);
                        const int lo = ((v + 64) & 127) - 64, hi = (v - lo) / 128;
                        ab[base + b] = (uint8_t)(int8_t)(dsel == 0u ? v : (dsel == 1u ? lo : hi));
                    }
                }
}

// The plan of S streams x K tap rows, row sk mixed by inc[sk]: taps, constants, digits, and A fragments for `ndelta` offsets.
inline void fmd_ddc_build_plan(const int16_t* h, uint32_t T, const uint32_t* inc, uint32_t S, uint32_t K, uint32_t ndelta,
                               uint32_t nkc, FmdDdcPlan& P)
{
    int16_t tab[1024];
    fmd_st_nco_table(tab);
    P.K = K; P.T = T; P.S = S;
    std::vector<int32_t> wr((size_t)S * K * T), wi((size_t)S * K * T);
    bool small = true;
    P.max_gain = 0;
    P.kconst.assign((size_t)S * K * 2, 0);
    for (size_t sk = 0; sk < (size_t)S * K; ++sk) {
        int32_t* r = &wr[sk * T];
        int32_t* i = &wi[sk * T];
        fmd_st_complex_taps(h, T, inc[sk], tab, r, i);
        uint64_t g = 0;
        int64_t cre = 0, cim = 0;
        for (uint32_t t = 0; t < T; ++t) {
            g += (uint64_t)(r[t] < 0 ? -r[t] : r[t]) + (uint64_t)(i[t] < 0 ? -i[t] : i[t]);
            if (r[t] > 127 || r[t] < -127 || i[t] > 127 || i[t] < -127) small = false;
            cre += r[t] - i[t];
            cim += r[t] + i[t];
        }
        if (g > P.max_gain) P.max_gain = g;
        P.kconst[2 * sk] = (int32_t)cre;
        P.kconst[2 * sk + 1] = (int32_t)cim;
    }
    P.digits = small ? 1u : 2u;
    P.spt = small ? 8u : 4u;
    P.nrt = (K + P.spt - 1u) / P.spt;
    P.nkc = nkc;
    const size_t per_stream = (size_t)ndelta * P.nrt * P.nkc * 64 * 4;
    P.amat.assign(S * per_stream, 0u);
    for (uint32_t s = 0; s < S; ++s)
        fmd_ddc_pack_a(&wr[(size_t)s * K * T], &wi[(size_t)s * K * T], T, K, P.nrt, P.nkc, ndelta, small,
                       reinterpret_cast<uint8_t*>(P.amat.data() + s * per_stream));
}

// The down-converters' plan (bank, channelizer): a window starts 0, 4, 8 or 12 bytes past a 16-byte boundary.
inline void fmd_st_build_plan(const int16_t* h, uint32_t T, uint32_t decim, const uint32_t* inc, uint32_t S, uint32_t K,
                              FmdDdcPlan& P)
{
    fmd_ddc_build_plan(h, T, inc, S, K, 4u, (12u + 2u * T + 63u) / 64u, P);
    P.dinc.assign((size_t)S * K, 0u);
    for (size_t sk = 0; sk < (size_t)S * K; ++sk) P.dinc[sk] = decim * inc[sk];
}

// ---- device front end of the down-converters ----------------------------------------------------------------------------------
// One workgroup stages the raw bytes of a tile's filter windows of ONE stream and forms the tile's outputs for every station:
// wave w takes the outputs w + 4 i, whose windows sit 8 D i bytes apart -- 16-byte aligned for even D -- at a common offset delta
// from an aligned address; the host built the A fragments for each delta, and the wave loads the set that fits its offset.
// `Launch` is the kernel's launch struct; the fields read here have the same names in both.

#if defined(__HIP_DEVICE_COMPILE__)
#define FMD_DDC_GLOBAL __attribute__((address_space(1)))
#else
#define FMD_DDC_GLOBAL
#endif

namespace fmd_ddc {

constexpr int kThreads = 256;
constexpr uint32_t kGroups = 4;                           // 16-column MFMA groups per wave: at most 4 waves x 4 x 16 = 256 outputs per tile
constexpr uint32_t kTableBytes = 2048;                    // 1024 x i16
typedef int i4 __attribute__((ext_vector_type(4)));

template <class Launch>
__device__ __forceinline__ uint32_t virt_dword(const Launch& L, uint32_t s, uint32_t v)   // v: virtual byte, multiple of 4
{
    typedef const FMD_DDC_GLOBAL uint32_t* gw;
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
__device__ __forceinline__ uint32_t rotate(const int16_t* tab, int zr, int zi, uint32_t psi, uint32_t sh)
{
    const uint32_t ix = psi >> 22;
    const int64_t C = tab[ix], S = tab[(ix - 256u) & 1023u];
    const int yr = (int)(((int64_t)zr * C + (int64_t)zi * S) >> sh);
    const int yi = (int)(((int64_t)zi * C - (int64_t)zr * S) >> sh);
    return ((uint32_t)yr & 0xFFFFu) | ((uint32_t)yi << 16);
}

// The nq 16-byte chunks from virtual byte `base` (history ++ call) into LDS at 0 -- global_load_lds_dwordx4 when the range is
// whole, aligned and inside the call, through registers otherwise -- and the NCO table into `tab`.  The caller waits (vmcnt(0))
// and synchronises.
template <class Launch>
__device__ __forceinline__ void stage(const Launch& L, uint32_t s, uint32_t base, uint32_t nq, uint32_t* lds, int16_t* tab,
                                      uint32_t tid, uint32_t wave)
{
    const uint8_t* const row = L.iq + (uint64_t)s * L.nbytes;
    const bool whole = base >= L.HB && (uint64_t)(base - L.HB) + 16ull * nq <= L.nbytes && (((uintptr_t)row + (base - L.HB)) & 15u) == 0u;
    if (whole) {
        const unsigned char* src = row + (base - L.HB) + 16u * tid;
        unsigned char* dst = reinterpret_cast<unsigned char*>(lds) + 1024u * wave;
        const uint32_t nfull = nq / kThreads, ntail = nq - nfull * kThreads;
        for (uint32_t l = 0; l < nfull; ++l) dma16(src + (16u * kThreads) * l, dst + (16u * kThreads) * l);
        if (tid < ntail) dma16(src + (16u * kThreads) * nfull, dst + (16u * kThreads) * nfull);
    } else {
        i4* lq = reinterpret_cast<i4*>(lds);
        for (uint32_t i = tid; i < nq; i += kThreads) {
            const uint32_t v = base + 16u * i;
            lq[i] = i4{(int)virt_dword(L, s, v), (int)virt_dword(L, s, v + 4u), (int)virt_dword(L, s, v + 8u), (int)virt_dword(L, s, v + 12u)};
        }
    }
    typedef const FMD_DDC_GLOBAL uint32_t* gw;
    uint32_t* const tw = reinterpret_cast<uint32_t*>(tab);
    for (uint32_t i = tid; i < kTableBytes / 4u; i += kThreads) tw[i] = ((gw)(uintptr_t)L.tab)[i];
}

// the next call's history of stream s (virtual bytes nbytes ... nbytes + HB); one tile per stream writes it
template <class Launch>
__device__ __forceinline__ void write_history(const Launch& L, uint32_t s, uint32_t tid)
{
    typedef FMD_DDC_GLOBAL uint32_t* gwo;
    for (uint32_t i = tid; i < L.HB / 4u; i += kThreads)
        ((gwo)(uintptr_t)(L.hist_out + (uint64_t)s * L.HB))[i] = virt_dword(L, s, (uint32_t)L.nbytes + 4u * i);
}

// The contraction on the matrix cores (A = the stream's tap fragments, B = the staged window bytes xor 0x80 -> s8, one column per
// output), then per (station k, output o < no of the tile): the centring constants, the rotation by the NCO, the normalising
// shift, packed into ypk[k stride + col + o].  d0: offset of output 0's window from the staged base; m0: global index (mod 2^32)
// of output 0.
template <class Launch>
__device__ __forceinline__ void contract(const Launch& L, uint32_t s, uint32_t wave, uint32_t lane, uint32_t d0, uint32_t no,
                                         uint32_t m0, const uint32_t* lds, const int16_t* tab, uint32_t* ypk, uint32_t stride,
                                         uint32_t col)
{
    const uint8_t* lb = reinterpret_cast<const uint8_t*>(lds);
    const uint32_t j = lane & 15u, q = lane >> 4;
    const uint32_t pw = d0 + 2u * L.D * wave;               // window of the wave's first output
    const uint32_t aw = pw & ~15u, dl = (pw & 15u) >> 2;
    const uint32_t nout_w = no > wave ? (no - wave + 3u) >> 2 : 0u;
    const uint32_t groups = (nout_w + 15u) >> 4;            // wave-uniform, <= kGroups
    typedef const FMD_DDC_GLOBAL i4* gq;
    const gq amat = (gq)(uintptr_t)L.amat + (((uint64_t)s * 4u + dl) * L.nrt) * L.nkc * 64u + lane;
    const uint32_t bcol = aw + 8u * L.D * j + 16u * q;      // this lane's B bytes of group 0, chunk 0
    const uint32_t sh = 14u + L.shift;
    for (uint32_t rt = 0; rt < L.nrt; ++rt) {
        i4 acc[kGroups];
#pragma unroll
        for (uint32_t g = 0; g < kGroups; ++g) acc[g] = i4{0, 0, 0, 0};
        for (uint32_t kc = 0; kc < L.nkc; ++kc) {
            const i4 A = amat[(rt * L.nkc + kc) * 64u];
#pragma unroll
            for (uint32_t g = 0; g < kGroups; ++g) {
                if (g < groups) {
                    i4 B = *reinterpret_cast<const i4*>(lb + bcol + 128u * L.D * g + 64u * kc);
                    B = B ^ (int)0x80808080;                                                   // u8 -> s8
                    acc[g] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B, acc[g], 0, 0, 0);
                }
            }
        }
        // lane (j, q) holds rows 4 q ... 4 q + 3 of column j: two digits -> (zr_lo, zr_hi, zi_lo, zi_hi) of station 4 rt + q;
        // one digit -> (zr, zi) of stations 8 rt + 2 q and 8 rt + 2 q + 1
        const uint32_t ka = L.digits == 2u ? 4u * rt + q : 8u * rt + 2u * q;
        const uint32_t sk = s * L.K + ka;
        const bool has0 = ka < L.K, has1 = L.digits == 1u && ka + 1u < L.K;
        int c0r = 0, c0i = 0, c1r = 0, c1i = 0;               // centring constants and phase steps, once per row tile
        uint32_t i0 = 0u, i1 = 0u;
        if (has0) { c0r = L.kconst[2u * sk]; c0i = L.kconst[2u * sk + 1u]; i0 = L.dinc[sk]; }
        if (has1) { c1r = L.kconst[2u * sk + 2u]; c1i = L.kconst[2u * sk + 3u]; i1 = L.dinc[sk + 1u]; }
#pragma unroll
        for (uint32_t g = 0; g < kGroups; ++g) {
            const uint32_t o = wave + 4u * (16u * g + j);      // output o of the tile
            if (g < groups && o < no) {
                const uint32_t m = m0 + o;
                if (has0) {
                    if (L.digits == 2u) {
                        const int zr = (int)((uint32_t)acc[g].x + ((uint32_t)acc[g].y << 7)) + c0r;
                        const int zi = (int)((uint32_t)acc[g].z + ((uint32_t)acc[g].w << 7)) + c0i;
                        ypk[ka * stride + col + o] = rotate(tab, zr, zi, m * i0, sh);
                    } else {
                        ypk[ka * stride + col + o] = rotate(tab, acc[g].x + c0r, acc[g].y + c0i, m * i0, sh);
                    }
                }
                if (has1) ypk[(ka + 1u) * stride + col + o] = rotate(tab, acc[g].z + c1r, acc[g].w + c1i, m * i1, sh);
            }
        }
    }
}

}  // namespace fmd_ddc

// ---- handle core (host) -------------------------------------------------------------------------------------------------------

// A failed HIP call: the message, FMD_ERR_NOMEM / FMD_ERR_HIP.
#define FMD_DDC_TRY(expr)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            char m_[256];                                                                   \
            snprintf(m_, sizeof m_, "%s failed: %s", #expr, hipGetErrorString(e_));         \
            fmd_internal_set_err(m_);                                                       \
            return e_ == hipErrorOutOfMemory ? FMD_ERR_NOMEM : FMD_ERR_HIP;                 \
        }                                                                                   \
    } while (0)

#define FMD_DDC_ON_DEVICE(dev)                                                              \
    FmdDeviceGuard dev_guard_(dev);                                                         \
    if (dev_guard_.error() != hipSuccess) { fmd_internal_set_err("hipSetDevice failed"); return FMD_ERR_HIP; }

// Per-row state that one call reads and the next call's copy is written to: read [core.cur], written [core.cur ^ 1].
struct FmdDdcPair {
    void* p[2] = {nullptr, nullptr};
    size_t bytes = 0;
    template <class T> T* in(int cur) const { return static_cast<T*>(p[cur]); }
    template <class T> T* out(int cur) const { return static_cast<T*>(p[cur ^ 1]); }
};

// A further device buffer of the handle: a constant uploaded by the constructor (src != nullptr), a buffer the kernels update in
// place, which the constructor allocates and zeroes and reset leaves alone (src == nullptr, bytes != 0), or call-sized scratch that
// fmd_ddc_grow allocates in the calls (src == nullptr, bytes == 0).
struct FmdDdcOwned {
    void** slot = nullptr;
    const void* src = nullptr;
    size_t bytes = 0;
};

// What every handle holds on the device.
struct FmdDdcCore {
    int device = 0;
    hipStream_t stream = nullptr;                         // the host entry points' own stream
    FmdStreamOrder order;
    uint32_t* d_amat = nullptr;
    int32_t* d_kconst = nullptr;
    uint32_t* d_dinc = nullptr;                           // down-converters only: phase steps and the NCO table
    uint32_t* d_tab = nullptr;
    uint8_t* d_hist[2] = {nullptr, nullptr};              // down-converters only: raw-byte history, read [cur], written [cur ^ 1]
    size_t hist_bytes = 0;
    int cur = 0;
    uint64_t pos = 0;                                     // samples consumed per stream
    void* d_iq = nullptr; size_t d_iq_cap = 0;            // batch staging (bytes)
    void* d_out = nullptr; size_t d_out_cap = 0;
    // what the handle registered (members of the handle itself): the constructor's device step allocates them, reset zeroes the
    // pairs, release frees all of them
    FmdDdcPair* pairs[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t n_pairs = 0;
    FmdDdcOwned owned[4];
    uint32_t n_owned = 0;
};

inline void fmd_ddc_add_pair(FmdDdcCore& c, FmdDdcPair& pr, size_t bytes)
{
    assert(c.n_pairs < 4u);
    pr.bytes = bytes;
    c.pairs[c.n_pairs++] = &pr;
}
// `src` must stay valid until the constructor's device step
inline void fmd_ddc_add_owned(FmdDdcCore& c, void*& slot, const void* src = nullptr, size_t bytes = 0)
{
    assert(c.n_owned < 4u);
    c.owned[c.n_owned++] = FmdDdcOwned{&slot, src, bytes};
}

// The device of `dev` (device_id < 0: the current one) if it is a gfx950; FMD_ERR_NO_DEVICE otherwise.  Touches no allocation.
inline int fmd_ddc_open(FmdDdcCore& c, const fmd_device_config* dev)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { fmd_internal_set_err("no HIP device (this library has no CPU path)"); return FMD_ERR_NO_DEVICE; }
    int device = dev->device_id;
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    hipDeviceProp_t prop;
    if (device >= ndev || hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fmd_internal_set_err("device is not a gfx950"); return FMD_ERR_NO_DEVICE;
    }
    c.device = device;
    return FMD_OK;
}

// On c.device: the plan's buffers that are not empty (the NCO table with the phase steps; a handle whose front end is another
// handle's leaves its plan empty), a zeroed history of `hist_bytes` twice when non-zero, the stream, the registered pairs zeroed,
// the registered constants and the registered in-place buffers zeroed.  nullptr, or what failed.
inline const char* fmd_ddc_upload(FmdDdcCore& c, const FmdDdcPlan& P, size_t hist_bytes)
{
    if (!P.amat.empty() && (hipMalloc(&c.d_amat, P.amat.size() * 4) != hipSuccess || hipMemcpy(c.d_amat, P.amat.data(), P.amat.size() * 4, hipMemcpyHostToDevice) != hipSuccess))
        return "hipMalloc(tap matrix)";
    if (!P.kconst.empty() && (hipMalloc(&c.d_kconst, P.kconst.size() * 4) != hipSuccess || hipMemcpy(c.d_kconst, P.kconst.data(), P.kconst.size() * 4, hipMemcpyHostToDevice) != hipSuccess))
        return "hipMalloc(constants)";
    if (!P.dinc.empty()) {
        if (hipMalloc(&c.d_dinc, P.dinc.size() * 4) != hipSuccess || hipMemcpy(c.d_dinc, P.dinc.data(), P.dinc.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return "hipMalloc(phase steps)";
        int16_t tab[1024];
        fmd_st_nco_table(tab);
        if (hipMalloc(&c.d_tab, sizeof tab) != hipSuccess || hipMemcpy(c.d_tab, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess)
            return "hipMalloc(NCO table)";
    }
    c.hist_bytes = hist_bytes;
    for (int i = 0; i < 2 && hist_bytes; ++i)
        if (hipMalloc(&c.d_hist[i], hist_bytes) != hipSuccess || hipMemset(c.d_hist[i], 0, hist_bytes) != hipSuccess) return "hipMalloc(history)";
    if (hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess) return "hipStreamCreate";
    for (uint32_t k = 0; k < c.n_pairs; ++k)
        for (int i = 0; i < 2; ++i) {
            FmdDdcPair& pr = *c.pairs[k];
            if (hipMalloc(&pr.p[i], pr.bytes) != hipSuccess || hipMemset(pr.p[i], 0, pr.bytes) != hipSuccess) return "hipMalloc(per-row state)";
        }
    for (uint32_t k = 0; k < c.n_owned; ++k) {
        FmdDdcOwned& o = c.owned[k];
        if (o.src && (hipMalloc(o.slot, o.bytes) != hipSuccess || hipMemcpy(*o.slot, o.src, o.bytes, hipMemcpyHostToDevice) != hipSuccess))
            return "hipMalloc(handle constants)";
        if (!o.src && o.bytes && (hipMalloc(o.slot, o.bytes) != hipSuccess || hipMemset(*o.slot, 0, o.bytes) != hipSuccess))
            return "hipMalloc(handle buffers)";
        o.src = nullptr;
    }
    return nullptr;
}

// A constructor's device step: the device, the plan, the history, the stream, and what the handle registered on the core.
// FMD_OK; the device's refusal with *what == nullptr (nothing was allocated: the caller deletes the handle); or FMD_ERR_HIP and
// what failed (the caller sets the error text and calls its *_free).
inline int fmd_ddc_core_device(FmdDdcCore& c, const FmdDdcPlan& P, size_t hist_bytes, const fmd_device_config* dev, const char** what)
{
    *what = nullptr;
    if (const int rc = fmd_ddc_open(c, dev)) return rc;
    FmdDeviceGuard guard(c.device);
    if (guard.error() != hipSuccess) *what = "hipSetDevice";
    if (!*what) *what = fmd_ddc_upload(c, P, hist_bytes);
    if (!*what && hipDeviceSynchronize() != hipSuccess) *what = "hipDeviceSynchronize";
    return *what ? FMD_ERR_HIP : FMD_OK;
}

// Back to position 0 with an all-zero history and all-zero pairs (the caller has synchronised the device).  The position, the
// buffer index and the stream order change only once the device has finished the memsets, so a failure leaves them as they were.
inline hipError_t fmd_ddc_zero_history(FmdDdcCore& c)
{
    for (uint32_t k = 0; k < c.n_pairs; ++k)
        for (int i = 0; i < 2; ++i) {
            const hipError_t e = hipMemset(c.pairs[k]->p[i], 0, c.pairs[k]->bytes);
            if (e != hipSuccess) return e;
        }
    for (int i = 0; i < 2; ++i) {
        const hipError_t e = hipMemset(c.d_hist[i], 0, c.hist_bytes);
        if (e != hipSuccess) return e;
    }
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    c.pos = 0; c.cur = 0;
    c.order.reset();
    return hipSuccess;
}

// Everything the core holds and the handle registered (on c.device: the caller holds the device guard).
inline void fmd_ddc_release(FmdDdcCore& c)
{
    (void)hipDeviceSynchronize();
    c.order.destroy();
    for (uint32_t k = 0; k < c.n_pairs; ++k)
        for (void* p : c.pairs[k]->p) if (p) (void)hipFree(p);
    for (uint32_t k = 0; k < c.n_owned; ++k)
        if (*c.owned[k].slot) (void)hipFree(*c.owned[k].slot);
    for (void* p : {(void*)c.d_amat, (void*)c.d_kconst, (void*)c.d_dinc, (void*)c.d_tab, (void*)c.d_hist[0], (void*)c.d_hist[1], c.d_iq, c.d_out})
        if (p) (void)hipFree(p);
    if (c.stream) (void)hipStreamDestroy(c.stream);
}

// A batch staging or scratch buffer of at least `bytes` (at least 1) bytes, reallocated only when it grows.
inline hipError_t fmd_ddc_grow(void*& p, size_t& cap, size_t bytes)
{
    if (bytes <= cap) return hipSuccess;
    if (p) {
        const hipError_t e = hipFree(p);
        p = nullptr; cap = 0;
        if (e != hipSuccess) return e;
    }
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e == hipSuccess) cap = bytes;
    return e;
}

// snprintf's result in a `_kernel_name` entry point -> FMD_OK / FMD_ERR_CAPACITY
inline int fmd_ddc_name_rc(int n, size_t cap) { return n < 0 || (size_t)n >= cap ? FMD_ERR_CAPACITY : FMD_OK; }

// The handle's most recent launch has completed without an error.
inline int fmd_ddc_check(FmdDdcCore& c)
{
    FMD_DDC_ON_DEVICE(c.device);
    FMD_DDC_TRY(c.order.wait_last());
    FMD_DDC_TRY(hipGetLastError());
    return FMD_OK;
}

// ---- bank (host): a down-converter handle around its own kernels ------------------------------------------------------------------

// The front end's parameters, its plan and the core.  Every down-converter handle embeds one.
struct FmdDdcBank {
    uint32_t T = 0, D = 0, K = 0, S = 0, shift = 0;       // taps, decimation, stations per stream, streams, normalising shift
    uint32_t HB = 0;                                      // history bytes per stream (multiple of 16)
    FmdDdcPlan plan;
    FmdDdcCore core;
};

// The front end's argument checks, in a *_new: the ranges, then |tap| <= 2047.
inline int fmd_ddc_front_args(const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, uint32_t n_stations,
                              const fmd_device_config* dev)
{
    if (n_taps == 0 || n_taps > 256 || decim < 2 || decim % 2 != 0 || decim > 64 || shift > 24 || n_stations == 0 || n_stations > 32 ||
        dev->n_channels > 65535u) {
        fmd_internal_set_err("need 1 <= n_taps <= 256, an even 2 <= decim <= 64, shift <= 24, 1 <= n_stations <= 32, n_streams <= 65535");
        return FMD_ERR_UNSUPPORTED;
    }
    for (uint32_t t = 0; t < n_taps; ++t)
        if (taps[t] > 2047 || taps[t] < -2047) { fmd_internal_set_err("|tap| > 2047"); return FMD_ERR_UNSUPPORTED; }
    return FMD_OK;
}

// The front end's constructor step: the argument checks (again, for a caller whose own checks came after them), the bank's
// fields, the plan and the gain bound.  *bound = B_y = ceil(256 max_gain / 2^shift), the largest |y| component: |z| <= 128 G per
// component and the rotation adds two of them; the int16 outputs and the discriminator are exact while B_y <= 16384.
inline int fmd_ddc_bank_front(FmdDdcBank& b, const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift,
                              const uint32_t* phase_inc, uint32_t n_stations, const fmd_device_config* dev, uint64_t* bound)
{
    if (const int rc = fmd_ddc_front_args(taps, n_taps, decim, shift, n_stations, dev)) return rc;
    b.T = n_taps; b.D = decim; b.K = n_stations; b.S = dev->n_channels; b.shift = shift;
    b.HB = 2u * ((n_taps - 1u + 7u) & ~7u);
    fmd_st_build_plan(taps, n_taps, decim, phase_inc, b.S, b.K, b.plan);
    *bound = (256ull * b.plan.max_gain + ((1ull << shift) - 1ull)) >> shift;
    if (*bound > 16384ull) {
        fmd_internal_set_err("filter gain too large: need ceil(256 * max sum(|Wr| + |Wi|) / 2^shift) <= 16384");
        return FMD_ERR_UNSUPPORTED;
    }
    return FMD_OK;
}

// The constructor's device step of a down-converter: fmd_ddc_core_device with the bank's plan and history.
inline int fmd_ddc_bank_device(FmdDdcBank& b, const fmd_device_config* dev, const char** what)
{
    return fmd_ddc_core_device(b.core, b.plan, (size_t)b.S * (b.HB ? b.HB : 16), dev, what);
}

namespace fmd_ddc {
constexpr size_t kLdsBudget = 40960;                      // 4 tiles per CU
}

// Raw bytes of a tile of `cap` outputs, G 16-column groups per wave: what the matrix phase may read or the staging writes.
inline uint32_t fmd_ddc_raw_bytes(uint32_t D, uint32_t nkc, uint32_t T, uint32_t G, uint32_t cap)
{
    const uint64_t reads = 12 + 6ull * D + 8ull * D * (16 * G - 1) + 64ull * nkc;
    const uint64_t staged = 12 + 2ull * D * (cap - 1) + 2ull * T + 15;
    return (uint32_t)(((reads > staged ? reads : staged) + 15) & ~15ull);
}

// LDS of a tile of G groups per wave (64 G outputs): the raw bytes + the NCO table + one row of packed outputs per station
inline size_t fmd_ddc_tile_lds(uint32_t D, uint32_t nkc, uint32_t T, uint32_t K, uint32_t G, uint32_t* raw_bytes)
{
    *raw_bytes = fmd_ddc_raw_bytes(D, nkc, T, G, 64u * G);
    return (size_t)*raw_bytes + fmd_ddc::kTableBytes + 4ull * K * 64u * G;
}

// the largest tile (tile = 64 groups outputs) within the budget; G = 1 always fits (<= 19 KB)
struct FmdDdcTiling { uint32_t groups = 0, tile = 0, raw_bytes = 0; size_t lds = 0; };
inline FmdDdcTiling fmd_ddc_tiling(uint32_t D, uint32_t nkc, uint32_t T, uint32_t K)
{
    FmdDdcTiling t;
    for (t.groups = fmd_ddc::kGroups; t.groups >= 1; --t.groups) {
        t.lds = fmd_ddc_tile_lds(D, nkc, T, K, t.groups, &t.raw_bytes);
        if (t.lds <= fmd_ddc::kLdsBudget || t.groups == 1) break;
    }
    t.tile = 64u * t.groups;
    return t;
}

// front-end outputs completed once `samples` samples per stream have arrived
inline uint64_t fmd_ddc_outputs(uint32_t T, uint32_t D, uint64_t samples) { return samples >= T ? (samples - T) / D + 1 : 0; }
// outputs of a second filter of Ta taps at stride R over m inputs
inline uint64_t fmd_ddc_fir_outputs(uint32_t Ta, uint32_t R, uint64_t m) { return fmd_ddc_outputs(Ta, R, m); }
// a second stage's `_out_cap` entry point: its outputs per row that a call of nbytes can complete at most, at D samples per
// front-end output and R of those per output of the second filter
inline size_t fmd_ddc_fir_out_cap(uint32_t D, uint32_t R, size_t nbytes)
{
    if (!D || !R) return 0;
    const uint64_t d = 2ull * D * R;
    return (size_t)((nbytes + d - 1) / d);
}

// The checks every enqueue starts with; d_out must be aligned to `out_align` (a power of two) bytes.
inline int fmd_ddc_check_call(size_t nbytes, const void* d_iq, const void* d_out, uint32_t out_align)
{
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    if (nbytes > (1ull << 31) - (1ull << 20)) { fmd_internal_set_err("nbytes out of range"); return FMD_ERR_UNSUPPORTED; }
    if (((uintptr_t)d_iq & 3u) != 0 || ((uintptr_t)d_out & (out_align - 1u)) != 0) { fmd_internal_set_err("misaligned device buffer"); return FMD_ERR_INVALID_ARG; }
    return FMD_OK;
}

// The launch fields the device front end reads (same names in every launch struct), for a call whose first output has the global
// index m0.  The index itself (m0 / m0_lo) and the call's output count differ in name and width: the caller sets them.
template <class Launch>
inline void fmd_ddc_fill_front(Launch& L, const FmdDdcBank& b, const void* d_iq, size_t nbytes, uint64_t m0)
{
    const FmdDdcCore& c = b.core;
    L.iq = static_cast<const uint8_t*>(d_iq);
    L.nbytes = nbytes;
    L.hist_in = c.d_hist[c.cur]; L.hist_out = c.d_hist[c.cur ^ 1];
    L.HB = b.HB;
    L.vb_first = (uint32_t)(2ull * (b.D * m0 + b.HB / 2 - c.pos));   // >= 0: the window of output m0 starts at most n_taps - 1 samples back
    L.D = b.D; L.T = b.T; L.K = b.K; L.S = b.S; L.shift = b.shift;
    L.nrt = b.plan.nrt; L.nkc = b.plan.nkc; L.digits = b.plan.digits;
    L.amat = c.d_amat; L.kconst = c.d_kconst; L.dinc = c.d_dinc; L.tab = c.d_tab;
}

// The end of an enqueue whose launches were accepted: the stream order, the buffer index, the position.
inline void fmd_ddc_commit(FmdDdcCore& c, hipStream_t stream, uint64_t ns)
{
    (void)c.order.after(stream);
    c.cur ^= 1;
    c.pos += ns;
}

// A `_device` entry point: `enqueue()` on the handle's device.
template <class Enqueue>
inline int fmd_ddc_run_device(const FmdDdcCore* c, const void* d_iq, const void* d_out, Enqueue enqueue)
{
    if (!c || !d_iq || !d_out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(c->device);
    return enqueue();
}

// The first half of a `_batch` entry point (on the handle's device): the input of every stream into the staging buffer and
// enqueue(d_iq, nbytes, d_out, out_cap, &n, stream) on the handle's own stream, into a staging buffer of `out_bytes`.
template <class Enqueue>
inline int fmd_ddc_batch_enqueue(FmdDdcBank& b, const uint8_t* iq, size_t nbytes, size_t out_bytes, size_t out_cap, size_t* n,
                                 Enqueue enqueue)
{
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    FmdDdcCore& c = b.core;
    const size_t in_bytes = nbytes * (size_t)b.S;
    FMD_DDC_TRY(fmd_ddc_grow(c.d_iq, c.d_iq_cap, in_bytes));
    FMD_DDC_TRY(fmd_ddc_grow(c.d_out, c.d_out_cap, out_bytes));
    FMD_DDC_TRY(hipMemcpyAsync(c.d_iq, iq, in_bytes, hipMemcpyHostToDevice, c.stream));
    return enqueue(c.d_iq, nbytes, c.d_out, out_cap, n, c.stream);
}

// A `_batch` entry point: host in, host out (`out_bytes` for all rows), the call's outputs per row in *out_len.
template <class Enqueue>
inline int fmd_ddc_run_batch(FmdDdcBank& b, const uint8_t* iq, size_t nbytes, void* out, size_t out_bytes, size_t out_cap,
                             size_t* out_len, Enqueue enqueue)
{
    FmdDdcCore& c = b.core;
    FMD_DDC_ON_DEVICE(c.device);
    size_t n = 0;
    if (const int rc = fmd_ddc_batch_enqueue(b, iq, nbytes, out_bytes, out_cap, &n, enqueue)) {
        (void)hipStreamSynchronize(c.stream);
        return rc;
    }
    FMD_DDC_TRY(hipMemcpyAsync(out, c.d_out, out_bytes, hipMemcpyDeviceToHost, c.stream));
    FMD_DDC_TRY(hipStreamSynchronize(c.stream));
    *out_len = n;
    return FMD_OK;
}

// A `_reset` entry point: position 0, an all-zero history, all-zero pairs.
inline int fmd_ddc_reset(FmdDdcCore& c)
{
    FMD_DDC_ON_DEVICE(c.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    FMD_DDC_TRY(fmd_ddc_zero_history(c));                 // (ends with the device synchronised)
    return FMD_OK;
}

// A `_free` entry point's device side: everything but the handle itself.
inline void fmd_ddc_free(FmdDdcCore& c)
{
    FmdDeviceGuard guard(c.device);
    fmd_ddc_release(c);
}

// fmd_uniform_new in steps (fmd_uniform.hip), for the band-plan bank, which decides its own second stage between them: the domain
// of the arguments (pointers non-null, `channels` aside); that check again, the handle, its plan and *bound = B_y <= 16384; the
// device step, whose failure frees the handle.  Only the device step queries a device; discard drops a handle that has not run it.
int fmd_uniform_args(const int16_t* taps, uint32_t n_taps, uint32_t n_channels, uint32_t hop, uint32_t shift, const uint32_t* channels,
                     uint32_t n_selected, const fmd_device_config* dev);
int fmd_uniform_host(const int16_t* taps, uint32_t n_taps, uint32_t n_channels, uint32_t hop, uint32_t shift, const uint32_t* channels,
                     uint32_t n_selected, const fmd_device_config* dev, fmd_uniform** out, uint64_t* bound);
void fmd_uniform_discard(fmd_uniform* h);
int fmd_uniform_device(fmd_uniform* h, const fmd_device_config* dev);
