// fmd_stations.hip -- station bank: K FM stations demodulated out of one wideband IQ stream, in ONE gfx950 kernel.
//
// Definition (include/fmd.h, "station bank"; tests/stations_ref.py): per (stream, station k) the complex tapped FIR
//     z[k][m] = sum_t W[k][t] c[D m + t]      (W = the real prototype h mixed to the station's offset, c = raw bytes - 127)
// rotated back to baseband by the NCO, normalised by >> (14 + shift), then the reference's own fm_demod (:355-367, the f64 sample
// at the first output of every call) and low_pass_real (:408-426).  With inc = 0 it is fmd_firdemod on unrotated samples.
//
// One workgroup = one tile of `kt` audio samples of ONE stream, for all K stations of it (the tile geometry is fmd_firdemod's,
// fmd_index.h: every station of a stream has the same output and audio timing):
//   1. stage the raw bytes of the tile's filter windows in LDS (global_load_lds_dwordx4; through registers where the range touches
//      the stream's history or is not 16-byte aligned), and the NCO table;
//   2. the contraction on the matrix cores, v_mfma_i32_16x16x64_i8: A = the stream's station tap matrix (rows: station x
//      {zr, zi} x i8 digit, fmd_stations_common.h), B = window bytes (xor 0x80 -> s8), one column per filter output.  A window
//      starts at 2 D m bytes, only 4-byte aligned: wave w takes the outputs o = w + 4 i of the tile, whose windows sit 8 D i
//      bytes apart -- 16-byte aligned for even D -- at a common offset delta in {0, 4, 8, 12} from an aligned address; the host
//      built the A fragments for each delta, and the wave loads the set that fits its offset;
//   3. per (station, output): the additive centring constant, the rotation by the NCO (table in LDS, i64 products), the
//      normalising shift; packed re | im << 16 into LDS, one row per station;
//   4. per (station, audio group), one lane each: the discriminator over the group's outputs (fmd_device.h: f32 form when
//      |y| <= 2048, integer form otherwise, polar_f64 with its guard for the first output of the call), the group sum, one
//      exact small divide, the s16 store; the lane of a stream's trailing partial group writes the station's state.
// HBM traffic: the u8 input once, the (L2-resident) tap fragments once per block, 2 bytes per audio sample.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "fmd_device.h"
#include "fmd_host.h"
#include "fmd_internal.h"
#include "fmd_kernels.h"
#include "fmd_stations_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define FMD_ST_GLOBAL __attribute__((address_space(1)))
#else
#define FMD_ST_GLOBAL
#endif

namespace fmd_st {

using namespace fmd_dev;

constexpr int kThreads = 256;
constexpr uint32_t kGroupsPerWave = 4;                    // 16-column MFMA groups per wave: 4 waves x 4 x 16 = 256 outputs per tile
constexpr uint32_t kMaxOutputs = 4u * 16u * kGroupsPerWave;
constexpr uint32_t kTableBytes = 2048;                    // 1024 x i16
typedef int st_i4 __attribute__((ext_vector_type(4)));

struct StLaunch {
    const uint8_t* iq;         // [S][nbytes]
    uint64_t nbytes;
    const uint8_t* hist_in;    // [S][HB]: the last HB / 2 samples before the call
    uint8_t* hist_out;
    uint32_t HB;               // history bytes per stream (multiple of 16)
    uint32_t vb_first;         // virtual byte (history ++ call) of the window of the call's first output
    uint32_t m0_lo;            // global index of the call's first output, mod 2^32
    uint32_t D, T, K, S, shift;
    uint32_t nrt, nkc, digits;
    const uint32_t* amat;      // [S][4][nrt][nkc][64][4]
    const int32_t* kconst;     // [S][K][2]
    const uint32_t* dinc;      // [S][K]
    const uint32_t* tab;       // NCO table, 512 dwords
    FmdRates r;
    FmdClassPlan P;            // M = filter outputs of this call, K = audio samples, nt
    FmdTiling tl;
    uint32_t fa, fb, sr_shift;
    float inv_sr, inv_R;
    uint32_t lp_cap, raw_bytes;
    uint32_t f32_disc;
    const FmdChanState* st_in; // [S * K]
    FmdChanState* st_out;
    int16_t* out;              // [S][K][out_stride]
    uint64_t out_stride;
    FmdExcBuf* exc;
    double f64_guard;
    uint32_t seq;
    int32_t f64_skew;          // -DFMD_EXPERIMENT builds only
};

__device__ __forceinline__ uint32_t virt_dword(const StLaunch& L, uint32_t s, uint32_t v)   // v: virtual byte, multiple of 4
{
    typedef const FMD_ST_GLOBAL uint32_t* gw;
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

static __device__ __noinline__ void exc_emit_st(FmdExcBuf* exc, uint32_t c, uint32_t seq, int k, int sum, int d_gpu, int cr, int ci,
                                                int16_t* out_elem)
{
    FmdF64Exc e{};
    e.channel = c; e.cr = cr; e.ci = ci; e.d_gpu = d_gpu; e.seq = seq; e.k = k; e.sum = sum;
    e.out_elem = (uint64_t)(uintptr_t)out_elem;
    atomicAdd(&exc->guarded_total, 1u);
    const uint32_t slot = atomicAdd(&exc->count, 1u);
    if (slot < FMD_EXC_CAP) exc->rec[slot] = e; else atomicOr(&exc->err, FMD_DEVERR_EXC_CAP);
}

// rotation back to baseband and the normalising shift (include/fmd.h step 5), packed re | im << 16
__device__ __forceinline__ uint32_t st_rotate(const int16_t* tab, int zr, int zi, uint32_t psi, uint32_t sh)
{
    const uint32_t ix = psi >> 22;
    const int64_t C = tab[ix], S = tab[(ix - 256u) & 1023u];
    const int yr = (int)(((int64_t)zr * C + (int64_t)zi * S) >> sh);
    const int yi = (int)(((int64_t)zi * C - (int64_t)zr * S) >> sh);
    return pack_lp(yr, yi);
}

__global__ void __launch_bounds__(kThreads) fmd_stations_kernel(const StLaunch L)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t s = blockIdx.y, t = blockIdx.x;
    if (s >= L.S || t >= L.P.nt) return;

    const FmdRates& r = L.r;
    const FmdTile T = fmd_tile_fast(r, L.P, L.tl, 0u, t);
    const int jfirst = T.jA - 1, cnt = T.jB - jfirst + 1;    // y[jfirst .. jB] of every station; y[-1] is demod_pre
    const uint32_t o0 = jfirst > 0 ? (uint32_t)jfirst : 0u;  // first filter output (of this call) the tile forms
    const uint32_t no = (uint32_t)T.jB - o0 + 1u;
    const uint32_t vb = L.vb_first + 2u * L.D * o0;          // virtual byte of output o0's window
    const uint32_t base = vb & ~15u, d0 = vb - base;
    const uint32_t nq = (d0 + 2u * L.D * (no - 1u) + 2u * L.T + 15u) >> 4;   // 16-byte chunks staged
    if ((uint32_t)cnt > L.lp_cap || no > kMaxOutputs || nq * 16u > L.raw_bytes) {
        if (tid == 0) atomicOr(&L.exc->err, (uint32_t)cnt > L.lp_cap ? FMD_DEVERR_LP_CAP : FMD_DEVERR_RAW_CAP);
        return;
    }
    int16_t* const tab = reinterpret_cast<int16_t*>(lds + (L.raw_bytes >> 2));
    uint32_t* const ypk = lds + ((L.raw_bytes + kTableBytes) >> 2);          // [K][lp_cap]: y[jfirst + i] at i
    int* const gse = reinterpret_cast<int*>(ypk + L.K * L.lp_cap);           // (first, last) discriminator sample of each group

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
        st_i4* lq = reinterpret_cast<st_i4*>(lds);
        for (uint32_t i = tid; i < nq; i += kThreads) {
            const uint32_t v = base + 16u * i;
            lq[i] = st_i4{(int)virt_dword(L, s, v), (int)virt_dword(L, s, v + 4u), (int)virt_dword(L, s, v + 8u), (int)virt_dword(L, s, v + 12u)};
        }
    }
    {
        typedef const FMD_ST_GLOBAL uint32_t* gw;
        uint32_t* const tw = reinterpret_cast<uint32_t*>(tab);
        for (uint32_t i = tid; i < kTableBytes / 4u; i += kThreads) tw[i] = ((gw)(uintptr_t)L.tab)[i];
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
        const uint32_t groups = (nout_w + 15u) >> 4;        // wave-uniform, <= kGroupsPerWave
        typedef const FMD_ST_GLOBAL st_i4* gq;
        const gq amat = (gq)(uintptr_t)L.amat + (((uint64_t)s * 4u + dl) * L.nrt) * L.nkc * 64u + lane;
        const uint32_t col = aw + 8u * L.D * j + 16u * q;   // this lane's B bytes of group 0, chunk 0
        const uint32_t sh = 14u + L.shift;
        for (uint32_t rt = 0; rt < L.nrt; ++rt) {
            st_i4 acc[kGroupsPerWave];
#pragma unroll
            for (uint32_t g = 0; g < kGroupsPerWave; ++g) acc[g] = st_i4{0, 0, 0, 0};
            for (uint32_t kc = 0; kc < L.nkc; ++kc) {
                const st_i4 A = amat[(rt * L.nkc + kc) * 64u];
#pragma unroll
                for (uint32_t g = 0; g < kGroupsPerWave; ++g) {
                    if (g < groups) {
                        st_i4 B = *reinterpret_cast<const st_i4*>(lb + col + 128u * L.D * g + 64u * kc);
                        B = B ^ (int)0x80808080;                                               // u8 -> s8
                        acc[g] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B, acc[g], 0, 0, 0);
                    }
                }
            }
            // lane (j, q) holds rows 4 q ... 4 q + 3 of column j: two digits -> (zr_lo, zr_hi, zi_lo, zi_hi) of station 4 rt + q;
            // one digit -> (zr, zi) of stations 8 rt + 2 q and 8 rt + 2 q + 1
#pragma unroll
            for (uint32_t g = 0; g < kGroupsPerWave; ++g) {
                const uint32_t o = wave + 4u * (16u * g + j);  // output o0 + o of the call
                if (g < groups && o < no) {
                    const uint32_t m = L.m0_lo + o0 + o;
                    const uint32_t yi = o0 + o - (uint32_t)jfirst;
                    if (L.digits == 2u) {
                        const uint32_t k = 4u * rt + q;
                        if (k < L.K) {
                            const uint32_t sk = s * L.K + k;
                            const int zr = (int)((uint32_t)acc[g].x + ((uint32_t)acc[g].y << 7)) + L.kconst[2u * sk];
                            const int zi = (int)((uint32_t)acc[g].z + ((uint32_t)acc[g].w << 7)) + L.kconst[2u * sk + 1u];
                            ypk[k * L.lp_cap + yi] = st_rotate(tab, zr, zi, m * L.dinc[sk], sh);
                        }
                    } else {
                        const uint32_t k = 8u * rt + 2u * q;
                        if (k < L.K) {
                            const uint32_t sk = s * L.K + k;
                            ypk[k * L.lp_cap + yi] = st_rotate(tab, acc[g].x + L.kconst[2u * sk], acc[g].y + L.kconst[2u * sk + 1u],
                                                               m * L.dinc[sk], sh);
                        }
                        if (k + 1u < L.K) {
                            const uint32_t sk = s * L.K + k + 1u;
                            ypk[(k + 1u) * L.lp_cap + yi] = st_rotate(tab, acc[g].z + L.kconst[2u * sk], acc[g].w + L.kconst[2u * sk + 1u],
                                                                      m * L.dinc[sk], sh);
                        }
                    }
                }
            }
        }
    }
    if (jfirst < 0)                                          // y[-1] = demod_pre of every station
        for (uint32_t k = tid; k < L.K; k += kThreads) {
            const FmdChanState& st = L.st_in[s * L.K + k];
            ypk[k * L.lp_cap] = pack_lp(st.demod_pre_re, st.demod_pre_im);
        }
    // audio group k of the tile (k == nk: the trailing partial group): first and last discriminator sample (as fmd_firdemod.hip)
    for (uint32_t k = tid; k <= r.kt; k += kThreads) {
        const uint32_t x = T.er + k * L.fb;
        uint32_t u, xrem;
        if (L.sr_shift < 32u) { u = x >> L.sr_shift; xrem = x & (r.sr - 1u); }
        else { u = fmd_udiv_small(x, r.sr, L.inv_sr); xrem = x - u * r.sr; }
        int e = (int)(T.eq + k * L.fa + u);
        int s0 = e - (int)L.fa + (xrem < L.fb ? 0 : 1);
        s0 = s0 > 0 ? s0 : 0;                                // the call's first group starts at sample 0
        e = e < T.jB ? e : T.jB;                             // the carried group ends with the call
        gse[2u * k] = s0; gse[2u * k + 1u] = e;
    }
    // the stream's last tile also writes the next call's history (virtual bytes nbytes ... nbytes + HB)
    if (T.last) {
        typedef FMD_ST_GLOBAL uint32_t* gwo;
        for (uint32_t i = tid; i < L.HB / 4u; i += kThreads)
            ((gwo)(uintptr_t)(L.hist_out + (uint64_t)s * L.HB))[i] = virt_dword(L, s, (uint32_t)L.nbytes + 4u * i);
    }
    __syncthreads();

    // ---- 4. fm_demod (:355-367) + low_pass_real (:408-426), one lane per (station, audio group) ---------------------------------
    const uint32_t nk = T.k1 - T.k0;
    const uint32_t ng = nk + (T.last ? 1u : 0u);
    for (uint32_t idx = tid; idx < L.K * ng; idx += kThreads) {
        const uint32_t k = idx / ng, gq = idx - k * ng;
        const uint32_t c = s * L.K + k;
        const uint32_t* y = ypk + k * L.lp_cap;              // y[j - jfirst] = output j of the call
        const int s0 = gse[2u * gq], e = gse[2u * gq + 1u];
        int sum = 0, d_first = 0, cr0 = 0, ci0 = 0;
        bool guarded = false;
        for (int jj = s0; jj <= e; ++jj) {
            const uint32_t a = y[jj - jfirst], b = y[jj - 1 - jfirst];
            int d;
            if (jj == 0) {                                   // the first sample of the call takes the f64 path (:359)
                fmd_mul_conj(lp_re(a), lp_im(a), lp_re(b), lp_im(b), cr0, ci0);
                d = polar_f64(cr0, ci0, L.f64_guard, guarded);
#ifdef FMD_EXPERIMENT
                if (guarded) d += L.f64_skew;
#endif
                d = (int)(int16_t)d;
                d_first = d;
            } else if (L.f32_disc) {
                d = disc_f32_c((float)lp_re(a), (float)lp_im(a), (float)lp_re(b), (float)lp_im(b));
            } else {
                d = (int)(int16_t)disc_nosel(a, b);          // (:362) `as i16`, summed as i32 (:414)
            }
            sum += d;
        }
        int16_t* const outc = L.out + (uint64_t)c * L.out_stride;
        if (gq < nk) {
            const uint32_t ka = T.k0 + gq;
            if (ka == 0u) sum += L.st_in[c].now_lpr;         // continues the previous call's partial sum (:410-417)
            outc[ka] = (int16_t)fmd_sdiv_small(sum, r.R, L.inv_R);
            if (guarded) exc_emit_st(L.exc, c, L.seq, (int)ka, sum, d_first, cr0, ci0, outc + ka);
        } else {                                             // the trailing partial group: the station's state after the call
            const FmdChanState si = L.st_in[c];
            FmdChanState ns_{};
            ns_.now_lpr = sum + (L.P.K == 0u ? si.now_lpr : 0);
            ns_.lpr_index_r = fmd_next_lpr_index_r(r, L.P.i0r, L.P.M, L.P.K);
            const uint32_t l = y[cnt - 1];                   // demod_pre = the last filter output
            ns_.demod_pre_re = lp_re(l); ns_.demod_pre_im = lp_im(l);
            L.st_out[c] = ns_;
            if (guarded) exc_emit_st(L.exc, c, L.seq, -1, ns_.now_lpr, d_first, cr0, ci0, outc);
        }
    }
}

#define ST_TRY(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            char m_[256];                                                                   \
            snprintf(m_, sizeof m_, "%s failed: %s", #expr, hipGetErrorString(e_));         \
            fmd_internal_set_err(m_);                                                       \
            return e_ == hipErrorOutOfMemory ? FMD_ERR_NOMEM : FMD_ERR_HIP;                 \
        }                                                                                   \
    } while (0)

#define ST_ON_DEVICE(dev)                                                                   \
    FmdDeviceGuard dev_guard_(dev);                                                         \
    if (dev_guard_.error() != hipSuccess) { fmd_internal_set_err("hipSetDevice failed"); return FMD_ERR_HIP; }

}  // namespace fmd_st

struct fmd_stations {
    uint32_t T = 0, D = 0, K = 0, S = 0, shift = 0, HB = 0;
    uint32_t lp_bound = 0;                                // ceil(256 max_gain / 2^shift): the largest |y| component
    int device = 0;
    uint64_t pos = 0;                                     // samples consumed per stream
    FmdStationsPlan plan;
    uint32_t* d_amat = nullptr;
    int32_t* d_kconst = nullptr;
    uint32_t* d_dinc = nullptr;
    uint32_t* d_tab = nullptr;
    uint8_t* d_hist[2] = {nullptr, nullptr};
    FmdChanState* d_state[2] = {nullptr, nullptr};
    int cur = 0;
    FmdRates r{};
    uint32_t i0r = 0;                                     // resampler phase (identical for every station)
    uint32_t lp_cap = 0, raw_bytes = 0;
    size_t lds = 0;
    FmdExcBuf* d_exc = nullptr;
    uint32_t* h_head = nullptr;
    double f64_guard = 0x1p-20;
    int32_t f64_skew = 0;
    uint32_t seq = 0;
    uint64_t f64_guarded = 0, f64_patched = 0;
    FmdStreamOrder order;
    hipStream_t stream = nullptr;
    uint8_t* d_iq = nullptr; size_t d_iq_cap = 0;
    int16_t* d_out = nullptr; size_t d_out_cap = 0;
};

namespace {

using fmd_st::kMaxOutputs;
using fmd_st::kTableBytes;

constexpr size_t kLdsBudget = 40960;                      // 4 tiles per CU

// LDS of a tile of `kt` audio samples: raw bytes the matrix phase may read + NCO table + packed outputs + group table
bool st_sizes(const fmd_stations* b, uint32_t kt, uint32_t* lp_cap, uint32_t* raw_bytes, size_t* lds)
{
    FmdRates r = b->r; r.kt = kt;
    const uint32_t cap = fmd_tile_lp_cap(r);
    if (cap > kMaxOutputs) return false;
    const uint64_t D = b->D;
    const uint64_t groups = ((cap + 3u) / 4u + 15u) / 16u;           // 16-column groups of a wave
    const uint64_t reads = 12 + 6 * D + 8 * D * (16 * groups - 1) + 64ull * b->plan.nkc;
    const uint64_t staged = 12 + 2 * D * (cap - 1) + 2ull * b->T + 15;
    const uint64_t raw = ((reads > staged ? reads : staged) + 15) & ~15ull;
    const uint64_t total = raw + kTableBytes + 4ull * b->K * cap + 8ull * (kt + 2);
    if (total > 64 * 1024) return false;
    *lp_cap = cap; *raw_bytes = (uint32_t)raw; *lds = (size_t)total;
    return true;
}

void st_counts(const fmd_stations* b, uint64_t ns, uint64_t* m0, uint64_t* m1)
{
    const uint64_t S = b->pos, T = b->T, M = b->D;
    *m0 = S >= T ? (S - T) / M + 1 : 0;
    *m1 = S + ns >= T ? (S + ns - T) / M + 1 : 0;
}

int st_enqueue(fmd_stations* b, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* n_each, hipStream_t stream)
{
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0 (simple_fm.rs:286 would panic)"); return FMD_ERR_BAD_LENGTH; }
    if (nbytes == 0 || nbytes > (1ull << 31) - (1ull << 20)) { fmd_internal_set_err("nbytes out of range"); return FMD_ERR_UNSUPPORTED; }
    if (((uintptr_t)d_iq & 3u) != 0 || ((uintptr_t)d_out & 1u) != 0) { fmd_internal_set_err("misaligned device buffer"); return FMD_ERR_INVALID_ARG; }
    const uint64_t ns = nbytes / 2;
    uint64_t m0, m1;
    st_counts(b, ns, &m0, &m1);
    const uint64_t Mdec = m1 - m0;
    if (Mdec < 2) { fmd_internal_set_err("the call yields fewer than 2 filter outputs (simple_fm.rs:356 asserts > 1)"); return FMD_ERR_TOO_SHORT; }
    const FmdRates r = b->r;
    if (!fmd_ranges_fit32(r, Mdec * r.D)) { fmd_internal_set_err("call exceeds the 32-bit index range for these rates"); return FMD_ERR_UNSUPPORTED; }
    fmd_st::StLaunch L{};
    L.P = fmd_make_plan(r, 0u, b->i0r, 0u);
    L.P.M = (uint32_t)Mdec;
    L.P.K = fmd_num_audio(r, b->i0r, L.P.M);
    L.P.nt = fmd_num_tiles(r, L.P.K);
    if (L.P.K > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    if (L.P.nt > (1u << 30) || b->S > 65535u) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }
    L.iq = static_cast<const uint8_t*>(d_iq);
    L.nbytes = nbytes;
    L.hist_in = b->d_hist[b->cur]; L.hist_out = b->d_hist[b->cur ^ 1];
    L.HB = b->HB;
    L.vb_first = (uint32_t)(2ull * (b->D * m0 + b->HB / 2 - b->pos));   // >= 0: the window of output m0 starts at most n_taps - 1 samples back
    L.m0_lo = (uint32_t)m0;
    L.D = b->D; L.T = b->T; L.K = b->K; L.S = b->S; L.shift = b->shift;
    L.nrt = b->plan.nrt; L.nkc = b->plan.nkc; L.digits = b->plan.digits;
    L.amat = b->d_amat; L.kconst = b->d_kconst; L.dinc = b->d_dinc; L.tab = b->d_tab;
    L.r = r; L.tl = fmd_make_tiling(r);
    L.fa = r.fr / r.sr; L.fb = r.fr % r.sr;
    L.sr_shift = 32u;
    if ((r.sr & (r.sr - 1u)) == 0u) { L.sr_shift = 0u; while ((1u << L.sr_shift) < r.sr) ++L.sr_shift; }
    L.inv_sr = 1.0f / (float)r.sr; L.inv_R = 1.0f / (float)r.R;
    L.lp_cap = b->lp_cap; L.raw_bytes = b->raw_bytes;
    L.f32_disc = b->lp_bound <= 2048u ? 1u : 0u;
    L.st_in = b->d_state[b->cur]; L.st_out = b->d_state[b->cur ^ 1];
    L.out = static_cast<int16_t*>(d_out); L.out_stride = out_cap;
    L.exc = b->d_exc; L.f64_guard = b->f64_guard; L.seq = b->seq + 1; L.f64_skew = b->f64_skew;
    ST_TRY(b->order.before(stream));
    hipLaunchKernelGGL(fmd_st::fmd_stations_kernel, dim3(L.P.nt, b->S), dim3(fmd_st::kThreads), b->lds, stream, L);
    ST_TRY(hipGetLastError());
    (void)b->order.after(stream);
    b->seq += 1;
    b->cur ^= 1;
    b->i0r = fmd_next_lpr_index_r(r, b->i0r, L.P.M, L.P.K);
    b->pos += ns;
    if (n_each) *n_each = L.P.K;
    return FMD_OK;
}

int st_settle(fmd_stations* b, int16_t* host_out, size_t host_cap)
{
    return fmd_internal_resolve_exc(b->d_exc, b->r.R, b->seq, b->seq, b->d_state[b->cur], host_out, host_cap, &b->f64_guarded,
                                    &b->f64_patched);
}

}  // namespace

extern "C" {

int fmd_stations_phase_inc(int32_t offset_hz, uint32_t capture_rate, uint32_t* inc)
{
    if (!inc) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (capture_rate == 0) { fmd_internal_set_err("capture_rate == 0"); return FMD_ERR_BAD_RATES; }
    const int64_t off = offset_hz;
    if (2 * (off < 0 ? -off : off) > (int64_t)capture_rate) { fmd_internal_set_err("need |offset_hz| <= capture_rate / 2"); return FMD_ERR_UNSUPPORTED; }
    const __int128 num = (__int128)off * ((__int128)1 << 32) + (capture_rate / 2u);
    __int128 q = num / capture_rate;
    if (num % capture_rate != 0 && num < 0) q -= 1;                 // floor
    *inc = (uint32_t)(uint64_t)(q & 0xFFFFFFFF);
    return FMD_OK;
}

int fmd_stations_nco_table(int16_t* table)
{
    if (!table) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    fmd_st_nco_table(table);
    return FMD_OK;
}

size_t fmd_stations_out_cap(uint32_t decim, uint32_t rate_out, uint32_t rate_resample, size_t nbytes)
{
    if (!decim || !rate_out) return 0;
    const uint64_t M = nbytes / 2 / decim + 2;
    return (size_t)((M * rate_resample + rate_out - 1) / rate_out + 1);
}

int fmd_stations_new(const int16_t* taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t* phase_inc,
                     uint32_t n_stations, uint32_t rate_out, uint32_t rate_resample, const fmd_device_config* dev,
                     fmd_stations** out)
{
    if (!taps || !phase_inc || !dev || !out || dev->n_channels == 0) { fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n_taps == 0 || n_taps > 256 || decim < 2 || decim % 2 != 0 || decim > 64 || shift > 24 || n_stations == 0 || n_stations > 32 ||
        dev->n_channels > 65535u) {
        fmd_internal_set_err("need 1 <= n_taps <= 256, an even 2 <= decim <= 64, shift <= 24, 1 <= n_stations <= 32, n_streams <= 65535");
        return FMD_ERR_UNSUPPORTED;
    }
    if (rate_resample == 0 || rate_out < rate_resample) {
        fmd_internal_set_err("need rate_out >= rate_resample >= 1 (simple_fm.rs:421 divides by rate_out / rate_resample)");
        return FMD_ERR_BAD_RATES;
    }
    for (uint32_t t = 0; t < n_taps; ++t)
        if (taps[t] > 2047 || taps[t] < -2047) { fmd_internal_set_err("|tap| > 2047"); return FMD_ERR_UNSUPPORTED; }
    fmd_stations* b = new (std::nothrow) fmd_stations();
    if (!b) return FMD_ERR_NOMEM;
    b->T = n_taps; b->D = decim; b->K = n_stations; b->S = dev->n_channels; b->shift = shift;
    fmd_st_build_plan(taps, n_taps, decim, phase_inc, b->S, b->K, b->plan);
    // |y| <= 256 G / 2^shift (|z| <= 128 G per component, the rotation adds two of them) must stay in the discriminator's range
    const uint64_t bound = (256ull * b->plan.max_gain + ((1ull << shift) - 1ull)) >> shift;
    if (bound > 16384ull) {
        delete b;
        fmd_internal_set_err("filter gain too large for the discriminator: need ceil(256 * max sum(|Wr| + |Wi|) / 2^shift) <= 16384");
        return FMD_ERR_UNSUPPORTED;
    }
    b->lp_bound = (uint32_t)bound;
    FmdRates& r = b->r;
    r.D = decim; r.fast = rate_out; r.slow = rate_resample;
    r.g = fmd_gcd(r.fast, r.slow); r.fr = r.fast / r.g; r.sr = r.slow / r.g;
    r.R = (int32_t)(r.fast / r.slow);
    const uint64_t fa = r.fr / r.sr;
    if (r.fr > FMD_MAX_RATE_REDUCED || (fa + 2) * 32768ull >= (1u << 24) || (uint32_t)r.R >= (1u << 24)) {
        delete b; fmd_internal_set_err("rate ratio outside the exact-small-divide range"); return FMD_ERR_UNSUPPORTED;
    }
    const size_t budget = (size_t)fmd_knob_u32("FMD_ST_LDS", (uint32_t)kLdsBudget);
    uint32_t best = 0;
    for (uint32_t kt = 1; kt <= 1024; ++kt) {
        if ((uint64_t)r.sr * (kt + 2) >= (1u << 24)) break;
        uint32_t lc, rb; size_t l;
        if (!st_sizes(b, kt, &lc, &rb, &l)) break;
        if (l > budget && best) break;
        best = kt;
    }
    if (!best) { delete b; fmd_internal_set_err("one audio sample does not fit a tile: rate_out / rate_resample x decim too large"); return FMD_ERR_UNSUPPORTED; }
    r.kt = best;
    if (!st_sizes(b, r.kt, &b->lp_cap, &b->raw_bytes, &b->lds)) { delete b; return FMD_ERR_UNSUPPORTED; }
    b->HB = 2u * ((n_taps - 1u + 7u) & ~7u);
    if (const char* g = fmd_knob("FMD_F64_GUARD_LOG2")) b->f64_guard = ldexp(1.0, atoi(g));   // experiment build only
    b->f64_skew = fmd_knob_i32("FMD_F64_SKEW", 0);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { delete b; fmd_internal_set_err("no HIP device (this library has no CPU path)"); return FMD_ERR_NO_DEVICE; }
    int device = dev->device_id;
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    hipDeviceProp_t prop;
    if (device >= ndev || hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        delete b; fmd_internal_set_err("device is not a gfx950"); return FMD_ERR_NO_DEVICE;
    }
    b->device = device;
    auto fail = [&](const char* what) { fmd_internal_set_err(what); fmd_stations_free(b); return FMD_ERR_HIP; };
    FmdDeviceGuard guard(device);
    if (guard.error() != hipSuccess) return fail("hipSetDevice");
    const FmdStationsPlan& P = b->plan;
    if (hipMalloc(&b->d_amat, P.amat.size() * 4) != hipSuccess || hipMemcpy(b->d_amat, P.amat.data(), P.amat.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMalloc(tap matrix)");
    if (hipMalloc(&b->d_kconst, P.kconst.size() * 4) != hipSuccess || hipMemcpy(b->d_kconst, P.kconst.data(), P.kconst.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMalloc(constants)");
    if (hipMalloc(&b->d_dinc, P.dinc.size() * 4) != hipSuccess || hipMemcpy(b->d_dinc, P.dinc.data(), P.dinc.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMalloc(phase steps)");
    int16_t tab[1024];
    fmd_st_nco_table(tab);
    if (hipMalloc(&b->d_tab, sizeof tab) != hipSuccess || hipMemcpy(b->d_tab, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMalloc(NCO table)");
    const size_t hb = (size_t)b->S * (b->HB ? b->HB : 16), sb = (size_t)b->S * b->K * sizeof(FmdChanState);
    for (int i = 0; i < 2; ++i) {
        if (hipMalloc(&b->d_hist[i], hb) != hipSuccess || hipMemset(b->d_hist[i], 0, hb) != hipSuccess) return fail("hipMalloc(history)");
        if (hipMalloc(&b->d_state[i], sb) != hipSuccess || hipMemset(b->d_state[i], 0, sb) != hipSuccess) return fail("hipMalloc(state)");
    }
    if (hipMalloc(&b->d_exc, sizeof(FmdExcBuf)) != hipSuccess || hipMemset(b->d_exc, 0, sizeof(FmdExcBuf)) != hipSuccess) return fail("hipMalloc(reports)");
    if (hipHostMalloc(reinterpret_cast<void**>(&b->h_head), 16, hipHostMallocDefault) != hipSuccess) return fail("hipHostMalloc(report head)");
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate");
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    *out = b;
    return FMD_OK;
}

void fmd_stations_free(fmd_stations* b)
{
    if (!b) return;
    FmdDeviceGuard guard(b->device);
    (void)hipDeviceSynchronize();
    b->order.destroy();
    if (b->d_amat) (void)hipFree(b->d_amat);
    if (b->d_kconst) (void)hipFree(b->d_kconst);
    if (b->d_dinc) (void)hipFree(b->d_dinc);
    if (b->d_tab) (void)hipFree(b->d_tab);
    for (int i = 0; i < 2; ++i) { if (b->d_hist[i]) (void)hipFree(b->d_hist[i]); if (b->d_state[i]) (void)hipFree(b->d_state[i]); }
    if (b->d_exc) (void)hipFree(b->d_exc);
    if (b->h_head) (void)hipHostFree(b->h_head);
    if (b->d_iq) (void)hipFree(b->d_iq);
    if (b->d_out) (void)hipFree(b->d_out);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int fmd_stations_reset(fmd_stations* b)
{
    if (!b) return FMD_ERR_INVALID_ARG;
    ST_ON_DEVICE(b->device);
    ST_TRY(hipDeviceSynchronize());
    const size_t hb = (size_t)b->S * (b->HB ? b->HB : 16), sb = (size_t)b->S * b->K * sizeof(FmdChanState);
    for (int i = 0; i < 2; ++i) { ST_TRY(hipMemset(b->d_hist[i], 0, hb)); ST_TRY(hipMemset(b->d_state[i], 0, sb)); }
    ST_TRY(hipMemset(b->d_exc, 0, 16));
    ST_TRY(hipDeviceSynchronize());
    b->pos = 0; b->cur = 0; b->i0r = 0;
    b->order.reset();
    return FMD_OK;
}

int fmd_stations_demodulate_device(fmd_stations* b, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap,
                                   size_t* out_len_each, void* stream)
{
    if (!b || !d_iq || !d_out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    ST_ON_DEVICE(b->device);
    return st_enqueue(b, d_iq, nbytes, d_out, out_cap, out_len_each, static_cast<hipStream_t>(stream));
}

int fmd_stations_check(fmd_stations* b)
{
    if (!b) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    ST_ON_DEVICE(b->device);
    if (b->order.have_last && b->h_head) {                   // one stream synchronisation in the common case (see fmd_demod_check)
        b->h_head[0] = b->h_head[1] = ~0u;
        hipError_t e = hipMemcpyAsync(b->h_head, b->d_exc, 16, hipMemcpyDeviceToHost, b->order.last);
        if (e == hipSuccess) e = hipStreamSynchronize(b->order.last);
        if (e == hipSuccess && b->h_head[0] == 0u && b->h_head[1] == 0u) return FMD_OK;
        if (e != hipSuccess) (void)hipGetLastError();
    }
    ST_TRY(hipDeviceSynchronize());
    return st_settle(b, nullptr, 0);
}

int fmd_stations_demodulate_batch(fmd_stations* b, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!b || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    ST_ON_DEVICE(b->device);
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0"); return FMD_ERR_BAD_LENGTH; }
    const size_t rows = (size_t)b->S * b->K;
    const size_t in_bytes = nbytes * (size_t)b->S, out_elems = out_cap * rows;
    if (in_bytes > b->d_iq_cap) {
        if (b->d_iq) { ST_TRY(hipFree(b->d_iq)); b->d_iq = nullptr; b->d_iq_cap = 0; }
        ST_TRY(hipMalloc(&b->d_iq, in_bytes ? in_bytes : 1));
        b->d_iq_cap = in_bytes;
    }
    if (out_elems > b->d_out_cap) {
        if (b->d_out) { ST_TRY(hipFree(b->d_out)); b->d_out = nullptr; b->d_out_cap = 0; }
        ST_TRY(hipMalloc(&b->d_out, (out_elems ? out_elems : 1) * sizeof(int16_t)));
        b->d_out_cap = out_elems;
    }
    ST_TRY(hipMemcpyAsync(b->d_iq, iq, in_bytes, hipMemcpyHostToDevice, b->stream));
    size_t n = 0;
    int rc = st_enqueue(b, b->d_iq, nbytes, b->d_out, out_cap, &n, b->stream);
    if (rc) return rc;
    if (n) ST_TRY(hipMemcpyAsync(out, b->d_out, out_elems * sizeof(int16_t), hipMemcpyDeviceToHost, b->stream));
    ST_TRY(hipStreamSynchronize(b->stream));
    for (size_t c = 0; c < rows; ++c) out_len[c] = n;
    return st_settle(b, out, out_cap);
}

int fmd_stations_get_state(fmd_stations* b, uint32_t stream, uint32_t station, fmd_demod_state* state)
{
    if (!b || !state || stream >= b->S || station >= b->K) { fmd_internal_set_err("bad argument"); return FMD_ERR_INVALID_ARG; }
    ST_ON_DEVICE(b->device);
    ST_TRY(hipDeviceSynchronize());
    int rc = st_settle(b, nullptr, 0);
    if (rc) return rc;
    FmdChanState s;
    ST_TRY(hipMemcpy(&s, b->d_state[b->cur] + ((size_t)stream * b->K + station), sizeof(s), hipMemcpyDeviceToHost));
    memset(state, 0, sizeof(*state));
    state->now_lpr = s.now_lpr;
    state->prev_lpr_index = (int32_t)(s.lpr_index_r * b->r.g);
    state->demod_pre_re = s.demod_pre_re; state->demod_pre_im = s.demod_pre_im;
    return FMD_OK;
}

int fmd_stations_f64_stats(const fmd_stations* b, uint64_t* guarded, uint64_t* patched)
{
    if (!b) return FMD_ERR_INVALID_ARG;
    if (guarded) *guarded = b->f64_guarded;
    if (patched) *patched = b->f64_patched;
    return FMD_OK;
}

int fmd_stations_kernel_name(const fmd_stations* b, char* name, size_t cap)
{
    if (!b || !name || cap == 0) return FMD_ERR_INVALID_ARG;
    const int n = snprintf(name, cap, "fmd_st::fmd_stations_kernel");
    return n < 0 || (size_t)n >= cap ? FMD_ERR_CAPACITY : FMD_OK;
}

}  // extern "C"
