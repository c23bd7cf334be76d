// fmd_resample.hip -- rational resampler: a polyphase L / M filter over the int16 rows a bank leaves on the device, in ONE gfx950
// kernel.  Width 1 is mono audio, width 2 interleaved (L, R) or (I, Q); a row is one (stream, station) or (stream, channel).
//
// Definition (include/fmd.h, "rational resampler"; tests/resample_ref.py), per row and component c < width:
//     q_n = n M,  i_n = floor(q_n / L),  p_n = q_n mod L
//     v[n][c]   = sum_{t < T} g[p_n][t] x[i_n + t][c]          (exact in i32: every phase has sum |g| <= 32767)
//     out[n][c] = sat16(v[n][c] >> shift)
// Output n comes with the call in which x[i_n + T - 1] arrives; the handle carries the at most T - 1 samples the next call's
// first output still reads.
//
// One workgroup = one (row, tile of `tile` consecutive outputs of the call); the tile plan depends on the call's first output and
// its output count only, never on how the stream was cut before:
//   1. stage the tile's input span [i_first, i_last + T) in LDS, one int16 PLANE per component: 16-byte loads of the chunks that
//      lie whole inside the row's valid samples (the LDS origin is shifted so that a 16-byte chunk of the row lands on a 16-byte
//      (width 1) or two 8-byte (width 2, de-interleaved in registers) aligned LDS stores), element loads for the unaligned head
//      and tail and for the carried history, which sits in front of the call's own samples;
//   2. the tap table in LDS as dwords (g[2 d], g[2 d + 1]), every phase padded with zero taps to an ODD number of dwords, so that
//      lanes on different phases start on different banks: the whole table, phase-major, when L <= tile; otherwise only the
//      tile's own phases, in lane order;
//   3. one lane per output, both components: per tap pair one dword of taps, one dword of each plane (a sliding window: each is
//      read once), v_alignbit_b32 by the lane's sample parity, v_dot2_i32_i16;
//   4. shift, saturate, one dword (width 2) or one short (width 1) per lane, consecutive lanes consecutive addresses.
// The row's last tile also writes the next call's history.  HBM traffic: the input once (plus T samples per tile), 2 width bytes
// per output, the (L2-resident) tap table once per tile.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_rows.h"

namespace fmd_rs {

constexpr int kThreads = 256;
constexpr uint32_t kMaxTile = 256;                        // one lane per output
constexpr size_t kLdsBudget = 61440;                      // planes + taps of a tile
constexpr uint32_t kPlaneSlack = 32;                      // samples: the origin shift, the whole chunks at both ends, the window's last dword

typedef int i4 __attribute__((ext_vector_type(4)));
typedef short s2 __attribute__((ext_vector_type(2)));

struct RsLaunch {
    const int16_t* in;         // [n_rows][in_cap][W]
    uint64_t in_cap;
    uint32_t n_in;             // valid samples per row
    uint32_t n_rows;
    const int16_t* hist_in;    // [n_rows][hcap][W]: the first h are the samples in front of the call
    int16_t* hist_out;
    uint32_t hcap, h, h_next;
    uint32_t v_first;          // virtual sample (history ++ call) of x[i] of the call's first output
    uint32_t p_first;          // its phase
    uint32_t n_out;            // outputs of this call per row
    uint32_t L, M, T, shift;
    uint32_t npair, tdw;       // tap pairs per phase (ceil(T / 2)); dwords per phase in the table (npair | 1)
    uint32_t tile, ntiles;
    uint32_t plane_len;        // int16 per plane (a multiple of 8)
    uint32_t whole;            // 1: the whole table is staged, phase-major; 0: the tile's phases in lane order
    const uint32_t* taps;      // [L][tdw]
    int16_t* out;              // [n_rows][out_cap][W]
    uint64_t out_cap;
};

__device__ __forceinline__ int dot2(uint32_t g, uint32_t x, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s2, g), __builtin_bit_cast(s2, x), acc, false);
}

__device__ __forceinline__ int sat16(int v) { return v > 32767 ? 32767 : (v < -32768 ? -32768 : v); }

template <int W>
__global__ void __launch_bounds__(kThreads) fmd_resample_kernel(const RsLaunch P)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / P.ntiles, t = blockIdx.x - row * P.ntiles;
    if (row >= P.n_rows) return;
    int16_t* const plane = reinterpret_cast<int16_t*>(lds);  // [W][plane_len]
    uint32_t* const tp = lds + ((W * P.plane_len) >> 1);

    constexpr uint32_t E = 8u / W;                           // samples per 16-byte chunk
    constexpr uint32_t EB = 2u * W;                          // bytes per sample
    const uint32_t o0 = t * P.tile;                          // first output (of this call) of the tile
    const uint32_t no = P.n_out - o0 < P.tile ? P.n_out - o0 : P.tile;
    const uint64_t qq = (uint64_t)P.p_first + (uint64_t)o0 * P.M;
    const uint32_t i0 = (uint32_t)(qq / P.L), p0 = (uint32_t)(qq - (uint64_t)i0 * P.L);   // block-uniform
    const uint32_t va = P.v_first + i0;                                                   // virtual samples [va, vb) are staged
    const uint32_t vb = va + (p0 + (no - 1u) * P.M) / P.L + P.T;                          // (vb > h: every output reads a new sample)
    const uint32_t hh = va < P.h ? P.h - va : 0u;                                         // of them history
    const uint32_t ja = va > P.h ? va - P.h : 0u, jb = vb - P.h;                          // call samples [ja, jb), jb <= n_in

    // ---- 1. staging ---------------------------------------------------------------------------------------------------------
    const int16_t* const rowp = P.in + (uint64_t)row * P.in_cap * W;
    const uintptr_t R = (uintptr_t)rowp, Rend = R + (uintptr_t)P.n_in * EB;
    const uintptr_t a0 = R + (uintptr_t)ja * EB, a1 = R + (uintptr_t)jb * EB;
    const uintptr_t c_lo = a0 >> 4, c_hi = (a1 + 15u) >> 4;
    const uint32_t koff = (uint32_t)(a0 & 15u) / EB;
    const uint32_t kc = hh + (koff + E - hh % E) % E;        // LDS index of call sample ja: kc - koff is a multiple of E, >= 0
    const uint32_t k_lo = kc - koff;                         // LDS index of the first sample of chunk c_lo
    for (uint32_t i = tid; i < (uint32_t)(c_hi - c_lo); i += kThreads) {
        const uintptr_t ca = (c_lo + i) << 4;
        const uint32_t k = k_lo + i * E;
        if (ca >= R && ca + 16u <= Rend) {                   // whole inside the row's valid samples
            const i4 q = *(const FMD_DDC_GLOBAL i4*)ca;
            if (W == 1) {
                *reinterpret_cast<i4*>(plane + k) = q;
            } else {
                const uint32_t x = (uint32_t)q.x, y = (uint32_t)q.y, z = (uint32_t)q.z, w = (uint32_t)q.w;
                uint2 c0, c1;
                c0.x = (x & 0xFFFFu) | (y << 16); c0.y = (z & 0xFFFFu) | (w << 16);
                c1.x = (x >> 16) | (y & 0xFFFF0000u); c1.y = (z >> 16) | (w & 0xFFFF0000u);
                *reinterpret_cast<uint2*>(plane + k) = c0;
                *reinterpret_cast<uint2*>(plane + P.plane_len + k) = c1;
            }
        } else {                                             // the unaligned head or tail: only what the tile needs
            for (uint32_t e = 0; e < E; ++e) {
                const uintptr_t a = ca + e * EB;
                if (a < a0 || a >= a1) continue;
                const FMD_DDC_GLOBAL int16_t* src = (const FMD_DDC_GLOBAL int16_t*)a;
                plane[k + e] = src[0];
                if (W == 2) plane[P.plane_len + k + e] = src[1];
            }
        }
    }
    {
        const FMD_DDC_GLOBAL int16_t* hin = (const FMD_DDC_GLOBAL int16_t*)(uintptr_t)(P.hist_in + ((uint64_t)row * P.hcap + va) * W);
        for (uint32_t i = tid; i < hh; i += kThreads) {
            plane[kc - hh + i] = hin[i * W];
            if (W == 2) plane[P.plane_len + kc - hh + i] = hin[i * W + 1u];
        }
    }

    // ---- 2. the tap table ---------------------------------------------------------------------------------------------------
    const FMD_DDC_GLOBAL uint32_t* gt = (const FMD_DDC_GLOBAL uint32_t*)(uintptr_t)P.taps;
    if (P.whole) {
        for (uint32_t i = tid; i < P.L * P.tdw; i += kThreads) tp[i] = gt[i];
    } else {
        for (uint32_t i = tid; i < no * P.tdw; i += kThreads) {
            const uint32_t j = i / P.tdw, d = i - j * P.tdw;
            tp[i] = gt[((p0 + j * P.M) % P.L) * P.tdw + d];
        }
    }

    // the row's last tile also writes the next call's history: the last h_next virtual samples
    if (t == P.ntiles - 1u) {
        const uint32_t v0 = P.h + P.n_in - P.h_next;
        const FMD_DDC_GLOBAL int16_t* hin = (const FMD_DDC_GLOBAL int16_t*)(uintptr_t)(P.hist_in + (uint64_t)row * P.hcap * W);
        const FMD_DDC_GLOBAL int16_t* cin = (const FMD_DDC_GLOBAL int16_t*)(uintptr_t)rowp;
        FMD_DDC_GLOBAL int16_t* hout = (FMD_DDC_GLOBAL int16_t*)(uintptr_t)(P.hist_out + (uint64_t)row * P.hcap * W);
        for (uint32_t i = tid; i < P.h_next * W; i += kThreads) {
            const uint32_t v = v0 + i / W, c = i % W;
            hout[i] = v < P.h ? hin[v * W + c] : cin[(uint64_t)(v - P.h) * W + c];
        }
    }
    __syncthreads();

    // ---- 3./4. one lane per output ------------------------------------------------------------------------------------------
    if (tid >= no) return;
    const uint32_t r = p0 + tid * P.M, di = r / P.L, p = r - di * P.L;
    const uint32_t kn = kc - hh + di;                        // LDS index of x[i_n]
    const uint32_t sh = (kn & 1u) << 4;
    const uint32_t* const g = tp + (P.whole ? p : tid) * P.tdw;
    const uint32_t* const x0 = reinterpret_cast<const uint32_t*>(plane) + (kn >> 1);
    const uint32_t* const x1 = x0 + (P.plane_len >> 1);
    int acc0 = 0, acc1 = 0;
    uint32_t w0 = x0[0], w1 = W == 2 ? x1[0] : 0u;
    for (uint32_t d = 0; d < P.npair; ++d) {
        const uint32_t gd = g[d];
        const uint32_t n0 = x0[d + 1u];
        acc0 = dot2(gd, __builtin_amdgcn_alignbit(n0, w0, sh), acc0);
        w0 = n0;
        if (W == 2) {
            const uint32_t n1 = x1[d + 1u];
            acc1 = dot2(gd, __builtin_amdgcn_alignbit(n1, w1, sh), acc1);
            w1 = n1;
        }
    }
    const int y0 = sat16(acc0 >> P.shift);
    const uint64_t oi = ((uint64_t)row * P.out_cap + o0 + tid) * W;
    if (W == 2) {
        const int y1 = sat16(acc1 >> P.shift);
        ((FMD_DDC_GLOBAL uint32_t*)(uintptr_t)(P.out + oi))[0] = ((uint32_t)y0 & 0xFFFFu) | ((uint32_t)y1 << 16);
    } else {
        ((FMD_DDC_GLOBAL int16_t*)(uintptr_t)(P.out + oi))[0] = (int16_t)y0;
    }
}

}  // namespace fmd_rs

struct fmd_resample {
    FmdRows rows;                                         // hcap = max(1, T - 1)
    void* d_taps = nullptr;                               // [L][tdw] dwords
    uint32_t L = 0, M = 0, T = 0, shift = 0;
    uint32_t npair = 0, tdw = 0;
    uint32_t tile = 0, plane_len = 0, whole = 0;
};

namespace {

// outputs completed once `n` samples per row have arrived
uint64_t rs_outputs(const fmd_resample* h, uint64_t n)
{
    return n >= h->T ? ((n - h->T + 1) * h->L + h->M - 1) / h->M : 0;
}

// "need ..." with FMD_ERR_UNSUPPORTED when `L / M` lies outside the domain
int rs_ratio_ok(uint64_t L, uint64_t M)
{
    if (L < 1 || L > 1024 || M < 1 || M > 1024) { fmd_internal_set_err("need 1 <= L <= 1024 and 1 <= M <= 1024"); return FMD_ERR_UNSUPPORTED; }
    if (M > 32 * L) { fmd_internal_set_err("need M <= 32 L"); return FMD_ERR_UNSUPPORTED; }
    if (L > 8 * M) { fmd_internal_set_err("need L <= 8 M"); return FMD_ERR_UNSUPPORTED; }
    return FMD_OK;
}

// The largest tile (a power of two <= 256 outputs) whose planes and taps fit the LDS budget; 32 always does (< 42 KiB).
void rs_tiling(fmd_resample* h)
{
    for (h->tile = fmd_rs::kMaxTile;; h->tile /= 2) {
        const uint32_t span = (uint32_t)(((uint64_t)(h->tile - 1) * h->M + h->L - 1) / h->L) + h->T;
        h->plane_len = (span + fmd_rs::kPlaneSlack + 7u) & ~7u;
        h->whole = h->L <= h->tile ? 1u : 0u;
        h->rows.lds = 2ull * h->rows.width * h->plane_len + 4ull * (h->whole ? h->L : h->tile) * h->tdw;
        if (h->rows.lds <= fmd_rs::kLdsBudget || h->tile == 32) break;
    }
}

int rs_enqueue(fmd_resample* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, hipStream_t stream)
{
    FmdRows& r = h->rows;
    if (const int rc = fmd_rows_check_call(r, d_in, n_in, in_cap, d_out)) return rc;
    const uint64_t N0 = r.core.pos, N1 = N0 + n_in;
    const uint64_t out0 = rs_outputs(h, N0), out1 = rs_outputs(h, N1), cnt = out1 - out0;
    if (cnt < 1) { fmd_internal_set_err("the call completes no output"); return FMD_ERR_TOO_SHORT; }
    if (cnt > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    const uint64_t ntiles = (cnt + h->tile - 1) / h->tile;
    if (ntiles * r.n_rows >= (1ull << 31)) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }
    const uint64_t q0 = out0 * h->M, i0 = q0 / h->L, i1 = out1 * h->M / h->L;   // x[i0]: the first sample of the call's first output
    fmd_rs::RsLaunch P{};
    fmd_rows_fill(P, r, d_in, n_in, in_cap, d_out, out_cap);
    P.h = N0 > i0 ? (uint32_t)(N0 - i0) : 0u;             // <= T - 1
    P.h_next = N1 > i1 ? (uint32_t)(N1 - i1) : 0u;        // <= T - 1 and <= h + n_in
    P.v_first = N0 > i0 ? 0u : (uint32_t)(i0 - N0);       // (inputs before x[i0] are skipped where M / L > T)
    P.p_first = (uint32_t)(q0 - i0 * h->L);
    P.n_out = (uint32_t)cnt;
    P.L = h->L; P.M = h->M; P.T = h->T; P.shift = h->shift; P.npair = h->npair; P.tdw = h->tdw;
    P.tile = h->tile; P.ntiles = (uint32_t)ntiles; P.plane_len = h->plane_len; P.whole = h->whole;
    P.taps = static_cast<const uint32_t*>(h->d_taps);
    return fmd_rows_launch(r, fmd_rs::fmd_resample_kernel<1>, fmd_rs::fmd_resample_kernel<2>, (uint32_t)(ntiles * r.n_rows), fmd_rs::kThreads, P,
                           stream, n_in, cnt, n_out);
}

}  // namespace

extern "C" {

int fmd_resample_ratio(uint64_t rate_in_num, uint64_t rate_in_den, uint64_t rate_out, uint32_t* L, uint32_t* M)
{
    if (!L || !M) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (!rate_in_num || !rate_in_den || !rate_out || rate_in_den >> 32 || rate_out >> 32) {
        fmd_internal_set_err("need non-zero rates, rate_in_den and rate_out below 2^32");
        return FMD_ERR_UNSUPPORTED;
    }
    uint64_t a = rate_out * rate_in_den, b = rate_in_num;  // L / M = a / b
    uint64_t x = a, y = b;
    while (y) { const uint64_t r = x % y; x = y; y = r; }
    a /= x; b /= x;
    if (const int rc = rs_ratio_ok(a, b)) return rc;
    *L = (uint32_t)a; *M = (uint32_t)b;
    return FMD_OK;
}

size_t fmd_resample_out_cap(uint32_t L, uint32_t M, size_t n_in)
{
    if (!L || !M) return 0;
    return (size_t)(((uint64_t)n_in * L + M - 1) / M) + 1;   // outputs(N + n) - outputs(N) <= ceil(n L / M) + 1 for every N
}

int fmd_resample_new(const int16_t* taps, uint32_t L, uint32_t M, uint32_t T, uint32_t shift, uint32_t width,
                     const fmd_device_config* dev, fmd_resample** out)
{
    if (const int rc = fmd_rows_new_args(taps, dev, out, width)) return rc;
    if (const int rc = rs_ratio_ok(L, M)) return rc;
    if (T < 1 || T > 256) { fmd_internal_set_err("need 1 <= T <= 256"); return FMD_ERR_UNSUPPORTED; }
    if ((uint64_t)L * T > 16384) { fmd_internal_set_err("need L T <= 16384"); return FMD_ERR_UNSUPPORTED; }
    if (shift > 24) { fmd_internal_set_err("need shift <= 24"); return FMD_ERR_UNSUPPORTED; }
    if (const int rc = fmd_rows_count_arg(dev)) return rc;
    for (uint32_t p = 0; p < L; ++p) {
        uint32_t s = 0;
        for (uint32_t t = 0; t < T; ++t) { const int v = taps[(size_t)p * T + t]; s += (uint32_t)(v < 0 ? -v : v); }
        if (s > 32767) { fmd_internal_set_err("need sum |g| <= 32767 in every phase"); return FMD_ERR_UNSUPPORTED; }
    }
    fmd_resample* h = new (std::nothrow) fmd_resample();
    if (!h) return FMD_ERR_NOMEM;
    h->L = L; h->M = M; h->T = T; h->shift = shift;
    h->npair = (T + 1) / 2; h->tdw = h->npair | 1u;
    h->rows.width = width; h->rows.n_rows = dev->n_channels; h->rows.hcap = T > 1 ? T - 1 : 1;
    rs_tiling(h);
    std::vector<uint32_t> gp((size_t)L * h->tdw, 0u);        // (g[2 d], g[2 d + 1]), zero taps behind T
    for (uint32_t p = 0; p < L; ++p)
        for (uint32_t t = 0; t < T; ++t)
            gp[(size_t)p * h->tdw + t / 2] |= (uint32_t)(uint16_t)taps[(size_t)p * T + t] << (16 * (t & 1u));
    fmd_ddc_add_owned(h->rows.core, h->d_taps, gp.data(), gp.size() * sizeof(uint32_t));
    return fmd_rows_device(h, dev, fmd_resample_free, out);
}

void fmd_resample_free(fmd_resample* h) { fmd_rows_free(h); }
int fmd_resample_reset(fmd_resample* h) { return fmd_rows_reset(h); }
int fmd_resample_check(fmd_resample* h) { return fmd_rows_check(h); }
int fmd_resample_outputs(const fmd_resample* h, uint64_t* inputs, uint64_t* outputs) { return fmd_rows_outputs(h, inputs, outputs, rs_outputs); }

int fmd_resample_run_device(fmd_resample* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out,
                            void* stream)
{
    return fmd_ddc_run_device(h ? &h->rows.core : nullptr, d_in, d_out,
                              [&] { return rs_enqueue(h, d_in, n_in, in_cap, d_out, out_cap, n_out, static_cast<hipStream_t>(stream)); });
}

// (a call of no samples completes no output: rs_enqueue refuses it like every other such call)
int fmd_resample_run_batch(fmd_resample* h, const int16_t* in, size_t n_in, size_t in_cap, int16_t* out, size_t out_cap, size_t* n_out)
{
    return fmd_rows_run_batch(h, rs_enqueue, in, n_in, in_cap, out, out_cap, n_out, [](size_t) { return false; });
}

int fmd_resample_kernel_name(const fmd_resample* h, char* name, size_t cap) { return fmd_rows_kernel_name(h, name, cap, "fmd_rs::fmd_resample_kernel<%u>"); }

}  // extern "C"
