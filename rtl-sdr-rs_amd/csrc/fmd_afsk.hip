// fmd_afsk.hip -- tone-pair demodulator: every mono int16 row a bank leaves on the device correlated against a mark and a space tone,
// one signed soft decision per D samples, in ONE gfx950 kernel.  The front half of the packet demodulator; the host's AX.25 decoder
// (fmd_ax25_decode.cpp) reads the signs and crossings of what this writes.  A row is one (stream, channel); width is 1.
//
// Definition (include/fmd.h, "packet demodulator"; tests/afsk_ref.py), per row, tab[4][T] = mark-cos, mark-sin, space-cos, space-sin:
//     i_n = n D
//     S_q[n] = sum_{t < T} tab[q][t] x[i_n + t]              (exact in i32: T <= 64, |tab| <= 1023)
//     A_q    = S_q >> pre_shift
//     out[n] = sat16(((A_0^2 + A_1^2) - (A_2^2 + A_3^2)) >> out_shift)      (i64)
// Output n comes with the call in which x[i_n + T - 1] arrives; the handle carries the at most T - 1 samples the next call's first
// output still reads.  It is the resampler's counting at L = 1, M = D, and the resampler's kernel shape:
//
// One workgroup = one (row, tile of 256 consecutive outputs of the call):
//   1. stage the tile's input span [i_first, i_last + T) as an int16 plane in LDS: 16-byte loads of the chunks that lie whole inside
//      the row's valid samples (the LDS origin is shifted so that a 16-byte chunk of the row lands on a 16-byte aligned LDS store),
//      element loads for the unaligned head and tail and for the carried history, which sits in front of the call's own samples;
//   2. the table in LDS as [ceil(T / 2)][4] dwords (tab[q][2 d], tab[q][2 d + 1]), q the fast index, an odd T padded with a zero tap:
//      one 16-byte read, the same address in every lane (a broadcast), gives a tap pair of all four rows;
//   3. one lane per output: per tap pair one dword of the plane (a sliding window: each is read once), v_alignbit_b32 by the lane's
//      sample parity, four v_dot2_i32_i16;
//   4. the shifts, four squares and the difference in i64, the saturation, one short per lane, consecutive lanes consecutive addresses.
// The row's last tile also writes the next call's history.  HBM traffic: the input once (plus T - D samples per tile), 2 bytes per
// output.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_rows.h"

namespace fmd_af {

constexpr int kThreads = 256;
constexpr uint32_t kTile = 256;                           // one lane per output
constexpr uint32_t kPlaneSlack = 32;                      // samples: the origin shift, the whole chunks at both ends, the window's last dword

typedef int i4 __attribute__((ext_vector_type(4)));
typedef short s2 __attribute__((ext_vector_type(2)));

struct AfLaunch {
    const int16_t* in;         // [n_rows][in_cap]
    uint64_t in_cap;
    uint32_t n_in;             // valid samples per row
    uint32_t n_rows;
    const int16_t* hist_in;    // [n_rows][hcap]: the first h are the samples in front of the call
    int16_t* hist_out;
    uint32_t hcap, h, h_next;
    uint32_t n_out;            // outputs of this call per row
    uint32_t D, T, pre_shift, out_shift;
    uint32_t npair;            // tap pairs per table row (ceil(T / 2))
    uint32_t ntiles;
    uint32_t plane_len;        // int16 in the plane (a multiple of 8)
    const uint32_t* tab;       // [npair][4]
    int16_t* out;              // [n_rows][out_cap]
    uint64_t out_cap;
};

__device__ __forceinline__ int dot2(uint32_t g, uint32_t x, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s2, g), __builtin_bit_cast(s2, x), acc, false);
}

__global__ void __launch_bounds__(kThreads) fmd_afsk_kernel(const AfLaunch P)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / P.ntiles, t = blockIdx.x - row * P.ntiles;
    if (row >= P.n_rows) return;
    int16_t* const plane = reinterpret_cast<int16_t*>(lds);  // [plane_len]
    uint32_t* const tp = lds + (P.plane_len >> 1);           // 16-byte aligned: plane_len is a multiple of 8

    // virtual samples: the h carried ones, then the call's; output o of the call reads [o D, o D + T)
    const uint32_t o0 = t * kTile;                           // first output (of this call) of the tile
    const uint32_t no = P.n_out - o0 < kTile ? P.n_out - o0 : kTile;
    const uint32_t va = o0 * P.D;                            // virtual samples [va, vb) are staged
    const uint32_t vb = va + (no - 1u) * P.D + P.T;          // (vb > h: every output reads a new sample; vb <= h + n_in)
    const uint32_t hh = va < P.h ? P.h - va : 0u;            // of them history
    const uint32_t ja = va > P.h ? va - P.h : 0u, jb = vb - P.h;   // call samples [ja, jb), jb <= n_in

    // ---- 1. staging ---------------------------------------------------------------------------------------------------------
    const int16_t* const rowp = P.in + (uint64_t)row * P.in_cap;
    const uintptr_t R = (uintptr_t)rowp, Rend = R + (uintptr_t)P.n_in * 2u;
    const uintptr_t a0 = R + (uintptr_t)ja * 2u, a1 = R + (uintptr_t)jb * 2u;
    const uintptr_t c_lo = a0 >> 4, c_hi = (a1 + 15u) >> 4;
    const uint32_t koff = (uint32_t)(a0 & 15u) >> 1;
    const uint32_t kc = hh + ((koff + 8u - (hh & 7u)) & 7u); // LDS index of call sample ja: kc - koff is a multiple of 8, >= 0
    const uint32_t k_lo = kc - koff;                         // LDS index of the first sample of chunk c_lo
    for (uint32_t i = tid; i < (uint32_t)(c_hi - c_lo); i += kThreads) {
        const uintptr_t ca = (c_lo + i) << 4;
        const uint32_t k = k_lo + i * 8u;
        if (ca >= R && ca + 16u <= Rend) {                   // whole inside the row's valid samples
            *reinterpret_cast<i4*>(plane + k) = *(const FMD_DDC_GLOBAL i4*)ca;
        } else {                                             // the unaligned head or tail: only what the tile needs
            for (uint32_t e = 0; e < 8u; ++e) {
                const uintptr_t a = ca + e * 2u;
                if (a < a0 || a >= a1) continue;
                plane[k + e] = *(const FMD_DDC_GLOBAL int16_t*)a;
            }
        }
    }
    {
        const FMD_DDC_GLOBAL int16_t* hin = (const FMD_DDC_GLOBAL int16_t*)(uintptr_t)(P.hist_in + ((uint64_t)row * P.hcap + va));
        for (uint32_t i = tid; i < hh; i += kThreads) plane[kc - hh + i] = hin[i];
    }

    // ---- 2. the table -------------------------------------------------------------------------------------------------------
    {
        const FMD_DDC_GLOBAL uint32_t* gt = (const FMD_DDC_GLOBAL uint32_t*)(uintptr_t)P.tab;
        for (uint32_t i = tid; i < 4u * P.npair; i += kThreads) tp[i] = gt[i];
    }

    // the row's last tile also writes the next call's history: the last h_next virtual samples
    if (t == P.ntiles - 1u) {
        const uint32_t v0 = P.h + P.n_in - P.h_next;
        const FMD_DDC_GLOBAL int16_t* hin = (const FMD_DDC_GLOBAL int16_t*)(uintptr_t)(P.hist_in + (uint64_t)row * P.hcap);
        const FMD_DDC_GLOBAL int16_t* cin = (const FMD_DDC_GLOBAL int16_t*)(uintptr_t)rowp;
        FMD_DDC_GLOBAL int16_t* hout = (FMD_DDC_GLOBAL int16_t*)(uintptr_t)(P.hist_out + (uint64_t)row * P.hcap);
        for (uint32_t i = tid; i < P.h_next; i += kThreads) {
            const uint32_t v = v0 + i;
            hout[i] = v < P.h ? hin[v] : cin[v - P.h];
        }
    }
    __syncthreads();

    // ---- 3./4. one lane per output ------------------------------------------------------------------------------------------
    if (tid >= no) return;
    const uint32_t kn = kc - hh + tid * P.D;                 // LDS index of x[i_n]
    const uint32_t sh = (kn & 1u) << 4;
    const uint32_t* const x0 = reinterpret_cast<const uint32_t*>(plane) + (kn >> 1);
    const uint4* const g = reinterpret_cast<const uint4*>(tp);
    int s0 = 0, s1 = 0, s2_ = 0, s3 = 0;
    uint32_t w = x0[0];
    for (uint32_t d = 0; d < P.npair; ++d) {
        const uint4 gd = g[d];
        const uint32_t nx = x0[d + 1u];
        const uint32_t xs = __builtin_amdgcn_alignbit(nx, w, sh);
        s0 = dot2(gd.x, xs, s0);
        s1 = dot2(gd.y, xs, s1);
        s2_ = dot2(gd.z, xs, s2_);
        s3 = dot2(gd.w, xs, s3);
        w = nx;
    }
    const int64_t A0 = s0 >> P.pre_shift, A1 = s1 >> P.pre_shift, A2 = s2_ >> P.pre_shift, A3 = s3 >> P.pre_shift;
    const int64_t v = ((A0 * A0 + A1 * A1) - (A2 * A2 + A3 * A3)) >> P.out_shift;      // each square < 2^62
    const int y = v > 32767 ? 32767 : (v < -32768 ? -32768 : (int)v);
    ((FMD_DDC_GLOBAL int16_t*)(uintptr_t)(P.out + ((uint64_t)row * P.out_cap + o0 + tid)))[0] = (int16_t)y;
}

}  // namespace fmd_af

struct fmd_afsk {
    FmdRows rows;                                         // width 1, hcap = T - 1
    void* d_tab = nullptr;                                // [npair][4] dwords
    uint32_t T = 0, D = 0, pre_shift = 0, out_shift = 0;
    uint32_t npair = 0, plane_len = 0;
};

namespace {

// outputs completed once `n` samples per row have arrived
uint64_t af_outputs(const fmd_afsk* h, uint64_t n)
{
    return n >= h->T ? (n - h->T) / h->D + 1 : 0;
}

int af_enqueue(fmd_afsk* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, hipStream_t stream)
{
    FmdRows& r = h->rows;
    if (const int rc = fmd_rows_check_call(r, d_in, n_in, in_cap, d_out)) return rc;
    const uint64_t N0 = r.core.pos, N1 = N0 + n_in;
    const uint64_t out0 = af_outputs(h, N0), out1 = af_outputs(h, N1), cnt = out1 - out0;
    if (cnt < 1) { fmd_internal_set_err("the call completes no output"); return FMD_ERR_TOO_SHORT; }
    if (cnt > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    const uint64_t ntiles = (cnt + fmd_af::kTile - 1) / fmd_af::kTile;
    if (ntiles * r.n_rows >= (1ull << 31)) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }
    fmd_af::AfLaunch P{};
    fmd_rows_fill(P, r, d_in, n_in, in_cap, d_out, out_cap);
    P.h = (uint32_t)(N0 - out0 * h->D);                   // out0 D <= N0 because D <= T; <= T - 1
    P.h_next = (uint32_t)(N1 - out1 * h->D);              // <= T - 1 and <= h + n_in
    P.n_out = (uint32_t)cnt;
    P.D = h->D; P.T = h->T; P.pre_shift = h->pre_shift; P.out_shift = h->out_shift; P.npair = h->npair;
    P.ntiles = (uint32_t)ntiles; P.plane_len = h->plane_len;
    P.tab = static_cast<const uint32_t*>(h->d_tab);
    return fmd_rows_launch(r, fmd_af::fmd_afsk_kernel, fmd_af::fmd_afsk_kernel, (uint32_t)(ntiles * r.n_rows), fmd_af::kThreads, P, stream, n_in,
                           cnt, n_out);
}

}  // namespace

extern "C" {

size_t fmd_afsk_out_cap(uint32_t D, size_t n_in)
{
    if (!D) return 0;
    return (size_t)(((uint64_t)n_in + D - 1) / D) + 1;      // outputs(N + n) - outputs(N) <= ceil(n / D) for every N
}

int fmd_afsk_new(const int16_t* table, uint32_t T, uint32_t D, uint32_t pre_shift, uint32_t out_shift, uint32_t width,
                 const fmd_device_config* dev, fmd_afsk** out)
{
    if (const int rc = fmd_rows_new_args(table, dev, out, 1)) return rc;     // (the pointers)
    if (width != 1) { fmd_internal_set_err("need width 1"); return FMD_ERR_UNSUPPORTED; }
    if (T < 2 || T > 64) { fmd_internal_set_err("need 2 <= T <= 64"); return FMD_ERR_UNSUPPORTED; }
    if (D < 1 || D > T || D > 32) { fmd_internal_set_err("need 1 <= D <= min(T, 32)"); return FMD_ERR_UNSUPPORTED; }
    if (pre_shift > 16) { fmd_internal_set_err("need pre_shift <= 16"); return FMD_ERR_UNSUPPORTED; }
    if (out_shift > 48) { fmd_internal_set_err("need out_shift <= 48"); return FMD_ERR_UNSUPPORTED; }
    for (uint32_t i = 0; i < 4 * T; ++i)
        if (table[i] > 1023 || table[i] < -1023) { fmd_internal_set_err("|table entry| > 1023"); return FMD_ERR_UNSUPPORTED; }
    if (const int rc = fmd_rows_count_arg(dev)) return rc;
    fmd_afsk* h = new (std::nothrow) fmd_afsk();
    if (!h) return FMD_ERR_NOMEM;
    h->T = T; h->D = D; h->pre_shift = pre_shift; h->out_shift = out_shift;
    h->npair = (T + 1) / 2;
    h->rows.width = 1; h->rows.n_rows = dev->n_channels; h->rows.hcap = T - 1;
    h->plane_len = ((fmd_af::kTile - 1) * D + T + fmd_af::kPlaneSlack + 7u) & ~7u;         // <= 8264 samples
    h->rows.lds = 2ull * h->plane_len + 16ull * h->npair;
    std::vector<uint32_t> gp((size_t)4 * h->npair, 0u);      // [d][q] = (tab[q][2 d], tab[q][2 d + 1]), a zero tap behind an odd T
    for (uint32_t q = 0; q < 4; ++q)
        for (uint32_t t = 0; t < T; ++t)
            gp[(size_t)(t / 2) * 4 + q] |= (uint32_t)(uint16_t)table[(size_t)q * T + t] << (16 * (t & 1u));
    fmd_ddc_add_owned(h->rows.core, h->d_tab, gp.data(), gp.size() * sizeof(uint32_t));
    return fmd_rows_device(h, dev, fmd_afsk_free, out);
}

void fmd_afsk_free(fmd_afsk* h) { fmd_rows_free(h); }
int fmd_afsk_reset(fmd_afsk* h) { return fmd_rows_reset(h); }
int fmd_afsk_check(fmd_afsk* h) { return fmd_rows_check(h); }
int fmd_afsk_outputs(const fmd_afsk* h, uint64_t* inputs, uint64_t* outputs) { return fmd_rows_outputs(h, inputs, outputs, af_outputs); }

int fmd_afsk_run_device(fmd_afsk* h, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap, size_t* n_out, void* stream)
{
    return fmd_ddc_run_device(h ? &h->rows.core : nullptr, d_in, d_out,
                              [&] { return af_enqueue(h, d_in, n_in, in_cap, d_out, out_cap, n_out, static_cast<hipStream_t>(stream)); });
}

// (a call of no samples completes no output: af_enqueue refuses it like every other such call)
int fmd_afsk_run_batch(fmd_afsk* h, const int16_t* in, size_t n_in, size_t in_cap, int16_t* out, size_t out_cap, size_t* n_out)
{
    return fmd_rows_run_batch(h, af_enqueue, in, n_in, in_cap, out, out_cap, n_out, [](size_t) { return false; });
}

int fmd_afsk_kernel_name(const fmd_afsk* h, char* name, size_t cap) { return fmd_rows_kernel_name(h, name, cap, "fmd_af::fmd_afsk_kernel"); }

}  // extern "C"
