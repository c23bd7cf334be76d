// fmd_uniform.hip -- uniform channelizer: all N equally spaced channels of a band plan (or a selection of them) of every wideband
// IQ stream, each channel's decimated complex baseband, in ONE gfx950 kernel.
//
// Definition (include/fmd.h, "uniform channelizer"; tests/uniform_ref.py): the channelizer's steps with decim = hop and the fixed
// grid inc_k = round(k 2^32 / N), over a wider domain (N <= 256 channels, T <= 2048 taps, hop <= 256):
//     z[k][m] = sum_{t < T} W[k][t] c[hop m + t],   y[k][m] = (z (cosq psi + j sinq psi)) >> (14 + shift),  psi = m hop inc_k.
// The tap matrix is the same for every stream and every frame (the window of one output) starts 16-byte aligned in the stream
// (hop % 8 == 0, whole hops per call), so this is a GEMM proper, as the scanner's (fmd_spectrum.hip):
//   rows    = channel x {zr, zi} x i8 digit (a 16-row tile holds (zr_lo, zr_hi, zi_lo, zi_hi) of 4 channels, or (zr, zi) of 8),
//   K       = the frame's 2 T bytes, padded with zero A entries to whole 64-byte chunks (up to 64 of them),
//   columns = frames, 2 hop bytes apart: consecutive frames overlap T / hop-fold.
// One workgroup = one tile of 16 G consecutive frames of ONE stream (G = 8, or 4 where 8 would not fit 64 KiB of LDS), all rows:
//   1. stage the tile's bytes, 2 (hop (16 G - 1) + T) of them, in LDS ONCE, in 1 KiB pieces: global_load_lds_dwordx4 where the
//      piece lies in the call's buffer and the stream's row is 16-byte aligned, through registers where it touches the history
//      or the row is only 4-byte aligned; and the NCO table.  The 16-byte slots of every 256-byte LDS row are permuted (slot ^
//      row, on the SOURCE side of the LDS-DMA) so that the 16 frames a B read gathers -- 2 hop bytes apart, a multiple of 256 at
//      hop 128 / 256 -- spread over the banks;
//   2. the contraction, v_mfma_i32_16x16x64_i8: a wave takes batches of R row tiles (R = 1, 2 or 4 by the row-tile count) and
//      loops over the K chunks with R x G accumulators in registers: per chunk R A fragments from L2 (1 KiB each, one chunk
//      ahead) and G B fragments from LDS (xor 0x80 -> s8) feed R G MFMAs.  So one fetched A fragment serves G = 8 (4) MFMAs --
//      all the tile's column groups -- and is fetched by ONE wave of the block; one B fragment read serves R;
//   3. epilogue, lane-local (lane (j, q) holds rows 4 q ... 4 q + 3 of column j): digits recombined, centring constants, rotation
//      by the NCO (table in LDS, i64 products), shift, packed re | im << 16;
//   4. stores straight from the 16-column layout: the 16 lanes of one q hold 16 consecutive outputs of one channel, so every
//      store instruction writes whole 64-byte pieces of 4 channels' rows.  Not through LDS rows as the channelizer: a wave owns
//      its channels' rows over the whole tile, so no other wave contributes to a piece, and N x 16 G dwords (128 KiB at N = 256)
//      would not fit beside the staged bytes.
//   The stream's last tile also writes the next call's history (double-buffered, FmdDdcCore).
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_ddc.h"
#include "fmd_internal.h"

namespace fmd_uv {

using fmd_ddc::kThreads;
using fmd_ddc::kTableBytes;
using fmd_ddc::i4;
constexpr uint32_t kWaves = kThreads / 64;

struct UvLaunch {
    const uint8_t* iq;         // [S][nbytes]
    uint64_t nbytes;
    const uint8_t* hist_in;    // [S][HB]: the last HB / 2 samples before the call
    uint8_t* hist_out;
    uint32_t HB;               // history bytes per stream: 2 hop (ceil(T / hop) - 1)
    uint32_t vb_first;         // virtual byte (history ++ call) of the frame of the call's first output: a multiple of 16
    uint32_t m0_lo;            // global index of the call's first output, mod 2^32
    uint32_t M;                // outputs of this call per (stream, channel)
    uint32_t D, T, K, S, shift;     // D: the hop; K: selected channels (tap rows)
    uint32_t nrt, nkc, digits;
    uint32_t ntiles, raw_bytes;
    const uint32_t* amat;      // [nrt][nkc][64][4]
    const int32_t* kconst;     // [K][2]
    const uint32_t* dinc;      // [K]: hop inc_k
    const uint32_t* tab;       // NCO table, 512 dwords
    uint32_t* out;             // [S][K][out_stride] packed (yr, yi)
    uint64_t out_stride;
};

// LDS slot (16 bytes) of chunk c and back: the low 4 bits -- the slot inside the 256-byte row -- xor the row's low 4 bits
__device__ __forceinline__ uint32_t swz(uint32_t c) { return c ^ ((c >> 4) & 15u); }

template <int R, int G>
__global__ void __launch_bounds__(kThreads) fmd_uniform_kernel(const UvLaunch L)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    constexpr uint32_t kTile = 16u * G;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t s = blockIdx.y, t = blockIdx.x;
    if (s >= L.S || t >= L.ntiles) return;

    const uint32_t o0 = t * kTile;                           // first output (of this call) of the tile
    const uint32_t no = L.M - o0 < kTile ? L.M - o0 : kTile;
    const uint32_t vb = L.vb_first + 2u * L.D * o0;          // virtual byte of output o0's frame (16-byte aligned)
    const uint32_t nq = (2u * L.D * (no - 1u) + 2u * L.T + 15u) >> 4;
    const uint32_t nq16 = (nq + 15u) & ~15u;                 // whole 256-byte rows (<= raw_bytes / 16: host plan)
    int16_t* const tab = reinterpret_cast<int16_t*>(lds + (L.raw_bytes >> 2));

    // ---- 1. staging: slot i of LDS holds chunk swz(i) ---------------------------------------------------------------------------
    {
        const uint8_t* const row = L.iq + (uint64_t)s * L.nbytes;
        const bool aligned = ((uintptr_t)row & 15u) == 0u;
        i4* const lq = reinterpret_cast<i4*>(lds);
        for (uint32_t p = wave; 64u * p < nq16; p += kWaves) {
            const uint32_t slot = 64u * p + lane, c = swz(slot);
            const uint32_t v0 = vb + 1024u * p;              // the piece's first virtual byte
            const bool dma = aligned && 64u * p + 64u <= nq16 && v0 >= L.HB && (uint64_t)(v0 - L.HB) + 1024ull <= L.nbytes;
            if (dma) {                                       // (vb alone may lie in the history: subtract HB from the chunk's byte, >= v0)
                fmd_ddc::dma16(row + (vb + 16u * c - L.HB), reinterpret_cast<unsigned char*>(lds) + 1024u * p);
            } else if (slot < nq16) {
                const uint32_t v = vb + 16u * c;
                lq[slot] = i4{(int)fmd_ddc::virt_dword(L, s, v), (int)fmd_ddc::virt_dword(L, s, v + 4u),
                              (int)fmd_ddc::virt_dword(L, s, v + 8u), (int)fmd_ddc::virt_dword(L, s, v + 12u)};
            }
        }
        typedef const FMD_DDC_GLOBAL uint32_t* gw;
        uint32_t* const tw = reinterpret_cast<uint32_t*>(tab);
        for (uint32_t i = tid; i < kTableBytes / 4u; i += kThreads) tw[i] = ((gw)(uintptr_t)L.tab)[i];
    }
    if (t == L.ntiles - 1u) fmd_ddc::write_history(L, s, tid);   // the stream's last tile also writes the next call's history
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0): the LDS-DMAs have landed
    __syncthreads();

    // ---- 2. contraction: batches of R row tiles x all G column groups, looping over the K chunks --------------------------------
    const uint8_t* const lb = reinterpret_cast<const uint8_t*>(lds);
    const uint32_t j = lane & 15u, q = lane >> 4;
    const uint32_t hc = L.D >> 3;                            // 16-byte chunks per hop
    typedef const FMD_DDC_GLOBAL i4* gq;
    const gq amat = (gq)(uintptr_t)L.amat + lane;
    const uint32_t sh = 14u + L.shift;
    const uint32_t nb = (L.nrt + R - 1u) / R;
    typedef FMD_DDC_GLOBAL uint32_t* gwo;
    gwo const out = (gwo)(uintptr_t)(L.out + (uint64_t)s * L.K * L.out_stride + o0);
    const uint32_t m0 = L.m0_lo + o0;

    for (uint32_t b = wave; b < nb; b += kWaves) {
        const uint32_t rt0 = b * R;
        const uint32_t rn = L.nrt - rt0 < (uint32_t)R ? L.nrt - rt0 : (uint32_t)R;   // wave-uniform
        i4 acc[R][G], A[R], An[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int g = 0; g < G; ++g) acc[r][g] = i4{0, 0, 0, 0};
            An[r] = i4{0, 0, 0, 0};
            if ((uint32_t)r < rn) An[r] = amat[((rt0 + r) * L.nkc) * 64u];
        }
        for (uint32_t kc = 0; kc < L.nkc; ++kc) {
#pragma unroll
            for (int r = 0; r < R; ++r) A[r] = An[r];
            if (kc + 1u < L.nkc) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if ((uint32_t)r < rn) An[r] = amat[((rt0 + r) * L.nkc + kc + 1u) * 64u];
            }
            i4 B[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const uint32_t c = hc * (16u * g + j) + 4u * kc + q;
                B[g] = *reinterpret_cast<const i4*>(lb + 16u * swz(c)) ^ (int)0x80808080;   // u8 -> s8
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if ((uint32_t)r < rn) {
#pragma unroll
                    for (int g = 0; g < G; ++g) acc[r][g] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[r], B[g], acc[r][g], 0, 0, 0);
                }
            }
        }
        // ---- 3./4. epilogue and stores: two digits -> (zr_lo, zr_hi, zi_lo, zi_hi) of row 4 rt + q; one -> (zr, zi) of rows
        // 8 rt + 2 q and 8 rt + 2 q + 1
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if ((uint32_t)r >= rn) continue;
            const uint32_t rt = rt0 + r;
            const uint32_t ka = L.digits == 2u ? 4u * rt + q : 8u * rt + 2u * q;
            const bool has0 = ka < L.K, has1 = L.digits == 1u && ka + 1u < L.K;
            int c0r = 0, c0i = 0, c1r = 0, c1i = 0;
            uint32_t i0 = 0u, i1 = 0u;
            if (has0) { c0r = L.kconst[2u * ka]; c0i = L.kconst[2u * ka + 1u]; i0 = L.dinc[ka]; }
            if (has1) { c1r = L.kconst[2u * ka + 2u]; c1i = L.kconst[2u * ka + 3u]; i1 = L.dinc[ka + 1u]; }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const uint32_t o = 16u * g + j;                // output o of the tile
                if (o >= no) continue;
                const uint32_t m = m0 + o;
                if (has0) {
                    if (L.digits == 2u) {
                        const int zr = (int)((uint32_t)acc[r][g].x + ((uint32_t)acc[r][g].y << 7)) + c0r;
                        const int zi = (int)((uint32_t)acc[r][g].z + ((uint32_t)acc[r][g].w << 7)) + c0i;
                        out[(uint64_t)ka * L.out_stride + o] = fmd_ddc::rotate(tab, zr, zi, m * i0, sh);
                    } else {
                        out[(uint64_t)ka * L.out_stride + o] = fmd_ddc::rotate(tab, acc[r][g].x + c0r, acc[r][g].y + c0i, m * i0, sh);
                    }
                }
                if (has1) out[(uint64_t)(ka + 1u) * L.out_stride + o] = fmd_ddc::rotate(tab, acc[r][g].z + c1r, acc[r][g].w + c1i, m * i1, sh);
            }
        }
    }
}

}  // namespace fmd_uv

struct fmd_uniform {
    FmdDdcBank bank;                                      // T, D = hop, K = selected channels, S, shift, HB, plan, core
    uint32_t N = 0;
    uint32_t R = 1, G = 8, raw_bytes = 0;                 // row tiles per batch, column groups per tile, staged bytes of a tile
    size_t lds = 0;
};

namespace {

bool uv_inc(uint32_t k, uint32_t N, uint32_t* inc)
{
    if (N < 2 || N > 256 || k >= N) return false;
    *inc = (uint32_t)(((((uint64_t)k << 33) / N) + 1ull) >> 1);
    return true;
}

// staged bytes of a tile of 16 G frames: what the B reads touch, in whole 256-byte rows (the slot permutation stays inside a row)
uint32_t uv_raw_bytes(uint32_t hop, uint32_t nkc, uint32_t G) { return (2u * hop * (16u * G - 1u) + 64u * nkc + 255u) & ~255u; }

template <int R, int G>
void uv_launch_rg(const fmd_uv::UvLaunch& L, size_t lds, hipStream_t stream)
{
    hipLaunchKernelGGL((fmd_uv::fmd_uniform_kernel<R, G>), dim3(L.ntiles, L.S), dim3(fmd_uv::kThreads), lds, stream, L);
}

template <int G>
void uv_launch_g(uint32_t R, const fmd_uv::UvLaunch& L, size_t lds, hipStream_t stream)
{
    if (R == 1) uv_launch_rg<1, G>(L, lds, stream);
    else if (R == 2) uv_launch_rg<2, G>(L, lds, stream);
    else uv_launch_rg<4, G>(L, lds, stream);
}

int uv_enqueue(fmd_uniform* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, hipStream_t stream)
{
    const FmdDdcBank& b = h->bank;
    FmdDdcCore& c = h->bank.core;
    if (nbytes % (2ull * b.D) != 0) { fmd_internal_set_err("nbytes % (2 hop) != 0"); return FMD_ERR_BAD_LENGTH; }
    if (const int rc = fmd_ddc_check_call(nbytes, d_iq, d_out, 4u)) return rc;
    const uint64_t ns = nbytes / 2;
    const uint64_t m0 = fmd_ddc_outputs(b.T, b.D, c.pos), M = fmd_ddc_outputs(b.T, b.D, c.pos + ns) - m0;
    if (M < 1) { fmd_internal_set_err("the call completes no filter output"); return FMD_ERR_TOO_SHORT; }
    if (M > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    const uint32_t tile = 16u * h->G;
    const uint64_t ntiles = (M + tile - 1) / tile;
    fmd_uv::UvLaunch L{};
    fmd_ddc_fill_front(L, b, d_iq, nbytes, m0);              // (every frame of the call starts at most HB / 2 samples back)
    L.m0_lo = (uint32_t)m0; L.M = (uint32_t)M;
    L.ntiles = (uint32_t)ntiles; L.raw_bytes = h->raw_bytes;
    L.out = static_cast<uint32_t*>(d_out); L.out_stride = out_cap;
    FMD_DDC_TRY(c.order.before(stream));
    if (h->G == 8) uv_launch_g<8>(h->R, L, h->lds, stream);
    else uv_launch_g<4>(h->R, L, h->lds, stream);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(c, stream, ns);
    if (out_len) *out_len = (size_t)M;
    return FMD_OK;
}

}  // namespace

// ---- the constructor's steps (fmd_ddc.h): fmd_uniform_new is fmd_uniform_host, then fmd_uniform_device ------------------------

int fmd_uniform_args(const int16_t* taps, uint32_t n_taps, uint32_t n_channels, uint32_t hop, uint32_t shift, const uint32_t* channels,
                     uint32_t n_selected, const fmd_device_config* dev)
{
    if (n_channels < 2 || n_channels > 256 || hop < 8 || hop > 256 || hop % 8 != 0 || n_taps == 0 || n_taps > 2048 || shift > 24 ||
        dev->n_channels > 65535u) {
        fmd_internal_set_err("need 2 <= n_channels <= 256, hop a multiple of 8 in 8 ... 256, 1 <= n_taps <= 2048, shift <= 24, n_streams <= 65535");
        return FMD_ERR_UNSUPPORTED;
    }
    for (uint32_t t = 0; t < n_taps; ++t)
        if (taps[t] > 2047 || taps[t] < -2047) { fmd_internal_set_err("|tap| > 2047"); return FMD_ERR_UNSUPPORTED; }
    if (!channels) n_selected = n_channels;
    if (n_selected == 0 || n_selected > n_channels) { fmd_internal_set_err("need 1 <= n_selected <= n_channels"); return FMD_ERR_UNSUPPORTED; }
    for (uint32_t i = 0; i < n_selected; ++i) {
        const uint32_t k = channels ? channels[i] : i;
        if (k >= n_channels || (channels && i > 0 && k <= channels[i - 1])) {
            fmd_internal_set_err("channels must be strictly increasing and < n_channels");
            return FMD_ERR_UNSUPPORTED;
        }
    }
    return FMD_OK;
}

int fmd_uniform_host(const int16_t* taps, uint32_t n_taps, uint32_t n_channels, uint32_t hop, uint32_t shift, const uint32_t* channels,
                     uint32_t n_selected, const fmd_device_config* dev, fmd_uniform** out, uint64_t* bound)
{
    if (const int rc = fmd_uniform_args(taps, n_taps, n_channels, hop, shift, channels, n_selected, dev)) return rc;
    if (!channels) n_selected = n_channels;
    std::vector<uint32_t> inc(n_selected), dinc(n_selected);
    for (uint32_t i = 0; i < n_selected; ++i) {
        uv_inc(channels ? channels[i] : i, n_channels, &inc[i]);
        dinc[i] = hop * inc[i];
    }
    fmd_uniform* h = new (std::nothrow) fmd_uniform();
    if (!h) return FMD_ERR_NOMEM;
    FmdDdcBank& b = h->bank;
    h->N = n_channels;
    b.T = n_taps; b.D = hop; b.K = n_selected; b.S = dev->n_channels; b.shift = shift;
    b.HB = 2u * hop * ((n_taps + hop - 1u) / hop - 1u);
    // one plan for all streams: every frame starts 16-byte aligned (one delta, no slack in K)
    fmd_ddc_build_plan(taps, n_taps, inc.data(), 1u, n_selected, 1u, (2u * n_taps + 63u) / 64u, b.plan);
    b.plan.dinc = dinc;
    *bound = (256ull * b.plan.max_gain + ((1ull << shift) - 1ull)) >> shift;
    if (*bound > 16384ull) {
        fmd_internal_set_err("filter gain too large: need ceil(256 * max sum(|Wr| + |Wi|) / 2^shift) <= 16384");
        delete h;
        return FMD_ERR_UNSUPPORTED;
    }
    h->R = b.plan.nrt > 8u ? 4u : (b.plan.nrt > 4u ? 2u : 1u);
    h->G = (size_t)uv_raw_bytes(hop, b.plan.nkc, 8u) + fmd_uv::kTableBytes <= 65536u ? 8u : 4u;
    h->raw_bytes = uv_raw_bytes(hop, b.plan.nkc, h->G);
    h->lds = (size_t)h->raw_bytes + fmd_uv::kTableBytes;
    *out = h;
    return FMD_OK;
}

void fmd_uniform_discard(fmd_uniform* h) { delete h; }

int fmd_uniform_device(fmd_uniform* h, const fmd_device_config* dev)
{
    const char* what;
    if (const int rc = fmd_ddc_bank_device(h->bank, dev, &what)) {
        if (!what) { delete h; return rc; }
        fmd_internal_set_err(what); fmd_uniform_free(h); return rc;
    }
    std::vector<uint32_t>().swap(h->bank.plan.amat);      // (up to 4 MiB; the device holds it now)
    return FMD_OK;
}

extern "C" {

int fmd_uniform_channel_inc(uint32_t channel, uint32_t n_channels, uint32_t* inc)
{
    if (!inc) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (!uv_inc(channel, n_channels, inc)) { fmd_internal_set_err("need 2 <= n_channels <= 256 and channel < n_channels"); return FMD_ERR_UNSUPPORTED; }
    return FMD_OK;
}

size_t fmd_uniform_out_cap(uint32_t hop, size_t nbytes)
{
    if (!hop) return 0;
    return nbytes / (2ull * hop);
}

int fmd_uniform_new(const int16_t* taps, uint32_t n_taps, uint32_t n_channels, uint32_t hop, uint32_t shift, const uint32_t* channels,
                    uint32_t n_selected, const fmd_device_config* dev, fmd_uniform** out)
{
    if (!taps || !dev || !out || dev->n_channels == 0) { fmd_internal_set_err("null / empty argument"); return FMD_ERR_INVALID_ARG; }
    *out = nullptr;
    uint64_t bound;
    if (const int rc = fmd_uniform_host(taps, n_taps, n_channels, hop, shift, channels, n_selected, dev, out, &bound)) return rc;
    if (const int rc = fmd_uniform_device(*out, dev)) { *out = nullptr; return rc; }
    return FMD_OK;
}

void fmd_uniform_free(fmd_uniform* h)
{
    if (!h) return;
    fmd_ddc_free(h->bank.core);
    delete h;
}

int fmd_uniform_reset(fmd_uniform* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_reset(h->bank.core);
}

int fmd_uniform_run_device(fmd_uniform* h, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* out_len, void* stream)
{
    return fmd_ddc_run_device(h ? &h->bank.core : nullptr, d_iq, d_out,
                              [&] { return uv_enqueue(h, d_iq, nbytes, d_out, out_cap, out_len, static_cast<hipStream_t>(stream)); });
}

int fmd_uniform_check(fmd_uniform* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_check(h->bank.core);
}

int fmd_uniform_run_batch(fmd_uniform* h, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!h || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (nbytes % (2ull * h->bank.D) != 0) { fmd_internal_set_err("nbytes % (2 hop) != 0"); return FMD_ERR_BAD_LENGTH; }
    const size_t out_bytes = out_cap * h->bank.S * h->bank.K * sizeof(uint32_t);   // (yr, yi) pairs
    return fmd_ddc_run_batch(h->bank, iq, nbytes, out, out_bytes, out_cap, out_len, [h](auto... a) { return uv_enqueue(h, a...); });
}

int fmd_uniform_outputs(const fmd_uniform* h, uint64_t* outputs)
{
    if (!h || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *outputs = fmd_ddc_outputs(h->bank.T, h->bank.D, h->bank.core.pos);
    return FMD_OK;
}

int fmd_uniform_tap_digits(const fmd_uniform* h)
{
    if (!h) return FMD_ERR_INVALID_ARG;
    return (int)h->bank.plan.digits;
}

int fmd_uniform_kernel_name(const fmd_uniform* h, char* name, size_t cap)
{
    if (!h || !name || cap == 0) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, "fmd_uv::fmd_uniform_kernel<%u, %u>", h->R, h->G), cap);
}

}  // extern "C"
