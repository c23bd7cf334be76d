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
//      {zr, zi} x i8 digit, fmd_ddc.h), B = window bytes (xor 0x80 -> s8), one column per filter output.  A window
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
#include <cstdlib>
#include <new>

#include "fmd_ddc.h"
#include "fmd_device.h"
#include "fmd_internal.h"
#include "fmd_kernels.h"

namespace fmd_st {

using namespace fmd_dev;
using fmd_ddc::kThreads;
using fmd_ddc::kTableBytes;

constexpr uint32_t kMaxOutputs = 4u * 16u * fmd_ddc::kGroups;   // 4 waves x 4 groups x 16 columns = 256 outputs per tile

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
    fmd_ddc::stage(L, s, base, nq, lds, tab, tid, wave);
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0): the LDS-DMAs have landed
    __syncthreads();

    // ---- 2./3. contraction on the matrix cores, rotation, packing -----------------------------------------------------------
    fmd_ddc::contract(L, s, wave, lane, d0, no, L.m0_lo + o0, lds, tab, ypk, L.lp_cap, o0 - (uint32_t)jfirst);
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
    if (T.last) fmd_ddc::write_history(L, s, tid);
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

}  // namespace fmd_st

struct fmd_stations {
    FmdDdcBank bank;
    uint32_t lp_bound = 0;                                // ceil(256 max_gain / 2^shift): the largest |y| component
    FmdDdcPair state;                                     // [S * K] FmdChanState
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
};

namespace {

using fmd_st::kMaxOutputs;
using fmd_ddc::kTableBytes;

// LDS of a tile of `kt` audio samples: raw bytes the matrix phase may read + NCO table + packed outputs + group table
bool st_sizes(const fmd_stations* b, uint32_t kt, uint32_t* lp_cap, uint32_t* raw_bytes, size_t* lds)
{
    FmdRates r = b->r; r.kt = kt;
    const uint32_t cap = fmd_tile_lp_cap(r);
    if (cap > kMaxOutputs) return false;
    const uint32_t groups = ((cap + 3u) / 4u + 15u) / 16u;           // 16-column groups of a wave
    const uint32_t raw = fmd_ddc_raw_bytes(b->bank.D, b->bank.plan.nkc, b->bank.T, groups, cap);
    const uint64_t total = raw + kTableBytes + 4ull * b->bank.K * cap + 8ull * (kt + 2);
    if (total > 64 * 1024) return false;
    *lp_cap = cap; *raw_bytes = raw; *lds = (size_t)total;
    return true;
}

int st_enqueue(fmd_stations* b, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap, size_t* n_each, hipStream_t stream)
{
    if (nbytes % 8 != 0) { fmd_internal_set_err("nbytes % 8 != 0 (simple_fm.rs:286 would panic)"); return FMD_ERR_BAD_LENGTH; }
    if (nbytes == 0) { fmd_internal_set_err("nbytes out of range"); return FMD_ERR_UNSUPPORTED; }
    if (const int rc = fmd_ddc_check_call(nbytes, d_iq, d_out, 2u)) return rc;
    const FmdDdcBank& bk = b->bank;
    FmdDdcCore& c = b->bank.core;
    const uint64_t ns = nbytes / 2;
    const uint64_t m0 = fmd_ddc_outputs(bk.T, bk.D, c.pos), Mdec = fmd_ddc_outputs(bk.T, bk.D, c.pos + ns) - m0;
    if (Mdec < 2) { fmd_internal_set_err("the call yields fewer than 2 filter outputs (simple_fm.rs:356 asserts > 1)"); return FMD_ERR_TOO_SHORT; }
    const FmdRates r = b->r;
    if (!fmd_ranges_fit32(r, Mdec * r.D)) { fmd_internal_set_err("call exceeds the 32-bit index range for these rates"); return FMD_ERR_UNSUPPORTED; }
    fmd_st::StLaunch L{};
    L.P = fmd_make_plan(r, 0u, b->i0r, 0u);
    L.P.M = (uint32_t)Mdec;
    L.P.K = fmd_num_audio(r, b->i0r, L.P.M);
    L.P.nt = fmd_num_tiles(r, L.P.K);
    if (L.P.K > out_cap) { fmd_internal_set_err("out_cap too small"); return FMD_ERR_CAPACITY; }
    if (L.P.nt > (1u << 30) || bk.S > 65535u) { fmd_internal_set_err("call too large for the grid"); return FMD_ERR_UNSUPPORTED; }
    fmd_ddc_fill_front(L, bk, d_iq, nbytes, m0);
    L.m0_lo = (uint32_t)m0;
    L.r = r; L.tl = fmd_make_tiling(r);
    L.fa = r.fr / r.sr; L.fb = r.fr % r.sr;
    L.sr_shift = 32u;
    if ((r.sr & (r.sr - 1u)) == 0u) { L.sr_shift = 0u; while ((1u << L.sr_shift) < r.sr) ++L.sr_shift; }
    L.inv_sr = 1.0f / (float)r.sr; L.inv_R = 1.0f / (float)r.R;
    L.lp_cap = b->lp_cap; L.raw_bytes = b->raw_bytes;
    L.f32_disc = b->lp_bound <= 2048u ? 1u : 0u;
    L.st_in = b->state.in<FmdChanState>(c.cur); L.st_out = b->state.out<FmdChanState>(c.cur);
    L.out = static_cast<int16_t*>(d_out); L.out_stride = out_cap;
    L.exc = b->d_exc; L.f64_guard = b->f64_guard; L.seq = b->seq + 1; L.f64_skew = b->f64_skew;
    FMD_DDC_TRY(c.order.before(stream));
    hipLaunchKernelGGL(fmd_st::fmd_stations_kernel, dim3(L.P.nt, bk.S), dim3(fmd_st::kThreads), b->lds, stream, L);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(c, stream, ns);
    b->seq += 1;
    b->i0r = fmd_next_lpr_index_r(r, b->i0r, L.P.M, L.P.K);
    if (n_each) *n_each = L.P.K;
    return FMD_OK;
}

int st_settle(fmd_stations* b, int16_t* host_out, size_t host_cap)
{
    return fmd_internal_resolve_exc(b->d_exc, b->r.R, b->seq, b->seq, b->state.in<FmdChanState>(b->bank.core.cur), host_out, host_cap, &b->f64_guarded,
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
    if (const int rc = fmd_ddc_front_args(taps, n_taps, decim, shift, n_stations, dev)) return rc;
    if (rate_resample == 0 || rate_out < rate_resample) {
        fmd_internal_set_err("need rate_out >= rate_resample >= 1 (simple_fm.rs:421 divides by rate_out / rate_resample)");
        return FMD_ERR_BAD_RATES;
    }
    fmd_stations* b = new (std::nothrow) fmd_stations();
    if (!b) return FMD_ERR_NOMEM;
    uint64_t bound;                                          // must stay in the discriminator's range
    if (const int rc = fmd_ddc_bank_front(b->bank, taps, n_taps, decim, shift, phase_inc, n_stations, dev, &bound)) { delete b; return rc; }
    b->lp_bound = (uint32_t)bound;
    FmdRates& r = b->r;
    r.D = decim; r.fast = rate_out; r.slow = rate_resample;
    r.g = fmd_gcd(r.fast, r.slow); r.fr = r.fast / r.g; r.sr = r.slow / r.g;
    r.R = (int32_t)(r.fast / r.slow);
    const uint64_t fa = r.fr / r.sr;
    if (r.fr > FMD_MAX_RATE_REDUCED || (fa + 2) * 32768ull >= (1u << 24) || (uint32_t)r.R >= (1u << 24)) {
        delete b; fmd_internal_set_err("rate ratio outside the exact-small-divide range"); return FMD_ERR_UNSUPPORTED;
    }
    const size_t budget = (size_t)fmd_knob_u32("FMD_ST_LDS", (uint32_t)fmd_ddc::kLdsBudget);
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
    if (const char* g = fmd_knob("FMD_F64_GUARD_LOG2")) b->f64_guard = ldexp(1.0, atoi(g));   // experiment build only
    b->f64_skew = fmd_knob_i32("FMD_F64_SKEW", 0);

    fmd_ddc_add_pair(b->bank.core, b->state, (size_t)n_stations * dev->n_channels * sizeof(FmdChanState));
    const char* what;
    if (const int rc = fmd_ddc_bank_device(b->bank, dev, &what)) {
        if (!what) { delete b; return rc; }
        fmd_internal_set_err(what); fmd_stations_free(b); return rc;
    }
    auto fail = [&](const char* w) { fmd_internal_set_err(w); fmd_stations_free(b); return FMD_ERR_HIP; };
    FmdDeviceGuard guard(b->bank.core.device);
    if (guard.error() != hipSuccess) return fail("hipSetDevice");
    if (hipMalloc(&b->d_exc, sizeof(FmdExcBuf)) != hipSuccess || hipMemset(b->d_exc, 0, sizeof(FmdExcBuf)) != hipSuccess) return fail("hipMalloc(reports)");
    if (hipHostMalloc(reinterpret_cast<void**>(&b->h_head), 16, hipHostMallocDefault) != hipSuccess) return fail("hipHostMalloc(report head)");
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    *out = b;
    return FMD_OK;
}

void fmd_stations_free(fmd_stations* b)
{
    if (!b) return;
    FmdDeviceGuard guard(b->bank.core.device);
    fmd_ddc_release(b->bank.core);
    if (b->d_exc) (void)hipFree(b->d_exc);
    if (b->h_head) (void)hipHostFree(b->h_head);
    delete b;
}

int fmd_stations_reset(fmd_stations* b)
{
    if (!b) return FMD_ERR_INVALID_ARG;
    FMD_DDC_ON_DEVICE(b->bank.core.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    FMD_DDC_TRY(hipMemset(b->d_exc, 0, 16));
    FMD_DDC_TRY(fmd_ddc_zero_history(b->bank.core));     // (the state too; ends with the device synchronised)
    b->i0r = 0;
    return FMD_OK;
}

int fmd_stations_demodulate_device(fmd_stations* b, const void* d_iq, size_t nbytes, void* d_out, size_t out_cap,
                                   size_t* out_len_each, void* stream)
{
    return fmd_ddc_run_device(b ? &b->bank.core : nullptr, d_iq, d_out,
                              [&] { return st_enqueue(b, d_iq, nbytes, d_out, out_cap, out_len_each, static_cast<hipStream_t>(stream)); });
}

int fmd_stations_check(fmd_stations* b)
{
    if (!b) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(b->bank.core.device);
    const FmdStreamOrder& order = b->bank.core.order;
    if (order.have_last && b->h_head) {                      // one stream synchronisation in the common case (see fmd_demod_check)
        b->h_head[0] = b->h_head[1] = ~0u;
        hipError_t e = hipMemcpyAsync(b->h_head, b->d_exc, 16, hipMemcpyDeviceToHost, order.last);
        if (e == hipSuccess) e = hipStreamSynchronize(order.last);
        if (e == hipSuccess && b->h_head[0] == 0u && b->h_head[1] == 0u) return FMD_OK;
        if (e != hipSuccess) (void)hipGetLastError();
    }
    FMD_DDC_TRY(hipDeviceSynchronize());
    return st_settle(b, nullptr, 0);
}

int fmd_stations_demodulate_batch(fmd_stations* b, const uint8_t* iq, size_t nbytes, int16_t* out, size_t out_cap, size_t* out_len)
{
    if (!b || !iq || !out || !out_len) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FmdDdcCore& c = b->bank.core;
    FMD_DDC_ON_DEVICE(c.device);
    const size_t rows = (size_t)b->bank.S * b->bank.K, out_bytes = out_cap * rows * sizeof(int16_t);
    size_t n = 0;
    // (a refused call returns without waiting for the stream)
    if (const int rc = fmd_ddc_batch_enqueue(b->bank, iq, nbytes, out_bytes, out_cap, &n, [b](auto... a) { return st_enqueue(b, a...); })) return rc;
    if (n) FMD_DDC_TRY(hipMemcpyAsync(out, c.d_out, out_bytes, hipMemcpyDeviceToHost, c.stream));
    FMD_DDC_TRY(hipStreamSynchronize(c.stream));
    for (size_t row = 0; row < rows; ++row) out_len[row] = n;
    return st_settle(b, out, out_cap);
}

int fmd_stations_get_state(fmd_stations* b, uint32_t stream, uint32_t station, fmd_demod_state* state)
{
    if (!b || !state || stream >= b->bank.S || station >= b->bank.K) { fmd_internal_set_err("bad argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(b->bank.core.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    int rc = st_settle(b, nullptr, 0);
    if (rc) return rc;
    FmdChanState s;
    FMD_DDC_TRY(hipMemcpy(&s, b->state.in<FmdChanState>(b->bank.core.cur) + ((size_t)stream * b->bank.K + station), sizeof(s), hipMemcpyDeviceToHost));
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
    return fmd_ddc_name_rc(snprintf(name, cap, "fmd_st::fmd_stations_kernel"), cap);
}

}  // extern "C"
