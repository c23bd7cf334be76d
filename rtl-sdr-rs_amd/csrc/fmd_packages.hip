// fmd_packages.hip -- the package bank: the pulse records of many streams sliced into PWM / PPM bit packages on the device.
//
// Definition: include/fmd.h, "Package bank"; tests/packages_ref.py -- per stream an fmd_pulse_slicer (fmd_pulse_slice.cpp) that is
// pushed the call's first min(count, rec_cap) records, is given idle(state, run) and has room for every package.
//
// One wave per stream, four streams per workgroup (no barrier, no LDS: the waves share nothing).  The records are read 64 at a time,
// lane l the 16 bytes of record l of the chunk.  Everything a record decides is a ballot:
//   F     the record opens a package: gap >= reset, or lane 0 of a call that finds no package open;
//   BADM  the record fits neither window;  VAL  its bit;  G  it gives a bit: it fits, and no bad record stands between the last set
//         bit of F at or below it and itself (for the lanes below F's first bit: and the carried package is not BAD).
// A segment -- the lanes from one set bit of F to the next -- is one package.  Its bits are one contiguous run of G, so they are one
// extraction from VAL, bit-reversed for MSB first.  The lane that opens a segment owns it: it forms the whole package from the masks
// (at most 64 bits, never truncated) and, when another set bit of F follows, stores it as seven 8-byte pieces at its rank among
// the call's delivered packages -- the popcount of the delivered closes below it.  Only two segments touch the carried package:
// the lanes below F's first bit extend it (n_pulses, the bits appended at n_bits, BAD, TRUNCATED beyond 256) and that bit closes it;
// the segment of F's last bit becomes the new carry.  The carry lives in wave-uniform values and, for the 256 bits, in lanes 4 ...
// 11 as big-endian words -- lane i holds dword i of the package, so a close is one dword store of lanes 0 ... 13.  After the last
// chunk the idle test may close the carry; then the count, the totals and the carry are written.  Nothing depends on scheduling.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_rows.h"

namespace fmd_pk {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;                // streams per workgroup
constexpr uint32_t kState = 24;                           // dwords per stream: the open package (14, `rsv` holding open), 0, 0,
                                                          // records, packages, skipped, bad (u64 each)
constexpr uint32_t kPkg = 14;                             // dwords of a package
constexpr uint32_t kMaxBits = 256;

typedef int i4 __attribute__((ext_vector_type(4)));

struct PackagesLaunch {
    const uint32_t* cnt_in;    // [n_streams]; unread when flush
    const uint8_t* rec_in;     // [n_streams][rec_cap] fmd_pulses_rec
    const uint32_t* tot_in;    // [n_streams][tot_stride] dwords: samples (u64) at 0, the state at off_state, the run (u64) at off_run
    uint32_t rec_cap, n_streams;
    uint32_t tot_stride, off_state, off_run;
    uint32_t n_samples;        // of the call that left the records
    uint32_t flush;            // no records, and the idle test passes
    uint32_t modulation, short_w, long_w, tol, reset, min_bits, pkg_cap;
    const uint32_t* st_in;     // [n_streams][kState]
    uint32_t* st_out;
    uint32_t* cnt_out;         // [n_streams]
    uint8_t* pkg_out;          // [n_streams][pkg_cap] fmd_pulse_package
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t lane_of(uint32_t v, uint32_t from) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)from); }
__device__ __forceinline__ uint64_t below(uint32_t l) { return l >= 64u ? ~0ull : (1ull << l) - 1ull; }    // the lanes under l
__device__ __forceinline__ bool near(uint32_t v, uint32_t centre, uint32_t tol) { return (v > centre ? v - centre : centre - v) <= tol; }
__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b) { const uint64_t v = (uint64_t)a + b; return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// Big-endian word w of a bit string that has X (its first bit at bit 63, zeros behind its last) at bit p: bit k of the word is bit
// 32 w + k - p of X.
__device__ __forceinline__ uint32_t word_of(uint64_t X, uint32_t w, uint32_t p)
{
    const int d = (int)(32u * w) - (int)p;
    if (d >= 0) return d < 64 ? (uint32_t)((X << d) >> 32) : 0u;
    return d > -32 ? (uint32_t)((X >> -d) >> 32) : 0u;
}

__global__ void __launch_bounds__(kThreads) fmd_packages_kernel(const PackagesLaunch L)
{
    typedef const FMD_DDC_GLOBAL uint32_t* gw;
    typedef FMD_DDC_GLOBAL uint32_t* gwo;
    typedef FMD_DDC_GLOBAL uint64_t* gdo;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * kWaves + uni(threadIdx.x >> 6);
    if (s >= L.n_streams) return;                            // (wave-uniform; the kernel has no barrier)

    const gw si = (gw)(uintptr_t)(L.st_in + (uint64_t)s * kState);
    const gw ti = (gw)(uintptr_t)(L.tot_in + (uint64_t)s * L.tot_stride);
    // the carried package: wave-uniform but for its bits, whose big-endian word w stands in lane 4 + w
    uint32_t open = uni(si[13]) & 1u, np = uni(si[2]), nb = uni(si[3]), flags = uni(si[12]);
    uint64_t start = uni(si[0]) | (uint64_t)uni(si[1]) << 32;
    uint32_t cw = lane >= 4u && lane < 12u ? __builtin_bswap32(si[lane]) : 0u;
    const uint64_t pos = (uni(ti[0]) | (uint64_t)uni(ti[1]) << 32) - L.n_samples;
    const uint32_t R = L.flush ? 0u : uni(min(((gw)(uintptr_t)L.cnt_in)[s], L.rec_cap));
    uint32_t count = 0u, closed = 0u, skipped = 0u, badc = 0u;     // of this call
    const gwo out = (gwo)(uintptr_t)(L.pkg_out + (uint64_t)s * L.pkg_cap * sizeof(fmd_pulse_package));

    // closes the carried package: lane i < 14 holds its dword i
    const auto close_carry = [&]() {
        const uint32_t deliver = nb >= L.min_bits ? 1u : 0u;
        if (deliver && count < L.pkg_cap && lane < kPkg) {
            const uint32_t v = lane == 0u ? (uint32_t)start : lane == 1u ? (uint32_t)(start >> 32) : lane == 2u ? np : lane == 3u ? nb
                             : lane < 12u ? __builtin_bswap32(cw) : lane == 12u ? flags : 0u;
            out[count * kPkg + lane] = v;
        }
        count += deliver; skipped += 1u - deliver; closed += 1u; badc += flags & FMD_PULSE_BAD;
        open = 0u;
    };

    const FMD_DDC_GLOBAL i4* const recs = (const FMD_DDC_GLOBAL i4*)(uintptr_t)(L.rec_in + (uint64_t)s * L.rec_cap * sizeof(fmd_pulses_rec));
    for (uint32_t c0 = 0; c0 < R; c0 += 64u) {
        const uint32_t nv = R - c0 < 64u ? R - c0 : 64u;     // records of this chunk
        const bool valid = lane < nv;
        i4 r = i4{0, 0, 0, 0};
        if (valid) r = recs[c0 + lane];
        const uint32_t width = (uint32_t)r.y, gap = (uint32_t)r.z;
        const bool first = valid && (gap >= L.reset || (lane == 0u && !open));
        const uint32_t v = L.modulation == FMD_PULSE_PWM ? width : gap;
        const bool ns = near(v, L.short_w, L.tol), fits = ns || near(v, L.long_w, L.tol);
        const bool judged = valid && !(L.modulation == FMD_PULSE_PPM && first);     // (a PPM package's first pulse only opens it)
        const uint64_t F = __ballot(first), BADM = __ballot(judged && !fits);
        const uint64_t VAL = __ballot(judged && fits && (ns == (L.modulation == FMD_PULSE_PWM)));
        // dead: a bad record of the same package stands in front
        const uint64_t f_le = F & (below(lane) | 1ull << lane);
        const uint64_t seg_below = f_le ? below(lane) & ~below(63u - (uint32_t)__builtin_clzll(f_le)) : below(lane);
        const bool dead = (BADM & seg_below) != 0ull || (f_le == 0ull && (flags & FMD_PULSE_BAD) != 0u);
        const uint64_t G = __ballot(judged && fits && !dead);
        const uint32_t f0 = F ? (uint32_t)__builtin_ctzll(F) : nv;       // the carried package takes the lanes below f0

        if (open) {
            np = sat_add(np, f0);
            const uint64_t g = G & below(f0);
            if (g) {                                         // (one run from lane 0 on)
                const uint32_t n = (uint32_t)__builtin_popcountll(g), g0 = (uint32_t)__builtin_ctzll(g);
                const uint64_t X = __builtin_bitreverse64((VAL >> g0) & below(n));
                if (lane >= 4u && lane < 12u) cw |= word_of(X, lane - 4u, nb);
                if (nb + n > kMaxBits) { flags |= FMD_PULSE_TRUNCATED; nb = kMaxBits; } else nb += n;
            }
            if (BADM & below(f0)) flags |= FMD_PULSE_BAD;
            if (F) close_carry();
        }
        if (F) {
            // the segments of this chunk, each with the lane that opens it
            const uint64_t f_above = F & ~(below(lane) | 1ull << lane);
            const bool ends = first && f_above != 0ull;      // closed by the next set bit of F
            const uint32_t e = f_above ? (uint32_t)__builtin_ctzll(f_above) : nv;
            const uint64_t seg = below(e) & ~below(lane), g = G & seg;
            const uint32_t n = (uint32_t)__builtin_popcountll(g);
            const uint64_t X = g ? __builtin_bitreverse64((VAL >> (uint32_t)__builtin_ctzll(g)) & below(n)) : 0ull;
            const uint32_t flg = (BADM & seg) ? FMD_PULSE_BAD : 0u;
            const uint64_t fall = pos + (uint64_t)(int64_t)r.x;
            const uint64_t st = fall >= width ? fall - width : 0ull;
            const bool deliver = ends && n >= L.min_bits;
            const uint64_t C = __ballot(ends), D = __ballot(deliver), B = __ballot(ends && flg != 0u);
            const uint32_t slot = count + (uint32_t)__builtin_popcountll(D & below(lane));
            if (deliver && slot < L.pkg_cap) {
                const gdo p = (gdo)(uintptr_t)(out + slot * kPkg);
                p[0] = st;
                p[1] = (uint64_t)(e - lane) | (uint64_t)n << 32;
                p[2] = (uint64_t)__builtin_bswap32((uint32_t)(X >> 32)) | (uint64_t)__builtin_bswap32((uint32_t)X) << 32;
                p[3] = 0ull; p[4] = 0ull; p[5] = 0ull;
                p[6] = flg;
            }
            count += (uint32_t)__builtin_popcountll(D);
            closed += (uint32_t)__builtin_popcountll(C);
            skipped += (uint32_t)__builtin_popcountll(C & ~D);
            badc += (uint32_t)__builtin_popcountll(B);
            // the last segment is the new carry
            const uint32_t lf = 63u - (uint32_t)__builtin_clzll(F);
            start = lane_of((uint32_t)st, lf) | (uint64_t)lane_of((uint32_t)(st >> 32), lf) << 32;
            np = lane_of(e - lane, lf); nb = lane_of(n, lf); flags = lane_of(flg, lf);
            const uint32_t x0 = lane_of((uint32_t)(X >> 32), lf), x1 = lane_of((uint32_t)X, lf);
            cw = lane == 4u ? x0 : lane == 5u ? x1 : 0u;
            open = 1u;
        }
    }

    if (open && (L.flush || (ti[L.off_state] == 0u && (ti[L.off_run] | (uint64_t)ti[L.off_run + 1u] << 32) >= L.reset))) close_carry();

    if (lane < kState) {
        uint32_t v;
        if (lane < 16u) {
            v = lane == 0u ? (uint32_t)start : lane == 1u ? (uint32_t)(start >> 32) : lane == 2u ? np : lane == 3u ? nb
              : lane < 12u ? __builtin_bswap32(cw) : lane == 12u ? flags : lane == 13u ? 1u : 0u;
            if (!open) v = 0u;
        } else {
            const uint32_t add = lane < 18u ? R : lane < 20u ? closed : lane < 22u ? skipped : badc, at = lane & ~1u;
            const uint64_t t = (si[at] | (uint64_t)si[at + 1u] << 32) + add;
            v = lane & 1u ? (uint32_t)(t >> 32) : (uint32_t)t;
        }
        ((gwo)(uintptr_t)(L.st_out + (uint64_t)s * kState))[lane] = v;
    }
    if (lane == 0u) ((gwo)(uintptr_t)L.cnt_out)[s] = count;
}

}  // namespace fmd_pk

static_assert(sizeof(fmd_pulse_package) == 56 && offsetof(fmd_pulse_package, n_pulses) == 8 && offsetof(fmd_pulse_package, bits) == 16 &&
              offsetof(fmd_pulse_package, flags) == 48, "the kernel writes fmd_pulse_package as 14 dwords or seven 8-byte pieces");
static_assert(sizeof(fmd_packages_totals) == 40 && sizeof(fmd_pulses_totals) == 40 && offsetof(fmd_pulses_totals, state) == 24 &&
              offsetof(fmd_pulses_totals, run) == 32, "the kernel reads fmd_pulses_totals as dwords");

struct fmd_packages {
    FmdRows rows;                                         // width 1 (its history is unused: hcap = 1, the smallest the layer takes)
    FmdDdcPair state;                                     // [n_streams][kState] uint32
    FmdRowRecords recs;                                   // fmd_pulse_package, pkg_cap per stream
    fmd_packages_config cfg{};
};

namespace {

// what a call reads, on the device
struct PkSource {
    const uint32_t* counts; const uint8_t* recs; const uint32_t* totals;
    uint32_t rec_cap, tot_stride, off_state, off_run, n_samples, flush;
};

int pk_enqueue(fmd_packages* h, const PkSource& src, hipStream_t stream)
{
    using namespace fmd_pk;
    FmdRows& r = h->rows;
    FMD_DDC_TRY(r.core.order.before(stream));
    PackagesLaunch L{};
    L.cnt_in = src.counts; L.rec_in = src.recs; L.tot_in = src.totals;
    L.rec_cap = src.rec_cap; L.n_streams = r.n_rows;
    L.tot_stride = src.tot_stride; L.off_state = src.off_state; L.off_run = src.off_run;
    L.n_samples = src.n_samples; L.flush = src.flush;
    const fmd_pulse_slicer_config& c = h->cfg.slicer;
    L.modulation = c.modulation; L.short_w = c.short_w; L.long_w = c.long_w; L.tol = c.tol; L.reset = c.reset;
    L.min_bits = h->cfg.min_bits; L.pkg_cap = h->cfg.pkg_cap;
    L.st_in = h->state.in<uint32_t>(r.core.cur); L.st_out = h->state.out<uint32_t>(r.core.cur);
    L.cnt_out = h->recs.cnt_out(r.core.cur); L.pkg_out = h->recs.rec_out(r.core.cur);
    hipLaunchKernelGGL(fmd_packages_kernel, dim3((r.n_rows + kWaves - 1u) / kWaves), dim3(kThreads), 0, stream, L);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(r.core, stream, src.n_samples);
    return FMD_OK;
}

int pk_rec_cap(size_t rec_cap)
{
    if (rec_cap < 1 || rec_cap > 1024) { fmd_internal_set_err("need 1 <= rec_cap <= 1024"); return FMD_ERR_UNSUPPORTED; }
    return FMD_OK;
}

}  // namespace

extern "C" {

size_t fmd_packages_max(size_t n_records) { return n_records + 1; }

int fmd_packages_new(const fmd_packages_config* cfg, const fmd_device_config* dev, fmd_packages** out)
{
    if (const int rc = fmd_rows_new_args(cfg, dev, out, 1)) return rc;       // (the pointers)
    const fmd_pulse_slicer_config& c = cfg->slicer;                          // the host slicer's tests, in its order
    if (c.modulation > FMD_PULSE_PPM) { fmd_internal_set_err("need modulation 0 (PWM) or 1 (PPM)"); return FMD_ERR_UNSUPPORTED; }
    if (c.short_w < 1u || c.long_w < 1u) { fmd_internal_set_err("need short_w and long_w >= 1"); return FMD_ERR_UNSUPPORTED; }
    if (c.reset < 1u) { fmd_internal_set_err("need reset >= 1"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->min_bits > fmd_pk::kMaxBits) { fmd_internal_set_err("need min_bits <= 256"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->pkg_cap < 1u || cfg->pkg_cap > 1025u) { fmd_internal_set_err("need 1 <= pkg_cap <= 1025"); return FMD_ERR_UNSUPPORTED; }
    if (dev->n_channels < 1u) { fmd_internal_set_err("need n_streams >= 1"); return FMD_ERR_UNSUPPORTED; }
    fmd_packages* h = new (std::nothrow) fmd_packages();
    if (!h) return FMD_ERR_NOMEM;
    h->cfg = *cfg;
    h->rows.width = 1; h->rows.n_rows = dev->n_channels; h->rows.hcap = 1u;
    fmd_ddc_add_pair(h->rows.core, h->state, (size_t)dev->n_channels * fmd_pk::kState * sizeof(uint32_t));
    fmd_rows_add_records(h->rows, h->recs, cfg->pkg_cap, sizeof(fmd_pulse_package));
    return fmd_rows_device(h, dev, fmd_packages_free, out);
}

void fmd_packages_free(fmd_packages* h) { fmd_rows_free(h); }
int fmd_packages_reset(fmd_packages* h) { return fmd_rows_reset(h); }
int fmd_packages_check(fmd_packages* h) { return fmd_rows_check(h); }
int fmd_packages_counts(fmd_packages* h, uint32_t* counts) { return fmd_rows_counts(h, counts); }
int fmd_packages_pkgs(fmd_packages* h, const uint32_t* streams, size_t n_sel, fmd_pulse_package* pkgs) { return fmd_rows_records(h, streams, n_sel, pkgs); }

int fmd_packages_info(fmd_packages* h, fmd_packages_totals* info)
{
    if (!h || !info) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    std::vector<uint32_t> st;
    if (const int rc = fmd_rows_read_state(h->rows, h->state, fmd_pk::kState, st)) return rc;
    for (size_t s = 0; s < h->rows.n_rows; ++s) {
        const uint32_t* const p = &st[s * fmd_pk::kState];
        const auto u64 = [p](int i) { return p[16 + 2 * i] | (uint64_t)p[17 + 2 * i] << 32; };
        info[s] = fmd_packages_totals{u64(0), u64(1), u64(2), u64(3), p[13], p[13] ? p[2] : 0u};
    }
    return FMD_OK;
}

int fmd_packages_run_batch(fmd_packages* h, const uint32_t* counts, const fmd_pulses_rec* recs, size_t rec_cap, const fmd_pulses_totals* totals,
                           size_t n_samples)
{
    if (!h || !counts || !recs || !totals) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (const int rc = pk_rec_cap(rec_cap)) return rc;
    if (n_samples > 0xFFFFFFFFull) { fmd_internal_set_err("n_samples out of range"); return FMD_ERR_UNSUPPORTED; }
    if (n_samples == 0) return FMD_OK;                       // nothing to take: no launch, the last call's results stay
    FmdDdcCore& c = h->rows.core;
    FMD_DDC_ON_DEVICE(c.device);
    const size_t n = h->rows.n_rows, cnt_bytes = fmd_rows_counts_bytes(n), rec_bytes = n * rec_cap * sizeof(fmd_pulses_rec);
    FMD_DDC_TRY(fmd_ddc_grow(c.d_iq, c.d_iq_cap, cnt_bytes + rec_bytes + n * sizeof(fmd_pulses_totals)));
    uint8_t* const d = static_cast<uint8_t*>(c.d_iq);
    FMD_DDC_TRY(hipMemcpyAsync(d, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
    FMD_DDC_TRY(hipMemcpyAsync(d + cnt_bytes, recs, rec_bytes, hipMemcpyHostToDevice, c.stream));
    FMD_DDC_TRY(hipMemcpyAsync(d + cnt_bytes + rec_bytes, totals, n * sizeof(fmd_pulses_totals), hipMemcpyHostToDevice, c.stream));
    const PkSource src{reinterpret_cast<const uint32_t*>(d), d + cnt_bytes, reinterpret_cast<const uint32_t*>(d + cnt_bytes + rec_bytes),
                       (uint32_t)rec_cap, (uint32_t)(sizeof(fmd_pulses_totals) / 4), 6u, 8u, (uint32_t)n_samples, 0u};
    const int rc = pk_enqueue(h, src, c.stream);
    const hipError_t e = hipStreamSynchronize(c.stream);
    if (rc) return rc;                                       // (the enqueue's status wins over the synchronise's)
    FMD_DDC_TRY(e);
    return FMD_OK;
}

int fmd_packages_run_bank(fmd_packages* h, fmd_pulses* bank, void* stream)
{
    if (!h || !bank) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FmdPulsesLast last{};
    fmd_pulses_last(bank, &last);
    if (last.device != h->rows.core.device || last.n_streams != h->rows.n_rows) {
        fmd_internal_set_err("the pulse bank is on another device or has another n_streams"); return FMD_ERR_INVALID_ARG;
    }
    if (!last.launched) { fmd_internal_set_err("the pulse bank has not launched since creation or reset"); return FMD_ERR_BAD_STATE; }
    FMD_DDC_ON_DEVICE(h->rows.core.device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    FMD_DDC_TRY(last.order->before(st));                     // behind the pulse bank's call, whatever stream it went to
    // (fmd_pulses.hip's state: samples at dword 0, the run at 6, s at 8)
    const PkSource src{last.d_counts, last.d_recs, last.d_state, last.pulse_cap, last.state_dwords, 8u, 6u, last.n_samples, 0u};
    return pk_enqueue(h, src, st);
}

int fmd_packages_flush(fmd_packages* h, void* stream)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->rows.core.device);
    // (the kernel reads a stream's samples for `pos`, which no record uses: its own state stands in for the totals)
    const PkSource src{nullptr, nullptr, h->state.in<uint32_t>(h->rows.core.cur), 1u, fmd_pk::kState, 0u, 0u, 0u, 1u};
    return pk_enqueue(h, src, static_cast<hipStream_t>(stream));
}

int fmd_packages_kernel_name(const fmd_packages* h, char* name, size_t cap)
{
    if (!h || !name || cap == 0) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, "%s", "fmd_pk::fmd_packages_kernel"), cap);
}

}  // extern "C"
