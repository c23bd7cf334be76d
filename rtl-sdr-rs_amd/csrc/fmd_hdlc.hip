// fmd_hdlc.hip -- the frame bank: the AX.25 frame decoder of every row on the device.  The soft decisions the tone-pair demodulator
// (fmd_afsk.hip) leaves for every NFM row go through clock recovery, NRZI, HDLC and the FCS in ONE gfx950 kernel, one lane per row,
// and only the frames come back.  No new arithmetic: row r behaves as an fmd_ax25_decoder (fmd_ax25_decode.cpp, tests/ax25_ref.py)
// of its own would that is pushed exactly row r's samples of each call, with room for every frame.
//
// Per sample (include/fmd.h, "AX.25 frame decoder"): cur = (v >= 0); a sign change pulls ph a quarter of the way to mod / 2; ph +=
// step; ph >= mod takes a bit (NRZI against the level at the previous take).  Per bit: the 8-bit shift register, the flag, seven 1s,
// the stuffed 0, the store.  The decoder's closing rule runs the CRC over the whole frame when the flag arrives; here the CRC runs
// with the bits:
//     hist   the last 16 stored bits, the newest at bit 15.  Storing bit number nbits (from 0): when nbits >= 7 the bit stored seven
//            bits ago (bit 9 of hist) enters the CRC register (reflected 0x1021: fb = (crc ^ x) & 1, crc = crc >> 1 ^ (fb ? 0x8408 :
//            0)); then hist = hist >> 1 | bit << 15; when nbits % 8 == 7 the byte hist >> 8 goes to byte nbits / 8 of the row's open
//            frame in device memory.
//     flag   crc = 0xFFFF, nbits = 0.  At the next flag nbits stored bits are the frame's nbits - 7 and the flag's first seven, and
//            the register has taken exactly the frame's.  Over a frame with its FCS it is 0xF0B8 exactly when the last two bytes are
//            the CRC-16/X.25 of the others (the X.25 residue), so closing is the definition's tests on nbits and one compare.
// A frame that passed is copied by the whole wave -- 64 lanes x 8 bytes, zero behind len -- from the row's open frame into the row's
// next record before the next sample can overwrite byte 0 (frames may share one flag).
//
// One workgroup = one wave = 64 consecutive rows for the whole call, walked in chunks of 64 soft decisions.  The rows lie in_cap
// apart, so the wave stages 64 rows x 64 samples into LDS: eight lanes per row, 16-byte loads of the pieces that lie whole inside
// the chunk, element loads at the unaligned head and tail (rows start at any 2-byte address).  The tile's row pitch is 33 dwords:
// lane l reading tile[l][i] touches 64 different banks.  A lane first collects the 64 signs of its row's chunk into a register pair,
// so the sequential loop reads no memory.  The state lives in registers for the whole call; the loop over a chunk's samples is
// uniform, the per-bit step is written as selects, and only the predicates differ between lanes.  The clock runs in 32 bits where
// mod < 2^31 and in 64 otherwise (ph + step does not fit 32 bits at the top of the domain).
// Carried per row: 12 dwords in a pair of the handle (all-zero is the reset state: prev and level are stored inverted), and the open
// frame's whole bytes, 520 per row, updated in place (a refused call launches nothing and no launch is replayed).  The counts and
// records go to the pair's written side and are read behind the call.
#include "../../include/fmd.h"

#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "fmd_rows.h"

namespace fmd_hd {

constexpr int kThreads = 64;                              // one wave: a lane per row
constexpr uint32_t kRows = 64;
constexpr uint32_t kChunk = 64;                           // soft decisions per chunk and row
constexpr uint32_t kPitch = 33;                           // dwords per row of the tile (odd: no bank conflicts down a column)
constexpr uint32_t kState = 12;                           // dwords per row in the handle's pair
constexpr uint32_t kOpen = 520;                           // bytes per row of the open frame (515 used; a multiple of 8)
constexpr uint32_t kMaxBytes = 514, kMinBytes = 17, kMaxBits = kMaxBytes * 8 + 7;
constexpr uint32_t kResidue = 0xF0B8;

typedef int i4 __attribute__((ext_vector_type(4)));

// State words of a row: 0: ph.  1: bit 0 !prev, bit 1 !level, bit 2 in_frame, bits 3-5 ones, bits 8-15 sr, bits 16-31 hist.
// 2: nbits | crc << 16.  3: 0.  4-5 frames_ok, 6-7 bad_fcs, 8-9 aborts (low dword first).  10-11: 0.
struct HdlcLaunch {
    const int16_t* in;         // [n_rows][in_cap]
    uint64_t in_cap;
    uint32_t n_in;             // valid samples per row, >= 1
    uint32_t n_rows;
    const uint32_t* st_in;     // [n_rows][kState]
    uint32_t* st_out;
    uint8_t* open;             // [n_rows][kOpen], in place
    uint32_t* cnt_out;         // [n_rows]: the frames that passed in this call
    uint8_t* rec_out;          // [n_rows][frame_cap] fmd_ax25_frame
    uint64_t pos;              // core.pos: samples per row before the call
    uint32_t mod, step, frame_cap;
};

// A row's decoder between two samples, in registers.  The three counters count the call; the kernel adds them to the carried ones.
struct Row {
    uint32_t prev, level, inf, ones, sr, hist, nbits, crc;
    uint32_t d_ok, d_bad, d_ab, count;
};

// The clock over one sample.  Narrow (mod < 2^31: ph + step < 2^32 and the signed difference fits 32 bits) or in 64 bits.
template <bool Wide>
__device__ __forceinline__ bool clock_step(uint64_t& ph, uint32_t changed, uint64_t mod, uint64_t step, int64_t half)
{
    if (Wide) {
        if (changed) ph = (uint64_t)((int64_t)ph - (((int64_t)ph - half) >> 2));
        ph += step;
        const bool take = ph >= mod;
        if (take) ph -= mod;
        return take;
    }
    uint32_t p = (uint32_t)ph;
    const int pull = ((int)p - (int)(uint32_t)half) >> 2;
    p -= changed ? (uint32_t)pull : 0u;
    p += (uint32_t)step;
    const bool take = p >= (uint32_t)mod;
    p -= take ? (uint32_t)mod : 0u;
    ph = p;
    return take;
}

// One taken bit (the order of include/fmd.h: shift register, flag, seven 1s, stuffed 0, store), as selects: the lanes differ only in
// predicates.  Returns whether a frame passed, its length without the FCS in *plen.
__device__ __forceinline__ bool bit_step(Row& r, uint32_t bit, bool live, FMD_DDC_GLOBAL uint8_t* open, uint32_t* plen)
{
    r.sr = (r.sr >> 1) | (bit << 7);
    const bool flag = r.sr == 0x7Eu, inf = r.inf != 0u;
    // the flag: close the open frame
    const uint32_t nb = r.nbits - 7u, bytes = nb >> 3;
    const bool closing = flag && inf && r.nbits > 7u;
    const bool good = closing && (nb & 7u) == 0u && r.nbits <= kMaxBits && bytes >= kMinBytes && r.crc == kResidue;   // (bytes <= kMaxBytes with it)
    r.d_ok += good ? 1u : 0u;
    r.d_bad += closing && !good ? 1u : 0u;
    *plen = bytes - 2u;
    // no flag: seven 1s, the stuffed 0, the store
    const uint32_t ones1 = bit ? r.ones + 1u : 0u;
    const bool abort = !flag && ones1 >= 7u;
    const bool stuffed = !flag && !bit && r.ones == 5u;
    r.d_ab += abort && inf ? 1u : 0u;
    const bool store = !flag && inf && !abort && !stuffed;
    const bool kept = store && r.nbits < kMaxBits;
    const uint32_t fb = (r.crc ^ (r.hist >> 9)) & 1u;
    const uint32_t crc1 = (r.crc >> 1) ^ (fb ? 0x8408u : 0u);
    const uint32_t hist1 = (r.hist >> 1) | (bit << 15);
    if (kept && (r.nbits & 7u) == 7u && live) open[r.nbits >> 3] = (uint8_t)(hist1 >> 8);     // nbits >> 3 <= 514
    r.crc = flag ? 0xFFFFu : (kept && r.nbits >= 7u ? crc1 : r.crc);
    r.hist = kept ? hist1 : r.hist;
    r.nbits = flag ? 0u : r.nbits + (store && r.nbits <= kMaxBits ? 1u : 0u);  // one past the limit marks a frame that is too long
    r.inf = flag ? 1u : (abort ? 0u : r.inf);
    r.ones = flag ? 0u : (abort ? 7u : ones1);
    return good && live;
}

// The whole wave copies the frames that passed at this sample (mask: their lanes) into their rows' next records.
__device__ __forceinline__ void deliver(const HdlcLaunch& A, unsigned long long mask, uint32_t plen, uint32_t count, uint64_t row0,
                                        uint32_t l, uint64_t end_sample)
{
    __threadfence();                                         // the lanes' byte stores, before other lanes read them
    while (mask) {
        const int j = __builtin_ctzll(mask);
        mask &= mask - 1ull;
        const uint32_t jlen = (uint32_t)__shfl((int)plen, j), slot = (uint32_t)__shfl((int)count, j);
        if (slot >= A.frame_cap) continue;                   // counted, not delivered
        const uint64_t jrow = row0 + (uint32_t)j;
        uint64_t d = ((const FMD_DDC_GLOBAL uint64_t*)(uintptr_t)(A.open + jrow * kOpen))[l];
        const uint32_t b0 = 8u * l;
        if (b0 >= jlen) d = 0ull;
        else if (jlen - b0 < 8u) d &= (1ull << (8u * (jlen - b0))) - 1ull;
        FMD_DDC_GLOBAL uint8_t* const rec =
            (FMD_DDC_GLOBAL uint8_t*)(uintptr_t)(A.rec_out + (jrow * A.frame_cap + slot) * sizeof(fmd_ax25_frame));
        ((FMD_DDC_GLOBAL uint64_t*)rec)[l] = d;
        if (l == 0u) {
            ((FMD_DDC_GLOBAL uint64_t*)rec)[64] = (uint64_t)jlen;                // len, and the padding behind it
            ((FMD_DDC_GLOBAL uint64_t*)rec)[65] = end_sample;
        }
    }
    __threadfence();                                         // the copies' loads, before the rows' next byte stores
}

// A chunk's `len` samples of the lane's row: bit i of `signs` is v[i] >= 0.
template <bool Wide>
__device__ __forceinline__ void chunk_step(const HdlcLaunch& A, Row& r, uint64_t& ph, uint64_t signs, uint32_t len, bool live,
                                           FMD_DDC_GLOBAL uint8_t* open, uint64_t row0, uint32_t l, uint64_t pos0)
{
    const uint64_t mod = A.mod, step = A.step;
    const int64_t half = (int64_t)(mod >> 1);
    for (uint32_t i = 0; i < len; ++i) {                     // wave-uniform
        const uint32_t cur = (uint32_t)(signs >> i) & 1u;
        const bool take = clock_step<Wide>(ph, cur ^ r.prev, mod, step, half);
        r.prev = cur;
        bool passed = false;
        uint32_t plen = 0;
        if (take) {
            passed = bit_step(r, cur == r.level ? 1u : 0u, live, open, &plen);
            r.level = cur;
        }
        const unsigned long long mask = __ballot(passed);    // nearly always zero: one scalar branch
        if (mask) deliver(A, mask, plen, r.count, row0, l, pos0 + i);
        r.count += passed ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(kThreads) fmd_hdlc_kernel(const HdlcLaunch A)
{
    typedef const FMD_DDC_GLOBAL int16_t* gsrc;
    __shared__ __attribute__((aligned(16))) uint32_t tileL[kRows * kPitch];
    int16_t* const tile = reinterpret_cast<int16_t*>(tileL);

    const uint32_t l = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * kRows, row = row0 + l;
    const bool live = row < A.n_rows;

    uint64_t ph = 0, ok = 0, bad = 0, ab = 0;
    uint32_t fl = 0, nc = 0;
    if (live) {
        const FMD_DDC_GLOBAL i4* const s = (const FMD_DDC_GLOBAL i4*)(uintptr_t)(A.st_in + row * kState);
        const i4 a = s[0], b = s[1], c = s[2];
        ph = (uint32_t)a.x; fl = (uint32_t)a.y; nc = (uint32_t)a.z;
        ok = (uint32_t)b.x | (uint64_t)(uint32_t)b.y << 32;
        bad = (uint32_t)b.z | (uint64_t)(uint32_t)b.w << 32;
        ab = (uint32_t)c.x | (uint64_t)(uint32_t)c.y << 32;
    }
    Row r{(fl & 1u) ^ 1u, ((fl >> 1) & 1u) ^ 1u, (fl >> 2) & 1u, (fl >> 3) & 7u, (fl >> 8) & 0xFFu, fl >> 16, nc & 0xFFFFu, nc >> 16,
          0u, 0u, 0u, 0u};
    const bool wide = A.mod >= (1u << 31);
    FMD_DDC_GLOBAL uint8_t* const open = (FMD_DDC_GLOBAL uint8_t*)(uintptr_t)(A.open + (live ? row : 0) * kOpen);

    for (uint32_t cs = 0; cs < A.n_in; cs += kChunk) {       // wave-uniform
        const uint32_t ce = cs + kChunk < A.n_in ? cs + kChunk : A.n_in;
        __syncthreads();                                     // (the chunk before has been read)
        // ---- the samples: eight lanes per row, eight rows per pass ----------------------------------------------------------------
        for (uint32_t pass = 0; pass < 8u; ++pass) {
            const uint32_t rr = pass * 8u + (l >> 3), p = l & 7u;
            const uint64_t grow = row0 + rr;
            if (grow >= A.n_rows) continue;
            const uintptr_t R = (uintptr_t)(A.in + grow * A.in_cap);
            const uintptr_t a0 = R + 2u * (uintptr_t)cs, a1 = R + 2u * (uintptr_t)ce;
            int16_t* const raw = tile + rr * (2u * kPitch);
            for (uintptr_t ca = ((a0 >> 4) + p) << 4; ca < a1; ca += 8u * 16u) {
                if (ca >= a0 && ca + 16u <= a1) {            // a piece whole inside the chunk
                    const i4 v = *(const FMD_DDC_GLOBAL i4*)ca;
                    const uint32_t e0 = (uint32_t)((ca - a0) >> 1);
                    const uint32_t d[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
#pragma unroll
                    for (uint32_t e = 0; e < 8u; ++e) raw[e0 + e] = (int16_t)(d[e >> 1] >> (16u * (e & 1u)));
                } else {                                     // the unaligned head or tail: exactly the samples of the chunk
                    for (uint32_t e = 0; e < 8u; ++e) {
                        const uintptr_t a = ca + 2u * e;
                        if (a < a0 || a >= a1) continue;
                        raw[(uint32_t)((a - a0) >> 1)] = *(gsrc)a;
                    }
                }
            }
        }
        __syncthreads();

        // ---- the signs of the lane's row (what lies behind the chunk's samples is not used), then the decoder ----------------------
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (uint32_t i = 0; i < 32u; ++i) {
            const uint32_t w = tileL[l * kPitch + i];        // samples 2 i and 2 i + 1
            const uint32_t two = ((w & 0x8000u) ? 0u : 1u) | ((w & 0x80000000u) ? 0u : 2u);
            if (i < 16u) lo |= two << (2u * i); else hi |= two << (2u * i - 32u);
        }
        const uint64_t signs = lo | (uint64_t)hi << 32;
        if (wide) chunk_step<true>(A, r, ph, signs, ce - cs, live, open, row0, l, A.pos + cs);
        else chunk_step<false>(A, r, ph, signs, ce - cs, live, open, row0, l, A.pos + cs);
    }

    if (!live) return;
    ok += r.d_ok; bad += r.d_bad; ab += r.d_ab;
    fl = (r.prev ^ 1u) | (r.level ^ 1u) << 1 | r.inf << 2 | r.ones << 3 | r.sr << 8 | r.hist << 16;
    nc = r.nbits | r.crc << 16;
    FMD_DDC_GLOBAL i4* const s = (FMD_DDC_GLOBAL i4*)(uintptr_t)(A.st_out + row * kState);
    s[0] = i4{(int)(uint32_t)ph, (int)fl, (int)nc, 0};
    s[1] = i4{(int)(uint32_t)ok, (int)(uint32_t)(ok >> 32), (int)(uint32_t)bad, (int)(uint32_t)(bad >> 32)};
    s[2] = i4{(int)(uint32_t)ab, (int)(uint32_t)(ab >> 32), 0, 0};
    ((FMD_DDC_GLOBAL uint32_t*)(uintptr_t)A.cnt_out)[row] = r.count;
}

}  // namespace fmd_hd

static_assert(sizeof(fmd_ax25_frame) == 528 && offsetof(fmd_ax25_frame, len) == 512 && offsetof(fmd_ax25_frame, end_sample) == 520,
              "the kernel writes fmd_ax25_frame as 66 qwords");

struct fmd_hdlc {
    FmdRows rows;                                         // width 1 (its history is unused: hcap = 1, the smallest the layer takes)
    FmdDdcPair state;                                     // [n_rows][kState] uint32
    FmdRowRecords recs;                                   // fmd_ax25_frame, frame_cap per row
    void* d_open = nullptr;                               // [n_rows][kOpen] bytes, in place (reset need not clear it: with nbits = 0
                                                          // nothing of it is read before it is written)
    uint32_t mod = 0, step = 0;
};

namespace {

int hd_enqueue(fmd_hdlc* h, const void* d_in, size_t n_in, size_t in_cap, hipStream_t stream)
{
    FmdRows& r = h->rows;
    if (const int rc = fmd_rows_check_call(r, d_in, n_in, in_cap, nullptr)) return rc;
    if (n_in == 0) return FMD_OK;                            // nothing to take: no launch, the last call's results stay
    fmd_hd::HdlcLaunch A{};
    A.in = static_cast<const int16_t*>(d_in); A.in_cap = in_cap; A.n_in = (uint32_t)n_in; A.n_rows = r.n_rows;
    A.st_in = h->state.in<uint32_t>(r.core.cur); A.st_out = h->state.out<uint32_t>(r.core.cur);
    A.open = static_cast<uint8_t*>(h->d_open);
    A.cnt_out = h->recs.cnt_out(r.core.cur);
    A.rec_out = h->recs.rec_out(r.core.cur);
    A.pos = r.core.pos;
    A.mod = h->mod; A.step = h->step; A.frame_cap = h->recs.cap;
    const uint32_t grid = (r.n_rows + fmd_hd::kRows - 1u) / fmd_hd::kRows;
    return fmd_rows_launch(r, fmd_hd::fmd_hdlc_kernel, fmd_hd::fmd_hdlc_kernel, grid, fmd_hd::kThreads, A, stream, n_in, 0, nullptr);
}

}  // namespace

extern "C" {

int fmd_hdlc_new(uint32_t rate_num, uint32_t rate_den, uint32_t baud, uint32_t frame_cap, const fmd_device_config* dev, fmd_hdlc** out)
{
    if (const int rc = fmd_rows_new_args(dev, dev, out, 1)) return rc;       // (the pointers)
    const uint64_t mod = rate_num, step = (uint64_t)baud * rate_den;
    // the host decoder's test (fmd_ax25_decode.cpp): `step > mod / 4` comes first and bounds step by 2^30, so that 64 * step cannot wrap
    if (step < 1 || step > mod / 4 || mod > 64 * step) { fmd_internal_set_err("need 4 <= rate / baud <= 64"); return FMD_ERR_UNSUPPORTED; }
    if (frame_cap < 1 || frame_cap > 16) { fmd_internal_set_err("need 1 <= frame_cap <= 16"); return FMD_ERR_UNSUPPORTED; }
    if (const int rc = fmd_rows_count_arg(dev)) return rc;
    fmd_hdlc* h = new (std::nothrow) fmd_hdlc();
    if (!h) return FMD_ERR_NOMEM;
    h->mod = (uint32_t)mod; h->step = (uint32_t)step;
    h->rows.width = 1; h->rows.n_rows = dev->n_channels; h->rows.hcap = 1u;
    h->rows.lds = 0;                                         // the tile is static
    const size_t n = dev->n_channels;
    fmd_ddc_add_pair(h->rows.core, h->state, n * fmd_hd::kState * sizeof(uint32_t));
    fmd_rows_add_records(h->rows, h->recs, frame_cap, sizeof(fmd_ax25_frame));
    fmd_ddc_add_owned(h->rows.core, h->d_open, nullptr, n * fmd_hd::kOpen);
    return fmd_rows_device(h, dev, fmd_hdlc_free, out);
}

void fmd_hdlc_free(fmd_hdlc* h) { fmd_rows_free(h); }
int fmd_hdlc_reset(fmd_hdlc* h) { return fmd_rows_reset(h); }
int fmd_hdlc_check(fmd_hdlc* h) { return fmd_rows_check(h); }
int fmd_hdlc_inputs(const fmd_hdlc* h, uint64_t* inputs) { return fmd_rows_inputs(h, inputs); }
int fmd_hdlc_counts(fmd_hdlc* h, uint32_t* counts) { return fmd_rows_counts(h, counts); }
int fmd_hdlc_frames(fmd_hdlc* h, const uint32_t* rows, size_t n_sel, fmd_ax25_frame* frames) { return fmd_rows_records(h, rows, n_sel, frames); }

int fmd_hdlc_info(fmd_hdlc* h, fmd_ax25_info* info)
{
    if (!h || !info) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    std::vector<uint32_t> st;
    if (const int rc = fmd_rows_read_state(h->rows, h->state, fmd_hd::kState, st)) return rc;
    for (size_t r = 0; r < h->rows.n_rows; ++r) {
        const uint32_t* const s = &st[r * fmd_hd::kState];
        memset(&info[r], 0, sizeof info[r]);
        info[r].frames_ok = s[4] | (uint64_t)s[5] << 32;
        info[r].bad_fcs = s[6] | (uint64_t)s[7] << 32;
        info[r].aborts = s[8] | (uint64_t)s[9] << 32;
        info[r].in_frame = (int)((s[1] >> 2) & 1u);
    }
    return FMD_OK;
}

int fmd_hdlc_run_device(fmd_hdlc* h, const void* d_in, size_t n_in, size_t in_cap, void* stream)
{
    return fmd_ddc_run_device(h ? &h->rows.core : nullptr, d_in, d_in,
                              [&] { return hd_enqueue(h, d_in, n_in, in_cap, static_cast<hipStream_t>(stream)); });
}

int fmd_hdlc_run_batch(fmd_hdlc* h, const int16_t* in, size_t n_in, size_t in_cap)
{
    return fmd_rows_feed_batch(h, in, n_in, in_cap, [](FmdDdcCore&) -> int { return FMD_OK; },
                               [&](const void* d_in, hipStream_t s) { return hd_enqueue(h, d_in, n_in, in_cap, s); });
}

int fmd_hdlc_kernel_name(const fmd_hdlc* h, char* name, size_t cap) { return fmd_rows_kernel_name(h, name, cap, "fmd_hd::fmd_hdlc_kernel"); }

}  // extern "C"
