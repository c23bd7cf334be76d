// fmd_pocsag_decode.cpp -- the sequential half of pager reception, on the host (include/fmd.h, "pager decoder"): one row's soft
// decisions and sync-word records from the FSK front end (fmd_fsk.hip, a few samples per bit) -> POCSAG messages.  No GPU, integers
// only, sample by sample, so the result does not depend on how the samples and records are cut into pushes (tests/pocsag_ref.py
// restates it line for line).  There is no clock recovery here either: a record gives the index of a sync word's last bit, the
// slicer level and the polarity; the 512 bits of the batch behind it are read at positions counted from that index, and the record
// found where the next sync word is due re-anchors all three.
// This code parses whatever the air sends: every buffer is a fixed array and every write into one is bounded by its size.
// It needs nothing of the GPU side and no other file of the library but the header (tests/cpp/pocsag_fuzz.cpp builds it alone).
#include "../../include/fmd.h"

#include <cstring>
#include <new>

void fmd_internal_set_err(const char* msg);

namespace {

constexpr uint32_t kIdle = 0x7A89C197u;
constexpr uint32_t kPoly = 0x769u;                        // x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
constexpr uint32_t kMaxBits = 2560;
constexpr uint32_t kQueue = 64;                           // messages held for a caller whose `msgs` is full
constexpr uint32_t kRing = 64;                            // soft samples kept

bool valid(uint32_t w)
{
    uint32_t c = w >> 1;                                     // bits 31 ... 1 as a polynomial of degree 30
    for (int i = 30; i >= 10; --i)
        if ((c >> i) & 1u) c ^= kPoly << (i - 10);
    return c == 0 && (__builtin_popcount(w) & 1) == 0;
}

// the valid codeword within `e` bits of w (unique: the code's minimum distance is 6 and e <= 2)
bool correct(uint32_t w, uint32_t e, uint32_t* cw, uint32_t* nfix)
{
    if (valid(w)) { *cw = w; *nfix = 0; return true; }
    if (e >= 1)
        for (uint32_t a = 0; a < 32; ++a)
            if (valid(w ^ (1u << a))) { *cw = w ^ (1u << a); *nfix = 1; return true; }
    if (e >= 2)
        for (uint32_t a = 0; a < 32; ++a)
            for (uint32_t b = a + 1; b < 32; ++b)
                if (valid(w ^ (1u << a) ^ (1u << b))) { *cw = w ^ (1u << a) ^ (1u << b); *nfix = 2; return true; }
    return false;
}

uint32_t mag(int32_t c) { return c < 0 ? 0u - (uint32_t)c : (uint32_t)c; }

}  // namespace

struct fmd_pocsag_decoder {
    uint64_t mod = 0, step = 0, r = 0;
    uint32_t max_errors = 1;
    int16_t ring[kRing];
    uint64_t n = 0;                                       // samples since creation or reset
    // search
    bool window = false, locked = false;
    uint64_t k1 = 0, cand_k = 0;
    int32_t cand_thr = 0, cand_corr = 0;
    bool cand_inv = false;
    // lock
    uint64_t k0 = 0, p544 = 0;
    int32_t thr = 0;
    bool inv = false;
    uint32_t nb = 1;                                      // the next bit of the batch, 1 ... 512; 513: waiting for slot 16
    uint32_t word = 0;
    bool best = false;                                    // a record at slot 16
    uint64_t best_k = 0;
    int32_t best_thr = 0, best_corr = 0;
    // the open message
    bool open = false;
    fmd_pocsag_msg cur;
    uint64_t messages = 0, batches = 0, bad_codewords = 0, orphans = 0;
    fmd_pocsag_msg queue[kQueue];                         // a ring: q_len messages from q_head on
    uint32_t q_head = 0, q_len = 0;
    // the caller's array during a push
    fmd_pocsag_msg* dst = nullptr;
    size_t cap = 0, k = 0;

    void reset_state()
    {
        memset(ring, 0, sizeof ring);
        n = 0; window = locked = false; k1 = cand_k = 0; cand_thr = cand_corr = 0; cand_inv = false;
        k0 = p544 = 0; thr = 0; inv = false; nb = 1; word = 0; best = false; best_k = 0; best_thr = best_corr = 0;
        open = false; memset(&cur, 0, sizeof cur);
        messages = batches = bad_codewords = orphans = 0;
        q_head = q_len = 0;
    }

    void drain()
    {
        while (k < cap && q_len) {
            dst[k++] = queue[q_head];
            q_head = (q_head + 1) % kQueue; --q_len;
        }
    }

    // straight into the caller's array while it has room and nothing waits in front; else into the ring, whose oldest message
    // gives way when it is full
    fmd_pocsag_msg* slot()
    {
        if (!q_len && k < cap) return &dst[k++];
        if (q_len == kQueue) { q_head = (q_head + 1) % kQueue; --q_len; }
        return &queue[(q_head + q_len++) % kQueue];
    }

    void close_msg()
    {
        if (!open) return;
        open = false;
        ++messages;
        *slot() = cur;
    }

    uint64_t p(uint32_t i) const { return k0 + (2ull * i * mod + step) / (2ull * step); }

    void anchor(uint64_t k_, int32_t thr_)
    {
        k0 = k_; thr = thr_; nb = 1; word = 0; best = false;
        p544 = p(544);
        ++batches;
    }

    void codeword(uint32_t i, uint32_t raw, uint64_t at)
    {
        uint32_t cw = 0, nfix = 0;
        if (!correct(raw, max_errors, &cw, &nfix)) { ++bad_codewords; close_msg(); return; }
        if (cw == kIdle) { close_msg(); return; }
        if (!(cw >> 31)) {
            close_msg();
            memset(&cur, 0, sizeof cur);
            cur.address = ((cw >> 13) & 0x3FFFFu) << 3 | (i >> 1);
            cur.function = (cw >> 11) & 3u;
            cur.corrected = nfix; cur.inverted = inv ? 1u : 0u; cur.end_sample = at;
            open = true;
            return;
        }
        if (!open) { ++orphans; return; }
        for (int b = 19; b >= 0; --b) {
            if (cur.n_bits < kMaxBits && ((cw >> (11 + b)) & 1u)) cur.bits[cur.n_bits >> 3] |= (uint8_t)(0x80u >> (cur.n_bits & 7u));
            ++cur.n_bits;                                    // <= 20 per word, 16 words per batch: no wrap within any stream's life
        }
        cur.corrected += nfix; cur.end_sample = at;
    }

    void record(uint64_t kk, const fmd_fsk_hit& h)
    {
        const bool hinv = (h.d >> 31) != 0;
        if (!locked) {
            if (!window) { window = true; k1 = kk; cand_k = kk; cand_thr = h.thr; cand_corr = h.corr; cand_inv = hinv; }
            else if (kk <= k1 + r && mag(h.corr) > mag(cand_corr)) { cand_k = kk; cand_thr = h.thr; cand_corr = h.corr; cand_inv = hinv; }
            return;
        }
        const uint64_t dist = kk > p544 ? kk - p544 : p544 - kk;
        if (dist > r / 2 || hinv != inv) return;
        if (!best || mag(h.corr) > mag(best_corr)) { best = true; best_k = kk; best_thr = h.thr; best_corr = h.corr; }
    }

    // sample n has arrived and its records are taken
    void advance()
    {
        if (!locked) {
            if (!window || n < k1 + r) return;
            window = false; locked = true; inv = cand_inv;
            anchor(cand_k, cand_thr);
        }
        for (;;) {
            if (nb <= 512) {
                const uint64_t at = p(nb);                   // >= n - r / 2: inside the ring
                if (at > n) return;
                const uint32_t bit = ((32 * (int32_t)ring[at % kRing] > thr) ? 1u : 0u) ^ (inv ? 1u : 0u);
                word = word << 1 | bit;
                if (nb % 32 == 0) { codeword(nb / 32 - 1, word, at); word = 0; }
                ++nb;
                continue;
            }
            if (n < p544 + r / 2) return;
            if (best) { anchor(best_k, best_thr); continue; }
            locked = false;                                  // no sync word where one was due
            close_msg();
            return;
        }
    }
};

extern "C" {

int fmd_pocsag_correct(uint32_t word, uint32_t max_errors, uint32_t* cw, uint32_t* n_fixed)
{
    if (max_errors > 2) { fmd_internal_set_err("need max_errors <= 2"); return FMD_ERR_UNSUPPORTED; }
    uint32_t c = 0, f = 0;
    if (!correct(word, max_errors, &c, &f)) return FMD_ERR_BAD_STATE;
    if (cw) *cw = c;
    if (n_fixed) *n_fixed = f;
    return FMD_OK;
}

int fmd_pocsag_decoder_new(uint32_t rate_num, uint32_t rate_den, uint32_t baud, uint32_t max_errors, fmd_pocsag_decoder** out)
{
    if (!out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *out = nullptr;
    const uint64_t mod = rate_num, step = (uint64_t)baud * rate_den;
    // step up to 2^64 - 2^33 + 1: `step > mod / 2` (the same as 2 step > mod in integers) comes first and bounds step by 2^31, so
    // that 32 * step cannot wrap
    if (step < 1 || step > mod / 2 || mod > 32 * step) { fmd_internal_set_err("need 2 <= rate / baud <= 32"); return FMD_ERR_UNSUPPORTED; }
    if (max_errors > 2) { fmd_internal_set_err("need max_errors <= 2"); return FMD_ERR_UNSUPPORTED; }
    fmd_pocsag_decoder* d = new (std::nothrow) fmd_pocsag_decoder();
    if (!d) return FMD_ERR_NOMEM;
    d->mod = mod; d->step = step; d->r = (2 * mod + step) / (2 * step); d->max_errors = max_errors;
    d->reset_state();
    *out = d;
    return FMD_OK;
}

void fmd_pocsag_decoder_free(fmd_pocsag_decoder* d) { delete d; }

int fmd_pocsag_decoder_reset(fmd_pocsag_decoder* d)
{
    if (!d) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    d->reset_state();
    return FMD_OK;
}

int fmd_pocsag_decoder_push(fmd_pocsag_decoder* d, const int16_t* soft, size_t n, const fmd_fsk_hit* hits, size_t n_hits,
                            fmd_pocsag_msg* msgs, size_t cap, size_t* n_msgs)
{
    if (!d || !n_msgs || (n && !soft) || (n_hits && !hits) || (cap && !msgs)) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    d->dst = msgs; d->cap = cap; d->k = 0;
    d->drain();
    size_t hi = 0;
    for (size_t i = 0; i < n; ++i) {
        d->ring[d->n % kRing] = soft[i];
        for (; hi < n_hits && hits[hi].k_rel <= i; ++hi)     // (a record out of order is passed over; one at or behind n never comes up)
            if (hits[hi].k_rel == i) d->record(d->n, hits[hi]);
        d->advance();
        ++d->n;
    }
    *n_msgs = d->k;
    d->dst = nullptr; d->cap = 0; d->k = 0;
    return FMD_OK;
}

int fmd_pocsag_decoder_info(const fmd_pocsag_decoder* d, fmd_pocsag_info* info)
{
    if (!d || !info) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    info->messages = d->messages; info->batches = d->batches; info->bad_codewords = d->bad_codewords; info->orphans = d->orphans;
    info->locked = d->locked ? 1 : 0; info->searching = !d->locked && d->window ? 1 : 0;
    return FMD_OK;
}

}  // extern "C"
