// pocsag_fuzz.cpp -- a stand-alone program for tests/test_pocsag.py: csrc/fmd_pocsag_decode.cpp alone, built with
// -fsanitize=address,undefined, fed what the air and a careless caller might send.  Seeded, so every run is the same run:
//   1. random soft streams with random records: any d, corr (INT32_MIN among them) and thr, k_rel in and out of order and at or
//      beyond n, which the rule says are passed over and which must never be used as an index;
//   2. transmissions (an address word in its frame, message words, idle words, one or more batches) as soft decisions at 2 ... 32
//      samples per bit with a record on every sync word, intact, with bits flipped, and cut off at a random place;
// in random push sizes (0 and 1 among them) with `cap` 0, 1 and 16.  It checks what must hold whatever comes in: n_msgs <= cap,
// address < 2^21, function < 4, end_sample inside the stream, nothing delivered that was not counted, every intact page delivered
// bit for bit once the queue is drained -- and ends with exit code 0 and `ok ...` when the sanitizers saw nothing.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/fmd.h"

void fmd_internal_set_err(const char*) {}                 // (the library's error text lives in fmd_api.cpp, which is not part of this build)

static std::mt19937_64 rng(20261020);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

static const uint32_t kSync = 0x7CD215D8u, kIdle = 0x7A89C197u;

static uint32_t codeword(uint32_t data21)
{
    const uint32_t c = (data21 & 0x1FFFFFu) << 10;
    uint32_t rem = c;
    for (int i = 30; i >= 10; --i)
        if ((rem >> i) & 1u) rem ^= 0x769u << (i - 10);
    uint32_t w = (c | rem) << 1;
    return w | (uint32_t)(__builtin_popcount(w) & 1);
}

struct Page {
    uint32_t address, function;
    std::vector<uint32_t> words;                          // 20 message bits each
};

// the codewords of one transmission: whole batches
static std::vector<uint32_t> batches(const Page& p)
{
    std::vector<uint32_t> cw;
    while ((cw.size() % 16) >> 1 != (p.address & 7u)) cw.push_back(kIdle);
    cw.push_back(codeword((p.address >> 3) << 2 | p.function));
    for (uint32_t w : p.words) cw.push_back(codeword(1u << 20 | w));
    cw.push_back(kIdle);
    while (cw.size() % 16) cw.push_back(kIdle);
    return cw;
}

struct Stream {
    std::vector<int16_t> soft;
    std::vector<fmd_fsk_hit> hits;                        // k_rel counted from the start of the stream
};

// `spb` soft samples per bit of +-amp around `dc`, a record on the middle sample of the last bit of every sync word
static void transmit(const std::vector<uint32_t>& cw, uint32_t spb, int amp, int dc, bool inverted, int flips, size_t cut, Stream& s)
{
    std::vector<int> bits;
    std::vector<size_t> syncs;                            // index of the last bit of each sync word
    for (int i = 0; i < 64; ++i) bits.push_back((i + 1) & 1);
    for (size_t i = 0; i < cw.size(); ++i) {
        if (i % 16 == 0) {
            for (int b = 31; b >= 0; --b) bits.push_back((int)((kSync >> b) & 1u));
            syncs.push_back(bits.size() - 1);
        }
        for (int b = 31; b >= 0; --b) bits.push_back((int)((cw[i] >> b) & 1u));
    }
    for (int i = 0; i < flips; ++i) bits[64 + rnd((uint32_t)bits.size() - 64)] ^= 1;
    if (cut < bits.size()) bits.resize(cut);
    const size_t base = s.soft.size();
    for (int b : bits)
        for (uint32_t i = 0; i < spb; ++i) s.soft.push_back((int16_t)(dc + ((b != 0) != inverted ? amp : -amp)));
    for (size_t at : syncs) {
        if (at >= bits.size()) break;
        fmd_fsk_hit h;
        h.k_rel = (uint32_t)(base + at * spb + spb / 2);
        h.d = inverted ? 32u | 1u << 31 : 0u;
        h.corr = inverted ? -32 * amp : 32 * amp;
        h.thr = 32 * dc;
        s.hits.push_back(h);
    }
    // (behind a transmission that was cut off the decoder reads on to where the next sync word was due: the carrier stays that long)
    for (uint32_t i = 0, gap = (cut < 64 + 32 * (cw.size() + cw.size() / 16) ? 600 : 3) * spb + rnd(40 * spb); i < gap; ++i) s.soft.push_back((int16_t)dc);
}

struct Sink {
    std::vector<fmd_pocsag_msg> msgs;
    uint64_t pushed = 0;
};

static int fail(const char* what) { fprintf(stderr, "pocsag_fuzz: %s\n", what); return 1; }

static int take(const fmd_pocsag_msg* out, size_t k, Sink& sink)
{
    for (size_t i = 0; i < k; ++i) {
        if (out[i].address >= 1u << 21 || out[i].function > 3) return fail("address or function out of bounds");
        if (out[i].inverted > 1) return fail("polarity out of bounds");
        if (out[i].end_sample >= sink.pushed) return fail("end_sample behind the stream");
        sink.msgs.push_back(out[i]);
    }
    return 0;
}

// the stream in random push sizes and caps, each push with the records that fall into it (k_rel counted into the push) and, with
// `junk`, some that do not: at or beyond n, and out of order
static int feed(fmd_pocsag_decoder* d, const Stream& s, bool junk, Sink& sink)
{
    fmd_pocsag_msg out[16];
    static const size_t caps[3] = {0, 1, 16};
    size_t hi = 0;
    for (size_t lo = 0; lo <= s.soft.size();) {
        size_t n = rnd(4) == 0 ? rnd(3) : rnd(5000);
        if (n > s.soft.size() - lo) n = s.soft.size() - lo;
        std::vector<fmd_fsk_hit> hits;
        for (; hi < s.hits.size() && s.hits[hi].k_rel < lo + n; ++hi) {
            fmd_fsk_hit h = s.hits[hi];
            h.k_rel -= (uint32_t)lo;
            hits.push_back(h);
        }
        if (junk)
            for (uint32_t i = 0, m = rnd(4); i < m; ++i) {
                fmd_fsk_hit h;
                static const uint32_t far[4] = {0u, 1u, 1000000u, 0xFFFFFFFFu};
                h.k_rel = rnd(2) ? (uint32_t)n + far[rnd(4)] : rnd((uint32_t)n + 1);
                h.d = (uint32_t)rng();
                h.corr = rnd(8) == 0 ? INT_MIN : (int32_t)(uint32_t)rng();
                h.thr = (int32_t)(uint32_t)rng();
                hits.insert(hits.begin() + rnd((uint32_t)hits.size() + 1), h);
            }
        const size_t cap = caps[rnd(3)];
        size_t k = 99;
        memset(out, 0xA5, sizeof out);
        if (fmd_pocsag_decoder_push(d, n ? s.soft.data() + lo : nullptr, n, hits.empty() ? nullptr : hits.data(), hits.size(),
                                    cap ? out : nullptr, cap, &k) != FMD_OK)
            return fail("push failed");
        sink.pushed += n;
        if (k > cap) return fail("n_msgs > cap");
        if (take(out, k, sink)) return 1;
        lo += n;
        if (lo == s.soft.size() && n == 0) break;
        if (lo == s.soft.size() && rnd(2)) break;
    }
    return 0;
}

static int drain(fmd_pocsag_decoder* d, Sink& sink)
{
    fmd_pocsag_msg out[16];
    for (;;) {
        size_t k = 0;
        if (fmd_pocsag_decoder_push(d, nullptr, 0, nullptr, 0, out, 16, &k) != FMD_OK) return fail("drain failed");
        if (k > 16 || take(out, k, sink)) return fail("drain out of bounds");
        if (k < 16) return 0;
    }
}

static bool same(const fmd_pocsag_msg& m, const Page& p)
{
    if (m.address != p.address || m.function != p.function || m.n_bits != 20 * p.words.size()) return false;
    for (size_t i = 0; i < p.words.size() && i < 128; ++i)
        for (int b = 0; b < 20; ++b) {
            const size_t at = 20 * i + (size_t)b;
            if (((m.bits[at >> 3] >> (7 - (at & 7))) & 1u) != ((p.words[i] >> (19 - b)) & 1u)) return false;
        }
    return true;
}

int main()
{
    uint64_t total_msgs = 0, total_bad = 0, total_orphans = 0, intact = 0;
    // ---- 1. random streams, random records ----------------------------------------------------------------------------------
    for (int round = 0; round < 24; ++round) {
        const uint32_t spb = 2 + rnd(31);
        fmd_pocsag_decoder* d = nullptr;
        if (fmd_pocsag_decoder_new(spb * 1200u, 1, 1200, rnd(3), &d) != FMD_OK || !d) return fail("new failed");
        Stream s;
        for (int i = 0; i < 200000; ++i) s.soft.push_back((int16_t)(rng() & 0xFFFF));
        for (uint32_t k = rnd(2000); k < s.soft.size(); k += 1 + rnd(round % 2 ? 40 * spb : 3000 * spb)) {
            fmd_fsk_hit h;
            h.k_rel = k; h.d = rnd(2) ? rnd(3) : (32 - rnd(3)) | 1u << 31;
            h.corr = (int32_t)rnd(1u << 20) * (rnd(2) ? 1 : -1); h.thr = (int32_t)rnd(1u << 20) - (1 << 19);
            s.hits.push_back(h);
        }
        Sink sink;
        if (feed(d, s, true, sink) || drain(d, sink)) return 1;
        fmd_pocsag_info info;
        if (fmd_pocsag_decoder_info(d, &info) != FMD_OK) return fail("info failed");
        if (sink.msgs.size() > info.messages) return fail("delivered more than counted");
        total_msgs += info.messages; total_bad += info.bad_codewords; total_orphans += info.orphans;
        if (round % 5 == 0 && fmd_pocsag_decoder_reset(d) != FMD_OK) return fail("reset failed");
        fmd_pocsag_decoder_free(d);
    }
    // ---- 2. transmissions, intact and damaged -----------------------------------------------------------------------------------
    for (int round = 0; round < 60; ++round) {
        const uint32_t spb = 2 + rnd(31);
        fmd_pocsag_decoder* d = nullptr;
        if (fmd_pocsag_decoder_new(spb * 1200u, 1, 1200, 1, &d) != FMD_OK || !d) return fail("new failed");
        Stream s;
        std::vector<Page> want;
        const int n_pages = 1 + (int)rnd(6);               // (few enough for the ring of 64 never to lose one)
        for (int f = 0; f < n_pages; ++f) {
            static const uint32_t sizes[6] = {0, 1, 15, 16, 128, 140};
            Page p;
            p.address = rnd(1u << 21); p.function = rnd(4);
            p.words.resize(rnd(3) == 0 ? sizes[rnd(6)] : 1 + rnd(30));
            for (uint32_t& w : p.words) w = rnd(1u << 20);
            const std::vector<uint32_t> cw = batches(p);
            const int damage = (int)rnd(3);                  // 0: intact
            const size_t nbits = 64 + cw.size() * 32 + cw.size() / 16 * 32;
            transmit(cw, spb, 1 + (int)rnd(12000), (int)rnd(8000) - 4000, rnd(2) != 0, damage == 1 ? 1 + (int)rnd(40) : 0,
                     damage == 2 ? rnd((uint32_t)nbits) : nbits, s);
            if (damage == 0) want.push_back(p);
        }
        Sink sink;
        if (feed(d, s, false, sink) || drain(d, sink)) return 1;
        fmd_pocsag_info info;
        if (fmd_pocsag_decoder_info(d, &info) != FMD_OK) return fail("info failed");
        if (sink.msgs.size() != info.messages) return fail("delivered and counted differ");
        size_t at = 0;                                       // every intact page, in order, among the delivered ones
        for (const Page& w : want) {
            while (at < sink.msgs.size() && !same(sink.msgs[at], w)) ++at;
            if (at == sink.msgs.size()) return fail("an intact page was not delivered");
            ++at; ++intact;
        }
        total_msgs += info.messages; total_bad += info.bad_codewords; total_orphans += info.orphans;
        fmd_pocsag_decoder_free(d);
    }
    // ---- the arguments ---------------------------------------------------------------------------------------------------------
    fmd_pocsag_decoder* d = nullptr;
    size_t k = 0;
    if (fmd_pocsag_decoder_new(2399, 1, 1200, 1, &d) != FMD_ERR_UNSUPPORTED || d) return fail("rate below 2 per bit accepted");
    if (fmd_pocsag_decoder_new(38401, 1, 1200, 1, &d) != FMD_ERR_UNSUPPORTED || d) return fail("rate above 32 per bit accepted");
    if (fmd_pocsag_decoder_new(4800, 0, 1200, 1, &d) != FMD_ERR_UNSUPPORTED || d) return fail("zero denominator accepted");
    if (fmd_pocsag_decoder_new(4800, 1, 1200, 3, &d) != FMD_ERR_UNSUPPORTED || d) return fail("max_errors 3 accepted");
    // baud * rate_den = 2^62: twice and 32 times that are 0 in 64 bits (no push follows a refusal)
    if (fmd_pocsag_decoder_new(0, 1u << 31, 1u << 31, 1, &d) != FMD_ERR_UNSUPPORTED || d) return fail("a step of 2^62 against rate 0 accepted");
    if (fmd_pocsag_decoder_new(1, 1u << 31, 1u << 31, 1, &d) != FMD_ERR_UNSUPPORTED || d) return fail("a step of 2^62 against rate 1 accepted");
    if (fmd_pocsag_decoder_new(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 1, &d) != FMD_ERR_UNSUPPORTED || d) return fail("the largest step accepted");
    if (fmd_pocsag_decoder_new(0xFFFFFFFFu, 0xFFFFFFFFu / 2400u, 1200, 2, &d) != FMD_OK || !d) return fail("the largest numbers refused");
    int16_t one = -5;
    fmd_fsk_hit h = {7, 0, 5000, 0};
    if (fmd_pocsag_decoder_push(d, &one, 1, &h, 1, nullptr, 0, &k) != FMD_OK || k != 0) return fail("push with cap 0 failed");
    if (fmd_pocsag_decoder_push(d, nullptr, 1, nullptr, 0, nullptr, 0, &k) != FMD_ERR_INVALID_ARG) return fail("null soft accepted");
    if (fmd_pocsag_decoder_push(d, &one, 1, nullptr, 1, nullptr, 0, &k) != FMD_ERR_INVALID_ARG) return fail("null hits accepted");
    fmd_pocsag_decoder_free(d);
    fmd_pocsag_decoder_free(nullptr);
    printf("ok messages %llu intact %llu bad_codewords %llu orphans %llu\n", (unsigned long long)total_msgs, (unsigned long long)intact,
           (unsigned long long)total_bad, (unsigned long long)total_orphans);
    return intact > 0 ? 0 : fail("no intact page was ever sent");
}
