// ax25_fuzz.cpp -- a stand-alone program for tests/test_afsk.py: csrc/fmd_ax25_decode.cpp alone, built with -fsanitize=address,undefined,
// fed what the air might send.  Seeded, so every run is the same run:
//   1. random soft streams: white int16, and runs of one sign of random lengths (every bit pattern the clock can produce);
//   2. valid frames (also longer than the largest frame, and of 0xFF bytes) as soft decisions at 4 ... 64 samples per bit, intact,
//      with bits flipped, cut off at a random place, and padded with runs of flags;
// in random call sizes (0 and 1 among them) with `cap` 0, 1 and 16.  It checks what must hold whatever comes in: n_frames <= cap,
// len <= 512, end_sample inside the stream, nothing delivered that was not counted, every intact frame of a legal size delivered
// byte for byte once the queue is drained -- and ends with exit code 0 and `ok ...` when the sanitizers saw nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/fmd.h"

void fmd_internal_set_err(const char*) {}                 // (the library's error text lives in fmd_api.cpp, which is not part of this build)

static std::mt19937_64 rng(20261020);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

static uint16_t crc16(const std::vector<uint8_t>& d)
{
    uint32_t crc = 0xFFFF;
    for (uint8_t b : d) {
        crc ^= b;
        for (int k = 0; k < 8; ++k) crc = (crc & 1u) ? (crc >> 1) ^ 0x8408u : crc >> 1;
    }
    return (uint16_t)(crc ^ 0xFFFFu);
}

static void flags(std::vector<int>& bits, int n)
{
    static const int f[8] = {0, 1, 1, 1, 1, 1, 1, 0};
    for (int i = 0; i < n; ++i) bits.insert(bits.end(), f, f + 8);
}

// flags, the frame with its FCS and stuffing, flags
static std::vector<int> frame_bits(std::vector<uint8_t> d, int lead, int tail)
{
    const uint16_t c = crc16(d);
    d.push_back((uint8_t)(c & 0xFF)); d.push_back((uint8_t)(c >> 8));
    std::vector<int> bits;
    flags(bits, lead);
    int ones = 0;
    for (uint8_t b : d)
        for (int k = 0; k < 8; ++k) {
            const int bit = (b >> k) & 1;
            bits.push_back(bit);
            ones = bit ? ones + 1 : 0;
            if (ones == 5) { bits.push_back(0); ones = 0; }
        }
    flags(bits, tail);
    return bits;
}

// NRZI and `spb_num / spb_den` soft samples per bit of amplitude `amp`
static void to_soft(const std::vector<int>& bits, uint32_t spb_num, uint32_t spb_den, int amp, int& level, std::vector<int16_t>& soft)
{
    uint64_t acc = 0;
    for (int b : bits) {
        if (!b) level = !level;
        acc += spb_num;
        while (acc >= spb_den) { acc -= spb_den; soft.push_back((int16_t)(level ? amp : -amp)); }
    }
}

struct Sink {
    std::vector<std::vector<uint8_t>> frames;
    uint64_t pushed = 0;
};

static int fail(const char* what) { fprintf(stderr, "ax25_fuzz: %s\n", what); return 1; }

// the stream in random call sizes and caps; everything delivered goes to `sink`
static int feed(fmd_ax25_decoder* d, const std::vector<int16_t>& soft, Sink& sink)
{
    fmd_ax25_frame out[16];
    static const size_t caps[3] = {0, 1, 16};
    for (size_t lo = 0; lo <= soft.size();) {
        size_t n = rnd(4) == 0 ? rnd(3) : rnd(5000);
        if (n > soft.size() - lo) n = soft.size() - lo;
        const size_t cap = caps[rnd(3)];
        size_t k = 99;
        memset(out, 0xA5, sizeof out);
        if (fmd_ax25_decoder_push(d, n ? soft.data() + lo : nullptr, n, cap ? out : nullptr, cap, &k) != FMD_OK) return fail("push failed");
        sink.pushed += n;
        if (k > cap) return fail("n_frames > cap");
        for (size_t i = 0; i < k; ++i) {
            if (out[i].len > 512 || out[i].len < 15) return fail("frame length out of bounds");
            if (out[i].end_sample >= sink.pushed) return fail("end_sample behind the stream");
            sink.frames.emplace_back(out[i].data, out[i].data + out[i].len);
        }
        lo += n;
        if (lo == soft.size() && n == 0) break;
        if (lo == soft.size() && rnd(2)) break;
    }
    return 0;
}

static int drain(fmd_ax25_decoder* d, Sink& sink)
{
    fmd_ax25_frame out[16];
    for (;;) {
        size_t k = 0;
        if (fmd_ax25_decoder_push(d, nullptr, 0, out, 16, &k) != FMD_OK) return fail("drain failed");
        for (size_t i = 0; i < k; ++i) {
            if (out[i].len > 512) return fail("frame length out of bounds");
            sink.frames.emplace_back(out[i].data, out[i].data + out[i].len);
        }
        if (k < 16) return 0;
    }
}

int main()
{
    uint64_t total_frames = 0, total_bad = 0, total_aborts = 0, intact = 0;
    // ---- 1. random streams -------------------------------------------------------------------------------------------------
    for (int round = 0; round < 24; ++round) {
        const uint32_t spb = 4 + rnd(61);
        fmd_ax25_decoder* d = nullptr;
        if (fmd_ax25_decoder_new(spb * 1200u, 1, 1200, &d) != FMD_OK || !d) return fail("new failed");
        std::vector<int16_t> soft;
        if (round % 2 == 0) {
            for (int i = 0; i < 200000; ++i) soft.push_back((int16_t)(rng() & 0xFFFF));
        } else {
            int level = 1;
            while (soft.size() < 200000) {
                const uint32_t run = 1 + rnd(rnd(2) ? 2 * spb : 8 * spb);
                for (uint32_t i = 0; i < run; ++i) soft.push_back((int16_t)(level ? 1 + rnd(32767) : -1 - (int)rnd(32768)));
                level = !level;
            }
        }
        Sink sink;
        if (feed(d, soft, sink) || drain(d, sink)) return 1;
        fmd_ax25_info info;
        if (fmd_ax25_decoder_info(d, &info) != FMD_OK) return fail("info failed");
        if (sink.frames.size() > info.frames_ok) return fail("delivered more than counted");
        total_frames += info.frames_ok; total_bad += info.bad_fcs; total_aborts += info.aborts;
        if (round % 5 == 0 && fmd_ax25_decoder_reset(d) != FMD_OK) return fail("reset failed");
        fmd_ax25_decoder_free(d);
    }
    // ---- 2. frames, intact and damaged ---------------------------------------------------------------------------------------
    for (int round = 0; round < 60; ++round) {
        const uint32_t spb_num = 4 + rnd(61), spb_den = 1 + (spb_num > 8 ? rnd(2) : 0);       // >= 4 samples per bit
        fmd_ax25_decoder* d = nullptr;
        if (fmd_ax25_decoder_new(spb_num * 1200u, spb_den, 1200, &d) != FMD_OK || !d) return fail("new failed");
        std::vector<int16_t> soft;
        std::vector<std::vector<uint8_t>> want;
        int level = 1;
        const int n_frames = 1 + (int)rnd(6);              // (few enough for the ring of 64 never to lose one)
        for (int f = 0; f < n_frames; ++f) {
            static const uint32_t sizes[8] = {0, 1, 14, 15, 512, 513, 700, 2000};
            const uint32_t len = rnd(3) == 0 ? sizes[rnd(8)] : 15 + rnd(200);
            std::vector<uint8_t> data(len);
            const int kind = (int)rnd(4);
            for (uint8_t& b : data) b = kind == 0 ? 0xFF : (uint8_t)rng();
            std::vector<int> bits = frame_bits(data, 4 + (int)rnd(40), 1 + (int)rnd(40));
            const int damage = (int)rnd(4);                  // 0: intact
            if (damage == 1) for (int i = 0, m = 1 + (int)rnd(4); i < m; ++i) bits[rnd((uint32_t)bits.size())] ^= 1;
            if (damage == 2) bits.resize(rnd((uint32_t)bits.size()));
            if (damage == 3) for (int i = 0, m = 8 + (int)rnd(30); i < m; ++i) bits.insert(bits.begin() + rnd((uint32_t)bits.size()), 1);
            to_soft(bits, spb_num, spb_den, 1 + (int)rnd(32767), level, soft);
            if (damage == 0 && len >= 15 && len <= 512) want.push_back(data);
            if (damage == 2) { std::vector<int> idle; flags(idle, 2); to_soft(idle, spb_num, spb_den, 1000, level, soft); }
        }
        Sink sink;
        if (feed(d, soft, sink) || drain(d, sink)) return 1;
        fmd_ax25_info info;
        if (fmd_ax25_decoder_info(d, &info) != FMD_OK) return fail("info failed");
        if (sink.frames.size() != info.frames_ok) return fail("delivered and counted differ");
        size_t at = 0;                                       // every intact frame, in order, among the delivered ones
        for (const std::vector<uint8_t>& w : want) {
            while (at < sink.frames.size() && sink.frames[at] != w) ++at;
            if (at == sink.frames.size()) return fail("an intact frame was not delivered");
            ++at; ++intact;
        }
        total_frames += info.frames_ok; total_bad += info.bad_fcs; total_aborts += info.aborts;
        fmd_ax25_decoder_free(d);
    }
    // ---- the arguments ---------------------------------------------------------------------------------------------------------
    fmd_ax25_decoder* d = nullptr;
    size_t k = 0;
    if (fmd_ax25_decoder_new(4799, 1, 1200, &d) != FMD_ERR_UNSUPPORTED || d) return fail("rate below 4 per bit accepted");
    if (fmd_ax25_decoder_new(76801, 1, 1200, &d) != FMD_ERR_UNSUPPORTED || d) return fail("rate above 64 per bit accepted");
    if (fmd_ax25_decoder_new(4800, 0, 1200, &d) != FMD_ERR_UNSUPPORTED || d) return fail("zero denominator accepted");
    // baud * rate_den = 2^62: four times and 64 times that are 0 in 64 bits (no push follows a refusal)
    if (fmd_ax25_decoder_new(0, 1u << 31, 1u << 31, &d) != FMD_ERR_UNSUPPORTED || d) return fail("a step of 2^62 against rate 0 accepted");
    if (fmd_ax25_decoder_new(1, 1u << 31, 1u << 31, &d) != FMD_ERR_UNSUPPORTED || d) return fail("a step of 2^62 against rate 1 accepted");
    if (fmd_ax25_decoder_new(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, &d) != FMD_ERR_UNSUPPORTED || d) return fail("the largest step accepted");
    if (fmd_ax25_decoder_new(0xFFFFFFFFu, 0xFFFFFFFFu / 4800u, 1200, &d) != FMD_OK || !d) return fail("the largest numbers refused");
    int16_t one = -5;
    if (fmd_ax25_decoder_push(d, &one, 1, nullptr, 0, &k) != FMD_OK || k != 0) return fail("push with cap 0 failed");
    if (fmd_ax25_decoder_push(d, nullptr, 1, nullptr, 0, &k) != FMD_ERR_INVALID_ARG) return fail("null soft accepted");
    fmd_ax25_decoder_free(d);
    fmd_ax25_decoder_free(nullptr);
    printf("ok frames %llu intact %llu bad_fcs %llu aborts %llu\n", (unsigned long long)total_frames, (unsigned long long)intact,
           (unsigned long long)total_bad, (unsigned long long)total_aborts);
    return intact > 0 ? 0 : fail("no intact frame was ever sent");
}
