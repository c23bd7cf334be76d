// fmd_ax25_decode.cpp -- the sequential half of packet reception, on the host (include/fmd.h, "AX.25 frame decoder"): one row's soft
// decisions from the tone-pair demodulator (fmd_afsk.hip, a few samples per bit) -> AX.25 frames.  No GPU, integers only, sample by
// sample, so the result does not depend on how the samples are cut into pushes (tests/ax25_ref.py restates it line for line).
//   1. clock: a phase accumulator that wraps once per bit; every sign change of the soft decision pulls it a quarter of the way to
//      the half-bit point, so the bits are taken half a bit after the changes;
//   2. NRZI: a bit is 1 when the level equals the level at the previous take;
//   3. HDLC: flags, bit un-stuffing, aborts; the frame's bits LSB first into a fixed buffer;
//   4. the FCS (CRC-16/X.25) over all but the last two bytes.
// This code parses whatever the air sends: every buffer is a fixed array and every write into one is bounded by its size.
// It needs nothing of the GPU side and no other file of the library but the header (tests/cpp/ax25_fuzz.cpp builds it alone).
#include "../../include/fmd.h"

#include <cstring>
#include <new>

void fmd_internal_set_err(const char* msg);

namespace {

constexpr uint32_t kMaxBytes = 514;                       // a frame with its FCS
constexpr uint32_t kMinBytes = 17;
constexpr uint32_t kMaxBits = kMaxBytes * 8 + 7;          // and the seven bits of the closing flag that arrive before it is known
constexpr uint32_t kQueue = 64;                           // frames held for a caller whose `frames` is full

uint16_t crc16_x25(const uint8_t* p, size_t n)
{
    uint32_t crc = 0xFFFF;
    for (size_t i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int k = 0; k < 8; ++k) crc = (crc & 1u) ? (crc >> 1) ^ 0x8408u : crc >> 1;
    }
    return (uint16_t)(crc ^ 0xFFFFu);
}

}  // namespace

struct fmd_ax25_decoder {
    int64_t mod = 0, step = 0, half = 0;
    int64_t ph = 0;
    int prev = 1, level = 1;
    uint32_t sr = 0, ones = 0, nbits = 0;
    bool in_frame = false;
    uint64_t n = 0;                                       // samples since creation or reset
    uint64_t frames_ok = 0, bad_fcs = 0, aborts = 0;
    uint8_t buf[kMaxBytes + 1];                           // kMaxBits bits
    fmd_ax25_frame queue[kQueue];                         // a ring: q_len frames from q_head on
    uint32_t q_head = 0, q_len = 0;
    // the caller's array during a push
    fmd_ax25_frame* dst = nullptr;
    size_t cap = 0, k = 0;

    void reset_state()
    {
        ph = 0; prev = 1; level = 1; sr = 0; ones = 0; nbits = 0; in_frame = false; n = 0;
        frames_ok = bad_fcs = aborts = 0;
        q_head = q_len = 0;
        memset(buf, 0, sizeof buf);
    }

    void drain()
    {
        while (k < cap && q_len) {
            dst[k++] = queue[q_head];
            q_head = (q_head + 1) % kQueue; --q_len;
        }
    }

    // straight into the caller's array while it has room and nothing waits in front; else into the ring, whose oldest frame gives
    // way when it is full
    fmd_ax25_frame* slot()
    {
        if (!q_len && k < cap) return &dst[k++];
        if (q_len == kQueue) { q_head = (q_head + 1) % kQueue; --q_len; }
        return &queue[(q_head + q_len++) % kQueue];
    }

    void close_frame()
    {
        if (nbits <= 7) return;                              // flags back to back
        const uint32_t nb = nbits - 7, bytes = nb / 8;
        if (nb % 8 == 0 && nbits <= kMaxBits && bytes >= kMinBytes && bytes <= kMaxBytes &&
            crc16_x25(buf, bytes - 2) == (uint16_t)(buf[bytes - 2] | buf[bytes - 1] << 8)) {
            ++frames_ok;
            fmd_ax25_frame* f = slot();
            memset(f, 0, sizeof *f);
            memcpy(f->data, buf, bytes - 2);                 // <= 512
            f->len = bytes - 2;
            f->end_sample = n;
            return;
        }
        ++bad_fcs;
    }

    void push_bit(uint32_t bit)
    {
        sr = (sr >> 1) | (bit << 7);
        if (sr == 0x7E) {
            if (in_frame) close_frame();
            in_frame = true; nbits = 0; ones = 0;
            return;
        }
        if (bit) {
            if (++ones >= 7) {
                if (in_frame) ++aborts;
                in_frame = false; ones = 7;
                return;
            }
        } else {
            const bool stuffed = ones == 5;
            ones = 0;
            if (stuffed) return;
        }
        if (!in_frame) return;
        if (nbits < kMaxBits) {
            uint8_t& b = buf[nbits >> 3];                    // nbits >> 3 <= kMaxBytes
            if ((nbits & 7u) == 0) b = 0;
            b = (uint8_t)(b | bit << (nbits & 7u));
        }
        if (nbits <= kMaxBits) ++nbits;                      // one past the limit marks a frame that is too long
    }

    void push_sample(int16_t v)
    {
        const int cur = v >= 0 ? 1 : 0;
        if (cur != prev) ph -= (ph - half) >> 2;
        prev = cur;
        ph += step;
        if (ph >= mod) {
            ph -= mod;
            push_bit(cur == level ? 1u : 0u);
            level = cur;
        }
        ++n;
    }
};

extern "C" {

int fmd_ax25_decoder_new(uint32_t rate_num, uint32_t rate_den, uint32_t baud, fmd_ax25_decoder** out)
{
    if (!out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *out = nullptr;
    const uint64_t mod = rate_num, step = (uint64_t)baud * rate_den;
    // step up to 2^64 - 2^33 + 1: `step > mod / 4` (the same as 4 step > mod in integers) comes first and bounds step by 2^30, so that
    // 64 * step cannot wrap
    if (step < 1 || step > mod / 4 || mod > 64 * step) { fmd_internal_set_err("need 4 <= rate / baud <= 64"); return FMD_ERR_UNSUPPORTED; }
    fmd_ax25_decoder* d = new (std::nothrow) fmd_ax25_decoder();
    if (!d) return FMD_ERR_NOMEM;
    d->mod = (int64_t)mod; d->step = (int64_t)step; d->half = (int64_t)(mod / 2);
    d->reset_state();
    *out = d;
    return FMD_OK;
}

void fmd_ax25_decoder_free(fmd_ax25_decoder* d) { delete d; }

int fmd_ax25_decoder_reset(fmd_ax25_decoder* d)
{
    if (!d) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    d->reset_state();
    return FMD_OK;
}

int fmd_ax25_decoder_push(fmd_ax25_decoder* d, const int16_t* soft, size_t n, fmd_ax25_frame* frames, size_t cap, size_t* n_frames)
{
    if (!d || !n_frames || (n && !soft) || (cap && !frames)) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    d->dst = frames; d->cap = cap; d->k = 0;
    d->drain();
    for (size_t i = 0; i < n; ++i) d->push_sample(soft[i]);
    *n_frames = d->k;
    d->dst = nullptr; d->cap = 0; d->k = 0;
    return FMD_OK;
}

int fmd_ax25_decoder_info(const fmd_ax25_decoder* d, fmd_ax25_info* info)
{
    if (!d || !info) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    info->frames_ok = d->frames_ok; info->bad_fcs = d->bad_fcs; info->aborts = d->aborts;
    info->in_frame = d->in_frame ? 1 : 0;
    return FMD_OK;
}

}  // extern "C"
