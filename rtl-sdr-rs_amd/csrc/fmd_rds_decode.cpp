// fmd_rds_decode.cpp -- the sequential half of RDS reception, on the host (include/fmd.h, "RDS decoder"): one station's complex
// baseband from the RDS bank (fmd_rds.hip, a few kHz) -> groups, PI, PS, RadioText.  No GPU, floating point, sample by sample, so
// the result does not depend on how the samples are cut into pushes.
//   1. matched filter: one cycle of a sine over a bit period -- the biphase symbol (two half-symbols of opposite sign) after the
//      transmitter's shaping; its output at the bit centre is the difference of the two halves;
//   2. carrier: second-order Costas loop on the filter output, error re im / mean power, natural frequency 20 Hz, damping 0.707
//      (pull-in of a +-20 Hz residual takes a few hundred samples); the loop frequency is clamped to +-40 Hz;
//   3. timing: |m|^2 has a line at the bit rate whose phase is the bit centre (square-law timing, feed-forward: no false lock on the
//      half-bit side peak of the biphase correlation); the line is averaged over 64 bits and the bit value is interpolated linearly
//      between the two samples around the centre;
//   4. differential decoding, 26-bit blocks, groups.
// The offset words and the generator are those of include/fmd.h; the check of a block is the remainder of its 26 bits by the
// generator, computed here -- for a block without errors that remainder IS the offset word, so no second table is typed in.
#include "../../include/fmd.h"

#include <cmath>
#include <cstring>
#include <deque>
#include <new>
#include <vector>

#include "fmd_host.h"

namespace {

constexpr double kBitRate = 1187.5;
constexpr uint32_t kPoly = 0x5B9;                          // x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
constexpr uint16_t kOffset[5] = {0x0FC, 0x198, 0x168, 0x1B4, 0x350};   // A, B, C, D, C'
constexpr int kBadRun = 10;                                // bad blocks in a row that drop the lock
constexpr double kTwoPi = 6.28318530717958647692528676655900577;

uint32_t remainder26(uint32_t v)
{
    for (int i = 25; i >= 10; --i)
        if (v >> i & 1u) v ^= kPoly << (i - 10);
    return v & 0x3FFu;
}

// position 0 ... 3 of the block whose remainder is `syn` (2 for C and C'), or -1
int position_of(uint32_t syn)
{
    for (int i = 0; i < 4; ++i)
        if (syn == kOffset[i]) return i;
    return syn == kOffset[4] ? 2 : -1;
}

}  // namespace

struct fmd_rds_decoder {
    double fs = 0, spb = 0;
    std::vector<double> w;                                 // matched filter, oldest sample first
    std::vector<double> hr, hi;                            // the last w.size() samples (ring)
    size_t hpos = 0;
    uint64_t n = 0;                                        // samples pushed since reset
    // carrier
    double phase = 0, freq = 0, alpha = 0, beta = 0, fmax = 0, pavg = 0;
    // timing
    double ph = 0, sr = 0, si = 0, theta_prev = 0, zprev = 0;
    uint64_t last_strobe = 0;
    bool have_strobe = false;
    // bits
    int prev_sym = 0;
    uint32_t reg = 0;
    uint64_t nbits = 0;
    uint64_t strobes[128] = {0};                           // sample index of bit (nbits - 1 - i) at [(nbits - 1 - i) & 127]
    // blocks
    bool synced = false;
    int pos = 0, bits_in_block = 0, bad_run = 0;
    // a valid block seen while searching, one per bit phase (nbits mod 26): a chance match between two true blocks must not
    // displace the first of them, or the lock would not be taken on two consecutive valid blocks
    struct Cand { uint64_t bit = 0; int pos = 0; uint16_t data = 0; bool have = false; };
    Cand cand[26];
    fmd_rds_group cur{};
    // groups
    std::deque<fmd_rds_group> queue;
    fmd_rds_info info{};
    char rtbuf[64] = {0};
    int rt_flag = -1;

    void reset_state()
    {
        std::fill(hr.begin(), hr.end(), 0.0); std::fill(hi.begin(), hi.end(), 0.0);
        hpos = 0; n = 0;
        phase = freq = pavg = 0;
        ph = sr = si = theta_prev = zprev = 0;
        last_strobe = 0; have_strobe = false;
        prev_sym = 0; reg = 0; nbits = 0;
        memset(strobes, 0, sizeof strobes);
        synced = false; pos = bits_in_block = bad_run = 0;
        drop_cands();
        cur = fmd_rds_group{};
        queue.clear();
        info = fmd_rds_info{};
        memset(info.ps, ' ', 8);
        memset(rtbuf, 0, sizeof rtbuf);
        rt_flag = -1;
    }

    void drop_cands() { for (Cand& c : cand) c = Cand{}; }

    uint64_t bit_sample(uint64_t bits_back) const         // sample index of the bit `bits_back` before the newest (0 if before the start)
    {
        if (bits_back >= nbits || bits_back >= 128) return 0;
        return strobes[(nbits - 1 - bits_back) & 127u];
    }

    void refresh_rt()
    {
        size_t i = 0;
        while (i < 64 && rtbuf[i] != 0 && rtbuf[i] != 0x0D) { info.rt[i] = rtbuf[i]; ++i; }
        info.rt[i] = 0;
    }

    void finish_group()
    {
        const uint8_t ok = cur.ok_mask;
        if (ok == 0x0F) ++info.groups_ok;
        if (ok & 1u) info.pi = cur.block[0];
        if (ok & 2u) {
            const uint16_t B = cur.block[1];
            const unsigned type = B >> 12, ver = B >> 11 & 1u;
            if (ver && (ok & 4u)) info.pi = cur.block[2];
            if (type == 0 && (ok & 8u)) {
                const unsigned a = B & 3u;
                info.ps[2 * a] = (char)(cur.block[3] >> 8); info.ps[2 * a + 1] = (char)(cur.block[3] & 0xFF);
            } else if (type == 2) {
                const int flag = B >> 4 & 1;
                if (rt_flag >= 0 && flag != rt_flag) memset(rtbuf, 0, sizeof rtbuf);
                rt_flag = flag;
                const unsigned a = B & 15u;
                if (!ver) {
                    if (ok & 4u) { rtbuf[4 * a] = (char)(cur.block[2] >> 8); rtbuf[4 * a + 1] = (char)(cur.block[2] & 0xFF); }
                    if (ok & 8u) { rtbuf[4 * a + 2] = (char)(cur.block[3] >> 8); rtbuf[4 * a + 3] = (char)(cur.block[3] & 0xFF); }
                } else if (ok & 8u) {
                    rtbuf[2 * a] = (char)(cur.block[3] >> 8); rtbuf[2 * a + 1] = (char)(cur.block[3] & 0xFF);
                }
                refresh_rt();
            }
        }
        queue.push_back(cur);
        cur = fmd_rds_group{};
    }

    void block_done(int p, bool ok, uint16_t data)
    {
        if (ok) { cur.block[p] = data; cur.ok_mask |= (uint8_t)(1u << p); }
        if (p == 3) finish_group();
    }

    void push_bit(int bit)
    {
        reg = (reg << 1 | (uint32_t)bit) & 0x3FFFFFFu;
        if (nbits < 26) return;                             // (nbits already counts this bit: the first 26 fill the register)
        const uint16_t data = (uint16_t)(reg >> 10);
        if (!synced) {
            const int p = position_of(remainder26(reg));
            if (p < 0) return;
            Cand& c = cand[nbits % 26u];
            if (c.have && nbits - c.bit == 26 && p == (c.pos + 1) % 4) {
                const int cand_pos = c.pos;
                const uint16_t cand_data = c.data;
                synced = true; bad_run = 0; bits_in_block = 0; drop_cands();
                cur = fmd_rds_group{};
                cur.first_sample = bit_sample(26u * (unsigned)(p + 1) - 1u);
                if (p == 0) {                               // D then A: the group that starts here
                    cur.first_sample = bit_sample(25);
                } else {
                    cur.block[cand_pos] = cand_data; cur.ok_mask |= (uint8_t)(1u << cand_pos);
                }
                block_done(p, true, data);
                pos = (p + 1) % 4;
                return;
            }
            c = Cand{nbits, p, data, true};
            return;
        }
        if (++bits_in_block < 26) return;
        bits_in_block = 0;
        if (pos == 0) cur.first_sample = bit_sample(25);
        const uint32_t syn = remainder26(reg);
        const bool ok = syn == kOffset[pos] || (pos == 2 && syn == kOffset[4]);
        if (ok) bad_run = 0;
        else { ++info.blocks_bad; ++bad_run; }
        block_done(pos, ok, data);
        pos = (pos + 1) % 4;
        if (bad_run >= kBadRun) { synced = false; drop_cands(); cur = fmd_rds_group{}; }
    }

    void push_sample(double xr, double xi)
    {
        const size_t L = w.size();
        hr[hpos] = xr; hi[hpos] = xi;
        hpos = (hpos + 1) % L;
        double mr = 0, mi = 0;                               // matched filter: w[j] meets the sample L - 1 - j back
        for (size_t j = 0, k = hpos; j < L; ++j) {
            mr += w[j] * hr[k]; mi += w[j] * hi[k];
            k = k + 1 == L ? 0 : k + 1;
        }
        const double e2 = mr * mr + mi * mi;
        // carrier
        const double ap = 1.0 / (8.0 * spb);
        pavg += (e2 - pavg) * (n < (uint64_t)(8.0 * spb) ? 1.0 / (double)(n + 1) : ap);
        const double c = std::cos(phase), s = std::sin(phase);
        const double zr = mr * c + mi * s, zi = mi * c - mr * s;
        double err = pavg > 0 ? zr * zi / pavg : 0.0;
        err = err > 1.0 ? 1.0 : (err < -1.0 ? -1.0 : err);
        freq += beta * err;
        freq = freq > fmax ? fmax : (freq < -fmax ? -fmax : freq);
        phase += freq + alpha * err;
        if (phase > kTwoPi) phase -= kTwoPi;
        else if (phase < -kTwoPi) phase += kTwoPi;
        // timing
        const double nw = 64.0 * spb;
        const double at = (double)(n + 1) < nw ? 1.0 / (double)(n + 1) : 1.0 / nw;
        const double a = kTwoPi * ph;
        sr += (e2 * std::cos(a) - sr) * at;
        si += (-e2 * std::sin(a) - si) * at;
        const double p0 = -std::atan2(si, sr) / kTwoPi;      // nominal phase at the bit centres
        double theta = ph - p0;
        theta -= std::floor(theta);
        if (n > 0 && theta < theta_prev - 0.5 && (!have_strobe || (double)(n - last_strobe) > 0.6 * spb)) {
            const double d0 = 1.0 - theta_prev, mu = d0 / (d0 + theta);
            const double v = zprev + mu * (zr - zprev);
            const int sym = v > 0 ? 1 : 0;
            const uint64_t centre = n - (mu < 0.5 ? 1 : 0);
            const uint64_t delay = (L - 1) / 2;
            strobes[nbits & 127u] = centre > delay ? centre - delay : 0;
            ++nbits;
            push_bit(sym ^ prev_sym);
            prev_sym = sym;
            last_strobe = n; have_strobe = true;
        }
        theta_prev = theta; zprev = zr;
        ph += 1.0 / spb;
        if (ph >= 1.0) ph -= 1.0;
        ++n;
    }
};

extern "C" {

int fmd_rds_decoder_new(uint32_t rate_num, uint32_t rate_den, fmd_rds_decoder** out)
{
    if (!out || rate_den == 0) { fmd_internal_set_err("null argument or zero denominator"); return FMD_ERR_INVALID_ARG; }
    *out = nullptr;
    const double fs = (double)rate_num / (double)rate_den;
    if (!(fs >= 4000.0 && fs <= 32000.0)) { fmd_internal_set_err("need 4 kHz <= sample rate <= 32 kHz"); return FMD_ERR_UNSUPPORTED; }
    fmd_rds_decoder* d = new (std::nothrow) fmd_rds_decoder();
    if (!d) return FMD_ERR_NOMEM;
    d->fs = fs; d->spb = fs / kBitRate;
    const size_t L = 2 * (size_t)(d->spb / 2.0) + 1;         // odd, <= one bit period
    d->w.resize(L); d->hr.resize(L); d->hi.resize(L);
    for (size_t j = 0; j < L; ++j) d->w[j] = -std::sin(kTwoPi * ((double)j - (double)(L - 1) / 2.0) / d->spb);
    const double wn = kTwoPi * 20.0 / fs, zeta = 0.70710678118654752;
    d->alpha = 2.0 * zeta * wn; d->beta = wn * wn; d->fmax = kTwoPi * 40.0 / fs;
    d->reset_state();
    *out = d;
    return FMD_OK;
}

void fmd_rds_decoder_free(fmd_rds_decoder* d) { delete d; }

int fmd_rds_decoder_reset(fmd_rds_decoder* d)
{
    if (!d) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    d->reset_state();
    return FMD_OK;
}

int fmd_rds_decoder_push(fmd_rds_decoder* d, const int16_t* iq, size_t n, fmd_rds_group* groups, size_t cap, size_t* n_groups)
{
    if (!d || !n_groups || (n && !iq) || (cap && !groups)) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    for (size_t i = 0; i < n; ++i) d->push_sample((double)iq[2 * i], (double)iq[2 * i + 1]);
    size_t k = 0;
    while (k < cap && !d->queue.empty()) { groups[k++] = d->queue.front(); d->queue.pop_front(); }
    *n_groups = k;
    return FMD_OK;
}

int fmd_rds_decoder_info(const fmd_rds_decoder* d, fmd_rds_info* info)
{
    if (!d || !info) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *info = d->info;
    info->ps[8] = 0;
    info->synced = d->synced ? 1 : 0;
    return FMD_OK;
}

}  // extern "C"
