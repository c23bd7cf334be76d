// demod.hpp -- C++ host-side mirror of the reference's interface for this path, over the C ABI.
//
// The reference is Rust (ccostes/rtl-sdr-rs v0.3.1); this image has no rustc, so the host side above
// include/fmd.h is C++ with the reference's names and argument meaning (examples/simple_fm.rs):
//   optimal_settings(freq, rate)              :189-214  -> std::pair<RadioConfig, DemodConfig>
//   Demod::new(config)                        :243-252  -> fm::Demod(config)
//   Demod::demodulate(&mut self, Vec<u8>)     :256-269  -> fm::Demod::demodulate(const std::vector<uint8_t>&)
//   output(Vec<i16>)                          :430-438  -> fm::output(const std::vector<int16_t>&, FILE*)
// Where the reference panics (len % 8, < 2 decimated samples, rate_out < rate_resample) these throw
// fm::Error carrying the fmd_status.  Header-only; link with libfmd_hip.so.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/fmd.h"

namespace fm {

using RadioConfig = fmd_radio_config;   // simple_fm.rs:173-176
using DemodConfig = fmd_demod_config;   // simple_fm.rs:179-185

constexpr size_t DEFAULT_BUF_LENGTH = FMD_DEFAULT_BUF_LENGTH;   // src/lib.rs:25

struct Error : std::runtime_error {
    int status;
    explicit Error(int s)
        : std::runtime_error(std::string(fmd_strerror(s)) + ": " + fmd_last_error()), status(s) {}
};

inline void check(int status) { if (status != FMD_OK) throw Error(status); }

// Owner of a C handle: `h.out()` receives it from fmd_*_new, the destructor gives it to `Free`; not copyable, and so is no class
// that holds one.
template <class T, void (*Free)(T*)>
class Owned {
public:
    Owned() = default;
    ~Owned() { Free(h_); }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    operator T*() const { return h_; }
    T** out() { return &h_; }

private:
    T* h_ = nullptr;
};

// Rows of a flat batch result [rows][cap][width]: row r is its first lens[r] (or, for every row, n) outputs of `width` int16 each.
using Rows = std::vector<std::vector<int16_t>>;

inline Rows cut_rows(const std::vector<int16_t>& flat, size_t rows, size_t cap, const std::vector<size_t>& lens, size_t width = 1)
{
    Rows res(rows);
    for (size_t r = 0; r < rows; ++r) res[r].assign(flat.begin() + width * r * cap, flat.begin() + width * (r * cap + lens[r]));
    return res;
}
inline Rows cut_rows(const std::vector<int16_t>& flat, size_t rows, size_t cap, size_t n, size_t width = 1)
{
    return cut_rows(flat, rows, cap, std::vector<size_t>(rows, n), width);
}

// What an fmd_* getter writes through its last argument: outputs() of the five down-converters, and the other one-value getters.
template <class R, class Fn, class... Args>
inline R value_of(Fn getter, const Args&... args)
{
    R r{};
    check(getter(args..., &r));
    return r;
}

// (present, level) of a pilot, (open, rms) of a squelch: the last completed block of one (stream, station)
template <class Fn, class H>
inline std::pair<bool, uint32_t> flag_and_level(Fn getter, const H& h, uint32_t stream, uint32_t station)
{
    int flag = 0;
    uint32_t level = 0;
    check(getter(h, stream, station, &flag, &level));
    return {flag != 0, level};
}

// sin(x) / x and point i of an n-point Hamming window, for the windowed-sinc designers below
namespace detail {
constexpr double pi = 3.14159265358979323846;
inline double sinc(double x) { return x == 0 ? 1.0 : std::sin(x) / x; }
inline double hamming(size_t i, size_t n) { return n > 1 ? 0.54 - 0.46 * std::cos(2 * pi * (double)i / (double)(n - 1)) : 1.0; }
}  // namespace detail

// optimal_settings(freq, rate), simple_fm.rs:189-214 (rate_resample = RATE_RESAMPLE, :27).
inline std::pair<RadioConfig, DemodConfig> optimal_settings(uint32_t freq, uint32_t rate, uint32_t rate_resample = 32000)
{
    RadioConfig r{};
    DemodConfig d{};
    check(fmd_optimal_settings(freq, rate, rate_resample, &r, &d));
    return {r, d};
}

// struct Demod + impl, simple_fm.rs:232-269: one IQ stream, state carried across calls.
class Demod {
public:
    explicit Demod(const DemodConfig& config, int device_id = -1) : config_(config)
    {
        fmd_device_config dev{1u, device_id, 0u};
        check(fmd_demod_new(&config_, &dev, h_.out()));
    }

    // demodulate(&mut self, buf: Vec<u8>) -> Vec<i16>
    std::vector<int16_t> demodulate(const std::vector<uint8_t>& buf) { return demodulate(buf.data(), buf.size()); }
    std::vector<int16_t> demodulate(const uint8_t* buf, size_t len)
    {
        std::vector<int16_t> out(fmd_out_cap(&config_, len) + 1);
        size_t n = 0;
        check(fmd_demod_demodulate(h_, buf, len, out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }

    fmd_demod_state state() { return value_of<fmd_demod_state>(fmd_demod_get_state, h_, 0u); }
    void set_state(const fmd_demod_state& s) { check(fmd_demod_set_state(h_, 0, &s)); }
    // treat every buffer as consecutive reference calls of block_bytes each (0 = off); see fmd_demod_set_block_len
    void set_block_len(size_t block_bytes) { check(fmd_demod_set_block_len(h_, block_bytes)); }
    const DemodConfig& config() const { return config_; }

private:
    DemodConfig config_;
    Owned<fmd_demod, fmd_demod_free> h_;
};

// n independent Demods on one GPU behind one handle (one `Demod` per stream, simple_fm.rs:137): `iq` holds
// n_channels equal-sized read_sync buffers back to back.
class DemodBank {
public:
    DemodBank(const DemodConfig& config, uint32_t n_channels, int device_id = -1) : config_(config), n_(n_channels)
    {
        fmd_device_config dev{n_channels, device_id, 0u};
        check(fmd_demod_new(&config_, &dev, h_.out()));
    }

    // out[c] = Demod::demodulate(channel c's buffer); `len` bytes per channel
    Rows demodulate(const uint8_t* iq, size_t len)
    {
        const size_t cap = fmd_out_cap(&config_, len) + 1;
        std::vector<int16_t> flat(cap * n_);
        std::vector<size_t> lens(n_);
        check(fmd_demod_demodulate_batch(h_, iq, len, flat.data(), cap, lens.data()));
        return cut_rows(flat, n_, cap, lens);
    }
    uint32_t channels() const { return n_; }
    const DemodConfig& config() const { return config_; }

private:
    DemodConfig config_;
    uint32_t n_;
    Owned<fmd_demod, fmd_demod_free> h_;
};

// The receive -> mpsc -> process -> output hand-off of the example (simple_fm.rs:55-60,114-127,150-156) with the GPU(s)
// as consumer: fmd_sink_* (new surface, see include/fmd.h).  `on_audio(seq, channel, samples, n)` is output() per
// channel, called in submission order from inside acquire() / drain() on the caller's thread.
class Sink {
public:
    using Callback = std::function<void(uint64_t seq, uint32_t channel, const int16_t* samples, size_t n)>;

    Sink(const DemodConfig& config, uint32_t n_channels, size_t nbytes, const std::vector<int32_t>& device_ids,
         uint32_t depth, Callback on_audio)
        : n_(n_channels), nbytes_(nbytes), cb_(std::move(on_audio))
    {
        check(fmd_sink_new(&config, n_channels, device_ids.data(), (uint32_t)device_ids.size(), nbytes, depth, &Sink::trampoline,
                           this, h_.out()));
    }

    // the next slot to fill: n_channels buffers of nbytes back to back (page-locked; read_sync writes straight into it)
    uint8_t* acquire() { uint8_t* p = nullptr; check(fmd_sink_acquire(h_, &p)); return p; }
    void submit() { check(fmd_sink_submit(h_)); }
    void release() { check(fmd_sink_release(h_)); }      // give the acquired slot back unsubmitted (short read, simple_fm.rs:122-125)
    void drain() { check(fmd_sink_drain(h_)); if (status_ != FMD_OK) throw Error(status_); }
    uint32_t channels() const { return n_; }
    size_t nbytes() const { return nbytes_; }

private:
    static void trampoline(void* user, uint64_t seq, const int16_t* audio, const size_t* out_len, size_t out_cap, int status)
    {
        Sink* self = static_cast<Sink*>(user);
        if (status != FMD_OK) { if (self->status_ == FMD_OK) self->status_ = status; return; }
        for (uint32_t c = 0; c < self->n_; ++c) self->cb_(seq, c, audio + (size_t)c * out_cap, out_len[c]);
    }
    uint32_t n_;
    size_t nbytes_;
    Callback cb_;
    int status_ = FMD_OK;
    Owned<fmd_sink, fmd_sink_free> h_;
};

// An rtl_tcp server (the reference's examples/rtl_tcp.rs) as the producer: `read_sync` has the shape of
// RtlSdr::read_sync (src/lib.rs:153) -- bytes written, fewer than asked = the stream ended ("samples lost",
// simple_fm.rs:122).  Wire format and opcodes: include/fmd.h, fmd_rtltcp_*.
class RtlTcpSource {
public:
    RtlTcpSource(const std::string& host, uint16_t port, uint32_t timeout_ms = 10000)
    {
        check(fmd_rtltcp_open(host.c_str(), port, timeout_ms, h_.out()));
        check(fmd_rtltcp_info(h_, &tuner_type_, &gain_count_));
    }

    size_t read_sync(uint8_t* buf, size_t nbytes) { size_t n = 0; check(fmd_rtltcp_read_sync(h_, buf, nbytes, &n)); return n; }
    void command(uint8_t opcode, uint32_t param) { check(fmd_rtltcp_command(h_, opcode, param)); }
    // config_sdr of the example (simple_fm.rs:217-229), by name
    void set_tuner_gain_auto() { command(FMD_RTLTCP_SET_GAIN_MODE, 0); }
    void set_bias_tee(bool on) { command(FMD_RTLTCP_SET_BIAS_TEE, on ? 1u : 0u); }
    void set_center_freq(uint32_t hz) { command(FMD_RTLTCP_SET_FREQUENCY, hz); }
    void set_sample_rate(uint32_t hz) { command(FMD_RTLTCP_SET_SAMPLE_RATE, hz); }
    uint32_t tuner_type() const { return tuner_type_; }
    uint32_t gain_count() const { return gain_count_; }

private:
    Owned<fmd_rtltcp, fmd_rtltcp_close> h_;
    uint32_t tuner_type_ = 0, gain_count_ = 0;
};

// Station bank (fmd_stations_*): `phase_incs` is [n_streams][n_stations]; demodulate() takes [n_streams][nbytes] and
// returns audio [n_streams * n_stations] (row stream * n_stations + station).
inline uint32_t phase_inc(int32_t offset_hz, uint32_t capture_rate)
{
    return value_of<uint32_t>(fmd_stations_phase_inc, offset_hz, capture_rate);
}

// The boxcar prototype (h = 1...1, n_taps = decim: the reference's own low_pass) has |W| <= 1, so sum(|Wr| + |Wi|) <= 2 decim and
// every |y| component stays within ceil(512 decim / 2^shift); the smallest shift that keeps it within `limit` (the Python
// stations_auto_shift(taps, phase_incs, limit) works from the taps' exact gain instead).
inline uint64_t boxcar_y_bound(uint32_t decim, uint32_t shift) { return (512ull * decim + (1ull << shift) - 1) >> shift; }
inline uint32_t boxcar_shift(uint32_t decim, uint64_t limit)
{
    uint32_t shift = 0;
    while (boxcar_y_bound(decim, shift) > limit) ++shift;
    return shift;
}

class StationBank {
public:
    StationBank(const std::vector<int16_t>& taps, uint32_t decim, uint32_t shift, const std::vector<uint32_t>& phase_incs,
                uint32_t n_streams, uint32_t rate_out, uint32_t rate_resample, int32_t device_id = -1)
        : decim_(decim), rate_out_(rate_out), rate_resample_(rate_resample), n_streams_(n_streams),
          n_stations_(n_streams ? (uint32_t)(phase_incs.size() / n_streams) : 0u)
    {
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_stations_new(taps.data(), (uint32_t)taps.size(), decim, shift, phase_incs.data(), n_stations_, rate_out,
                               rate_resample, &dev, h_.out()));
    }

    Rows demodulate(const uint8_t* iq, size_t nbytes)
    {
        const size_t cap = std::max<size_t>(1, fmd_stations_out_cap(decim_, rate_out_, rate_resample_, nbytes));
        const size_t rows = (size_t)n_streams_ * n_stations_;
        std::vector<int16_t> out(cap * rows);
        std::vector<size_t> lens(rows);
        check(fmd_stations_demodulate_batch(h_, iq, nbytes, out.data(), cap, lens.data()));
        return cut_rows(out, rows, cap, lens);
    }
    void reset() { check(fmd_stations_reset(h_)); }
    uint32_t n_stations() const { return n_stations_; }

private:
    uint32_t decim_, rate_out_, rate_resample_, n_streams_, n_stations_;
    Owned<fmd_stations, fmd_stations_free> h_;
};

// Channelizer (fmd_channelizer_*): `phase_incs` is [n_streams][n_stations]; run() takes [n_streams][nbytes] and returns
// interleaved (yr, yi) baseband [n_streams * n_stations] (row stream * n_stations + station).
class Channelizer {
public:
    Channelizer(const std::vector<int16_t>& taps, uint32_t decim, uint32_t shift, const std::vector<uint32_t>& phase_incs,
                uint32_t n_streams, int32_t device_id = -1)
        : decim_(decim), n_streams_(n_streams), n_stations_(n_streams ? (uint32_t)(phase_incs.size() / n_streams) : 0u)
    {
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_channelizer_new(taps.data(), (uint32_t)taps.size(), decim, shift, phase_incs.data(), n_stations_, &dev, h_.out()));
    }

    Rows run(const uint8_t* iq, size_t nbytes)
    {
        const size_t cap = std::max<size_t>(1, fmd_channelizer_out_cap(decim_, nbytes));
        const size_t rows = (size_t)n_streams_ * n_stations_;
        std::vector<int16_t> out(2 * cap * rows);
        size_t n = 0;
        check(fmd_channelizer_run_batch(h_, iq, nbytes, out.data(), cap, &n));
        return cut_rows(out, rows, cap, n, 2);
    }
    uint64_t outputs() const { return value_of<uint64_t>(fmd_channelizer_outputs, h_); }
    void reset() { check(fmd_channelizer_reset(h_)); }
    uint32_t n_stations() const { return n_stations_; }

private:
    uint32_t decim_, n_streams_, n_stations_;
    Owned<fmd_channelizer, fmd_channelizer_free> h_;
};

// Audio taps of a StereoBank, as the Python stereo_taps(): a Hamming-windowed sinc low-pass at cutoff_hz convolved with the
// sampled first-order de-emphasis response (tau_us 0: none), scaled to sum |g| <= 16383.
inline std::vector<int16_t> stereo_taps(double mpx_rate, uint32_t n_taps, double cutoff_hz = 15000, double tau_us = 75)
{
    if (n_taps < 1 || n_taps > 256) throw Error(FMD_ERR_INVALID_ARG);
    std::vector<double> d(1, 1.0);
    if (tau_us > 0) {
        const uint32_t nd = std::max<uint32_t>(1, n_taps / 2);
        const double a = std::exp(-1.0 / (tau_us * 1e-6 * mpx_rate));
        d.assign(nd, 0.0);
        for (uint32_t i = 0; i < nd; ++i) d[i] = (1 - a) * std::pow(a, (double)i);
    }
    const uint32_t nl = n_taps - (uint32_t)d.size() + 1;
    std::vector<double> lp(nl), g(n_taps, 0.0);
    const double fc = 2 * cutoff_hz / mpx_rate;
    for (uint32_t i = 0; i < nl; ++i) lp[i] = fc * detail::sinc(detail::pi * fc * (i - (nl - 1) / 2.0)) * detail::hamming(i, nl);
    for (uint32_t i = 0; i < nl; ++i)
        for (size_t j = 0; j < d.size(); ++j) g[i + j] += lp[i] * d[j];
    double sum = 0;
    for (double v : g) sum += std::fabs(v);
    std::vector<int16_t> out(n_taps);
    for (uint32_t i = 0; i < n_taps; ++i) out[i] = (int16_t)std::floor(g[i] / sum * (16383.0 - n_taps) + 0.5);
    return out;
}

// As the Python stereo.default_pilot_min(): a quarter of a nominal 6.75 kHz pilot at f_m = capture_rate / decim, in discriminator
// units (32768 f / f_m).
inline uint32_t default_pilot_min(uint32_t capture_rate, uint32_t decim)
{
    return (uint32_t)((32768ull * 6750 * decim) / (4ull * capture_rate));
}

// As the Python stereo.default_audio_shift(): the smallest shift (<= 16) at which mono at full deviation (75 kHz) stays inside
// int16, sum(g) 32768 75 kHz / f_m >> (shift + 1).
inline uint32_t default_audio_shift(const std::vector<int16_t>& audio_taps, uint32_t capture_rate, uint32_t decim)
{
    int64_t sum = 0;
    for (int16_t v : audio_taps) sum += v;
    const uint64_t peak = (uint64_t)(sum < 0 ? -sum : sum) * 32768ull * 75000ull * decim / capture_rate;
    uint32_t shift = 0;
    while (shift < 16 && (peak >> (shift + 1)) > 32767) ++shift;
    return shift;
}

// Stereo station bank (fmd_stereo_*): run() takes [n_streams][nbytes] and returns interleaved (L, R) audio
// [n_streams * n_stations] (row stream * n_stations + station) at capture_rate / (decim audio_decim).
class StereoBank {
public:
    StereoBank(const std::vector<int16_t>& taps, uint32_t decim, uint32_t shift, const std::vector<uint32_t>& phase_incs,
               uint32_t n_streams, const std::vector<int16_t>& audio_taps, const fmd_stereo_config& cfg, int32_t device_id = -1)
        : decim_(decim), audio_decim_(cfg.audio_decim), n_streams_(n_streams),
          n_stations_(n_streams ? (uint32_t)(phase_incs.size() / n_streams) : 0u)
    {
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_stereo_new(taps.data(), (uint32_t)taps.size(), decim, shift, phase_incs.data(), n_stations_, audio_taps.data(),
                             (uint32_t)audio_taps.size(), &cfg, &dev, h_.out()));
    }

    // FMD_ERR_TOO_SHORT (a call that completes no audio sample) returns empty rows and changes nothing.
    Rows run(const uint8_t* iq, size_t nbytes)
    {
        const size_t cap = std::max<size_t>(1, fmd_stereo_out_cap(decim_, audio_decim_, nbytes));
        const size_t rows = (size_t)n_streams_ * n_stations_;
        std::vector<int16_t> out(2 * cap * rows);
        size_t n = 0;
        const int rc = fmd_stereo_run_batch(h_, iq, nbytes, out.data(), cap, &n);
        if (rc == FMD_ERR_TOO_SHORT) return Rows(rows);
        check(rc);
        return cut_rows(out, rows, cap, n, 2);
    }
    std::pair<bool, uint32_t> pilot(uint32_t stream, uint32_t station) { return flag_and_level(fmd_stereo_pilot, h_, stream, station); }
    uint64_t outputs() const { return value_of<uint64_t>(fmd_stereo_outputs, h_); }
    void reset() { check(fmd_stereo_reset(h_)); }

private:
    uint32_t decim_, audio_decim_, n_streams_, n_stations_;
    Owned<fmd_stereo, fmd_stereo_free> h_;
};

// Taps of an RdsBank, as the Python rds_taps(): a Hamming-windowed sinc low-pass at +-cutoff_hz around the subcarrier, scaled to
// sum |g| <= 16383, and the smallest rds_shift at which the int16 store is exact.
inline std::pair<std::vector<int16_t>, uint32_t> rds_taps(double mpx_rate, uint32_t n_taps, double cutoff_hz = 2400)
{
    if (n_taps < 1 || n_taps > 256) throw Error(FMD_ERR_INVALID_ARG);
    const double fc = 2 * cutoff_hz / mpx_rate;
    std::vector<double> g(n_taps);
    double sum = 0;
    for (uint32_t i = 0; i < n_taps; ++i) {
        g[i] = fc * detail::sinc(detail::pi * fc * (i - (n_taps - 1) / 2.0)) * detail::hamming(i, n_taps);
        sum += std::fabs(g[i]);
    }
    std::vector<int16_t> out(n_taps);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_taps; ++i) {
        out[i] = (int16_t)std::floor(g[i] / sum * (16383.0 - n_taps) + 0.5);
        total += (uint64_t)std::abs((int)out[i]);
    }
    uint32_t shift = 0;
    while (((32768ull * total + (1ull << shift) - 1) >> shift) > 32767ull) ++shift;
    return {out, shift};
}

// A front-end prototype for an RdsBank where the boxcar would cut the 57 kHz subcarrier: a 64-tap Hamming-windowed sinc of +-62 kHz
// with peak 2047, and the front-end shift that keeps every |y| component <= 256 (where the reference's discriminator cannot wrap)
// with sum(|Wr| + |Wi|) <= 2 sum |h| + 2 n_taps (rounding).
inline std::pair<std::vector<int16_t>, uint32_t> rds_front_taps(uint32_t capture_rate)
{
    const double fc = 2.0 * 62000.0 / capture_rate;
    const double peak = detail::sinc(detail::pi * fc * 0.5) * detail::hamming(31, 64);
    std::vector<int16_t> h(64);
    uint64_t sum = 0;
    for (int i = 0; i < 64; ++i) {
        h[i] = (int16_t)std::lround(detail::sinc(detail::pi * fc * (i - 31.5)) * detail::hamming(i, 64) / peak * 2047.0);
        sum += (uint64_t)std::abs((int)h[i]);
    }
    uint32_t shift = 0;
    while ((256ull * (2 * sum + 128) + (1ull << shift) - 1) >> shift > 256ull) ++shift;
    return {h, shift};
}

// RDS bank (fmd_rds_*): run() takes [n_streams][nbytes] and returns interleaved (ur, ui) baseband
// [n_streams * n_stations] (row stream * n_stations + station) at capture_rate / (decim out_decim).
class RdsBank {
public:
    RdsBank(const std::vector<int16_t>& taps, uint32_t decim, uint32_t shift, const std::vector<uint32_t>& phase_incs,
            uint32_t n_streams, const std::vector<int16_t>& rds_taps, const fmd_rds_config& cfg, int32_t device_id = -1)
        : decim_(decim), out_decim_(cfg.out_decim), n_streams_(n_streams),
          n_stations_(n_streams ? (uint32_t)(phase_incs.size() / n_streams) : 0u)
    {
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_rds_new(taps.data(), (uint32_t)taps.size(), decim, shift, phase_incs.data(), n_stations_, rds_taps.data(),
                          (uint32_t)rds_taps.size(), &cfg, &dev, h_.out()));
    }

    // FMD_ERR_TOO_SHORT (a call that completes no output) returns empty rows and changes nothing.
    Rows run(const uint8_t* iq, size_t nbytes)
    {
        const size_t cap = std::max<size_t>(1, fmd_rds_out_cap(decim_, out_decim_, nbytes));
        const size_t rows = (size_t)n_streams_ * n_stations_;
        std::vector<int16_t> out(2 * cap * rows);
        size_t n = 0;
        const int rc = fmd_rds_run_batch(h_, iq, nbytes, out.data(), cap, &n);
        if (rc == FMD_ERR_TOO_SHORT) return Rows(rows);
        check(rc);
        return cut_rows(out, rows, cap, n, 2);
    }
    std::pair<bool, uint32_t> pilot(uint32_t stream, uint32_t station) { return flag_and_level(fmd_rds_pilot, h_, stream, station); }
    uint64_t outputs() const { return value_of<uint64_t>(fmd_rds_outputs, h_); }
    void reset() { check(fmd_rds_reset(h_)); }

private:
    uint32_t decim_, out_decim_, n_streams_, n_stations_;
    Owned<fmd_rds, fmd_rds_free> h_;
};

// RDS decoder of one (stream, station) (fmd_rds_decoder_*, host only): push() takes interleaved (ur, ui) pairs at rate_num / rate_den
// Hz and returns the groups completed since.
class RdsDecoder {
public:
    RdsDecoder(uint32_t rate_num, uint32_t rate_den) { check(fmd_rds_decoder_new(rate_num, rate_den, h_.out())); }

    std::vector<fmd_rds_group> push(const std::vector<int16_t>& iq)
    {
        std::vector<fmd_rds_group> res;
        fmd_rds_group buf[64];
        size_t n = 0;
        check(fmd_rds_decoder_push(h_, iq.data(), iq.size() / 2, buf, 64, &n));
        for (;;) {
            res.insert(res.end(), buf, buf + n);
            if (n < 64) return res;
            check(fmd_rds_decoder_push(h_, nullptr, 0, buf, 64, &n));
        }
    }
    fmd_rds_info info() const { return value_of<fmd_rds_info>(fmd_rds_decoder_info, h_); }
    void reset() { check(fmd_rds_decoder_reset(h_)); }

private:
    Owned<fmd_rds_decoder, fmd_rds_decoder_free> h_;
};

// FM receiver bank (fmd_receiver_*): a StereoBank and an RdsBank over the same stations out of one multiplex pass.  run() takes
// [n_streams][nbytes] and returns (audio, rds): the interleaved (L, R) audio and the interleaved (ur, ui) baseband, each
// [n_streams * n_stations] (row stream * n_stations + station), bit for bit what the two banks return.
class ReceiverBank {
public:
    ReceiverBank(const std::vector<int16_t>& taps, uint32_t decim, uint32_t shift, const std::vector<uint32_t>& phase_incs,
                 uint32_t n_streams, const std::vector<int16_t>& audio_taps, const std::vector<int16_t>& rds_taps,
                 const fmd_receiver_config& cfg, int32_t device_id = -1)
        : decim_(decim), audio_decim_(cfg.audio_decim), rds_decim_(cfg.rds_decim), n_streams_(n_streams),
          n_stations_(n_streams ? (uint32_t)(phase_incs.size() / n_streams) : 0u)
    {
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_receiver_new(taps.data(), (uint32_t)taps.size(), decim, shift, phase_incs.data(), n_stations_, audio_taps.data(),
                               (uint32_t)audio_taps.size(), rds_taps.data(), (uint32_t)rds_taps.size(), &cfg, &dev, h_.out()));
    }

    // FMD_ERR_TOO_SHORT (a call that does not complete an output of each stage) returns empty rows and changes nothing.
    std::pair<Rows, Rows> run(const uint8_t* iq, size_t nbytes)
    {
        const size_t ca = std::max<size_t>(1, fmd_stereo_out_cap(decim_, audio_decim_, nbytes));
        const size_t cr = std::max<size_t>(1, fmd_rds_out_cap(decim_, rds_decim_, nbytes));
        const size_t rows = (size_t)n_streams_ * n_stations_;
        std::vector<int16_t> audio(2 * ca * rows), rds(2 * cr * rows);
        size_t na = 0, nr = 0;
        const int rc = fmd_receiver_run_batch(h_, iq, nbytes, audio.data(), ca, &na, rds.data(), cr, &nr);
        if (rc == FMD_ERR_TOO_SHORT) return {Rows(rows), Rows(rows)};
        check(rc);
        return {cut_rows(audio, rows, ca, na, 2), cut_rows(rds, rows, cr, nr, 2)};
    }
    std::pair<bool, uint32_t> pilot(uint32_t stream, uint32_t station) { return flag_and_level(fmd_receiver_pilot, h_, stream, station); }
    // (audio samples, baseband samples) per row since creation or reset
    std::pair<uint64_t, uint64_t> outputs() const
    {
        uint64_t a = 0, r = 0;
        check(fmd_receiver_outputs(h_, &a, &r));
        return {a, r};
    }
    void reset() { check(fmd_receiver_reset(h_)); }

private:
    uint32_t decim_, audio_decim_, rds_decim_, n_streams_, n_stations_;
    Owned<fmd_receiver, fmd_receiver_free> h_;
};

// Channel taps of a NarrowBank, as the Python narrow_taps(): a Hamming-windowed complex band-pass from lo_hz to hi_hz at the
// channelizer's output rate, scaled to sum |gr| + |gi| <= 65535 with every tap within 16383.  The second vector is empty (real
// taps) when lo_hz == -hi_hz.  USB is e.g. (300, 3000), LSB (-3000, -300).
inline std::pair<std::vector<int16_t>, std::vector<int16_t>> narrow_taps(double rate, uint32_t n_taps, double lo_hz, double hi_hz)
{
    if (n_taps < 1 || n_taps > 256 || !(hi_hz > lo_hz)) throw Error(FMD_ERR_INVALID_ARG);
    const double pi = detail::pi;
    const uint32_t n = n_taps;
    const double bw = (hi_hz - lo_hz) / rate, fc = (hi_hz + lo_hz) / (2 * rate);
    const bool real = lo_hz == -hi_hz;
    std::vector<double> re(n), im(n, 0.0);
    double total = 0, peak = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const double t = i - (n - 1) / 2.0, x = pi * (bw * t);
        const double w = n > 1 ? 0.54 + 0.46 * std::cos(pi * (2.0 * i + 1.0 - n) / (n - 1.0)) : 1.0;
        const double lp = bw * detail::sinc(x) * w;
        if (real) re[i] = lp;
        else {
            const double ph = 2 * pi * fc * t;          // the correlation sum_t g[t] y[R n + t] passes +fc with g = lp exp(-j ph)
            re[i] = lp * std::cos(ph);
            im[i] = -(lp * std::sin(ph));
        }
        total += std::fabs(re[i]) + std::fabs(im[i]);
        peak = std::max(peak, std::max(std::fabs(re[i]), std::fabs(im[i])));
    }
    const double scale = std::min((65535.0 - 2.0 * n) / total, 16383.0 / peak);
    std::vector<int16_t> gr(n), gi(real ? 0 : n);
    for (uint32_t i = 0; i < n; ++i) {
        gr[i] = (int16_t)std::floor(re[i] * scale + 0.5);
        if (!real) gi[i] = (int16_t)std::floor(im[i] * scale + 0.5);
    }
    return {gr, gi};
}

// As the Python narrow_auto_shift(): the smallest chan_shift (<= 30) that keeps every |u| component <= limit -- 256 in FM mode
// (where the reference's discriminator cannot wrap), 16384 otherwise -- for a front end whose |y| components stay within y_bound.
inline uint32_t narrow_chan_shift(uint64_t y_bound, const std::vector<int16_t>& chan_taps_re, const std::vector<int16_t>& chan_taps_im,
                                  uint64_t limit)
{
    uint64_t sum = 0;
    for (int16_t v : chan_taps_re) sum += (uint64_t)std::abs((int)v);
    for (int16_t v : chan_taps_im) sum += (uint64_t)std::abs((int)v);
    const uint64_t peak = y_bound * sum;
    uint32_t shift = 0;
    while (shift < 30 && ((peak + (1ull << shift) - 1) >> shift) > limit) ++shift;
    return shift;
}

// Narrow-band bank (fmd_narrow_*): run() takes [n_streams][nbytes] and returns [n_streams * n_stations] rows (row stream *
// n_stations + station) of int16 audio -- interleaved (re, im) in IQ mode -- at capture_rate / (decim chan_decim).
class NarrowBank {
public:
    NarrowBank(const std::vector<int16_t>& taps, uint32_t decim, uint32_t shift, const std::vector<uint32_t>& phase_incs,
               uint32_t n_streams, const std::vector<int16_t>& chan_taps_re, const std::vector<int16_t>& chan_taps_im,
               const fmd_narrow_config& cfg, int32_t device_id = -1)
        : decim_(decim), chan_decim_(cfg.chan_decim), width_(fmd_narrow_out_width(cfg.mode)), n_streams_(n_streams),
          n_stations_(n_streams ? (uint32_t)(phase_incs.size() / n_streams) : 0u)
    {
        if (!chan_taps_im.empty() && chan_taps_im.size() != chan_taps_re.size()) throw Error(FMD_ERR_INVALID_ARG);
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_narrow_new(taps.data(), (uint32_t)taps.size(), decim, shift, phase_incs.data(), n_stations_, chan_taps_re.data(),
                             chan_taps_im.empty() ? nullptr : chan_taps_im.data(), (uint32_t)chan_taps_re.size(), &cfg, &dev, h_.out()));
    }

    // FMD_ERR_TOO_SHORT (a call that completes no audio sample) returns empty rows and changes nothing.
    Rows run(const uint8_t* iq, size_t nbytes)
    {
        const size_t cap = std::max<size_t>(1, fmd_narrow_out_cap(decim_, chan_decim_, nbytes));
        const size_t rows = (size_t)n_streams_ * n_stations_;
        std::vector<int16_t> out(width_ * cap * rows);
        size_t n = 0;
        const int rc = fmd_narrow_run_batch(h_, iq, nbytes, out.data(), cap, &n);
        if (rc == FMD_ERR_TOO_SHORT) return Rows(rows);
        check(rc);
        return cut_rows(out, rows, cap, n, width_);
    }
    std::pair<bool, uint32_t> level(uint32_t stream, uint32_t station) { return flag_and_level(fmd_narrow_level, h_, stream, station); }
    uint64_t outputs() const { return value_of<uint64_t>(fmd_narrow_outputs, h_); }
    void reset() { check(fmd_narrow_reset(h_)); }

private:
    uint32_t decim_, chan_decim_, width_, n_streams_, n_stations_;
    Owned<fmd_narrow, fmd_narrow_free> h_;
};

// Power spectrum (fmd_spectrum_*): power() takes [n_streams][nbytes] and returns u64 [n_streams][n_bins] in natural DFT order.
inline std::vector<int16_t> hann_window(uint32_t n_bins, uint32_t amplitude = 2047)
{
    std::vector<int16_t> w(n_bins);
    check(fmd_spectrum_hann(n_bins, amplitude, w.data()));
    return w;
}

class Spectrum {
public:
    Spectrum(const std::vector<int16_t>& window, uint32_t hop, uint32_t shift, uint32_t n_streams = 1, int32_t device_id = -1)
        : n_bins_((uint32_t)window.size()), n_streams_(n_streams)
    {
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_spectrum_new(window.data(), n_bins_, hop, shift, &dev, h_.out()));
    }

    std::vector<uint64_t> power(const uint8_t* iq, size_t nbytes)
    {
        std::vector<uint64_t> p((size_t)n_streams_ * n_bins_);
        check(fmd_spectrum_power_batch(h_, iq, nbytes, p.data()));
        return p;
    }
    uint32_t bin_inc(uint32_t bin) const { return value_of<uint32_t>(fmd_spectrum_bin_inc, bin, n_bins_); }
    // offset of bin k from the capture's centre, in Hz
    double bin_offset_hz(uint32_t k, double capture_rate) const
    {
        return (k < n_bins_ / 2 ? (double)k : (double)k - n_bins_) * capture_rate / n_bins_;
    }
    uint32_t n_bins() const { return n_bins_; }

private:
    uint32_t n_bins_, n_streams_;
    Owned<fmd_spectrum, fmd_spectrum_free> h_;
};

// Uniform channelizer (fmd_uniform_*).  The prototype, as the Python uniform_taps(): h[t] = floor(amplitude s[t] / max|s| + 1/2),
// s[t] = sinc((t - (T - 1) / 2) / N) hamming(T), T = N taps_per_channel.
inline std::vector<int16_t> uniform_taps(uint32_t n_channels, uint32_t taps_per_channel, uint32_t amplitude = 2047)
{
    const size_t T = (size_t)n_channels * taps_per_channel;
    std::vector<double> s(T);
    double peak = 0;
    for (size_t t = 0; t < T; ++t) {
        s[t] = detail::sinc(detail::pi * (((double)t - ((double)T - 1) / 2.0) / n_channels)) * detail::hamming(t, T);
        peak = std::max(peak, std::fabs(s[t]));
    }
    std::vector<int16_t> h(T);
    for (size_t t = 0; t < T; ++t) h[t] = (int16_t)std::floor(amplitude * s[t] / peak + 0.5);
    return h;
}

inline uint32_t uniform_channel_inc(uint32_t channel, uint32_t n_channels)
{
    return value_of<uint32_t>(fmd_uniform_channel_inc, channel, n_channels);
}

// The smallest shift with ceil(256 G / 2^shift) <= 16384, G = max over `channels` (empty: all) of sum_t |Wr| + |Wi|.
inline uint32_t uniform_auto_shift(const std::vector<int16_t>& taps, uint32_t n_channels, const std::vector<uint32_t>& channels = {})
{
    int16_t tab[1024];
    check(fmd_stations_nco_table(tab));
    uint64_t gain = 0;
    const size_t rows = channels.empty() ? n_channels : channels.size();
    for (size_t i = 0; i < rows; ++i) {
        const uint32_t inc = uniform_channel_inc(channels.empty() ? (uint32_t)i : channels[i], n_channels);
        uint64_t g = 0;
        for (size_t t = 0; t < taps.size(); ++t) {
            const uint32_t ix = ((uint32_t)t * inc) >> 22;
            const int32_t wr = (taps[t] * tab[ix] + 8192) >> 14, wi = (-taps[t] * tab[(ix - 256u) & 1023u] + 8192) >> 14;
            g += (uint64_t)std::abs(wr) + (uint64_t)std::abs(wi);
        }
        gain = std::max(gain, g);
    }
    uint32_t shift = 0;
    while (((256 * gain + ((1ull << shift) - 1)) >> shift) > 16384) ++shift;
    return shift;
}

// run() takes [n_streams][nbytes] (whole hops) and returns interleaved (yr, yi) baseband, row stream * n_selected + selected channel.
class UniformChannelizer {
public:
    // `channels` empty: all n_channels
    UniformChannelizer(const std::vector<int16_t>& taps, uint32_t n_channels, uint32_t hop, uint32_t shift,
                       const std::vector<uint32_t>& channels = {}, uint32_t n_streams = 1, int32_t device_id = -1)
        : hop_(hop), n_streams_(n_streams), n_selected_(channels.empty() ? n_channels : (uint32_t)channels.size())
    {
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_uniform_new(taps.data(), (uint32_t)taps.size(), n_channels, hop, shift, channels.empty() ? nullptr : channels.data(),
                              n_selected_, &dev, h_.out()));
    }

    Rows run(const uint8_t* iq, size_t nbytes)
    {
        const size_t cap = std::max<size_t>(1, fmd_uniform_out_cap(hop_, nbytes));
        const size_t rows = (size_t)n_streams_ * n_selected_;
        std::vector<int16_t> out(2 * cap * rows);
        size_t n = 0;
        check(fmd_uniform_run_batch(h_, iq, nbytes, out.data(), cap, &n));
        return cut_rows(out, rows, cap, n, 2);
    }
    uint64_t outputs() const { return value_of<uint64_t>(fmd_uniform_outputs, h_); }
    void reset() { check(fmd_uniform_reset(h_)); }
    int tap_digits() const { return fmd_uniform_tap_digits(h_); }
    uint32_t n_selected() const { return n_selected_; }

private:
    uint32_t hop_, n_streams_, n_selected_;
    Owned<fmd_uniform, fmd_uniform_free> h_;
};

// B_y of the uniform channelizer at `shift`: ceil(256 G / 2^shift), G = max over `channels` (empty: all) of sum_t |Wr| + |Wi|.
inline uint64_t uniform_y_bound(const std::vector<int16_t>& taps, uint32_t n_channels, uint32_t shift, const std::vector<uint32_t>& channels = {})
{
    int16_t tab[1024];
    check(fmd_stations_nco_table(tab));
    uint64_t gain = 0;
    const size_t rows = channels.empty() ? n_channels : channels.size();
    for (size_t i = 0; i < rows; ++i) {
        const uint32_t inc = uniform_channel_inc(channels.empty() ? (uint32_t)i : channels[i], n_channels);
        uint64_t g = 0;
        for (size_t t = 0; t < taps.size(); ++t) {
            const uint32_t ix = ((uint32_t)t * inc) >> 22;
            const int32_t wr = (taps[t] * tab[ix] + 8192) >> 14, wi = (-taps[t] * tab[(ix - 256u) & 1023u] + 8192) >> 14;
            g += (uint64_t)std::abs(wr) + (uint64_t)std::abs(wi);
        }
        gain = std::max(gain, g);
    }
    return (256 * gain + ((1ull << shift) - 1)) >> shift;
}

// Band-plan bank (fmd_bandplan_*): run() takes [n_streams][nbytes] (whole hops) and returns [n_streams * n_selected] rows (row
// stream * n_selected + selected channel) of int16 audio -- interleaved (re, im) in IQ mode -- at capture_rate / (hop chan_decim);
// levels() is the activity map of the last completed block, one (open, rms) per row.
class BandPlanBank {
public:
    // `channels` empty: all n_channels
    BandPlanBank(const std::vector<int16_t>& taps, uint32_t n_channels, uint32_t hop, uint32_t shift, const std::vector<uint32_t>& channels,
                 uint32_t n_streams, const std::vector<int16_t>& chan_taps_re, const std::vector<int16_t>& chan_taps_im,
                 const fmd_narrow_config& cfg, int32_t device_id = -1)
        : hop_(hop), chan_decim_(cfg.chan_decim), width_(fmd_narrow_out_width(cfg.mode)), n_streams_(n_streams),
          n_selected_(channels.empty() ? n_channels : (uint32_t)channels.size())
    {
        if (!chan_taps_im.empty() && chan_taps_im.size() != chan_taps_re.size()) throw Error(FMD_ERR_INVALID_ARG);
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_bandplan_new(taps.data(), (uint32_t)taps.size(), n_channels, hop, shift, channels.empty() ? nullptr : channels.data(),
                               n_selected_, chan_taps_re.data(), chan_taps_im.empty() ? nullptr : chan_taps_im.data(),
                               (uint32_t)chan_taps_re.size(), &cfg, &dev, h_.out()));
    }

    // FMD_ERR_TOO_SHORT (a call that completes no audio sample) returns empty rows and changes nothing.
    Rows run(const uint8_t* iq, size_t nbytes)
    {
        const size_t cap = std::max<size_t>(1, fmd_bandplan_out_cap(hop_, chan_decim_, nbytes));
        const size_t rows = (size_t)n_streams_ * n_selected_;
        std::vector<int16_t> out(width_ * cap * rows);
        size_t n = 0;
        const int rc = fmd_bandplan_run_batch(h_, iq, nbytes, out.data(), cap, &n);
        if (rc == FMD_ERR_TOO_SHORT) return Rows(rows);
        check(rc);
        return cut_rows(out, rows, cap, n, width_);
    }
    std::vector<std::pair<bool, uint32_t>> levels()
    {
        const size_t rows = (size_t)n_streams_ * n_selected_;
        std::vector<uint8_t> open(rows);
        std::vector<uint32_t> rms(rows);
        check(fmd_bandplan_levels(h_, open.data(), rms.data()));
        std::vector<std::pair<bool, uint32_t>> res(rows);
        for (size_t r = 0; r < rows; ++r) res[r] = {open[r] != 0, rms[r]};
        return res;
    }
    uint64_t outputs() const { return value_of<uint64_t>(fmd_bandplan_outputs, h_); }
    void reset() { check(fmd_bandplan_reset(h_)); }
    uint32_t n_selected() const { return n_selected_; }
    uint32_t width() const { return width_; }

private:
    uint32_t hop_, chan_decim_, width_, n_streams_, n_selected_;
    Owned<fmd_bandplan, fmd_bandplan_free> h_;
};

// As the Python resample_ratio(): (L, M) with L / M = rate_out rate_in_den / rate_in_num in lowest terms.
inline std::pair<uint32_t, uint32_t> resample_ratio(uint64_t rate_in_num, uint64_t rate_in_den, uint64_t rate_out)
{
    uint32_t L = 0, M = 0;
    check(fmd_resample_ratio(rate_in_num, rate_in_den, rate_out, &L, &M));
    return {L, M};
}

// Polyphase taps of a Resampler, tap for tap the Python resample_taps(): a Hamming-windowed sinc of L T points at cutoff / max(L, M)
// cycles per upsampled sample; g[p][t] takes prototype point L (T - 1 - t) + p; every phase is scaled to the sum 2^shift, rounded to
// nearest, and the rounding's remainder goes to the first of its largest taps; shift is the largest value <= 14 at which every
// phase has sum |g| <= 32767.  Phase-major [L][T].
inline std::pair<std::vector<int16_t>, uint32_t> resample_taps(uint32_t L, uint32_t M, uint32_t T, double cutoff = 0.45)
{
    if (L < 1 || M < 1 || T < 1) throw Error(FMD_ERR_INVALID_ARG);
    const size_t n = (size_t)L * T;
    const double fc = cutoff / (double)std::max(L, M);
    std::vector<double> h(n);
    for (size_t i = 0; i < n; ++i) {
        const double x = 2 * detail::pi * fc * ((double)i - (double)(n - 1) / 2.0);
        h[i] = detail::sinc(x) * detail::hamming(i, n);
    }
    std::vector<int16_t> g(n);
    std::vector<int64_t> row(T);
    for (int shift = 14; shift >= 0; --shift) {
        bool ok = true;
        for (uint32_t p = 0; p < L && ok; ++p) {
            double s = 0;
            for (uint32_t t = 0; t < T; ++t) s += h[(size_t)L * (T - 1 - t) + p];
            if (!(s > 0)) throw Error(FMD_ERR_INVALID_ARG);
            const double scale = std::ldexp(1.0, shift) / s;
            int64_t sum = 0;
            uint32_t big = 0;
            for (uint32_t t = 0; t < T; ++t) {
                row[t] = (int64_t)std::floor(h[(size_t)L * (T - 1 - t) + p] * scale + 0.5);
                sum += row[t];
                if (row[t] > row[big]) big = t;
            }
            row[big] += ((int64_t)1 << shift) - sum;
            int64_t mag = 0;
            for (uint32_t t = 0; t < T; ++t) mag += row[t] < 0 ? -row[t] : row[t];
            if (mag > 32767) { ok = false; break; }
            for (uint32_t t = 0; t < T; ++t) g[(size_t)p * T + t] = (int16_t)row[t];
        }
        if (ok) return {g, (uint32_t)shift};
    }
    throw Error(FMD_ERR_UNSUPPORTED);
}

// Base of the row processors (fmd_resample_*, fmd_agc_*, fmd_tonesq_*): owns the handle H of `n_rows` rows of `width` int16 per sample and runs it
// through its `_run_batch`, `_outputs` and `_reset` entry points.
template <class H, void (*Free)(H*), auto RunBatch, auto Outputs, auto Reset>
class RowProcessor {
public:
    // (inputs, outputs) per row since creation or reset
    std::pair<uint64_t, uint64_t> counts() const
    {
        uint64_t i = 0, o = 0;
        check(Outputs(h_, &i, &o));
        return {i, o};
    }
    void reset() { check(Reset(h_)); }

protected:
    RowProcessor(uint32_t n_rows, uint32_t width) : n_rows_(n_rows), width_(width) {}

    // [n_rows][n_in][width] through the handle into room for `cap` outputs per row: the call's outputs per row, interleaved by
    // `width`.  The status `empty` (FMD_OK: none) returns empty rows instead of throwing.
    Rows run_rows(const int16_t* x, size_t n_in, size_t cap, int empty = FMD_OK)
    {
        cap = std::max<size_t>(1, cap);
        std::vector<int16_t> out(width_ * cap * n_rows_);
        size_t n = 0;
        const int rc = RunBatch(h_, x, n_in, n_in, out.data(), cap, &n);
        if (rc != FMD_OK && rc == empty) return Rows(n_rows_);
        check(rc);
        return cut_rows(out, n_rows_, cap, n, width_);
    }

    uint32_t n_rows_, width_;
    Owned<H, Free> h_;
};

// Base of the record banks (fmd_hdlc_*, fmd_pager_*): owns the handle H of `n_rows` rows that leave up to `cap` records Rec per row
// and call.  Behind a run: counts() per row, records(rows) the first min(count, cap) of each listed row in the order they closed,
// info() the rows' cumulative counters.
template <class H, void (*Free)(H*), class Rec, class Info, auto Counts, auto Records, auto InfoOf, auto Inputs, auto Reset>
class RecordBank {
public:
    std::vector<uint32_t> counts()
    {
        std::vector<uint32_t> c(n_rows_);
        check(Counts(h_, c.data()));
        return c;
    }
    std::vector<Info> info()
    {
        std::vector<Info> i(n_rows_);
        check(InfoOf(h_, i.data()));
        return i;
    }
    uint64_t inputs() const { return value_of<uint64_t>(Inputs, h_); }
    void reset() { check(Reset(h_)); }

protected:
    RecordBank(uint32_t n_rows, uint32_t cap) : n_rows_(n_rows), cap_(cap) {}

    std::vector<std::vector<Rec>> records(const std::vector<uint32_t>& rows)
    {
        const std::vector<uint32_t> c = counts();
        std::vector<Rec> buf(std::max<size_t>(1, rows.size() * cap_));
        check(Records(h_, rows.data(), rows.size(), buf.data()));
        std::vector<std::vector<Rec>> res(rows.size());
        for (size_t s = 0; s < rows.size(); ++s)
            res[s].assign(buf.begin() + s * cap_, buf.begin() + s * cap_ + std::min<size_t>(c[rows[s]], cap_));
        return res;
    }

    uint32_t n_rows_, cap_;
    Owned<H, Free> h_;
};

// Rational resampler (fmd_resample_*): `taps` is [L][T] phase-major; run() takes [n_rows][n_in][width] int16 and returns the
// call's outputs per row, interleaved by `width`.
class Resampler : public RowProcessor<fmd_resample, fmd_resample_free, fmd_resample_run_batch, fmd_resample_outputs, fmd_resample_reset> {
public:
    Resampler(const std::vector<int16_t>& taps, uint32_t L, uint32_t M, uint32_t shift, uint32_t n_rows = 1, uint32_t width = 1,
              int32_t device_id = -1)
        : RowProcessor(n_rows, width), L_(L), M_(M)
    {
        fmd_device_config dev{n_rows, device_id, 0};
        check(fmd_resample_new(taps.data(), L, M, L ? (uint32_t)(taps.size() / L) : 0u, shift, width, &dev, h_.out()));
    }

    // FMD_ERR_TOO_SHORT (a call that completes no output) returns empty rows and changes nothing: the samples are not taken.
    Rows run(const int16_t* x, size_t n_in) { return run_rows(x, n_in, fmd_resample_out_cap(L_, M_, n_in), FMD_ERR_TOO_SHORT); }

private:
    uint32_t L_, M_;
};

// Automatic gain control (fmd_agc_*): run() takes [n_rows][n_in][width] int16 and returns the call's outputs per row, interleaved
// by `width`: block j comes with the call that completes block j + 1, so a call may return empty rows (its samples are taken), and
// the last block ... 2 block - 1 samples of a stream come out only behind 2 block further (zero) samples.
class Agc : public RowProcessor<fmd_agc, fmd_agc_free, fmd_agc_run_batch, fmd_agc_outputs, fmd_agc_reset> {
public:
    explicit Agc(const fmd_agc_config& cfg, uint32_t n_rows = 1, uint32_t width = 1, int32_t device_id = -1)
        : RowProcessor(n_rows, width), block_(cfg.block)
    {
        fmd_device_config dev{n_rows, device_id, 0};
        check(fmd_agc_new(&cfg, width, &dev, h_.out()));
    }

    Rows run(const int16_t* x, size_t n_in) { return run_rows(x, n_in, fmd_agc_out_cap(block_, n_in)); }
    // (G, h) of `row` after the last emitted block: the Q10 gain and the hang blocks left
    std::pair<uint32_t, uint32_t> gain(uint32_t row = 0)
    {
        uint32_t g = 0, h = 0;
        check(fmd_agc_gain(h_, row, &g, &h));
        return {g, h};
    }
    uint32_t block() const { return block_; }

private:
    uint32_t block_;
};

// The 38 standard CTCSS tones, Hz.
inline const std::vector<double>& ctcss_tones()
{
    static const std::vector<double> tones{67.0, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9,
                                           114.8, 118.8, 123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 162.2, 167.9, 173.8,
                                           179.9, 186.2, 192.8, 203.5, 210.7, 218.1, 225.7, 233.6, 241.8, 250.3};
    return tones;
}

// The table of a ToneSquelch, entry for entry the Python tone_table(): [freqs][block][2] = (c_f[r], s_f[r]) =
// rint(1023 w[r] cos(2 pi f r / rate)), rint(-1023 w[r] sin(2 pi f r / rate)) under w[r] = 0.5 - 0.5 cos(2 pi (r + 0.5) / block).
inline std::vector<int16_t> tone_table(double rate, const std::vector<double>& freqs, uint32_t block)
{
    if (!(rate > 0) || block < 1) throw Error(FMD_ERR_INVALID_ARG);
    std::vector<int16_t> tab(freqs.size() * block * 2);
    for (size_t k = 0; k < freqs.size(); ++k)
        for (uint32_t r = 0; r < block; ++r) {
            const double w = 0.5 - 0.5 * std::cos(2 * detail::pi * ((double)r + 0.5) / (double)block);
            const double a = 2 * detail::pi * freqs[k] * (double)r / rate;
            tab[(k * block + r) * 2] = (int16_t)std::rint(1023 * w * std::cos(a));
            tab[(k * block + r) * 2 + 1] = (int16_t)std::rint(-1023 * w * std::sin(a));
        }
    return tab;
}

// Tone squelch (fmd_tonesq_*): `table` is [n_tones][cfg.block][2] (tone_table); run() takes [n_rows][n_in][width] int16 and returns
// the same samples per row, gated by the tone the blocks before decided on.
class ToneSquelch : public RowProcessor<fmd_tonesq, fmd_tonesq_free, fmd_tonesq_run_batch, fmd_tonesq_outputs, fmd_tonesq_reset> {
public:
    struct Status { int32_t tone; uint64_t power; bool open; };

    ToneSquelch(const fmd_tonesq_config& cfg, const std::vector<int16_t>& table, uint32_t n_rows = 1, uint32_t width = 1,
                int32_t device_id = -1)
        : RowProcessor(n_rows, width), block_(cfg.block)
    {
        fmd_device_config dev{n_rows, device_id, 0};
        const uint32_t n_tones = cfg.block ? (uint32_t)(table.size() / (2ull * cfg.block)) : 0u;
        check(fmd_tonesq_new(&cfg, table.data(), n_tones, width, &dev, h_.out()));
    }

    Rows run(const int16_t* x, size_t n_in) { return run_rows(x, n_in, fmd_tonesq_out_cap(n_in)); }
    // per row after the last completed block: the selected tone (-1: none), W of the strongest tone, whether the gate opens
    std::vector<Status> status()
    {
        std::vector<int32_t> tone(n_rows_);
        std::vector<uint64_t> power(n_rows_);
        std::vector<uint8_t> open(n_rows_);
        check(fmd_tonesq_status(h_, tone.data(), power.data(), open.data()));
        std::vector<Status> res(n_rows_);
        for (size_t r = 0; r < n_rows_; ++r) res[r] = Status{tone[r], power[r], open[r] != 0};
        return res;
    }
    uint32_t block() const { return block_; }

private:
    uint32_t block_;
};

// The 104 standard DCS codes (written in octal).
inline const std::vector<uint32_t>& dcs_codes()
{
    static const std::vector<uint32_t> codes{
        0023, 0025, 0026, 0031, 0032, 0036, 0043, 0047, 0051, 0053, 0054, 0065, 0071, 0072, 0073, 0074,
        0114, 0115, 0116, 0122, 0125, 0131, 0132, 0134, 0143, 0145, 0152, 0155, 0156, 0162, 0165, 0172, 0174,
        0205, 0212, 0223, 0225, 0226, 0243, 0244, 0245, 0246, 0251, 0252, 0255, 0261, 0263, 0265, 0266, 0271, 0274,
        0306, 0311, 0315, 0325, 0331, 0332, 0343, 0346, 0351, 0356, 0364, 0365, 0371,
        0411, 0412, 0413, 0423, 0431, 0432, 0445, 0446, 0452, 0454, 0455, 0462, 0464, 0465, 0466,
        0503, 0506, 0516, 0523, 0526, 0532, 0546, 0565,
        0606, 0612, 0624, 0627, 0631, 0632, 0654, 0662, 0664,
        0703, 0712, 0723, 0731, 0732, 0734, 0743, 0754};
    return codes;
}

// c(x) mod the DCS polynomial x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1 (0xC75), c below 2^23.
inline uint32_t dcs_remainder(uint32_t c)
{
    for (int i = 22; i > 10; --i)
        if ((c >> i) & 1u) c ^= 0xC75u << (i - 11);
    return c;
}

// The 23-bit word c = (p << 12) | 0x800 | code of a 9-bit code, bit 0 sent first: the 11 parity bits p make c(x) divisible by the DCS
// polynomial.  dcs_codeword(023) = 0x763813.
inline uint32_t dcs_codeword(uint32_t code)
{
    if (code >= 512) throw Error(FMD_ERR_INVALID_ARG);
    const uint32_t d = 0x800u | code;
    for (uint32_t p = 0; p < 2048; ++p)
        if (dcs_remainder((p << 12) | d) == 0) return (p << 12) | d;
    throw Error(FMD_ERR_INVALID_ARG);
}

// The table word of a code for a CodeSquelch, word for word the Python dcs_word(): the codeword, complemented if `inverted`, in the
// order of arrival: table bit j = bit 22 - j of the codeword.  dcs_word(023) = 0x640E37.
inline uint32_t dcs_word(uint32_t code, bool inverted = false)
{
    uint32_t c = dcs_codeword(code), w = 0;
    if (inverted) c ^= 0x7FFFFFu;
    for (uint32_t j = 0; j < 23; ++j) w |= ((c >> (22 - j)) & 1u) << j;
    return w;
}

// The configuration of a CodeSquelch for DCS at the sample rate `rate`, entry for entry the Python dcs_design(): box the power of
// two that puts rate / box nearest 1500 Hz; lp a Hamming-windowed sinc of 32 taps at 200 Hz, scaled to peak 1023; lshift =
// ceil(log2(sum |lp|)); tap[j] = floor(j rate / (134.4 box) + 0.5); block two whole word periods, up to a multiple of 64; tol 1,
// min_hits 8, confirm 1, hang 1, ramp 64; accept every word.
inline fmd_dcs_config dcs_design(double rate)
{
    if (!(rate > 0)) throw Error(FMD_ERR_INVALID_ARG);
    fmd_dcs_config cfg{};
    uint32_t box = 1;
    double best = std::fabs(rate - 1500.0);
    for (uint32_t lg = 1; lg < 7; ++lg) {
        const double d = std::fabs(rate / (double)(1u << lg) - 1500.0);
        if (d < best) { box = 1u << lg; best = d; }
    }
    const uint32_t T = 32;
    const double fc = 200.0 * (double)box / rate;
    double h[32], peak = 0;
    for (uint32_t t = 0; t < T; ++t) {
        const double x = 2 * detail::pi * fc * ((double)t - (double)(T - 1) / 2.0);
        h[t] = detail::sinc(x) * (0.54 - 0.46 * std::cos(2 * detail::pi * (double)t / (double)(T - 1)));
        if (t == 0 || h[t] > peak) peak = h[t];
    }
    uint32_t mag = 0;
    for (uint32_t t = 0; t < T; ++t) {
        cfg.lp[t] = (int16_t)std::rint(1023.0 * h[t] / peak);
        mag += (uint32_t)(cfg.lp[t] < 0 ? -cfg.lp[t] : cfg.lp[t]);
    }
    while ((1u << cfg.lshift) < mag) ++cfg.lshift;
    for (uint32_t j = 0; j < 23; ++j) cfg.tap[j] = (uint32_t)std::floor((double)j * rate / (134.4 * (double)box) + 0.5);
    const double blocks = std::ceil(46.0 * rate / (134.4 * 64.0));
    if (cfg.tap[22] > 511 || blocks > 512) throw Error(FMD_ERR_UNSUPPORTED);
    cfg.block = 64u * (uint32_t)blocks;
    cfg.box = box; cfg.n_taps = T;
    cfg.tol = 1; cfg.min_hits = 8; cfg.confirm = 1; cfg.hang = 1; cfg.ramp = 64;
    cfg.accept[0] = cfg.accept[1] = ~0ull;
    return cfg;
}

// Code squelch (fmd_dcs_*): `words` is the table of 23-bit words (dcs_word); run() takes [n_rows][n_in][width] int16 and returns the
// same samples per row, gated by the code the blocks before decided on.  A station whose discriminator has the other sign is
// reported under its code's inverse partner (023 as 047).
class CodeSquelch : public RowProcessor<fmd_dcs, fmd_dcs_free, fmd_dcs_run_batch, fmd_dcs_outputs, fmd_dcs_reset> {
public:
    struct Status { int32_t code; uint32_t hits; bool open; };

    CodeSquelch(const fmd_dcs_config& cfg, const std::vector<uint32_t>& words, uint32_t n_rows = 1, uint32_t width = 1,
                int32_t device_id = -1)
        : RowProcessor(n_rows, width), block_(cfg.block)
    {
        fmd_device_config dev{n_rows, device_id, 0};
        check(fmd_dcs_new(&cfg, words.data(), (uint32_t)words.size(), width, &dev, h_.out()));
    }

    Rows run(const int16_t* x, size_t n_in) { return run_rows(x, n_in, fmd_dcs_out_cap(n_in)); }
    // per row after the last completed block: the selected word's index (-1: none), the hits of the block's most-hit word, whether
    // the gate opens
    std::vector<Status> status()
    {
        std::vector<int32_t> code(n_rows_);
        std::vector<uint32_t> hits(n_rows_);
        std::vector<uint8_t> open(n_rows_);
        check(fmd_dcs_status(h_, code.data(), hits.data(), open.data()));
        std::vector<Status> res(n_rows_);
        for (size_t r = 0; r < n_rows_; ++r) res[r] = Status{code[r], hits[r], open[r] != 0};
        return res;
    }
    uint32_t block() const { return block_; }

private:
    uint32_t block_;
};

// The table of an AfskDemod with its shifts, entry for entry the Python afsk_table(): rectangular windows one bit long, T = taps or
// round(rate / baud); tab[4][T] = mark-cos, mark-sin, space-cos, space-sin = rint(1023 cos(2 pi f t / rate)), rint(-1023 sin(...));
// pre_shift 8; out_shift the smallest at which a full window of either tone at amplitude 1024 stays inside int16.
struct AfskTable {
    std::vector<int16_t> tab;
    uint32_t T, pre_shift, out_shift;
};

inline AfskTable afsk_table(double rate, double baud = 1200, double mark = 1200, double space = 2200, uint32_t taps = 0)
{
    if (!(rate > 0) || !(baud > 0)) throw Error(FMD_ERR_INVALID_ARG);
    const double tr = taps ? (double)taps : std::rint(rate / baud);
    if (!(tr >= 2 && tr <= 64)) throw Error(FMD_ERR_UNSUPPORTED);
    const uint32_t T = (uint32_t)tr;
    AfskTable res{std::vector<int16_t>((size_t)4 * T), T, 8, 0};
    const double freqs[2] = {mark, space};
    for (size_t k = 0; k < 2; ++k)
        for (uint32_t t = 0; t < T; ++t) {
            const double a = 2 * detail::pi * freqs[k] * (double)t / rate;
            res.tab[2 * k * T + t] = (int16_t)std::rint(1023 * std::cos(a));
            res.tab[(2 * k + 1) * T + t] = (int16_t)std::rint(-1023 * std::sin(a));
        }
    int64_t peak = 0;
    for (size_t k = 0; k < 2; ++k) {
        int64_t A[4];
        for (size_t q = 0; q < 4; ++q) {
            int64_t s = 0;
            for (uint32_t t = 0; t < T; ++t)
                s += (int64_t)res.tab[q * T + t] * (int64_t)std::rint(1024 * std::cos(2 * detail::pi * freqs[k] * (double)t / rate));
            A[q] = s >> res.pre_shift;
        }
        const int64_t v = A[0] * A[0] + A[1] * A[1] - A[2] * A[2] - A[3] * A[3];
        peak = std::max(peak, v < 0 ? -v : v);
    }
    while ((peak >> res.out_shift) > 32767) ++res.out_shift;
    return res;
}

// The default stride of a window of `taps` samples: a fifth of a bit, at least 1 and at most 32.
inline uint32_t afsk_stride(uint32_t taps) { return std::max<uint32_t>(1, std::min<uint32_t>(std::min<uint32_t>(32, taps), (2 * taps + 5) / 10)); }

// Tone-pair demodulator (fmd_afsk_*): `table` is [4][T] (afsk_table); run() takes [n_rows][n_in] int16 and returns the call's soft
// decisions per row, one per `stride` samples, positive for mark.
class AfskDemod : public RowProcessor<fmd_afsk, fmd_afsk_free, fmd_afsk_run_batch, fmd_afsk_outputs, fmd_afsk_reset> {
public:
    AfskDemod(const std::vector<int16_t>& table, uint32_t stride, uint32_t pre_shift, uint32_t out_shift, uint32_t n_rows = 1,
              uint32_t width = 1, int32_t device_id = -1)
        : RowProcessor(n_rows, width), stride_(stride)
    {
        fmd_device_config dev{n_rows, device_id, 0};
        check(fmd_afsk_new(table.data(), (uint32_t)(table.size() / 4), stride, pre_shift, out_shift, width, &dev, h_.out()));
    }

    // FMD_ERR_TOO_SHORT (a call that completes no output) returns empty rows and changes nothing: the samples are not taken.
    Rows run(const int16_t* x, size_t n_in) { return run_rows(x, n_in, fmd_afsk_out_cap(stride_, n_in), FMD_ERR_TOO_SHORT); }
    uint32_t stride() const { return stride_; }

private:
    uint32_t stride_;
};

// AX.25 frame decoder of one row (fmd_ax25_decoder_*, host only): push() takes an AfskDemod's soft decisions at rate_num / rate_den
// per second (the audio rate over the stride) and returns the frames completed since.
class Ax25Decoder {
public:
    Ax25Decoder(uint32_t rate_num, uint32_t rate_den, uint32_t baud = 1200) { check(fmd_ax25_decoder_new(rate_num, rate_den, baud, h_.out())); }

    std::vector<fmd_ax25_frame> push(const int16_t* soft, size_t n)
    {
        std::vector<fmd_ax25_frame> res;
        fmd_ax25_frame buf[16];
        size_t k = 0;
        check(fmd_ax25_decoder_push(h_, soft, n, buf, 16, &k));
        for (;;) {
            res.insert(res.end(), buf, buf + k);
            if (k < 16) return res;
            check(fmd_ax25_decoder_push(h_, nullptr, 0, buf, 16, &k));
        }
    }
    std::vector<fmd_ax25_frame> push(const std::vector<int16_t>& soft) { return push(soft.data(), soft.size()); }
    fmd_ax25_info info() const { return value_of<fmd_ax25_info>(fmd_ax25_decoder_info, h_); }
    void reset() { check(fmd_ax25_decoder_reset(h_)); }

private:
    Owned<fmd_ax25_decoder, fmd_ax25_decoder_free> h_;
};

// The frame bank (fmd_hdlc_*): an Ax25Decoder per row on the device.  run() takes the soft decisions [n_rows][n_in] of an AfskDemod;
// behind it counts() gives the frames that passed in the call per row, frames(rows) the first min(count, frame_cap) of each listed
// row in the order they closed, info() the rows' cumulative counters.
class Ax25Framer : public RecordBank<fmd_hdlc, fmd_hdlc_free, fmd_ax25_frame, fmd_ax25_info, fmd_hdlc_counts, fmd_hdlc_frames, fmd_hdlc_info,
                                     fmd_hdlc_inputs, fmd_hdlc_reset> {
public:
    Ax25Framer(uint32_t rate_num, uint32_t rate_den, uint32_t baud = 1200, uint32_t frame_cap = 4, uint32_t n_rows = 1, int32_t device_id = -1)
        : RecordBank(n_rows, frame_cap)
    {
        fmd_device_config dev{n_rows, device_id, 0};
        check(fmd_hdlc_new(rate_num, rate_den, baud, frame_cap, &dev, h_.out()));
    }

    void run(const int16_t* soft, size_t n_in) { check(fmd_hdlc_run_batch(h_, soft, n_in, n_in)); }
    std::vector<std::vector<fmd_ax25_frame>> frames(const std::vector<uint32_t>& rows) { return records(rows); }
    uint32_t frame_cap() const { return cap_; }
};

namespace detail {
// "CALL" or "CALL-SSID" of a 7-byte address; empty where it is malformed (a character that is not shifted ASCII upper case or digit,
// or one behind a padding space)
inline std::string ax25_call(const uint8_t* a)
{
    std::string name;
    bool pad = false;
    for (int i = 0; i < 6; ++i) {
        if (a[i] & 1) return "";
        const char c = (char)(a[i] >> 1);
        if (c == ' ') { pad = true; continue; }
        if (pad || !((c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z'))) return "";
        name += c;
    }
    if (name.empty()) return "";
    const unsigned ssid = (a[6] >> 1) & 15u;
    return ssid ? name + "-" + std::to_string(ssid) : name;
}
}  // namespace detail

// A frame in TNC2 form `SRC>DST,DIGI*:info`, character for character the Python ax25_text(): `*` behind a digipeater whose has-been-
// repeated bit is set, non-printable bytes as `.`, control 0x03 and PID 0xF0 (UI) left out; hex where the address field is malformed.
inline std::string ax25_text(const uint8_t* data, size_t len)
{
    const auto hex = [&] {
        static const char* const digits = "0123456789abcdef";
        std::string s;
        for (size_t i = 0; i < len; ++i) { s += digits[data[i] >> 4]; s += digits[data[i] & 15]; }
        return s;
    };
    std::vector<std::pair<std::string, bool>> addrs;
    size_t pos = 0;
    for (;;) {
        if (pos + 7 > len || addrs.size() == 10) return hex();
        const std::string name = detail::ax25_call(data + pos);
        if (name.empty()) return hex();
        addrs.emplace_back(name, (data[pos + 6] & 0x80) != 0);
        pos += 7;
        if (data[pos - 1] & 1) break;
    }
    if (addrs.size() < 2) return hex();
    if (pos + 2 <= len && data[pos] == 0x03 && data[pos + 1] == 0xF0) pos += 2;
    std::string s = addrs[1].first + ">" + addrs[0].first;
    for (size_t i = 2; i < addrs.size(); ++i) s += "," + addrs[i].first + (addrs[i].second ? "*" : "");
    s += ":";
    for (; pos < len; ++pos) s += data[pos] >= 32 && data[pos] < 127 ? (char)data[pos] : '.';
    return s;
}
inline std::string ax25_text(const fmd_ax25_frame& f) { return ax25_text(f.data, std::min<size_t>(f.len, sizeof f.data)); }

// fsk_design(rate, baud) of the Python package, entry for entry (scalar libm in the same order): the FSK front end's parameters for
// POCSAG at `baud` bit/s in audio at `rate` Hz.  A pair whose result leaves the kernel's domain throws std::invalid_argument.
inline fmd_fsk_config fsk_design(double rate, double baud = 1200)
{
    if (!(rate > 0) || !(baud > 0)) throw std::invalid_argument("need rate > 0 and baud > 0");
    fmd_fsk_config cfg{};
    const double d = std::floor(rate / (5.0 * baud) + 0.5);
    if (d > 64) throw std::invalid_argument("rate / baud out of range");
    cfg.D = std::max<uint32_t>(1, (uint32_t)d);
    const double w = std::floor(rate / (baud * (double)cfg.D) + 0.5);
    if (!(w >= 1 && w <= 16)) throw std::invalid_argument("rate / baud out of range");
    cfg.W = (uint32_t)w;
    while ((1u << cfg.shift) < cfg.D * cfg.W) ++cfg.shift;
    bool ok = cfg.shift <= 10;
    for (uint32_t j = 0; j < 32; ++j) {
        const double t = std::floor((double)j * rate / (baud * (double)cfg.D) + 0.5);
        ok = ok && t <= 255;
        cfg.tap[j] = ok ? (uint32_t)t : 0;
        ok = ok && (j == 0 || cfg.tap[j] >= cfg.tap[j - 1]);
    }
    if (!ok) throw std::invalid_argument("rate / baud out of range");
    cfg.sync = 0x7CD215D8u; cfg.tol = 2; cfg.min_corr = 1024; cfg.hit_cap = 16;
    return cfg;
}

// FSK front end of the pager decoder (fmd_fsk_*): run() takes [n_rows][n_in] int16 and returns the call's soft decisions per row,
// one per cfg.D samples (none from a call that completes no box); hits() what that call found.
class FskDemod : public RowProcessor<fmd_fsk, fmd_fsk_free, fmd_fsk_run_batch, fmd_fsk_outputs, fmd_fsk_reset> {
public:
    explicit FskDemod(const fmd_fsk_config& cfg, uint32_t n_rows = 1, uint32_t width = 1, int32_t device_id = -1)
        : RowProcessor(n_rows, width), cfg_(cfg)
    {
        fmd_device_config dev{n_rows, device_id, 0};
        check(fmd_fsk_new(&cfg, width, &dev, h_.out()));
    }

    Rows run(const int16_t* x, size_t n_in) { return run_rows(x, n_in, fmd_fsk_out_cap(cfg_.D, n_in)); }

    // per row: the records of the last call that launched, the first min(count, hit_cap) of them; counts (optional): all hits
    std::vector<std::vector<fmd_fsk_hit>> hits(std::vector<uint32_t>* counts = nullptr)
    {
        std::vector<uint32_t> cnt(n_rows_);
        std::vector<fmd_fsk_hit> rec((size_t)n_rows_ * cfg_.hit_cap);
        check(fmd_fsk_hits(h_, cnt.data(), rec.data()));
        std::vector<std::vector<fmd_fsk_hit>> res(n_rows_);
        for (size_t r = 0; r < n_rows_; ++r)
            res[r].assign(rec.begin() + r * cfg_.hit_cap, rec.begin() + r * cfg_.hit_cap + std::min<uint32_t>(cnt[r], cfg_.hit_cap));
        if (counts) *counts = cnt;
        return res;
    }
    const fmd_fsk_config& config() const { return cfg_; }

private:
    fmd_fsk_config cfg_;
};

// POCSAG batch decoder of one row (fmd_pocsag_decoder_*, host only): push() takes an FskDemod's soft decisions at rate_num /
// rate_den per second (the audio rate over D) with the row's records of the same call and returns the messages closed since.
class PocsagDecoder {
public:
    PocsagDecoder(uint32_t rate_num, uint32_t rate_den, uint32_t baud = 1200, uint32_t max_errors = 1)
    {
        check(fmd_pocsag_decoder_new(rate_num, rate_den, baud, max_errors, h_.out()));
    }

    std::vector<fmd_pocsag_msg> push(const int16_t* soft, size_t n, const fmd_fsk_hit* hits, size_t n_hits)
    {
        std::vector<fmd_pocsag_msg> res;
        std::vector<fmd_pocsag_msg> buf(16);
        size_t k = 0;
        check(fmd_pocsag_decoder_push(h_, soft, n, hits, n_hits, buf.data(), 16, &k));
        for (;;) {
            res.insert(res.end(), buf.begin(), buf.begin() + k);
            if (k < 16) return res;
            check(fmd_pocsag_decoder_push(h_, nullptr, 0, nullptr, 0, buf.data(), 16, &k));
        }
    }
    std::vector<fmd_pocsag_msg> push(const std::vector<int16_t>& soft, const std::vector<fmd_fsk_hit>& hits)
    {
        return push(soft.data(), soft.size(), hits.data(), hits.size());
    }
    fmd_pocsag_info info() const { return value_of<fmd_pocsag_info>(fmd_pocsag_decoder_info, h_); }
    void reset() { check(fmd_pocsag_decoder_reset(h_)); }

private:
    Owned<fmd_pocsag_decoder, fmd_pocsag_decoder_free> h_;
};

// The page bank (fmd_pager_*): a PocsagDecoder per row on the device.  run() takes the soft decisions [n_rows][n_in] of an FskDemod
// with the records of the same call as FskDemod::hits() gives them; behind it counts() gives the messages that closed in the call
// per row, msgs(rows) the first min(count, msg_cap) of each listed row in the order they closed, info() the rows' cumulative counters.
class Pager : public RecordBank<fmd_pager, fmd_pager_free, fmd_pocsag_msg, fmd_pocsag_info, fmd_pager_counts, fmd_pager_msgs, fmd_pager_info,
                                fmd_pager_inputs, fmd_pager_reset> {
public:
    Pager(uint32_t rate_num, uint32_t rate_den, uint32_t baud = 1200, uint32_t max_errors = 1, uint32_t msg_cap = 4, uint32_t n_rows = 1,
          int32_t device_id = -1)
        : RecordBank(n_rows, msg_cap), rate_num_(rate_num), rate_den_(rate_den), baud_(baud)
    {
        fmd_device_config dev{n_rows, device_id, 0};
        check(fmd_pager_new(rate_num, rate_den, baud, max_errors, msg_cap, &dev, h_.out()));
    }

    void run(const int16_t* soft, size_t n_in, const std::vector<std::vector<fmd_fsk_hit>>& hits)
    {
        size_t cap = 1;
        for (const std::vector<fmd_fsk_hit>& h : hits) cap = std::max(cap, std::min<size_t>(h.size(), 64));
        std::vector<uint32_t> cnt(n_rows_, 0u);
        std::vector<fmd_fsk_hit> rec((size_t)n_rows_ * cap);
        for (size_t r = 0; r < n_rows_ && r < hits.size(); ++r) {
            cnt[r] = (uint32_t)std::min<size_t>(hits[r].size(), cap);
            std::copy(hits[r].begin(), hits[r].begin() + cnt[r], rec.begin() + r * cap);
        }
        check(fmd_pager_run_batch(h_, soft, n_in, n_in, cnt.data(), rec.data(), (uint32_t)cap));
    }
    std::vector<std::vector<fmd_pocsag_msg>> msgs(const std::vector<uint32_t>& rows) { return records(rows); }
    size_t max_messages(size_t n) const { return fmd_pager_max_messages(rate_num_, rate_den_, baud_, n); }
    uint32_t msg_cap() const { return cap_; }

private:
    uint32_t rate_num_, rate_den_, baud_;
};

namespace detail {
// message bit i, the first in bit 7 of bits[0]; the stored bits only
inline uint32_t pocsag_bit(const fmd_pocsag_msg& m, uint32_t i) { return (m.bits[i >> 3] >> (7 - (i & 7u))) & 1u; }
inline uint32_t pocsag_stored(const fmd_pocsag_msg& m) { return std::min<uint32_t>(m.n_bits, 8 * sizeof m.bits); }
}  // namespace detail

// The message's bits as numeric text, character for character the Python pocsag_numeric(): 4 bits per character, each nibble
// bit-reversed, from the table 0123456789*U -)(.
inline std::string pocsag_numeric(const fmd_pocsag_msg& m)
{
    static const char* const table = "0123456789*U -)(";
    std::string s;
    for (uint32_t i = 0; i + 4 <= detail::pocsag_stored(m); i += 4) {
        uint32_t v = 0;
        for (uint32_t j = 0; j < 4; ++j) v |= detail::pocsag_bit(m, i + j) << j;
        s += table[v];
    }
    return s;
}

// The message's bits as text, as pocsag_alpha() of the Python package: 7 bits per character, each reversed; trailing NUL, ETX and
// EOT dropped, other non-printable characters as `.`.
inline std::string pocsag_alpha(const fmd_pocsag_msg& m)
{
    std::vector<uint32_t> ch;
    for (uint32_t i = 0; i + 7 <= detail::pocsag_stored(m); i += 7) {
        uint32_t v = 0;
        for (uint32_t j = 0; j < 7; ++j) v |= detail::pocsag_bit(m, i + j) << j;
        ch.push_back(v);
    }
    while (!ch.empty() && (ch.back() == 0 || ch.back() == 3 || ch.back() == 4)) ch.pop_back();
    std::string s;
    for (uint32_t c : ch) s += c >= 32 && c < 127 ? (char)c : '.';
    return s;
}

// One line per message, as pocsag_text() of the Python package; mode 0: auto (function 0 numeric, the rest alpha), 1: numeric,
// 2: alpha.
inline std::string pocsag_text(const fmd_pocsag_msg& m, uint32_t baud = 1200, int mode = 0)
{
    char head[96];
    snprintf(head, sizeof head, "POCSAG%u: Address: %07u  Function: %u  ", baud, m.address, m.function);
    if (m.n_bits == 0) return std::string(head) + "Tone: ";
    if (mode == 1 || (mode == 0 && m.function == 0)) return std::string(head) + "Numeric: " + pocsag_numeric(m);
    return std::string(head) + "Alpha: " + pocsag_alpha(m);
}

// The Mode S bank (fmd_modes_*): the ADS-B messages of `n_streams` 2 Msample/s u8 IQ streams, decoded on the device.  run() takes
// [n_streams][nbytes]; behind it counts() gives every stream's acceptances in the call, messages(streams) the first min(count,
// msg_cap) records of each listed stream in increasing position, info() the streams' cumulative counters.
class ModeSBank {
public:
    explicit ModeSBank(const fmd_modes_config& cfg, uint32_t n_streams = 1, int32_t device_id = -1) : n_streams_(n_streams), cap_(cfg.msg_cap)
    {
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_modes_new(&cfg, &dev, h_.out()));
    }

    void run(const uint8_t* iq, size_t nbytes) { check(fmd_modes_run_batch(h_, iq, nbytes, nbytes)); }
    void reset() { check(fmd_modes_reset(h_)); }
    std::vector<uint32_t> counts()
    {
        std::vector<uint32_t> c(n_streams_);
        check(fmd_modes_counts(h_, c.data()));
        return c;
    }
    std::vector<std::vector<fmd_modes_msg>> messages(const std::vector<uint32_t>& streams)
    {
        const std::vector<uint32_t> c = counts();
        std::vector<fmd_modes_msg> buf(std::max<size_t>(1, streams.size() * cap_));
        check(fmd_modes_msgs(h_, streams.data(), streams.size(), buf.data()));
        std::vector<std::vector<fmd_modes_msg>> res(streams.size());
        for (size_t s = 0; s < streams.size(); ++s)
            res[s].assign(buf.begin() + s * cap_, buf.begin() + s * cap_ + std::min<size_t>(c[streams[s]], cap_));
        return res;
    }
    std::vector<fmd_modes_totals> info()
    {
        std::vector<fmd_modes_totals> i(n_streams_);
        check(fmd_modes_info(h_, i.data()));
        return i;
    }
    uint32_t msg_cap() const { return cap_; }

private:
    uint32_t n_streams_, cap_;
    Owned<fmd_modes, fmd_modes_free> h_;
};

// `*HEX;`, rtl_adsb's line for a message
inline std::string modes_hex(const fmd_modes_msg& m)
{
    std::string s = "*";
    char b[3];
    for (uint32_t i = 0; i < m.n_bytes && i < sizeof m.bytes; ++i) { snprintf(b, sizeof b, "%02X", m.bytes[i]); s += b; }
    return s + ";";
}

// The pulse bank (fmd_pulses_*): the on-off-keyed pulses of `n_streams` u8 IQ streams.  run() takes [n_streams][nbytes]; behind it
// counts() gives every stream's falls in the call, pulses(streams) the first min(count, pulse_cap) records of each listed stream in
// increasing position, info() the streams' cumulative counters with the current state and run.
class PulseBank {
public:
    explicit PulseBank(const fmd_pulses_config& cfg, uint32_t n_streams = 1, int32_t device_id = -1) : n_streams_(n_streams), cap_(cfg.pulse_cap)
    {
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_pulses_new(&cfg, &dev, h_.out()));
    }

    void run(const uint8_t* iq, size_t nbytes) { check(fmd_pulses_run_batch(h_, iq, nbytes, nbytes)); }
    void reset() { check(fmd_pulses_reset(h_)); }
    std::vector<uint32_t> counts()
    {
        std::vector<uint32_t> c(n_streams_);
        check(fmd_pulses_counts(h_, c.data()));
        return c;
    }
    std::vector<std::vector<fmd_pulses_rec>> pulses(const std::vector<uint32_t>& streams)
    {
        const std::vector<uint32_t> c = counts();
        std::vector<fmd_pulses_rec> buf(std::max<size_t>(1, streams.size() * cap_));
        check(fmd_pulses_recs(h_, streams.data(), streams.size(), buf.data()));
        std::vector<std::vector<fmd_pulses_rec>> res(streams.size());
        for (size_t s = 0; s < streams.size(); ++s)
            res[s].assign(buf.begin() + s * cap_, buf.begin() + s * cap_ + std::min<size_t>(c[streams[s]], cap_));
        return res;
    }
    std::vector<fmd_pulses_totals> info()
    {
        std::vector<fmd_pulses_totals> i(n_streams_);
        check(fmd_pulses_info(h_, i.data()));
        return i;
    }
    uint32_t pulse_cap() const { return cap_; }
    uint32_t n_streams() const { return n_streams_; }
    fmd_pulses* handle() { return h_; }                       // (for PackageBank::run_bank)

private:
    uint32_t n_streams_, cap_;
    Owned<fmd_pulses, fmd_pulses_free> h_;
};

// The package bank (fmd_packages_*): the slicer below for every stream of a pulse bank, on the device.  run_bank() takes what the
// pulse bank's last call left on the device, flush() ends the input; behind either counts() gives every stream's delivered packages
// of the call, packages(streams) the first min(count, pkg_cap) of each listed stream in the order they closed, info() the streams'
// cumulative counters.  Both calls are enqueued on the default stream; the accessors synchronise.
class PackageBank {
public:
    explicit PackageBank(const fmd_packages_config& cfg, uint32_t n_streams = 1, int32_t device_id = -1) : n_streams_(n_streams), cap_(cfg.pkg_cap)
    {
        fmd_device_config dev{n_streams, device_id, 0};
        check(fmd_packages_new(&cfg, &dev, h_.out()));
    }
    // matched to a pulse bank: its streams, and room for every package a call of it can close
    PackageBank(PulseBank& bank, const fmd_pulse_slicer_config& slicer, uint32_t min_bits = 0, int32_t device_id = -1)
        : PackageBank(fmd_packages_config{slicer, min_bits, (uint32_t)fmd_packages_max(bank.pulse_cap())}, bank.n_streams(), device_id) {}

    void run(const uint32_t* counts, const fmd_pulses_rec* recs, size_t rec_cap, const fmd_pulses_totals* totals, size_t n_samples)
    {
        check(fmd_packages_run_batch(h_, counts, recs, rec_cap, totals, n_samples));
    }
    void run_bank(PulseBank& bank, void* stream = nullptr) { check(fmd_packages_run_bank(h_, bank.handle(), stream)); }
    void flush(void* stream = nullptr) { check(fmd_packages_flush(h_, stream)); }
    void reset() { check(fmd_packages_reset(h_)); }
    std::vector<uint32_t> counts()
    {
        std::vector<uint32_t> c(n_streams_);
        check(fmd_packages_counts(h_, c.data()));
        return c;
    }
    std::vector<std::vector<fmd_pulse_package>> packages(const std::vector<uint32_t>& streams)
    {
        const std::vector<uint32_t> c = counts();
        std::vector<fmd_pulse_package> buf(std::max<size_t>(1, streams.size() * cap_));
        check(fmd_packages_pkgs(h_, streams.data(), streams.size(), buf.data()));
        std::vector<std::vector<fmd_pulse_package>> res(streams.size());
        for (size_t s = 0; s < streams.size(); ++s)
            res[s].assign(buf.begin() + s * cap_, buf.begin() + s * cap_ + std::min<size_t>(c[streams[s]], cap_));
        return res;
    }
    std::vector<fmd_packages_totals> info()
    {
        std::vector<fmd_packages_totals> i(n_streams_);
        check(fmd_packages_info(h_, i.data()));
        return i;
    }
    uint32_t pkg_cap() const { return cap_; }

private:
    uint32_t n_streams_, cap_;
    Owned<fmd_packages, fmd_packages_free> h_;
};

// The host slicer behind it (fmd_pulse_slicer_*): one stream's records in, its closed bit packages out.
class PulseSlicer {
public:
    explicit PulseSlicer(const fmd_pulse_slicer_config& cfg) { check(fmd_pulse_slicer_new(&cfg, h_.out())); }

    // the records of a call whose first sample is `pos`, then the stream's state and run behind the call
    void push(const std::vector<fmd_pulses_rec>& recs, uint64_t pos) { check(fmd_pulse_slicer_push(h_, recs.data(), recs.size(), pos)); }
    void idle(uint32_t state, uint64_t run) { check(fmd_pulse_slicer_idle(h_, state, run)); }
    std::vector<fmd_pulse_package> take()
    {
        std::vector<fmd_pulse_package> out(64);
        size_t n = 0;
        check(fmd_pulse_slicer_take(h_, out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }

private:
    Owned<fmd_pulse_slicer, fmd_pulse_slicer_free> h_;
};

// `start_sample n_bits hex`, ook_gpu's line for a package
inline std::string pulse_line(const fmd_pulse_package& k)
{
    char head[48];
    snprintf(head, sizeof head, "%llu %u ", (unsigned long long)k.start, k.n_bits);
    std::string s = head;
    char b[3];
    for (uint32_t i = 0; i < (k.n_bits + 7u) / 8u && i < sizeof k.bits; ++i) { snprintf(b, sizeof b, "%02X", k.bits[i]); s += b; }
    return s;
}

// output(buf: Vec<i16>), simple_fm.rs:430-438: raw native-endian s16 to stdout, flushed.
inline void output(const std::vector<int16_t>& buf, FILE* f = stdout)
{
    if (!buf.empty()) fwrite(buf.data(), sizeof(int16_t), buf.size(), f);
    fflush(f);
}

// An input or output file of an s16 tool; stdin and stdout stay open.
struct CloseFile { void operator()(FILE* f) const { if (f != stdin && f != stdout) fclose(f); } };
using File = std::unique_ptr<FILE, CloseFile>;

constexpr size_t kReadSamples = 65536;                   // the s16 tools read their input in blocks of this many samples

// Up to kReadSamples samples of `width` int16 from `in` into `dst`: the whole samples read -- fewer than kReadSamples at the end
// of the input, where the bytes of a broken last sample are dropped and reported.
inline size_t read_samples(FILE* in, int16_t* dst, size_t width)
{
    const size_t sample = width * sizeof(int16_t), want = kReadSamples * sample;
    uint8_t* const p = reinterpret_cast<uint8_t*>(dst);
    size_t fill = 0, got;
    while (fill < want && (got = fread(p + fill, 1, want - fill, in)) > 0) fill += got;
    if (fill % sample) fprintf(stderr, "dropped %zu trailing bytes\n", fill % sample);
    return fill / sample;
}

// A tool's exit code from `run()`: an fm::Error is its message on stderr and exit code 1.
template <class Run>
inline int exit_code(Run run)
{
    try { return run(); }
    catch (const Error& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
}

}  // namespace fm
