// simple_fm_cli.cpp -- file mode of the reference's simple_fm example on the GPU path.
//
// Mirrors main() of examples/simple_fm.rs with READ_FROM_FILE = true (:65-84): read DEFAULT_BUF_LENGTH
// (src/lib.rs:25) byte blocks of interleaved u8 IQ from a file (or stdin with "-"), demodulate, write raw
// s16 mono at the resample rate to stdout -- so the documented pipeline still works:
//     simple_fm_gpu capture.bin | play -r 32k -t raw -e s -b 16 -c 1 -V1 -      (readme.md:13,17)
// Defaults are the example's constants: FREQUENCY 94.9 MHz (unused here), SAMPLE_RATE 170 kHz, RATE_RESAMPLE 32 kHz
// (:25-27) through optimal_settings (:48,189-214).
//
// Several input files: one channel per file in ONE bank (one Demod per stream, :137), block-synchronous; audio of
// file k goes to <prefix>.<k>.s16 (-o prefix, default "audio") and the run ends with the shortest file.  With -g N the
// same goes through the pipelined multi-GPU sink (fmd_sink_*): channels split over N devices, byte-identical output.
//
// Live mode, -t host:port: the example with READ_FROM_FILE = false (:51-64, receive() :89-132, process() :135-170) with
// the dongle behind an rtl_tcp server (the reference's own examples/rtl_tcp.rs): config_sdr's settings (:217-229) go out
// as rtl_tcp commands, DEFAULT_BUF_LENGTH blocks come back through fm::RtlTcpSource::read_sync, a short read ends the run
// with the example's "samples lost" message (:122-125).
//
// Station bank, -S off1,off2,...: K stations at these offsets (Hz from the capture's centre) out of ONE capture file recorded at
// the capture rate optimal_settings derives from -s (downsample x rate); the reference's own boxcar (h = 1...1, n_taps =
// downsample) is the prototype filter, mixed to each station by fmd_stations_*; audio of station k goes to <prefix>.<k>.s16.
// With -I the same filter runs through the channelizer (fmd_channelizer_*) instead: station k's complex baseband at
// capture_rate / downsample goes to <prefix>.<k>.cs16 as interleaved s16 (I, Q) pairs, no demodulation.
// With -N mode[:R[:lo:hi]] [-q squelch] the narrow-band bank (fmd_narrow_*) instead: station k's channel from lo to hi Hz around its
// offset through 256 channel taps at stride R, detected as iq / fm / am / usb / lsb, s16 (interleaved I/Q as .cs16 in iq mode).
// With -2 the stereo station bank (fmd_stereo_*) instead: station k's pilot-locked stereo, interleaved s16 (L, R) at
// f_m / R (f_m = capture_rate / downsample, R = max(1, floor(f_m / 48000)); 127 audio taps from fm::stereo_taps, 75 us
// de-emphasis, blocks of 4096) goes to <prefix>.<k>.s16; the audio rate is printed on stderr.
// With -R the RDS bank (fmd_rds_*) and one host decoder per station (fmd_rds_decoder_*) instead: a 64-tap low-pass of +-62 kHz in
// front (the boxcar would cut the 57 kHz subcarrier), 255 taps from fm::rds_taps at stride R = max(1, floor(f_m / 7500)); at the end
// one line per station on stdout, `offset_hz PI PS "radiotext" groups_ok blocks_bad` (PI in hex).  With -I also station k's RDS
// baseband as interleaved s16 (ur, ui) in <prefix>.<k>.rds.cs16.
//
// Power spectrum, -P N [-H hop]: the N-bin power spectrum (fmd_spectrum_*, integer Hann window of amplitude 2047, shift 16) of
// ONE capture file whose sample rate is -s, integrated over the file's complete blocks; one line per bin in frequency order,
// "offset_hz power" with the exact u64 power -- the offsets are where the stations are (-S).
//
// Uniform channelizer, -U N:hop[:taps_per_channel] [-C k1,k2,...]: all N channels of a band plan (or the listed ones) out of ONE
// capture file whose sample rate is -s (fmd_uniform_*; prototype fm::uniform_taps(N, taps_per_channel = 8), the smallest
// admissible shift): channel k's complex baseband at capture_rate / hop goes to <prefix>.<k>.cs16 as interleaved s16 (I, Q) pairs;
// the channels' offsets and the output rate are printed on stderr.  Trailing bytes that do not fill a hop are dropped with a note.
//
// EOF policy (the reference ignores the read count and never terminates at EOF): only COMPLETE
// blocks are demodulated; a trailing partial block is dropped with a note on stderr.  Logging goes to stderr
// because stdout carries audio (:37-38).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "demod.hpp"

// A FILE* that is closed when it goes out of scope (stdin is left open); null, after perror(), when it did not open.
struct CloseFile { void operator()(FILE* f) const { if (f != stdin) fclose(f); } };
using File = std::unique_ptr<FILE, CloseFile>;

static File open_file(const std::string& path, const char* mode)
{
    File f(fopen(path.c_str(), mode));
    if (!f) perror(path.c_str());
    return f;
}
// a capture: `-` is stdin
static File open_input(const char* path) { return strcmp(path, "-") ? open_file(path, "rb") : File(stdin); }
// <prefix>.<k><suffix>
static File open_output(const char* prefix, size_t k, const char* suffix) { return open_file(std::string(prefix) + "." + std::to_string(k) + suffix, "wb"); }

// fread until `n` bytes are there or the stream ends: the bytes read
static size_t read_block(FILE* in, uint8_t* buf, size_t n)
{
    size_t fill = 0, got;
    while (fill < n && (got = fread(buf + fill, 1, n - fill, in)) > 0) fill += got;
    return fill;
}

// the EOF policy's note: `bytes` at the end of the capture filled no `unit`
static void note_dropped(size_t bytes, const std::string& unit)
{
    if (bytes) fprintf(stderr, "dropped %zu trailing bytes (not a complete %s)\n", bytes, unit.c_str());
}
static std::string block_of(size_t nbytes) { return std::to_string(nbytes) + "-byte block"; }

// one channel per file: capture c and its <prefix>.<c>.s16; false after perror() when one does not open
static bool open_channels(const std::vector<const char*>& paths, const char* prefix, std::vector<File>& in, std::vector<File>& out)
{
    for (size_t c = 0; c < paths.size(); ++c) {
        in.push_back(open_file(paths[c], "rb"));
        if (!in.back()) return false;
        out.push_back(open_output(prefix, c, ".s16"));
        if (!out.back()) return false;
    }
    return true;
}

// one block of every channel into `buf` ([C][N]); false when a file ends first (the shortest file ends the run; partial blocks dropped)
static bool read_channels(std::vector<File>& in, uint8_t* buf, size_t N)
{
    for (size_t c = 0; c < in.size(); ++c)
        if (read_block(in[c].get(), buf + c * N, N) != N) return false;
    return true;
}

// one channel per file through the pipelined sink (-g N): the channels are split over N GPUs (device k % visible), the
// file reads of block n+1 overlap the transfers and the kernel of block n
static int run_sink(const std::vector<const char*>& paths, const char* prefix, uint32_t freq, uint32_t rate, uint32_t resample, int gpus)
{
    const size_t C = paths.size(), N = fm::DEFAULT_BUF_LENGTH;
    std::vector<File> in, out;
    if (!open_channels(paths, prefix, in, out)) return 2;
    int visible = 0;
    fm::check(fmd_device_count(&visible));
    if (visible < 1) throw fm::Error(FMD_ERR_NO_DEVICE);
    if ((size_t)gpus > C) gpus = (int)C;
    std::vector<int32_t> ids;
    for (int k = 0; k < gpus; ++k) ids.push_back(k % visible);
    const auto settings = fm::optimal_settings(freq, rate, resample);
    fm::Sink sink(settings.second, (uint32_t)C, N, ids, 3,
                  [&](uint64_t, uint32_t c, const int16_t* a, size_t n) { if (n) fwrite(a, sizeof(int16_t), n, out[c].get()); });
    size_t loops = 0;
    for (;; ++loops) {
        if (!read_channels(in, sink.acquire(), N)) { sink.release(); break; }
        sink.submit();
    }
    sink.drain();
    fprintf(stderr, "%zu channels x %zu blocks on %d device part(s)\n", C, loops, gpus);
    return 0;
}

// one channel per file, all channels in one bank
static int run_bank(const std::vector<const char*>& paths, const char* prefix, uint32_t freq, uint32_t rate, uint32_t resample)
{
    const size_t C = paths.size(), N = fm::DEFAULT_BUF_LENGTH;
    std::vector<File> in, out;
    if (!open_channels(paths, prefix, in, out)) return 2;
    const auto settings = fm::optimal_settings(freq, rate, resample);
    fm::DemodBank bank(settings.second, (uint32_t)C);
    std::vector<uint8_t> buf(C * N);
    size_t loops = 0;
    for (; read_channels(in, buf.data(), N); ++loops) {
        const auto audio = bank.demodulate(buf.data(), N);
        for (size_t c = 0; c < C; ++c) fm::output(audio[c], out[c].get());
    }
    fprintf(stderr, "%zu channels x %zu blocks\n", C, loops);
    return 0;
}

// receive() + process() of the example over rtl_tcp (-t host:port)
static int run_rtl_tcp(const char* hostport, uint32_t freq, uint32_t rate, uint32_t resample, size_t max_blocks)
{
    // host, host:port, [v6-literal] or [v6-literal]:port (a bare IPv6 literal holds colons of its own); port 1 ... 65535
    std::string host(hostport), portstr;
    uint16_t port = 1234;                                    // rtl_tcp's default
    if (!host.empty() && host[0] == '[') {
        const size_t close = host.find(']');
        if (close == std::string::npos) { fprintf(stderr, "-t %s: missing ']'\n", hostport); return 2; }
        if (close + 1 < host.size()) {
            if (host[close + 1] != ':') { fprintf(stderr, "-t %s: expected ':port' after ']'\n", hostport); return 2; }
            portstr = host.substr(close + 2);
        }
        host = host.substr(1, close - 1);
    } else if (std::count(host.begin(), host.end(), ':') == 1) {
        const size_t colon = host.find(':');
        portstr = host.substr(colon + 1);
        host.resize(colon);
    }                                                        // (several colons without brackets: an IPv6 literal, default port)
    if (!portstr.empty()) {
        char* end = nullptr;
        const unsigned long v = strtoul(portstr.c_str(), &end, 10);
        if (*end != '\0' || v < 1 || v > 65535) { fprintf(stderr, "-t %s: port must be 1 ... 65535\n", hostport); return 2; }
        port = (uint16_t)v;
    }
    if (host.empty()) { fprintf(stderr, "-t %s: empty host\n", hostport); return 2; }
    const auto settings = fm::optimal_settings(freq, rate, resample);           // :48
    const fm::DemodConfig& dc = settings.second;
    fm::RtlTcpSource sdr(host, port);
    fprintf(stderr, "rtl_tcp %s:%u tuner type %u, %u gains\n", host.c_str(), (unsigned)port, sdr.tuner_type(), sdr.gain_count());
    sdr.set_tuner_gain_auto();                                                   // config_sdr, :217-229
    sdr.set_bias_tee(false);
    sdr.set_center_freq(settings.first.capture_freq);
    sdr.set_sample_rate(settings.first.capture_rate);
    fprintf(stderr, "Oversampling input by: %ux\n", dc.downsample);            // :138
    fprintf(stderr, "Output at %u Hz\n", dc.rate_in);                          // :139
    fm::Demod demod(dc);                                                         // :137
    std::vector<uint8_t> buf(fm::DEFAULT_BUF_LENGTH);
    size_t loops = 0;
    std::chrono::duration<double> total(0);
    while (max_blocks == 0 || loops < max_blocks) {
        const size_t n = sdr.read_sync(buf.data(), buf.size());                  // :116
        if (n < buf.size()) {                                                    // :122-125
            fprintf(stderr, "Short read (%zu bytes), samples lost, exiting!\n", n);
            break;
        }
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<int16_t> audio = demod.demodulate(buf);               // :153
        total += std::chrono::steady_clock::now() - t0;
        fm::output(audio);                                                       // :156
        ++loops;
    }
    if (loops) fprintf(stderr, "Average processing time: %.2fms (%zu loops)\n", 1e3 * total.count() / (double)loops, loops);   // :162-168
    return 0;
}

// What the -S loop needs of a mode: run() takes a block of the capture and returns one row per station.
struct StationMode {
    std::function<fm::Rows(const uint8_t*, size_t)> run;     // empty: the mode's arguments were bad (said on stderr)
    const char* suffix;                                      // station k's rows go to <prefix>.<k><suffix>; nullptr: to no file
    std::string banner;                                      // what the mode says on stderr once its bank exists
    bool run_tail = false;                                   // a short last block is still run
    std::function<void()> report = nullptr;                  // what the mode prints on stdout after the last block
};

// one capture and its stations: the capture rate, the front end's decimation, one phase increment and one offset per station
struct Stations {
    uint32_t capture, D;
    std::vector<uint32_t> incs;
    std::vector<long> offsets;
    std::vector<int16_t> boxcar() const { return std::vector<int16_t>(D, 1); }   // the reference's own prototype filter
};

template <class Bank>
static std::function<fm::Rows(const uint8_t*, size_t)> runner(std::shared_ptr<Bank> bank)
{
    return [bank](const uint8_t* buf, size_t n) { return bank->run(buf, n); };
}

static std::string rate_banner(const char* what, const Stations& s, uint32_t R, const char* format)
{
    char line[160];
    snprintf(line, sizeof line, "%s: %.3f Hz%s\n", what, (double)s.capture / s.D / R, format);
    return line;
}

static StationMode bank_mode(const Stations& s, const fm::DemodConfig& dc)
{
    auto bank = std::make_shared<fm::StationBank>(s.boxcar(), s.D, fm::boxcar_shift(s.D, 16384), s.incs, 1, dc.rate_out, dc.rate_resample);
    return {[bank](const uint8_t* buf, size_t n) { return bank->demodulate(buf, n); }, ".s16", ""};
}

// -I: the channelizer
static StationMode iq_mode(const Stations& s)
{
    return {runner(std::make_shared<fm::Channelizer>(s.boxcar(), s.D, fm::boxcar_shift(s.D, 16384), s.incs, 1)), ".cs16", ""};
}

// -2: the front end's shift keeps every |y| component <= 256, where the reference's discriminator cannot wrap
static StationMode stereo_mode(const Stations& s)
{
    const uint32_t f_m = s.capture / s.D, R = std::max<uint32_t>(1, f_m / 48000);
    const std::vector<int16_t> g = fm::stereo_taps((double)f_m, 127);
    const fmd_stereo_config cfg{s.capture, 4096, R, fm::default_audio_shift(g, s.capture, s.D), fm::default_pilot_min(s.capture, s.D)};
    return {runner(std::make_shared<fm::StereoBank>(s.boxcar(), s.D, fm::boxcar_shift(s.D, 256), s.incs, 1, g, cfg)), ".s16",
            rate_banner("stereo audio", s, R, " (interleaved L/R s16)")};
}

// -N mode[:R[:lo:hi]]: 256 channel taps from fm::narrow_taps; chan_shift keeps |u| <= 256 in fm mode (where the reference's
// discriminator cannot wrap), <= 16384 otherwise; squelch blocks of 256 samples, gain 1.0
static StationMode narrow_mode(const Stations& s, const char* spec, uint32_t squelch)
{
    char mode[8] = {0};
    unsigned R = 0;
    double lo = 0, hi = 0;
    const int got = sscanf(spec, "%7[a-z]:%u:%lf:%lf", mode, &R, &lo, &hi);
    const uint32_t f_m = s.capture / s.D;
    uint32_t m;
    if (!strcmp(mode, "iq") || !strcmp(mode, "raw")) m = FMD_NARROW_IQ;
    else if (!strcmp(mode, "fm")) m = FMD_NARROW_FM;
    else if (!strcmp(mode, "am")) m = FMD_NARROW_AM;
    else if (!strcmp(mode, "usb") || !strcmp(mode, "lsb")) m = FMD_NARROW_SSB;
    else { fprintf(stderr, "bad -N mode: %s (iq, fm, am, usb, lsb)\n", spec); return {nullptr, nullptr, ""}; }
    if (got < 2 || R == 0) R = std::max<uint32_t>(1, f_m / 12000);
    if (got < 4) {
        if (!strcmp(mode, "usb")) { lo = 300; hi = 3000; }
        else if (!strcmp(mode, "lsb")) { lo = -3000; hi = -300; }
        else { hi = m == FMD_NARROW_AM ? 4000 : 6000; lo = -hi; }
    }
    const bool iq = m == FMD_NARROW_IQ;
    const auto g = fm::narrow_taps((double)f_m, 256, lo, hi);
    const uint32_t shift = fm::boxcar_shift(s.D, 16384);
    const uint32_t cs = fm::narrow_chan_shift(fm::boxcar_y_bound(s.D, shift), g.first, g.second, m == FMD_NARROW_FM ? 256 : 16384);
    const fmd_narrow_config cfg{m, R, cs, 256, squelch, 256};
    return {runner(std::make_shared<fm::NarrowBank>(s.boxcar(), s.D, shift, s.incs, 1, g.first, g.second, cfg)), iq ? ".cs16" : ".s16",
            rate_banner((std::string("narrow-band ") + mode).c_str(), s, R, iq ? " (interleaved I/Q s16)" : " (s16)")};
}

// -R [-I]: fm::rds_front_taps in front (the boxcar would cut the 57 kHz subcarrier), one host decoder per station.  RDS is slow:
// the tail of a short capture may hold its last group, so it is still run.
static StationMode rds_mode(const Stations& s, bool iq_out)
{
    const uint32_t f_m = s.capture / s.D, R = std::max<uint32_t>(1, f_m / 7500);
    const auto h = fm::rds_front_taps(s.capture);
    const auto g = fm::rds_taps((double)f_m, 255);
    const fmd_rds_config cfg{s.capture, 4096, R, g.second, fm::default_pilot_min(s.capture, s.D)};
    auto bank = std::make_shared<fm::RdsBank>(h.first, s.D, h.second, s.incs, 1, g.first, cfg);
    auto decoders = std::make_shared<std::vector<std::unique_ptr<fm::RdsDecoder>>>();
    for (size_t k = 0; k < s.incs.size(); ++k) decoders->emplace_back(new fm::RdsDecoder(s.capture, s.D * R));
    const std::vector<long> offsets = s.offsets;
    return {[bank, decoders](const uint8_t* buf, size_t n) {
                fm::Rows rows = bank->run(buf, n);
                for (size_t k = 0; k < decoders->size(); ++k) (void)(*decoders)[k]->push(rows[k]);
                return rows;
            },
            iq_out ? ".rds.cs16" : nullptr, rate_banner("RDS baseband", s, R, ""), true,
            [decoders, offsets] {
                for (size_t k = 0; k < decoders->size(); ++k) {
                    const fmd_rds_info i = (*decoders)[k]->info();
                    printf("%ld %04X %s \"%s\" %llu %llu\n", offsets[k], (unsigned)i.pi, i.ps, i.rt, (unsigned long long)i.groups_ok,
                           (unsigned long long)i.blocks_bad);
                }
            }};
}

// -S: one capture, K stations (fmd_stations_*; -I, -2, -N, -R: another bank over the same stations)
static int run_stations(const char* path, const char* list, const char* prefix, uint32_t freq, uint32_t rate, uint32_t resample,
                        bool iq_out, bool stereo, const char* narrow, uint32_t squelch, bool rds)
{
    const File in = open_input(path);
    if (!in) return 2;
    const auto settings = fm::optimal_settings(freq, rate, resample);
    Stations s{settings.first.capture_rate, settings.second.downsample, {}, {}};
    for (const char* p = list; *p;) {
        char* end = nullptr;
        const long off = strtol(p, &end, 10);
        if (end == p) { fprintf(stderr, "bad -S list: %s\n", list); return 2; }
        s.incs.push_back(fm::phase_inc((int32_t)off, s.capture));
        s.offsets.push_back(off);
        p = *end == ',' ? end + 1 : end;
    }
    const StationMode mode = rds ? rds_mode(s, iq_out) : narrow ? narrow_mode(s, narrow, squelch) : stereo ? stereo_mode(s)
                             : iq_out ? iq_mode(s) : bank_mode(s, settings.second);
    if (!mode.run) return 2;
    fprintf(stderr, "%scapture_rate: %u, %zu stations, decimate %u\n", mode.banner.c_str(), s.capture, s.incs.size(), s.D);
    std::vector<File> out;
    for (size_t k = 0; k < s.incs.size() && mode.suffix; ++k) {
        out.push_back(open_output(prefix, k, mode.suffix));
        if (!out.back()) return 2;
    }
    std::vector<uint8_t> buf(fm::DEFAULT_BUF_LENGTH);
    for (;;) {
        size_t fill = read_block(in.get(), buf.data(), buf.size());
        if (fill < buf.size()) {
            if (!mode.run_tail || fill < 8) { note_dropped(fill, block_of(buf.size())); break; }
            fill &= ~(size_t)7;
        }
        const fm::Rows rows = mode.run(buf.data(), fill);
        for (size_t k = 0; k < out.size(); ++k) fm::output(rows[k], out[k].get());
        if (fill < buf.size()) break;
    }
    if (mode.report) mode.report();
    return 0;
}

// -P: one capture, its power spectrum (fmd_spectrum_*)
static int run_power(const char* path, uint32_t n_bins, uint32_t hop, uint32_t rate)
{
    const File in = open_input(path);
    if (!in) return 2;
    fm::Spectrum sp(fm::hann_window(n_bins), hop ? hop : n_bins, 16);
    std::vector<uint64_t> total(n_bins, 0);
    std::vector<uint8_t> buf(fm::DEFAULT_BUF_LENGTH);
    size_t blocks = 0, fill;
    for (; (fill = read_block(in.get(), buf.data(), buf.size())) == buf.size(); ++blocks) {
        const std::vector<uint64_t> p = sp.power(buf.data(), buf.size());
        for (uint32_t k = 0; k < n_bins; ++k) total[k] += p[k];          // modulo 2^64, as the device path accumulates
    }
    note_dropped(fill, block_of(buf.size()));
    fprintf(stderr, "%zu blocks, %u bins of %.1f Hz\n", blocks, n_bins, (double)rate / n_bins);
    for (uint32_t i = 0; i < n_bins; ++i) {
        const uint32_t k = (i + n_bins / 2) % n_bins;                    // frequency order: -N/2 ... N/2 - 1
        printf("%.3f %llu\n", sp.bin_offset_hz(k, rate), (unsigned long long)total[k]);
    }
    return 0;
}

// -U: one capture, every channel of a band plan (fmd_uniform_*)
static int run_uniform(const char* path, const char* spec, const char* select, const char* prefix, uint32_t rate)
{
    unsigned N = 0, hop = 0, P = 8;
    if (sscanf(spec, "%u:%u:%u", &N, &hop, &P) < 2 || !N || !hop || !P) { fprintf(stderr, "bad -U N:hop[:taps_per_channel]: %s\n", spec); return 2; }
    std::vector<uint32_t> sel;
    for (const char* p = select; p && *p;) {
        char* end = nullptr;
        const unsigned long k = strtoul(p, &end, 10);
        if (end == p) { fprintf(stderr, "bad -C list: %s\n", select); return 2; }
        sel.push_back((uint32_t)k);
        p = *end == ',' ? end + 1 : end;
    }
    const File in = open_input(path);
    if (!in) return 2;
    const std::vector<int16_t> taps = fm::uniform_taps(N, P);
    const uint32_t shift = fm::uniform_auto_shift(taps, N, sel);
    fm::UniformChannelizer uc(taps, N, hop, shift, sel);
    fprintf(stderr, "%u of %u channels of %.1f Hz, %zu taps, shift %u, output at %.1f Hz\n", uc.n_selected(), N, (double)rate / N,
            taps.size(), shift, (double)rate / hop);
    std::vector<File> out;
    for (uint32_t i = 0; i < uc.n_selected(); ++i) {
        const uint32_t k = sel.empty() ? i : sel[i];
        fprintf(stderr, "channel %u at %+.1f Hz -> %s.%u.cs16\n", k, (2 * k < N ? (double)k : (double)k - N) * rate / N, prefix, k);
        out.push_back(open_output(prefix, k, ".cs16"));
        if (!out.back()) return 2;
    }
    const size_t frame = 2 * (size_t)hop;
    std::vector<uint8_t> buf(std::max<size_t>(1, fm::DEFAULT_BUF_LENGTH / frame) * frame);   // whole hops per call
    for (;;) {
        const size_t fill = read_block(in.get(), buf.data(), buf.size()), whole = fill / frame * frame;
        if (whole) {
            const auto rows = uc.run(buf.data(), whole);
            for (size_t k = 0; k < out.size(); ++k) fm::output(rows[k], out[k].get());
        }
        if (fill < buf.size()) { note_dropped(fill - whole, "hop of " + std::to_string(frame) + " bytes"); break; }
    }
    return 0;
}

// one capture to stdout: main() of the example with READ_FROM_FILE = true (simple_fm.rs:65-84)
static int run_file(const char* path, uint32_t freq, uint32_t rate, uint32_t resample, size_t per_launch)
{
    const File in = open_input(path);
    if (!in) return 2;
    const auto settings = fm::optimal_settings(freq, rate, resample);
    const fm::DemodConfig& dc = settings.second;
    fprintf(stderr, "Oversampling input by: %ux\n", dc.downsample);             // simple_fm.rs:138
    fprintf(stderr, "Output at %u Hz\n", dc.rate_in);                           // :139
    fprintf(stderr, "Output scale: %u\n", dc.output_scale);                     // :140
    fprintf(stderr, "capture_rate: %u capture_freq: %u\n", settings.first.capture_rate, settings.first.capture_freq);
    fm::Demod demod(dc);
    // -b N: N blocks per launch with the result of N single calls (the f64 sample at every block start, :359)
    if (per_launch > 1) demod.set_block_len(fm::DEFAULT_BUF_LENGTH);
    std::vector<uint8_t> buf(fm::DEFAULT_BUF_LENGTH * per_launch);
    size_t fill, loops = 0;
    std::chrono::duration<double> total(0);
    while ((fill = read_block(in.get(), buf.data(), buf.size())) == buf.size()) {
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<int16_t> audio = demod.demodulate(buf);              // :80
        total += std::chrono::steady_clock::now() - t0;
        fm::output(audio);                                                      // :82
        loops += per_launch;
    }
    if (per_launch > 1 && fill >= fm::DEFAULT_BUF_LENGTH) {                     // complete blocks of a partly filled launch
        const size_t whole = fill / fm::DEFAULT_BUF_LENGTH * fm::DEFAULT_BUF_LENGTH;
        fm::output(demod.demodulate(buf.data(), whole));
        loops += whole / fm::DEFAULT_BUF_LENGTH;
        fill -= whole;
    }
    note_dropped(fill, block_of(fm::DEFAULT_BUF_LENGTH));
    if (loops)                                                                  // :162-168
        fprintf(stderr, "Average processing time: %.2fms (%zu loops)\n", 1e3 * total.count() / (double)loops, loops);
    return 0;
}

int main(int argc, char** argv)
{
    uint32_t rate = 170000, resample = 32000, freq = 94900000;
    size_t per_launch = 1;                                   // -b: reference blocks handed to the GPU per launch
    int gpus = 0;                                            // -g N: several files through the pipelined sink on N GPUs
    const char* prefix = "audio";
    const char* rtl_tcp = nullptr;                           // -t host:port: live mode over rtl_tcp
    const char* stations = nullptr;                          // -S off1,off2,...: station bank over one capture
    bool iq_out = false;                                     // -I: with -S, each station's baseband IQ instead of audio
    bool rds = false;                                        // -R: with -S, each station's RDS (fmd_rds_*, fmd_rds_decoder_*)
    bool stereo = false;                                     // -2: with -S, each station's stereo audio (fmd_stereo_*)
    const char* narrow = nullptr;                            // -N mode[:R[:lo:hi]]: with -S, narrow-band channels (fmd_narrow_*)
    uint32_t squelch = 0;                                    // -q: their squelch (RMS amplitude; 0 = always open)
    uint32_t power_bins = 0, power_hop = 0;                  // -P N [-H hop]: power spectrum of one capture
    const char* uniform = nullptr;                           // -U N:hop[:taps_per_channel]: uniform channelizer over one capture
    const char* uniform_sel = nullptr;                       // -C k1,k2,...: with -U, only these channels
    size_t max_blocks = 0;                                   // -n: stop after this many blocks (live mode; 0 = until the stream ends)
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-s") && i + 1 < argc) rate = (uint32_t)strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-r") && i + 1 < argc) resample = (uint32_t)strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-f") && i + 1 < argc) freq = (uint32_t)strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-o") && i + 1 < argc) prefix = argv[++i];
        else if (!strcmp(argv[i], "-g") && i + 1 < argc) gpus = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-t") && i + 1 < argc) rtl_tcp = argv[++i];
        else if (!strcmp(argv[i], "-S") && i + 1 < argc) stations = argv[++i];
        else if (!strcmp(argv[i], "-I")) iq_out = true;
        else if (!strcmp(argv[i], "-2")) stereo = true;
        else if (!strcmp(argv[i], "-R")) rds = true;
        else if (!strcmp(argv[i], "-N") && i + 1 < argc) narrow = argv[++i];
        else if (!strcmp(argv[i], "-q") && i + 1 < argc) squelch = (uint32_t)strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-P") && i + 1 < argc) power_bins = strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-H") && i + 1 < argc) power_hop = strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-U") && i + 1 < argc) uniform = argv[++i];
        else if (!strcmp(argv[i], "-C") && i + 1 < argc) uniform_sel = argv[++i];
        else if (!strcmp(argv[i], "-n") && i + 1 < argc) max_blocks = strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-b") && i + 1 < argc) { per_launch = strtoul(argv[++i], nullptr, 10); if (!per_launch) per_launch = 1; }
        else if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) {
            fprintf(stderr, "usage: %s [-f freq_hz] [-s sample_rate_hz] [-r resample_hz] [-b blocks_per_launch] <capture.bin | ->\n"
                            "       %s [-s ...] [-r ...] [-o prefix] [-g n_gpus] <a.bin> <b.bin> ...   (one channel per file)\n"
                            "       %s [-f freq_hz] [-s ...] [-r ...] [-n blocks] -t host:port            (live: IQ from an rtl_tcp server)\n"
                            "       %s [-s ...] [-r ...] [-o prefix] -S off1,off2,... <capture.bin | ->   (stations at these offsets in Hz)\n"
                            "       %s [-s ...] [-o prefix] -S off1,off2,... -I <capture.bin | ->        (their baseband: s16 I/Q at capture_rate / downsample)\n"
                            "       %s [-s ...] [-o prefix] -S off1,off2,... -2 <capture.bin | ->        (their stereo: s16 L/R at capture_rate / downsample / R)\n"
                            "       %s [-s ...] [-o prefix] -S off1,off2,... -N mode[:R[:lo:hi]] [-q squelch] <capture.bin | ->   (narrow-band channels: iq, fm, am, usb, lsb at capture_rate / downsample / R)\n"
                            "       %s [-s ...] [-o prefix] -S off1,off2,... -R [-I] <capture.bin | ->   (their RDS: offset_hz PI PS \"radiotext\" groups_ok blocks_bad; -I: baseband to prefix.k.rds.cs16)\n"
                            "       %s -s capture_rate_hz -P n_bins [-H hop] <capture.bin | ->       (power spectrum: offset_hz power per bin)\n"
                            "       %s -s capture_rate_hz [-o prefix] -U N:hop[:taps_per_channel] [-C k1,k2,...] <capture.bin | ->   (band plan: channel k's s16 I/Q at capture_rate / hop to prefix.k.cs16)\n",
                    argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
            return 0;
        } else paths.push_back(argv[i]);
    }
    try {                                                    // every path: an fm::Error is its message on stderr and exit code 1
        if (rtl_tcp) return run_rtl_tcp(rtl_tcp, freq, rate, resample, max_blocks);
        if (paths.empty()) { fprintf(stderr, "missing input file (use - for stdin)\n"); return 2; }
        if (power_bins) return run_power(paths[0], power_bins, power_hop, rate);
        if (uniform) return run_uniform(paths[0], uniform, uniform_sel, prefix, rate);
        if (stations) return run_stations(paths[0], stations, prefix, freq, rate, resample, iq_out, stereo, narrow, squelch, rds);
        if (paths.size() > 1 && gpus > 0) return run_sink(paths, prefix, freq, rate, resample, gpus);
        if (paths.size() > 1) return run_bank(paths, prefix, freq, rate, resample);
        return run_file(paths[0], freq, rate, resample, per_launch);
    } catch (const fm::Error& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
