// fm_receiver_gpu -- complete FM reception of K stations out of ONE wideband capture file: each station's pilot-locked stereo audio
// and its RDS name and text, over the C ABI (fmd_receiver_*, fmd_rds_decoder_*; host C++ only, through fm::ReceiverBank and
// fm::RdsDecoder of demod.hpp).  What simple_fm_gpu -S ... -2 and simple_fm_gpu -S ... -R give in two runs over the same capture, in
// one: the front end, the discriminator and the pilot sums run once per block.
//
//   fm_receiver_gpu [-s rate] [-o prefix] -S off1,off2,... [-I] <capture.bin | ->
//
// -s: as simple_fm_gpu's (default 170000): the capture was recorded at the capture rate optimal_settings derives from it
//     (downsample x rate), and downsample is the front end's decimation.
// -S: the stations' offsets in Hz from the capture's centre.
// The front end is fm::rds_front_taps (a 64-tap low-pass of +-62 kHz: the reference's boxcar would cut the 57 kHz subcarrier) at the
// shift that keeps every |y| component <= 256; the audio stage is the one simple_fm_gpu -2 chooses (127 taps from fm::stereo_taps
// at stride max(1, floor(f_m / 48000)), f_m = capture_rate / downsample, 75 us de-emphasis, blocks of 4096), the RDS stage the one
// -R chooses (255 taps from fm::rds_taps at stride max(1, floor(f_m / 7500))), one host decoder per station.
// Station k's interleaved s16 (L, R) goes to <prefix>.<k>.s16 and, with -I, its RDS baseband as interleaved s16 (ur, ui) to
// <prefix>.<k>.rds.cs16.  At the end stdout gets one line per station, `offset_hz PI PS "radiotext" groups_ok blocks_bad` (PI in
// hex); the rates go to stderr.  RDS is slow -- the tail of a short capture may hold its last group -- so a trailing partial block
// is still run (whole 8 bytes of it), unless it completes no output of one of the two stages.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// fread until `n` bytes are there or the stream ends: the bytes read
static size_t read_block(FILE* in, uint8_t* buf, size_t n)
{
    size_t fill = 0, got;
    while (fill < n && (got = fread(buf + fill, 1, n - fill, in)) > 0) fill += got;
    return fill;
}

static const char* const kUsage =
    "usage: %s [-s rate] [-o prefix] -S off1,off2,... [-I] <capture.bin | ->\n"
    "       (FM receiver: station k's stereo as s16 L/R at capture_rate / downsample / R to prefix.k.s16; -I: its RDS baseband to prefix.k.rds.cs16;\n"
    "        stdout: offset_hz PI PS \"radiotext\" groups_ok blocks_bad of every station)\n";

static int run(const char* path, const char* list, const char* prefix, uint32_t rate, bool iq_out)
{
    std::vector<long> offsets;
    for (const char* p = list; *p;) {
        char* end = nullptr;
        const long off = strtol(p, &end, 10);
        if (end == p) { fprintf(stderr, "bad -S list: %s\n", list); return 2; }
        offsets.push_back(off);
        p = *end == ',' ? end + 1 : end;
    }
    if (offsets.empty()) { fprintf(stderr, "bad -S list: %s\n", list); return 2; }
    const File in = strcmp(path, "-") ? open_file(path, "rb") : File(stdin);
    if (!in) return 2;
    const auto settings = fm::optimal_settings(94900000, rate);
    const uint32_t capture = settings.first.capture_rate, D = settings.second.downsample;
    std::vector<uint32_t> incs;
    for (long off : offsets) incs.push_back(fm::phase_inc((int32_t)off, capture));
    const uint32_t f_m = capture / D, Ra = std::max<uint32_t>(1, f_m / 48000), Rr = std::max<uint32_t>(1, f_m / 7500);
    const auto h = fm::rds_front_taps(capture);
    const std::vector<int16_t> ga = fm::stereo_taps((double)f_m, 127);
    const auto gr = fm::rds_taps((double)f_m, 255);
    const fmd_receiver_config cfg{capture, 4096, fm::default_pilot_min(capture, D), Ra, fm::default_audio_shift(ga, capture, D), Rr, gr.second};
    fm::ReceiverBank bank(h.first, D, h.second, incs, 1, ga, gr.first, cfg);
    std::vector<std::unique_ptr<fm::RdsDecoder>> decoders;
    for (size_t k = 0; k < incs.size(); ++k) decoders.emplace_back(new fm::RdsDecoder(capture, D * Rr));
    fprintf(stderr, "stereo audio: %.3f Hz (interleaved L/R s16)\nRDS baseband: %.3f Hz\ncapture_rate: %u, %zu stations, decimate %u\n",
            (double)capture / D / Ra, (double)capture / D / Rr, capture, incs.size(), D);
    std::vector<File> audio, rds;
    for (size_t k = 0; k < incs.size(); ++k) {
        audio.push_back(open_file(std::string(prefix) + "." + std::to_string(k) + ".s16", "wb"));
        if (!audio.back()) return 2;
        if (!iq_out) continue;
        rds.push_back(open_file(std::string(prefix) + "." + std::to_string(k) + ".rds.cs16", "wb"));
        if (!rds.back()) return 2;
    }
    std::vector<uint8_t> buf(fm::DEFAULT_BUF_LENGTH);
    for (;;) {
        size_t fill = read_block(in.get(), buf.data(), buf.size());
        if (fill < buf.size()) {
            if (fill < 8) { if (fill) fprintf(stderr, "dropped %zu trailing bytes\n", fill); break; }
            fill &= ~(size_t)7;
        }
        const std::pair<fm::Rows, fm::Rows> rows = bank.run(buf.data(), fill);   // (empty rows when a stage completes no output)
        for (size_t k = 0; k < incs.size(); ++k) {
            fm::output(rows.first[k], audio[k].get());
            if (iq_out) fm::output(rows.second[k], rds[k].get());
            (void)decoders[k]->push(rows.second[k]);
        }
        if (fill < buf.size()) break;
    }
    for (size_t k = 0; k < incs.size(); ++k) {
        const fmd_rds_info i = decoders[k]->info();
        printf("%ld %04X %s \"%s\" %llu %llu\n", offsets[k], (unsigned)i.pi, i.ps, i.rt, (unsigned long long)i.groups_ok,
               (unsigned long long)i.blocks_bad);
    }
    return 0;
}

int main(int argc, char** argv)
{
    uint32_t rate = 170000;                                  // SAMPLE_RATE of the reference's example
    const char* prefix = "audio";
    const char* stations = nullptr;                          // -S off1,off2,...
    bool iq_out = false;                                     // -I: the RDS baseband too
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-s") && i + 1 < argc) rate = (uint32_t)strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-o") && i + 1 < argc) prefix = argv[++i];
        else if (!strcmp(argv[i], "-S") && i + 1 < argc) stations = argv[++i];
        else if (!strcmp(argv[i], "-I")) iq_out = true;
        else if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) { fprintf(stderr, kUsage, argv[0]); return 0; }
        else paths.push_back(argv[i]);
    }
    if (!rate || !stations) { fprintf(stderr, "need -S off1,off2,... (and a non-zero -s rate)\n"); return 2; }
    if (paths.empty()) { fprintf(stderr, "missing input file (use - for stdin)\n"); return 2; }
    try {                                                    // an fm::Error is its message on stderr and exit code 1
        return run(paths[0], stations, prefix, rate, iq_out);
    } catch (const fm::Error& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
