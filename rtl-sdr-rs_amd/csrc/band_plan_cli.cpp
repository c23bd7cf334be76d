// band_plan_gpu -- a band plan's audio and its activity map out of ONE wideband capture file, over the C ABI (fmd_bandplan_*; host
// C++ only, through fm::BandPlanBank of demod.hpp).
//
//   band_plan_gpu -s capture_rate -U N:hop[:taps_per_channel] -N mode[:R[:lo:hi]] [-q squelch] [-C k1,k2,...] [-o prefix] <capture.bin | ->
//
// -U: the plan -- N equally spaced channels, one stage-one output per `hop` samples, prototype fm::uniform_taps(N, taps_per_channel
//     = 8) at the smallest admissible shift.  -C: only these channels (strictly increasing).
// -N: the detector (iq, fm, am, usb, lsb), the second stage's decimation R (1 ... 8; default capture_rate / hop / 12000, at least
//     1 and at most 8) and its band lo ... hi in Hz around the channel's centre (defaults as simple_fm_gpu -N); min(64, 8 R) taps
//     from fm::narrow_taps at capture_rate / hop; chan_shift keeps |u| <= 256 in fm mode, <= 16384 otherwise; squelch blocks of
//     256 samples, gain 1.0.  -q: the squelch (RMS amplitude; 0 = always open).
// Channel k's audio at capture_rate / (hop R) goes to <prefix>.<k>.s16, in iq mode as interleaved (I, Q) pairs to
// <prefix>.<k>.cs16.  At the end stdout gets one line per selected channel, `channel offset_hz open rms`: the activity map of the
// last completed squelch block.  The rate and the plan go to stderr.  Only whole hops are run: trailing bytes that do not fill a hop
// are dropped with a note.
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
    "usage: %s -s capture_rate_hz -U N:hop[:taps_per_channel] -N mode[:R[:lo:hi]] [-q squelch] [-C k1,k2,...] [-o prefix] <capture.bin | ->\n"
    "       (band plan: channel k's audio -- iq, fm, am, usb, lsb -- at capture_rate / hop / R to prefix.k.s16, prefix.k.cs16 in iq mode;\n"
    "        stdout: channel offset_hz open rms of every selected channel)\n";

static int run(const char* path, const char* plan, const char* detector, const char* select, const char* prefix, uint32_t rate, uint32_t squelch)
{
    unsigned N = 0, hop = 0, P = 8;
    if (sscanf(plan, "%u:%u:%u", &N, &hop, &P) < 2 || !N || !hop || !P) { fprintf(stderr, "bad -U N:hop[:taps_per_channel]: %s\n", plan); return 2; }
    char mode[8] = {0};
    unsigned R = 0;
    double lo = 0, hi = 0;
    const int got = sscanf(detector, "%7[a-z]:%u:%lf:%lf", mode, &R, &lo, &hi);
    uint32_t m;
    if (!strcmp(mode, "iq") || !strcmp(mode, "raw")) m = FMD_NARROW_IQ;
    else if (!strcmp(mode, "fm")) m = FMD_NARROW_FM;
    else if (!strcmp(mode, "am")) m = FMD_NARROW_AM;
    else if (!strcmp(mode, "usb") || !strcmp(mode, "lsb")) m = FMD_NARROW_SSB;
    else { fprintf(stderr, "bad -N mode: %s (iq, fm, am, usb, lsb)\n", detector); return 2; }
    std::vector<uint32_t> sel;
    for (const char* p = select; p && *p;) {
        char* end = nullptr;
        const unsigned long k = strtoul(p, &end, 10);
        if (end == p) { fprintf(stderr, "bad -C list: %s\n", select); return 2; }
        sel.push_back((uint32_t)k);
        p = *end == ',' ? end + 1 : end;
    }
    const File in = strcmp(path, "-") ? open_file(path, "rb") : File(stdin);
    if (!in) return 2;
    const double f_m = (double)rate / hop;
    if (got < 2 || R == 0) R = std::min<uint32_t>(8, std::max<uint32_t>(1, (uint32_t)(f_m / 12000)));
    if (got < 4) {
        if (!strcmp(mode, "usb")) { lo = 300; hi = 3000; }
        else if (!strcmp(mode, "lsb")) { lo = -3000; hi = -300; }
        else { hi = m == FMD_NARROW_AM ? 4000 : 6000; lo = -hi; }
    }
    const bool iq = m == FMD_NARROW_IQ;
    const std::vector<int16_t> taps = fm::uniform_taps(N, P);
    const uint32_t shift = fm::uniform_auto_shift(taps, N, sel);
    const auto g = fm::narrow_taps(f_m, std::min<uint32_t>(64, 8 * R), lo, hi);
    const uint32_t cs = fm::narrow_chan_shift(fm::uniform_y_bound(taps, N, shift, sel), g.first, g.second, m == FMD_NARROW_FM ? 256 : 16384);
    const fmd_narrow_config cfg{m, R, cs, 256, squelch, 256};
    fm::BandPlanBank bank(taps, N, hop, shift, sel, 1, g.first, g.second, cfg);
    fprintf(stderr, "%u of %u channels of %.1f Hz, %zu taps, shift %u; %s, %zu channel taps, chan_shift %u, squelch %u, output at %.1f Hz%s\n",
            bank.n_selected(), N, (double)rate / N, taps.size(), shift, mode, g.first.size(), cs, squelch, f_m / R,
            iq ? " (interleaved I/Q s16)" : " (s16)");
    std::vector<File> out;
    std::vector<double> offsets;
    for (uint32_t i = 0; i < bank.n_selected(); ++i) {
        const uint32_t k = sel.empty() ? i : sel[i];
        offsets.push_back((2 * k < N ? (double)k : (double)k - N) * rate / N);
        out.push_back(open_file(std::string(prefix) + "." + std::to_string(k) + (iq ? ".cs16" : ".s16"), "wb"));
        if (!out.back()) return 2;
    }
    const size_t frame = 2 * (size_t)hop;
    std::vector<uint8_t> buf(std::max<size_t>(1, fm::DEFAULT_BUF_LENGTH / frame) * frame);   // whole hops per call
    for (;;) {
        const size_t fill = read_block(in.get(), buf.data(), buf.size()), whole = fill / frame * frame;
        if (whole) {
            const fm::Rows rows = bank.run(buf.data(), whole);   // (empty rows when the call completes no audio sample)
            for (size_t k = 0; k < out.size(); ++k) fm::output(rows[k], out[k].get());
        }
        if (fill < buf.size()) {
            if (fill - whole) fprintf(stderr, "dropped %zu trailing bytes (not a complete hop of %zu bytes)\n", fill - whole, frame);
            break;
        }
    }
    const auto levels = bank.levels();
    for (uint32_t i = 0; i < bank.n_selected(); ++i)
        printf("%u %.1f %d %u\n", sel.empty() ? i : sel[i], offsets[i], levels[i].first ? 1 : 0, levels[i].second);
    return 0;
}

int main(int argc, char** argv)
{
    uint32_t rate = 0, squelch = 0;
    const char* prefix = "audio";
    const char* plan = nullptr;                              // -U N:hop[:taps_per_channel]
    const char* detector = nullptr;                          // -N mode[:R[:lo:hi]]
    const char* select = nullptr;                            // -C k1,k2,...
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-s") && i + 1 < argc) rate = (uint32_t)strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-o") && i + 1 < argc) prefix = argv[++i];
        else if (!strcmp(argv[i], "-U") && i + 1 < argc) plan = argv[++i];
        else if (!strcmp(argv[i], "-N") && i + 1 < argc) detector = argv[++i];
        else if (!strcmp(argv[i], "-C") && i + 1 < argc) select = argv[++i];
        else if (!strcmp(argv[i], "-q") && i + 1 < argc) squelch = (uint32_t)strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) { fprintf(stderr, kUsage, argv[0]); return 0; }
        else paths.push_back(argv[i]);
    }
    if (!rate || !plan || !detector) { fprintf(stderr, "need -s capture_rate_hz, -U N:hop[:taps_per_channel] and -N mode[:R[:lo:hi]]\n"); return 2; }
    if (paths.empty()) { fprintf(stderr, "missing input file (use - for stdin)\n"); return 2; }
    try {                                                    // an fm::Error is its message on stderr and exit code 1
        return run(paths[0], plan, detector, select, prefix, rate, squelch);
    } catch (const fm::Error& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
