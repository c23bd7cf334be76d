// resample_gpu -- an s16 file or pipe at another rate, through the rational resampler of the C ABI (fmd_resample_*; host C++ only,
// through fm::Resampler, fm::resample_ratio and fm::resample_taps of demod.hpp).  What the banks' CLIs write at
// capture_rate / (downsample R) -- 51.2 kHz, 170 kHz, 60 kHz -- becomes a rate a sound device or a codec takes:
//
//   fm_receiver_gpu -S 150000 -o out capture.bin && resample_gpu -i 51200 -r 48000 -c 2 out.0.s16 | play -t s16 -r 48k -c 2 -
//
//   resample_gpu -i rate_in[/den] -r rate_out [-c 1|2] [-T taps_per_phase] <in.s16 | ->
//
// -i: the input rate in Hz, as an integer or a fraction num/den (the banks' rates are rational).
// -r: the output rate in Hz.  rate_out / rate_in in lowest terms is L / M of the resampler and must lie in its domain.
// -c: int16 per sample: 1 mono (default), 2 interleaved L/R or I/Q.
// -T: taps per polyphase branch of fm::resample_taps (default 32).
// The output goes to stdout as raw s16; the ratio and the shift go to stderr.  The stream is read in blocks of 65536 samples; a
// block that completes no output (the first one of a very short input) is kept and handed over again with the next one, so the
// output is that of one call over the whole input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "demod.hpp"

static const char* const kUsage =
    "usage: %s -i rate_in[/den] -r rate_out [-c 1|2] [-T taps_per_phase] <in.s16 | ->\n"
    "       (rational resampler: raw s16 in, mono or interleaved pairs (-c 2), raw s16 at rate_out on stdout)\n";

static int run(const char* path, uint64_t num, uint64_t den, uint64_t rate_out, uint32_t width, uint32_t T)
{
    fm::File in(strcmp(path, "-") ? fopen(path, "rb") : stdin);
    if (!in) { perror(path); return 2; }
    const std::pair<uint32_t, uint32_t> lm = fm::resample_ratio(num, den, rate_out);
    const auto g = fm::resample_taps(lm.first, lm.second, T);
    fm::Resampler rs(g.first, lm.first, lm.second, g.second, 1, width);
    fprintf(stderr, "resample: L / M = %u / %u, %u taps per phase, shift %u, %u int16 per sample\n", lm.first, lm.second, T, g.second, width);
    std::vector<int16_t> buf;
    size_t held = 0;                                         // samples kept from blocks that completed no output
    for (;;) {
        buf.resize((held + fm::kReadSamples) * width);
        const size_t got = fm::read_samples(in.get(), buf.data() + held * width, width), n = held + got;
        if (got) {
            const fm::Rows rows = rs.run(buf.data(), n);
            if (rows[0].empty()) held = n;
            else { fm::output(rows[0]); held = 0; }
        }
        if (got < fm::kReadSamples) break;
    }
    return 0;
}

int main(int argc, char** argv)
{
    const char* rate_in = nullptr;                           // -i rate_in[/den]
    uint64_t rate_out = 0;
    uint32_t width = 1, T = 32;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-i") && i + 1 < argc) rate_in = argv[++i];
        else if (!strcmp(argv[i], "-r") && i + 1 < argc) rate_out = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-c") && i + 1 < argc) width = (uint32_t)strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-T") && i + 1 < argc) T = (uint32_t)strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) { fprintf(stderr, kUsage, argv[0]); return 0; }
        else paths.push_back(argv[i]);
    }
    if (!rate_in || !rate_out) { fprintf(stderr, "need -i rate_in[/den] and a non-zero -r rate_out\n"); return 2; }
    char* end = nullptr;
    const uint64_t num = strtoull(rate_in, &end, 10);
    uint64_t den = 1;
    bool bad = end == rate_in || !num;
    if (!bad && *end == '/') { const char* d = end + 1; den = strtoull(d, &end, 10); bad = end == d || !den; }
    if (bad || *end) { fprintf(stderr, "bad -i rate: %s\n", rate_in); return 2; }
    if (width != 1 && width != 2) { fprintf(stderr, "bad -c: need 1 or 2\n"); return 2; }
    if (T < 1 || T > 256) { fprintf(stderr, "bad -T: need 1 ... 256\n"); return 2; }
    if (paths.empty()) { fprintf(stderr, "missing input file (use - for stdin)\n"); return 2; }
    return fm::exit_code([&] { return run(paths[0], num, den, rate_out, width, T); });
}
