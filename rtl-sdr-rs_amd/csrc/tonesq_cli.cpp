// tonesq_gpu -- an s16 file or pipe gated by its sub-audible tone, through the tone squelch of the C ABI (fmd_tonesq_*; host C++
// only, through fm::ToneSquelch of demod.hpp).  What the narrow-band and band-plan banks' CLIs write for an NFM channel comes out
// muted except while one of the accepted CTCSS tones is sent:
//
//   band_plan_gpu ... -o out capture.bin && tonesq_gpu -r 12500 -a 100.0,123.0 out.3.s16 | agc_gpu -t 12000 | play -t s16 -r 12500 -c 1 -
//
//   tonesq_gpu -r rate [-c 1|2] [-b block] [-a tone_hz,...] [in.s16 [out.s16]]
//
// -r: the sample rate of the input in Hz (required).  -c: int16 per sample: 1 mono (default), 2 interleaved L/R.
// -b: samples per decision block, a power of two in [64, 4096] (default 4096; 64 CTCSS tones' worth of table ends there).
// -a: the tones that open the gate, Hz, each one of the 38 standard CTCSS tones (default: every one of them).
// in.s16 defaults to stdin (also "-"), out.s16 to stdout.  The gated audio has the input's length.  Whenever a completed block
// changes the selected tone or the gate, one line `block tone_hz power open` goes to stderr (tone_hz `-` for none).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "demod.hpp"

static const char* const kUsage =
    "usage: %s -r rate [-c 1|2] [-b block] [-a tone_hz,...] [in.s16 [out.s16]]\n"
    "       (tone squelch: raw s16 in, mono or interleaved pairs (-c 2), raw s16 of the same length, muted unless an accepted CTCSS tone is sent)\n";

static int run(const char* in_path, const char* out_path, const fmd_tonesq_config& cfg, double rate, uint32_t width)
{
    fm::File in(in_path && strcmp(in_path, "-") ? fopen(in_path, "rb") : stdin);
    if (!in) { perror(in_path); return 2; }
    const std::vector<double>& tones = fm::ctcss_tones();
    // (a block the library refuses anyway gets no table: its refusal is the message.  Out of the domain, or no device: before the
    // output exists)
    const bool sane = cfg.block >= 1 && cfg.block <= 8192;
    fm::ToneSquelch sq(cfg, sane ? fm::tone_table(rate, tones, cfg.block) : std::vector<int16_t>(2), 1, width);
    fm::File out(out_path ? fopen(out_path, "wb") : stdout);
    if (!out) { perror(out_path); return 2; }
    std::vector<int16_t> buf(fm::kReadSamples * width);
    uint64_t taken = 0;                                      // samples
    fm::ToneSquelch::Status last{-1, 0, false};
    for (;;) {
        const size_t n = fm::read_samples(in.get(), buf.data(), width);
        for (size_t lo = 0; lo < n;) {                       // call by call up to the next block end, for the report
            const size_t hi = std::min<size_t>(n, lo + (cfg.block - (taken % cfg.block)));
            fm::output(sq.run(buf.data() + lo * width, hi - lo)[0], out.get());
            taken += hi - lo;
            lo = hi;
            if (taken % cfg.block == 0) {
                const fm::ToneSquelch::Status st = sq.status()[0];
                if (st.tone != last.tone || st.open != last.open) {
                    if (st.tone >= 0) fprintf(stderr, "%llu %.1f %llu %d\n", (unsigned long long)(taken / cfg.block - 1), tones[st.tone],
                                              (unsigned long long)st.power, st.open ? 1 : 0);
                    else fprintf(stderr, "%llu - %llu %d\n", (unsigned long long)(taken / cfg.block - 1), (unsigned long long)st.power, st.open ? 1 : 0);
                }
                last = st;
            }
        }
        if (n < fm::kReadSamples) break;
    }
    return 0;
}

// a whole decimal number below 2^32
static bool number(const char* s, uint32_t* v)
{
    char* end = nullptr;
    const unsigned long long x = strtoull(s, &end, 10);
    if (end == s || *end || s[0] == '-' || x > 0xFFFFFFFFull) return false;
    *v = (uint32_t)x;
    return true;
}

// "100.0,123" -> the accept bits of those standard tones
static bool accept_list(const char* s, uint64_t* mask)
{
    const std::vector<double>& tones = fm::ctcss_tones();
    *mask = 0;
    while (*s) {
        char* end = nullptr;
        const double hz = strtod(s, &end);
        if (end == s || (*end && *end != ',')) return false;
        size_t k = 0;
        while (k < tones.size() && tones[k] != hz) ++k;
        if (k == tones.size()) return false;
        *mask |= 1ull << k;
        s = *end ? end + 1 : end;
        if (*end && !*s) return false;                       // a trailing comma
    }
    return *mask != 0;
}

int main(int argc, char** argv)
{
    fmd_tonesq_config cfg{4096, 1, 3, 2, 2, 64, 20000000ull, (1ull << 38) - 1};
    uint32_t width = 1, rate = 0;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        uint32_t* v = nullptr;
        if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) { fprintf(stderr, kUsage, argv[0]); return 0; }
        else if (!strcmp(argv[i], "-c")) v = &width;
        else if (!strcmp(argv[i], "-r")) v = &rate;
        else if (!strcmp(argv[i], "-b")) v = &cfg.block;
        else if (!strcmp(argv[i], "-a")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", argv[i]); return 2; }
            if (!accept_list(argv[i + 1], &cfg.accept)) { fprintf(stderr, "bad -a: %s\n", argv[i + 1]); return 2; }
            ++i;
            continue;
        }
        if (!v) { paths.push_back(argv[i]); continue; }
        if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", argv[i]); return 2; }
        if (!number(argv[i + 1], v)) { fprintf(stderr, "bad %s: %s\n", argv[i], argv[i + 1]); return 2; }
        ++i;
    }
    if (width != 1 && width != 2) { fprintf(stderr, "bad -c: need 1 or 2\n"); return 2; }
    if (rate == 0) { fprintf(stderr, "need -r rate\n"); return 2; }
    if (paths.size() > 2) { fprintf(stderr, "too many files\n"); return 2; }
    if (cfg.block && cfg.ramp > cfg.block) cfg.ramp = cfg.block;
    return fm::exit_code([&] { return run(paths.empty() ? nullptr : paths[0], paths.size() > 1 ? paths[1] : nullptr, cfg, rate, width); });
}
