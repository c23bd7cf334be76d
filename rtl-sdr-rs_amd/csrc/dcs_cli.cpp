// dcs_gpu -- an s16 file or pipe gated by its digital code (DCS), through the code squelch of the C ABI (fmd_dcs_*; host C++ only,
// through fm::CodeSquelch of demod.hpp).  What the narrow-band and band-plan banks' CLIs write for an NFM channel comes out muted
// except while one of the accepted DCS codes is sent:
//
//   band_plan_gpu ... -o out capture.bin && dcs_gpu -r 12500 -a 023,114 out.3.s16 | agc_gpu -t 12000 | play -t s16 -r 12500 -c 1 -
//
//   dcs_gpu -r rate [-c 1|2] [-a code,...] [-i] [in.s16 [out.s16]]
//
// -r: the sample rate of the input in Hz (required); the detector is fm::dcs_design(rate).
// -c: int16 per sample: 1 mono (default), 2 interleaved L/R.
// -a: the codes that open the gate, octal, each one of the 104 standard DCS codes (default: every one of them).
// -i: the input's polarity is inverted (a discriminator of the other sign): the table holds the complemented words.
// in.s16 defaults to stdin (also "-"), out.s16 to stdout.  The gated audio has the input's length.  Whenever a completed block
// changes the selected code or the gate, one line `block code hits open` goes to stderr (code in octal, `-` for none).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "demod.hpp"

static const char* const kUsage =
    "usage: %s -r rate [-c 1|2] [-a code,...] [-i] [in.s16 [out.s16]]\n"
    "       (code squelch: raw s16 in, mono or interleaved pairs (-c 2), raw s16 of the same length, muted unless an accepted DCS code is sent)\n";

static int run(const char* in_path, const char* out_path, const fmd_dcs_config& cfg, bool inverted, uint32_t width)
{
    fm::File in(in_path && strcmp(in_path, "-") ? fopen(in_path, "rb") : stdin);
    if (!in) { perror(in_path); return 2; }
    const std::vector<uint32_t>& codes = fm::dcs_codes();
    std::vector<uint32_t> words;
    for (uint32_t code : codes) words.push_back(fm::dcs_word(code, inverted));
    fm::CodeSquelch sq(cfg, words, 1, width);                // (out of the domain, or no device: before the output exists)
    fm::File out(out_path ? fopen(out_path, "wb") : stdout);
    if (!out) { perror(out_path); return 2; }
    std::vector<int16_t> buf(fm::kReadSamples * width);
    uint64_t taken = 0;                                      // samples
    fm::CodeSquelch::Status last{-1, 0, false};
    for (;;) {
        const size_t n = fm::read_samples(in.get(), buf.data(), width);
        for (size_t lo = 0; lo < n;) {                       // call by call up to the next block end, for the report
            const size_t hi = std::min<size_t>(n, lo + (cfg.block - (taken % cfg.block)));
            fm::output(sq.run(buf.data() + lo * width, hi - lo)[0], out.get());
            taken += hi - lo;
            lo = hi;
            if (taken % cfg.block == 0) {
                const fm::CodeSquelch::Status st = sq.status()[0];
                if (st.code != last.code || st.open != last.open) {
                    if (st.code >= 0) fprintf(stderr, "%llu %03o %u %d\n", (unsigned long long)(taken / cfg.block - 1), codes[st.code], st.hits, st.open ? 1 : 0);
                    else fprintf(stderr, "%llu - %u %d\n", (unsigned long long)(taken / cfg.block - 1), st.hits, st.open ? 1 : 0);
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

// "023,114" -> the accept bits of those standard codes
static bool accept_list(const char* s, uint64_t* mask)
{
    const std::vector<uint32_t>& codes = fm::dcs_codes();
    mask[0] = mask[1] = 0;
    while (*s) {
        char* end = nullptr;
        if (*s < '0' || *s > '7') return false;
        const unsigned long code = strtoul(s, &end, 8);
        if (end == s || (*end && *end != ',')) return false;
        size_t k = 0;
        while (k < codes.size() && codes[k] != code) ++k;
        if (k == codes.size()) return false;
        mask[k >> 6] |= 1ull << (k & 63);
        s = *end ? end + 1 : end;
        if (*end && !*s) return false;                       // a trailing comma
    }
    return (mask[0] | mask[1]) != 0;
}

int main(int argc, char** argv)
{
    uint32_t width = 1, rate = 0;
    uint64_t accept[2] = {~0ull, (1ull << 40) - 1};          // the 104 codes
    bool inverted = false;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        uint32_t* v = nullptr;
        if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) { fprintf(stderr, kUsage, argv[0]); return 0; }
        else if (!strcmp(argv[i], "-i")) { inverted = true; continue; }
        else if (!strcmp(argv[i], "-c")) v = &width;
        else if (!strcmp(argv[i], "-r")) v = &rate;
        else if (!strcmp(argv[i], "-a")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", argv[i]); return 2; }
            if (!accept_list(argv[i + 1], accept)) { fprintf(stderr, "bad -a: %s\n", argv[i + 1]); return 2; }
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
    return fm::exit_code([&] {
        fmd_dcs_config cfg = fm::dcs_design(rate);
        cfg.accept[0] = accept[0]; cfg.accept[1] = accept[1];
        return run(paths.empty() ? nullptr : paths[0], paths.size() > 1 ? paths[1] : nullptr, cfg, inverted, width);
    });
}
