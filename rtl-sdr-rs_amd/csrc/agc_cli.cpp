// agc_gpu -- an s16 file or pipe at a steady level, through the automatic gain control of the C ABI (fmd_agc_*; host C++ only,
// through fm::Agc of demod.hpp).  What the banks' CLIs write with a fixed gain comes out at `target`, without clipping:
//
//   band_plan_gpu ... -o out capture.bin && agc_gpu -t 12000 out.3.s16 | resample_gpu -i 12500 -r 48000 - | play -t s16 -r 48k -c 1 -
//
//   agc_gpu [-c 1|2] [-t target] [-b block] [-H hang] [-d decay] [-g gain_max] [in.s16 [out.s16]]
//
// -c: int16 per sample: 1 mono (default), 2 interleaved L/R or I/Q under one common gain.
// -t: the largest |out| (default 12000).  -b: samples per block, a power of two in [16, 4096] (default 256).
// -H: blocks the gain is held after an attack (default 4).  -d: release, decay / 256 of the gap per block (default 32).
// -g: the gain of a quiet input in Q10 (default 65536: 64 x).
// in.s16 defaults to stdin (also "-"), out.s16 to stdout.  The AGC emits a block once the next one is complete, so the tool appends
// 2 block zero samples at the end of the input and trims the output to the input's length: every input sample comes out.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "demod.hpp"

static const char* const kUsage =
    "usage: %s [-c 1|2] [-t target] [-b block] [-H hang] [-d decay] [-g gain_max] [in.s16 [out.s16]]\n"
    "       (automatic gain control: raw s16 in, mono or interleaved pairs (-c 2), raw s16 of the same length at |out| <= target)\n";

static int run(const char* in_path, const char* out_path, const fmd_agc_config& cfg, uint32_t width)
{
    fm::File in(in_path && strcmp(in_path, "-") ? fopen(in_path, "rb") : stdin);
    if (!in) { perror(in_path); return 2; }
    fm::Agc agc(cfg, 1, width);                              // (out of the domain, or no device: before the output exists)
    fm::File out(out_path ? fopen(out_path, "wb") : stdout);
    if (!out) { perror(out_path); return 2; }
    std::vector<int16_t> buf(fm::kReadSamples * width);
    uint64_t taken = 0, written = 0;                         // samples
    const auto emit = [&](const fm::Rows& rows) {
        std::vector<int16_t> y = rows[0];
        const uint64_t n = std::min<uint64_t>(y.size() / width, taken - written);
        y.resize(n * width);
        fm::output(y, out.get());
        written += n;
    };
    for (;;) {
        const size_t n = fm::read_samples(in.get(), buf.data(), width);
        if (n) { taken += n; emit(agc.run(buf.data(), n)); }
        if (n < fm::kReadSamples) break;
    }
    if (taken) {
        const std::vector<int16_t> zeros(2u * cfg.block * width, 0);
        emit(agc.run(zeros.data(), 2u * cfg.block));
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

int main(int argc, char** argv)
{
    fmd_agc_config cfg{256, 12000, 65536, 4, 32};
    uint32_t width = 1;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        uint32_t* v = nullptr;
        if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) { fprintf(stderr, kUsage, argv[0]); return 0; }
        else if (!strcmp(argv[i], "-c")) v = &width;
        else if (!strcmp(argv[i], "-t")) v = &cfg.target;
        else if (!strcmp(argv[i], "-b")) v = &cfg.block;
        else if (!strcmp(argv[i], "-H")) v = &cfg.hang;
        else if (!strcmp(argv[i], "-d")) v = &cfg.decay;
        else if (!strcmp(argv[i], "-g")) v = &cfg.gain_max;
        if (!v) { paths.push_back(argv[i]); continue; }
        if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", argv[i]); return 2; }
        if (!number(argv[i + 1], v)) { fprintf(stderr, "bad %s: %s\n", argv[i], argv[i + 1]); return 2; }
        ++i;
    }
    if (width != 1 && width != 2) { fprintf(stderr, "bad -c: need 1 or 2\n"); return 2; }
    if (paths.size() > 2) { fprintf(stderr, "too many files\n"); return 2; }
    return fm::exit_code([&] { return run(paths.empty() ? nullptr : paths[0], paths.size() > 1 ? paths[1] : nullptr, cfg, width); });
}
