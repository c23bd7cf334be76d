// afsk_gpu -- an s16 file or pipe of NFM audio to the AX.25 frames in it, through the packet demodulator of the C ABI (fmd_afsk_* on
// the GPU, fmd_ax25_decoder_* on the host; host C++ only, through fm::AfskDemod and fm::Ax25Decoder of demod.hpp).  What the
// narrow-band and band-plan banks' CLIs write for an NFM channel that carries 1200 baud packet (APRS) comes out as text:
//
//   band_plan_gpu ... -o out capture.bin && afsk_gpu -r 12000 out.3.s16
//
//   afsk_gpu -r rate [-b baud] [-m mark] [-s space] [-D stride] [-G] [in.s16]
//
// -r: the sample rate of the input in Hz (required).  -b: bits per second (default 1200).  -m, -s: the mark and space tones in Hz
// (default 1200 and 2200).  -D: samples between two soft decisions (default: a fifth of a bit).  in.s16 defaults to stdin (also
// "-").  One row, fed call by call as the input arrives.  One line per frame on stdout, `SRC>DST,DIGI*:info` (TNC2; hex where the
// address field is malformed); at the end `frames_ok N bad_fcs N aborts N` on stderr.  -G: the frames come from the frame bank on the
// GPU (fmd_hdlc_*, fm::Ax25Framer) instead of the host decoder; the output is the same.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "demod.hpp"

static const char* const kUsage =
    "usage: %s -r rate [-b baud] [-m mark] [-s space] [-D stride] [in.s16]\n"
    "       (packet demodulator: raw mono s16 of an NFM channel in, one TNC2 line per AX.25 frame out, the counters on stderr)\n";

// The soft decisions of one row through the frame bank, in pieces short enough that none can complete more than frame_cap frames (a
// sample takes at most one bit and a frame has 144): the frames in the order they closed.
static std::vector<fmd_ax25_frame> framed(fm::Ax25Framer& framer, const std::vector<int16_t>& soft)
{
    const size_t piece = (size_t)144 * framer.frame_cap() - 143;
    std::vector<fmd_ax25_frame> res;
    for (size_t lo = 0; lo < soft.size(); lo += piece) {
        framer.run(soft.data() + lo, std::min(piece, soft.size() - lo));
        const std::vector<std::vector<fmd_ax25_frame>> got = framer.frames({0u});
        res.insert(res.end(), got[0].begin(), got[0].end());
    }
    return res;
}

static int run(const char* in_path, uint32_t rate, uint32_t baud, uint32_t mark, uint32_t space, uint32_t stride, bool on_gpu)
{
    fm::File in(in_path && strcmp(in_path, "-") ? fopen(in_path, "rb") : stdin);
    if (!in) { perror(in_path); return 2; }
    // (a window the library refuses anyway gets no designed table: its refusal is the message.  Out of the domain, or no device:
    // before anything is printed)
    const uint64_t T = ((uint64_t)rate + baud / 2) / baud;
    fm::AfskTable tab{std::vector<int16_t>((size_t)std::max<uint64_t>(1, 4 * std::min<uint64_t>(T, 4096))), (uint32_t)T, 8, 12};
    if (T >= 2 && T <= 64) tab = fm::afsk_table(rate, baud, mark, space, (uint32_t)T);
    if (!stride) stride = fm::afsk_stride((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(T, 64)));
    fm::AfskDemod demod(tab.tab, stride, tab.pre_shift, tab.out_shift, 1, 1);
    fm::Ax25Decoder dec(rate, stride, baud);                 // (its refusal of the rate comes first either way)
    std::unique_ptr<fm::Ax25Framer> framer;
    if (on_gpu) framer.reset(new fm::Ax25Framer(rate, stride, baud, 16));
    std::vector<int16_t> buf, chunk(fm::kReadSamples);
    for (;;) {
        const size_t n = fm::read_samples(in.get(), chunk.data(), 1);
        buf.insert(buf.end(), chunk.begin(), chunk.begin() + n);
        if (!buf.empty()) {
            const fm::Rows soft = demod.run(buf.data(), buf.size());   // (empty: the call completed nothing and took nothing)
            if (!soft[0].empty()) {
                buf.clear();
                for (const fmd_ax25_frame& f : on_gpu ? framed(*framer, soft[0]) : dec.push(soft[0])) printf("%s\n", fm::ax25_text(f).c_str());
                fflush(stdout);
            }
        }
        if (n < fm::kReadSamples) break;
    }
    const fmd_ax25_info i = on_gpu ? framer->info()[0] : dec.info();
    fprintf(stderr, "frames_ok %llu bad_fcs %llu aborts %llu\n", (unsigned long long)i.frames_ok, (unsigned long long)i.bad_fcs,
            (unsigned long long)i.aborts);
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
    uint32_t rate = 0, baud = 1200, mark = 1200, space = 2200, stride = 0;
    bool on_gpu = false;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        uint32_t* v = nullptr;
        if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) { fprintf(stderr, kUsage, argv[0]); return 0; }
        else if (!strcmp(argv[i], "-r")) v = &rate;
        else if (!strcmp(argv[i], "-b")) v = &baud;
        else if (!strcmp(argv[i], "-m")) v = &mark;
        else if (!strcmp(argv[i], "-s")) v = &space;
        else if (!strcmp(argv[i], "-D")) v = &stride;
        else if (!strcmp(argv[i], "-G")) { on_gpu = true; continue; }
        if (!v) { paths.push_back(argv[i]); continue; }
        if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", argv[i]); return 2; }
        if (!number(argv[i + 1], v) || (v != &rate && *v == 0)) { fprintf(stderr, "bad %s: %s\n", argv[i], argv[i + 1]); return 2; }
        ++i;
    }
    if (rate == 0) { fprintf(stderr, "need -r rate\n"); return 2; }
    if (paths.size() > 1) { fprintf(stderr, "too many files\n"); return 2; }
    return fm::exit_code([&] { return run(paths.empty() ? nullptr : paths[0], rate, baud, mark, space, stride, on_gpu); });
}
