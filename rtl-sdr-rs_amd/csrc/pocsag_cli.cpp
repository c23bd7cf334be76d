// pocsag_gpu -- an s16 file or pipe of NFM audio to the POCSAG pages in it, through the pager decoder of the C ABI (fmd_fsk_* on the
// GPU, fmd_pocsag_decoder_* on the host; host C++ only, through fm::FskDemod and fm::PocsagDecoder of demod.hpp).  What the
// narrow-band and band-plan banks' CLIs write for an NFM channel that carries paging comes out as text:
//
//   band_plan_gpu ... -o out capture.bin && pocsag_gpu -r 12000 out.3.s16
//
//   pocsag_gpu -r rate [-b baud] [-e max_errors] [-m auto|numeric|alpha] [-G] [in.s16]
//
// -r: the sample rate of the input in Hz (required).  -b: bits per second, 512, 1200 or 2400 (default 1200).  -e: bit errors
// corrected per codeword, 0 to 2 (default 1).  -m: how message bits are shown (default auto: function 0 numeric, the rest alpha).
// in.s16 defaults to stdin (also "-").  One row, fed call by call as the input arrives.  One line per message on stdout,
// `POCSAG<baud>: Address: <7 digits>  Function: <f>  Numeric|Alpha|Tone: <text>`; at the end `messages N batches N bad_codewords N
// orphans N` on stderr.  -G: the messages come from the page bank on the GPU (fmd_pager_*, fm::Pager) instead of the host decoder;
// the output is the same.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "demod.hpp"

static const char* const kUsage =
    "usage: %s -r rate [-b baud] [-e max_errors] [-m auto|numeric|alpha] [in.s16]\n"
    "       (pager decoder: raw mono s16 of an NFM channel in, one line per POCSAG message out, the counters on stderr)\n";

static int run(const char* in_path, uint32_t rate, uint32_t baud, uint32_t max_errors, int mode, bool on_gpu)
{
    fm::File in(in_path && strcmp(in_path, "-") ? fopen(in_path, "rb") : stdin);
    if (!in) { perror(in_path); return 2; }
    fmd_fsk_config cfg;
    try { cfg = fm::fsk_design(rate, baud); }
    catch (const std::invalid_argument& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
    // out of the decoder's domain, or no device: before anything is printed
    fm::PocsagDecoder dec(rate, cfg.D, baud, max_errors);
    fm::FskDemod demod(cfg, 1, 1);
    std::unique_ptr<fm::Pager> pager;
    size_t piece = fm::kReadSamples;                         // input samples per call of the front end
    if (on_gpu) {
        // pieces short enough that none can complete more than msg_cap messages (the front end is exact under cuts)
        pager.reset(new fm::Pager(rate, cfg.D, baud, max_errors, 16));
        size_t soft_piece = 1;
        while (pager->max_messages(2 * soft_piece) <= pager->msg_cap()) soft_piece *= 2;
        piece = soft_piece * cfg.D;
    }
    std::vector<int16_t> chunk(fm::kReadSamples);
    for (;;) {
        const size_t n = fm::read_samples(in.get(), chunk.data(), 1);
        for (size_t lo = 0; lo < n; lo += piece) {
            const fm::Rows soft = demod.run(chunk.data() + lo, std::min(piece, n - lo));
            const std::vector<std::vector<fmd_fsk_hit>> hits = demod.hits();
            if (!on_gpu) {
                for (const fmd_pocsag_msg& m : dec.push(soft[0], hits[0])) printf("%s\n", fm::pocsag_text(m, baud, mode).c_str());
            } else if (!soft[0].empty()) {
                pager->run(soft[0].data(), soft[0].size(), hits);
                const std::vector<std::vector<fmd_pocsag_msg>> got = pager->msgs({0u});      // (kept: the loop reads its first row)
                for (const fmd_pocsag_msg& m : got[0]) printf("%s\n", fm::pocsag_text(m, baud, mode).c_str());
            }
        }
        if (n) fflush(stdout);
        if (n < fm::kReadSamples) break;
    }
    const fmd_pocsag_info i = on_gpu ? pager->info()[0] : dec.info();
    fprintf(stderr, "messages %llu batches %llu bad_codewords %llu orphans %llu\n", (unsigned long long)i.messages,
            (unsigned long long)i.batches, (unsigned long long)i.bad_codewords, (unsigned long long)i.orphans);
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
    uint32_t rate = 0, baud = 1200, max_errors = 1;
    int mode = 0;
    bool on_gpu = false;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        uint32_t* v = nullptr;
        if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) { fprintf(stderr, kUsage, argv[0]); return 0; }
        else if (!strcmp(argv[i], "-m")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", argv[i]); return 2; }
            ++i;
            if (!strcmp(argv[i], "auto")) mode = 0;
            else if (!strcmp(argv[i], "numeric")) mode = 1;
            else if (!strcmp(argv[i], "alpha")) mode = 2;
            else { fprintf(stderr, "bad -m: %s\n", argv[i]); return 2; }
            continue;
        }
        else if (!strcmp(argv[i], "-r")) v = &rate;
        else if (!strcmp(argv[i], "-b")) v = &baud;
        else if (!strcmp(argv[i], "-e")) v = &max_errors;
        else if (!strcmp(argv[i], "-G")) { on_gpu = true; continue; }
        if (!v) { paths.push_back(argv[i]); continue; }
        if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", argv[i]); return 2; }
        if (!number(argv[i + 1], v) || (v == &baud && *v == 0)) { fprintf(stderr, "bad %s: %s\n", argv[i], argv[i + 1]); return 2; }
        ++i;
    }
    if (rate == 0) { fprintf(stderr, "need -r rate\n"); return 2; }
    if (paths.size() > 1) { fprintf(stderr, "too many files\n"); return 2; }
    return fm::exit_code([&] { return run(paths.empty() ? nullptr : paths[0], rate, baud, max_errors, mode, on_gpu); });
}
