// adsb_gpu -- rtl_adsb's job over the C ABI: 2 Msample/s u8 IQ at 1090 MHz, from a capture file, a pipe or an rtl_tcp server, to the
// Mode S messages in it, through the Mode S bank (fmd_modes_* on the GPU; host C++ only, through fm::ModeSBank of demod.hpp).
//
//   adsb_gpu [-e] [-S] [-p min_power] [-v] [capture.bin | -t host:port]
//
// -e: single-bit errors of extended squitters are corrected.  -S: short DF 11 replies are taken too.  -p: the least sum of the four
// preamble pulses' power (default 0).  capture.bin defaults to stdin (also "-"); -t reads from an rtl_tcp server, tuned to 1090 MHz
// at 2 Msample/s.  One stream, fed in calls of 262144 bytes as the input arrives.  One `*HEX;` line per message on stdout, which is
// rtl_adsb's output format; a message that begins inside an earlier one is dropped (host policy: the device suppresses nothing).
// -v adds the decoded fields of extended squitters behind the line.  At the end `samples N candidates N messages N fixed N` on
// stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "demod.hpp"

static const char* const kUsage =
    "usage: %s [-e] [-S] [-p min_power] [-v] [capture.bin | -t host:port]\n"
    "       (Mode S bank: 2 Msample/s u8 IQ in, one *HEX; line per ADS-B message out, the counters on stderr)\n";

constexpr size_t kCallBytes = 262144;

static void print_fields(const fmd_modes_msg& m)
{
    fmd_modes_fields f;
    if (fmd_modes_decode(m.bytes, m.n_bytes, &f) != FMD_OK) return;
    printf("  DF %u ICAO %06X TC %u", f.df, f.icao, f.type_code);
    if (f.has & 1u) printf(" callsign %s", f.callsign);
    if (f.has & 2u) printf(" altitude %d ft", f.altitude_ft);
    if (f.has & 4u) printf(" cpr %s %u %u", f.cpr_odd ? "odd" : "even", f.cpr_lat, f.cpr_lon);
    if (f.has & 8u) printf(" speed %.0f kt track %.0f deg vrate %d ft/min", f.speed_kt, f.track_deg, f.vrate_fpm);
    if (m.fixed_bit != 0xFF) printf(" fixed bit %u", m.fixed_bit);
    printf("\n");
}

static int run(const char* in_path, const char* tcp, const fmd_modes_config& cfg, bool verbose)
{
    fm::File in;
    std::unique_ptr<fm::RtlTcpSource> src;
    if (tcp) {
        const char* colon = strrchr(tcp, ':');
        const long port = colon ? strtol(colon + 1, nullptr, 10) : 0;
        if (!colon || port < 1 || port > 65535) { fprintf(stderr, "bad -t: %s\n", tcp); return 2; }
        src.reset(new fm::RtlTcpSource(std::string(tcp, colon), (uint16_t)port));
        src->set_sample_rate(2000000);
        src->set_center_freq(1090000000);
        src->set_tuner_gain_auto();
    } else {
        in.reset(in_path && strcmp(in_path, "-") ? fopen(in_path, "rb") : stdin);
        if (!in) { perror(in_path); return 2; }
    }
    fm::ModeSBank bank(cfg, 1);                               // out of the domain, or no device: before anything is printed
    std::vector<uint8_t> buf(kCallBytes);
    uint64_t pos = 0, busy_until = 0;                         // samples taken; the end of the last message printed
    for (;;) {
        size_t fill = 0, got;
        if (src) fill = src->read_sync(buf.data(), kCallBytes);
        else while (fill < kCallBytes && (got = fread(buf.data() + fill, 1, kCallBytes - fill, in.get())) > 0) fill += got;
        const size_t nbytes = fill & ~(size_t)7;              // whole groups of four samples
        if (fill != nbytes && fill < kCallBytes) fprintf(stderr, "dropped %zu trailing bytes\n", fill - nbytes);
        if (nbytes) {
            bank.run(buf.data(), nbytes);
            const std::vector<std::vector<fmd_modes_msg>> got_msgs = bank.messages({0u});       // (kept: the loop reads its first stream)
            for (const fmd_modes_msg& m : got_msgs[0]) {
                const uint64_t p = pos + (uint64_t)(int64_t)m.k_rel;     // (k_rel >= -pos)
                if (p < busy_until) continue;
                busy_until = p + 16u + 16u * m.n_bytes;
                printf("%s\n", fm::modes_hex(m).c_str());
                if (verbose) print_fields(m);
            }
            fflush(stdout);
            pos += nbytes / 2;
        }
        if (fill < kCallBytes) break;
    }
    const fmd_modes_totals t = bank.info()[0];
    fprintf(stderr, "samples %llu candidates %llu messages %llu fixed %llu\n", (unsigned long long)t.samples,
            (unsigned long long)t.candidates, (unsigned long long)t.messages, (unsigned long long)t.fixed);
    return 0;
}

int main(int argc, char** argv)
{
    fmd_modes_config cfg{0, 0, 0, 256};
    bool verbose = false;
    const char* tcp = nullptr;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) { fprintf(stderr, kUsage, argv[0]); return 0; }
        else if (!strcmp(argv[i], "-e")) cfg.fix_errors = 1;
        else if (!strcmp(argv[i], "-S")) cfg.df11 = 1;
        else if (!strcmp(argv[i], "-v")) verbose = true;
        else if (!strcmp(argv[i], "-p") || !strcmp(argv[i], "-t")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", argv[i]); return 2; }
            if (argv[i][1] == 't') { tcp = argv[++i]; continue; }
            char* end = nullptr;
            const unsigned long long x = strtoull(argv[i + 1], &end, 10);
            if (end == argv[i + 1] || *end || argv[i + 1][0] == '-' || x > 0xFFFFFFFFull) { fprintf(stderr, "bad -p: %s\n", argv[i + 1]); return 2; }
            cfg.min_power = (uint32_t)x;
            ++i;
        }
        else if (argv[i][0] == '-' && argv[i][1]) { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
        else paths.push_back(argv[i]);
    }
    if (paths.size() > 1 || (tcp && !paths.empty())) { fprintf(stderr, "too many inputs\n"); return 2; }
    return fm::exit_code([&] { return run(paths.empty() ? nullptr : paths[0], tcp, cfg, verbose); });
}
