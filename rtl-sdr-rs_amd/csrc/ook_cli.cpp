// ook_gpu -- the front half of rtl_433 over the C ABI: u8 IQ of an ISM band, from a capture file or a pipe, to the on-off-keyed
// packages in it, through the pulse bank (fmd_pulses_* on the GPU) and the host slicer (fmd_pulse_slicer_*) or, with -G, the package
// bank (fmd_packages_* on the GPU); host C++ only, through fm::PulseBank, fm::PulseSlicer and fm::PackageBank of demod.hpp.
//
//   ook_gpu -W w -l lo -h hi -m pwm|ppm -S short -L long -t tol -R reset [-v] [-G] [capture.bin]
//
// -W: the box in samples (1 ... 64).  -l, -h: the comparator's thresholds on the box sum.  -m: the slicer.  -S, -L: the short and the
// long width (PWM) or gap (PPM) in samples, -t their tolerance, -R the gap that ends a package.  capture.bin defaults to stdin (also
// "-").  One stream, fed in calls of 262144 bytes as the input arrives.  One line `start_sample n_bits hex` per package on stdout;
// a package with a pulse that fits neither width, or with no bits, is printed only with -v (then with `bad` or `truncated` behind
// it).  -G: the packages come from the device bank -- fmd_packages_run_bank behind every call of the pulse bank, on the records where
// they lie, and fmd_packages_flush at the end of the input -- and the lines are the same.  At the end `samples N pulses N rises N
// dropped N` on stderr: dropped counts the pulses beyond pulse_cap (1024) of a call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "demod.hpp"

static const char* const kUsage =
    "usage: %s -W w -l lo -h hi -m pwm|ppm -S short -L long -t tol -R reset [-v] [-G] [capture.bin]\n"
    "       (pulse bank and slicer: u8 IQ in, one `start_sample n_bits hex` line per on-off-keyed package out;\n"
    "        -G: the packages are sliced on the device by the package bank instead of the host slicer, the lines are the same)\n";

constexpr size_t kCallBytes = 262144;

static void print(const std::vector<fmd_pulse_package>& got, bool verbose)
{
    for (const fmd_pulse_package& k : got) {
        const bool bad = (k.flags & FMD_PULSE_BAD) != 0;
        if (!verbose && (bad || k.n_bits == 0)) continue;
        printf("%s%s%s\n", fm::pulse_line(k).c_str(), verbose && bad ? " bad" : "", verbose && (k.flags & FMD_PULSE_TRUNCATED) ? " truncated" : "");
    }
}

static int run(const char* in_path, const fmd_pulses_config& cfg, const fmd_pulse_slicer_config& scfg, bool verbose, bool on_device)
{
    fm::File in;
    in.reset(in_path && strcmp(in_path, "-") ? fopen(in_path, "rb") : stdin);
    if (!in) { perror(in_path); return 2; }
    fm::PulseSlicer slicer(scfg);
    fm::PulseBank bank(cfg, 1);                               // out of the domain, or no device: before anything is printed
    std::unique_ptr<fm::PackageBank> sliced;
    if (on_device) sliced.reset(new fm::PackageBank(bank, scfg));
    std::vector<uint8_t> buf(kCallBytes);
    uint64_t pos = 0, dropped = 0;
    for (;;) {
        size_t fill = 0, got;
        while (fill < kCallBytes && (got = fread(buf.data() + fill, 1, kCallBytes - fill, in.get())) > 0) fill += got;
        const size_t nbytes = fill & ~(size_t)7;              // whole groups of four samples
        if (fill != nbytes && fill < kCallBytes) fprintf(stderr, "dropped %zu trailing bytes\n", fill - nbytes);
        if (nbytes) {
            bank.run(buf.data(), nbytes);
            const uint32_t count = bank.counts()[0];
            if (count > cfg.pulse_cap) dropped += count - cfg.pulse_cap;
            if (sliced) {
                sliced->run_bank(bank);                       // nothing but the packages comes back
                print(sliced->packages({0u})[0], verbose);
            } else {
                slicer.push(bank.pulses({0u})[0], pos);
                const fmd_pulses_totals t = bank.info()[0];
                slicer.idle(t.state, t.run);
                print(slicer.take(), verbose);
            }
            fflush(stdout);
            pos += nbytes / 2;
        }
        if (fill < kCallBytes) break;
    }
    if (sliced) {
        sliced->flush();
        print(sliced->packages({0u})[0], verbose);
    } else {
        slicer.idle(0, scfg.reset);                           // the end of the input ends the open package
        print(slicer.take(), verbose);
    }
    const fmd_pulses_totals t = bank.info()[0];
    fprintf(stderr, "samples %llu pulses %llu rises %llu dropped %llu\n", (unsigned long long)t.samples, (unsigned long long)t.pulses,
            (unsigned long long)t.rises, (unsigned long long)dropped);
    return 0;
}

int main(int argc, char** argv)
{
    fmd_pulses_config cfg{8, 30000, 60000, 1024};
    fmd_pulse_slicer_config scfg{FMD_PULSE_PWM, 0, 0, 0, 0};
    bool verbose = false, on_device = false;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--help")) { fprintf(stderr, kUsage, argv[0]); return 0; }
        else if (!strcmp(argv[i], "-v")) verbose = true;
        else if (!strcmp(argv[i], "-G")) on_device = true;
        else if (argv[i][0] == '-' && argv[i][1] && strchr("WlhmSLtR", argv[i][1]) && !argv[i][2]) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", argv[i]); return 2; }
            const char opt = argv[i][1], * const val = argv[++i];
            if (opt == 'm') {
                if (!strcmp(val, "pwm")) scfg.modulation = FMD_PULSE_PWM;
                else if (!strcmp(val, "ppm")) scfg.modulation = FMD_PULSE_PPM;
                else { fprintf(stderr, "bad -m: %s\n", val); return 2; }
                continue;
            }
            char* end = nullptr;
            const unsigned long long x = strtoull(val, &end, 10);
            if (end == val || *end || val[0] == '-' || x > 0xFFFFFFFFull) { fprintf(stderr, "bad -%c: %s\n", opt, val); return 2; }
            uint32_t* const into = opt == 'W' ? &cfg.W : opt == 'l' ? &cfg.lo : opt == 'h' ? &cfg.hi : opt == 'S' ? &scfg.short_w
                                 : opt == 'L' ? &scfg.long_w : opt == 't' ? &scfg.tol : &scfg.reset;
            *into = (uint32_t)x;
        }
        else if (argv[i][0] == '-' && argv[i][1]) { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
        else paths.push_back(argv[i]);
    }
    if (paths.size() > 1) { fprintf(stderr, "too many inputs\n"); return 2; }
    if (!scfg.short_w || !scfg.long_w || !scfg.reset) { fprintf(stderr, kUsage, argv[0]); return 2; }
    return fm::exit_code([&] { return run(paths.empty() ? nullptr : paths[0], cfg, scfg, verbose, on_device); });
}
