// afsk_probe.cpp -- for tests/test_afsk.py.  Needs the library but no device.
//   (no arguments)                             what fm::AfskDemod of csrc/demod.hpp answers to configurations on both sides of domain
//                                              edges, one `name status` line each (status 0: a handle was made; FMD_ERR_NO_DEVICE:
//                                              the arguments passed and only the device was missing)
//   table rate baud mark space taps            fm::afsk_table: `T pre_shift out_shift stride`, then one entry per line, row by row
//   decode rate_num rate_den baud file chunk   the int16 soft decisions of `file` through fm::Ax25Decoder in pushes of `chunk`
//                                              samples (0: one push): `frame end_sample hex` and `text ...` per frame, then
//                                              `info frames_ok bad_fcs aborts in_frame`
//   text hex                                   fm::ax25_text of the bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "demod.hpp"

static void probe(const char* name, uint32_t T, uint32_t D, uint32_t pre, uint32_t out, uint32_t rows, uint32_t width, int16_t entry = 1023)
{
    int status = 0;
    try {
        fm::AfskDemod d(std::vector<int16_t>((size_t)4 * T, entry), D, pre, out, rows, width);
        status = d.stride() == D ? 0 : 1;
    } catch (const fm::Error& e) {
        status = e.status;
    }
    printf("%s %d\n", name, status);
}

static std::vector<uint8_t> unhex(const char* s)
{
    std::vector<uint8_t> v;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
        const char b[3] = {s[i], s[i + 1], 0};
        v.push_back((uint8_t)strtoul(b, nullptr, 16));
    }
    return v;
}

int main(int argc, char** argv)
{
    if (argc == 7 && !strcmp(argv[1], "table")) {
        const fm::AfskTable t = fm::afsk_table(strtod(argv[2], nullptr), strtod(argv[3], nullptr), strtod(argv[4], nullptr),
                                               strtod(argv[5], nullptr), (uint32_t)strtoul(argv[6], nullptr, 10));
        printf("%u %u %u %u\n", t.T, t.pre_shift, t.out_shift, fm::afsk_stride(t.T));
        for (int16_t v : t.tab) printf("%d\n", v);
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "decode")) {
        fm::Ax25Decoder dec((uint32_t)strtoul(argv[2], nullptr, 10), (uint32_t)strtoul(argv[3], nullptr, 10), (uint32_t)strtoul(argv[4], nullptr, 10));
        fm::File f(fopen(argv[5], "rb"));
        if (!f) { perror(argv[5]); return 2; }
        std::vector<int16_t> soft;
        int16_t buf[4096];
        size_t got;
        while ((got = fread(buf, sizeof buf[0], 4096, f.get())) > 0) soft.insert(soft.end(), buf, buf + got);
        const size_t chunk = strtoul(argv[6], nullptr, 10);
        for (size_t lo = 0; lo < soft.size() || lo == 0;) {
            const size_t n = chunk ? std::min(chunk, soft.size() - lo) : soft.size() - lo;
            for (const fmd_ax25_frame& fr : dec.push(soft.data() + lo, n)) {
                printf("frame %llu ", (unsigned long long)fr.end_sample);
                for (uint32_t i = 0; i < fr.len; ++i) printf("%02x", fr.data[i]);
                printf("\ntext %s\n", fm::ax25_text(fr).c_str());
            }
            lo += n;
            if (!n) break;
        }
        const fmd_ax25_info i = dec.info();
        printf("info %llu %llu %llu %d\n", (unsigned long long)i.frames_ok, (unsigned long long)i.bad_fcs, (unsigned long long)i.aborts, i.in_frame);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "text")) {
        const std::vector<uint8_t> v = unhex(argv[2]);
        printf("%s\n", fm::ax25_text(v.data(), v.size()).c_str());
        return 0;
    }
    probe("defaults", 10, 2, 8, 14, 3, 1);
    probe("width_2", 10, 2, 8, 14, 1, 2);
    probe("width_0", 10, 2, 8, 14, 1, 0);
    probe("rows_0", 10, 2, 8, 14, 0, 1);
    probe("taps_1", 1, 1, 8, 14, 1, 1);
    probe("taps_65", 65, 2, 8, 14, 1, 1);
    probe("stride_0", 10, 0, 8, 14, 1, 1);
    probe("stride_11", 10, 11, 8, 14, 1, 1);
    probe("stride_33", 64, 33, 8, 14, 1, 1);
    probe("pre_17", 10, 2, 17, 14, 1, 1);
    probe("out_49", 10, 2, 8, 49, 1, 1);
    probe("entry_1024", 10, 2, 8, 14, 1, 1, 1024);
    probe("smallest", 2, 1, 0, 0, 1, 1, -1023);
    probe("largest", 64, 32, 16, 48, 1, 1);
    return 0;
}
