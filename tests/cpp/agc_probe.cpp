// agc_probe.cpp -- prints what fm::Agc of csrc/demod.hpp answers to configurations on both sides of every domain edge, one
// `name status` line each (status 0: a handle was made; FMD_ERR_NO_DEVICE: the arguments passed and only the device was missing),
// for tests/test_agc.py.  Needs the library but no device.
#include <cstdio>

#include "demod.hpp"

static void probe(const char* name, fmd_agc_config cfg, uint32_t rows, uint32_t width)
{
    int status = 0;
    try {
        fm::Agc agc(cfg, rows, width);
        status = agc.block() == cfg.block ? 0 : 1;
    } catch (const fm::Error& e) {
        status = e.status;
    }
    printf("%s %d\n", name, status);
}

int main()
{
    const fmd_agc_config ok{256, 12000, 65536, 4, 32};
    probe("defaults", ok, 3, 2);
    probe("width_3", ok, 1, 3);
    probe("rows_0", ok, 0, 1);
    fmd_agc_config c = ok;
    c.block = 48; probe("block_48", c, 1, 1);
    c = ok; c.block = 4096; probe("block_4096", c, 1, 1);
    c = ok; c.block = 8192; probe("block_8192", c, 1, 1);
    c = ok; c.target = 32768; probe("target_32768", c, 1, 1);
    c = ok; c.gain_max = 262145; probe("gain_max_262145", c, 1, 2);
    c = ok; c.hang = 65536; probe("hang_65536", c, 1, 1);
    c = ok; c.decay = 0; probe("decay_0", c, 1, 1);
    c = ok; c.decay = 256; c.hang = 65535; c.gain_max = 262144; c.target = 32767; c.block = 16; probe("largest", c, 1, 2);
    return 0;
}
