"""CPU check of the C++ wrapper (csrc/demod.hpp): its tap designers and named defaults against the Python package, exactly.
tests/cpp/wrapper_probe.cpp is compiled with g++ -Wall -Wextra -Werror against the header and the built library (which loads
without a device) and prints one `name v0 v1 ...` line per quantity."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rtl-sdr-rs_amd")
BANDS = {"am": (-4000, 4000), "fm": (-6000, 6000), "usb": (300, 3000), "lsb": (-3000, -300)}
RATES = (600000, 170000, 110000, 15800)                      # -s values whose downsample is 2, 6, 10 and 64


@pytest.fixture(scope="module")
def probe(fmd, tmp_path_factory):
    """{name: [int, ...]} as the probe prints it."""
    fmd.lib()                                                # the library is built
    exe = str(tmp_path_factory.mktemp("probe") / "wrapper_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "wrapper_probe.cpp"), "-o", exe, "-L", PKG, "-lfmd_hip", "-Wl,-rpath," + PKG],
                   check=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, timeout=120).stdout.decode()
    return {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out.splitlines()}


def test_designers_match_python(fmd, probe):
    for f_m in (170000, 240000):
        assert probe["stereo_%d" % f_m] == fmd.stereo_taps(f_m, 5, 127).tolist()
        g, shift = fmd.rds_taps(f_m, 22, 255)
        assert probe["rds_%d" % f_m] == g.tolist() and probe["rds_shift_%d" % f_m] == [shift]
        for mode, (lo, hi) in BANDS.items():
            gr, gi = fmd.narrow_taps(f_m, 256, lo, hi)
            assert probe["narrow_%s_%d_re" % (mode, f_m)] == gr.tolist(), (mode, f_m)
            assert probe["narrow_%s_%d_im" % (mode, f_m)] == ([] if gi is None else gi.tolist()), (mode, f_m)
            assert (gi is None) == (lo == -hi)
    assert probe["rds_shift_170000"] == [14]
    u = fmd.uniform_taps(16, 8)
    assert probe["uniform_16_8"] == u.tolist()
    assert probe["uniform_shift_16_8"] == [fmd.uniform_auto_shift(u, 16)] == [10]
    assert probe["uniform_shift_16_8_sel"] == [fmd.uniform_auto_shift(u, 16, [0, 3, 15])]


def ceil_shift(value, limit):
    """Smallest s with ceil(value / 2^s) <= limit, as the GPU CLI tests restate it."""
    s = 0
    while -(-value >> s) > limit:
        s += 1
    return s


def rds_front(capture):
    """The CLI's filter in front of the RDS bank, operation for operation: a 64-tap Hamming-windowed sinc of +-62 kHz with peak
    2047, and the shift that keeps every |y| component <= 256 with sum(|Wr| + |Wi|) <= 2 sum |h| + 2 n_taps."""
    fc = 2.0 * 62000.0 / capture
    v = lambda i: math.sin(math.pi * fc * (i - 31.5)) / (math.pi * fc * (i - 31.5)) * (0.54 - 0.46 * math.cos(2 * math.pi * i / 63.0))
    peak = math.sin(math.pi * fc * 0.5) / (math.pi * fc * 0.5) * (0.54 - 0.46 * math.cos(2 * math.pi * 31 / 63.0))
    h = [int(math.floor(abs(v(i) / peak * 2047.0) + 0.5)) * (1 if v(i) >= 0 else -1) for i in range(64)]      # lround
    return h, ceil_shift(256 * (2 * sum(abs(x) for x in h) + 128), 256)


def test_named_defaults_match_python(fmd, probe):
    seen = set()
    for rate in RATES:
        radio, cfg = fmd.optimal_settings(94_900_000, rate)
        capture, D = radio.capture_rate, cfg.downsample
        seen.add(D)
        shift = ceil_shift(512 * D, 16384)
        assert probe["front_%d" % rate] == [capture, D, ceil_shift(512 * D, 256), shift, -(-512 * D >> shift)]
        assert probe["pilot_min_%d" % rate] == [fmd.stereo.default_pilot_min(capture, D)]
        f_m = capture // D
        g = fmd.stereo_taps(f_m, max(1, f_m // 48000), 127)
        assert probe["audio_shift_%d" % rate] == [fmd.stereo.default_audio_shift(g, capture, D)]
        for mode, (lo, hi) in BANDS.items():
            gr, gi = fmd.narrow_taps(f_m, 256, lo, hi)
            peak = -(-512 * D >> shift) * fmd.narrow.narrow_gain_sum(gr, gi)
            assert probe["chan_shift_%s_%d" % (mode, rate)] == [ceil_shift(peak, 256 if mode == "fm" else 16384)], (mode, rate)
        h, rshift = rds_front(capture)
        assert probe["rds_front_%d" % rate] == h and probe["rds_front_shift_%d" % rate] == [rshift]
    assert seen == {2, 6, 10, 64}
