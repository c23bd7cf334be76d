"""CPU check of simple_fm_gpu's argument handling: the exit code and the stderr text of every path that returns before a device is
needed, and the no-device message.  The capture is os.devnull: no block is ever read."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "rtl-sdr-rs_amd", "simple_fm_gpu")

USAGE = """usage: %s [-f freq_hz] [-s sample_rate_hz] [-r resample_hz] [-b blocks_per_launch] <capture.bin | ->
       %s [-s ...] [-r ...] [-o prefix] [-g n_gpus] <a.bin> <b.bin> ...   (one channel per file)
       %s [-f freq_hz] [-s ...] [-r ...] [-n blocks] -t host:port            (live: IQ from an rtl_tcp server)
       %s [-s ...] [-r ...] [-o prefix] -S off1,off2,... <capture.bin | ->   (stations at these offsets in Hz)
       %s [-s ...] [-o prefix] -S off1,off2,... -I <capture.bin | ->        (their baseband: s16 I/Q at capture_rate / downsample)
       %s [-s ...] [-o prefix] -S off1,off2,... -2 <capture.bin | ->        (their stereo: s16 L/R at capture_rate / downsample / R)
       %s [-s ...] [-o prefix] -S off1,off2,... -N mode[:R[:lo:hi]] [-q squelch] <capture.bin | ->   (narrow-band channels: iq, fm, am, usb, lsb at capture_rate / downsample / R)
       %s [-s ...] [-o prefix] -S off1,off2,... -R [-I] <capture.bin | ->   (their RDS: offset_hz PI PS "radiotext" groups_ok blocks_bad; -I: baseband to prefix.k.rds.cs16)
       %s -s capture_rate_hz -P n_bins [-H hop] <capture.bin | ->       (power spectrum: offset_hz power per bin)
       %s -s capture_rate_hz [-o prefix] -U N:hop[:taps_per_channel] [-C k1,k2,...] <capture.bin | ->   (band plan: channel k's s16 I/Q at capture_rate / hop to prefix.k.cs16)
"""
MISSING = "/nonexistent-dir/capture.bin"
NO_FILE = ": No such file or directory\n"
NO_DEVICE = "error: no usable gfx950 device: "             # fmd_strerror(FMD_ERR_NO_DEVICE); the runtime's own reason follows
HEADER = "Oversampling input by: 6x\nOutput at 170000 Hz\nOutput scale: 42\ncapture_rate: 1020000 capture_freq: 95155000\n"

# (arguments, exit code, stderr)
EARLY = [
    (["-h"], 0, USAGE % ((CLI,) * 10)),
    (["--help"], 0, USAGE % ((CLI,) * 10)),
    ([], 2, "missing input file (use - for stdin)\n"),
    (["-s", "240000", "-o", "x"], 2, "missing input file (use - for stdin)\n"),
    ([MISSING], 2, MISSING + NO_FILE),
    (["-S", "100", MISSING], 2, MISSING + NO_FILE),
    (["-P", "256", MISSING], 2, MISSING + NO_FILE),
    (["-U", "16:8", MISSING], 2, MISSING + NO_FILE),
    ([os.devnull, MISSING], 2, MISSING + NO_FILE),
    (["-g", "2", os.devnull, MISSING], 2, MISSING + NO_FILE),
    (["-o", "/nonexistent-dir/out", os.devnull, os.devnull], 2, "/nonexistent-dir/out.0.s16" + NO_FILE),
    (["-S", "100,abc", os.devnull], 2, "bad -S list: 100,abc\n"),
    (["-S", "x", "-2", os.devnull], 2, "bad -S list: x\n"),
    (["-S", "100", "-N", "xx", os.devnull], 2, "bad -N mode: xx (iq, fm, am, usb, lsb)\n"),
    (["-S", "100", "-N", "ssb:10", os.devnull], 2, "bad -N mode: ssb:10 (iq, fm, am, usb, lsb)\n"),
    (["-U", "16", os.devnull], 2, "bad -U N:hop[:taps_per_channel]: 16\n"),
    (["-U", "0:8", os.devnull], 2, "bad -U N:hop[:taps_per_channel]: 0:8\n"),
    (["-U", "16:8:0", os.devnull], 2, "bad -U N:hop[:taps_per_channel]: 16:8:0\n"),
    (["-U", "16:8", "-C", "1,x", os.devnull], 2, "bad -C list: 1,x\n"),
    (["-U", "16:8", "-C", "1,x", MISSING], 2, "bad -C list: 1,x\n"),
    (["-t", "host:0"], 2, "-t host:0: port must be 1 ... 65535\n"),
    (["-t", "host:65536"], 2, "-t host:65536: port must be 1 ... 65535\n"),
    (["-t", "host:12x"], 2, "-t host:12x: port must be 1 ... 65535\n"),
    (["-t", "[::1"], 2, "-t [::1: missing ']'\n"),
    (["-t", "[::1]x"], 2, "-t [::1]x: expected ':port' after ']'\n"),
    (["-t", "[::1]:0"], 2, "-t [::1]:0: port must be 1 ... 65535\n"),
    (["-t", ":1234"], 2, "-t :1234: empty host\n"),
]

# (arguments in front of the capture, what stderr holds before the device is opened)
NEED_DEVICE = [
    ([], HEADER),
    (["-b", "4"], HEADER),
    (["-S", "0"], ""),
    (["-S", "0", "-I"], ""),
    (["-S", "0", "-2"], ""),
    (["-S", "0", "-N", "am"], ""),
    (["-S", "0", "-R"], ""),
    (["-P", "256"], ""),
    (["-U", "16:8"], ""),
    ([os.devnull], ""),
    (["-g", "1", os.devnull], ""),
]


def run(args, cwd):
    assert os.path.exists(CLI), "simple_fm_gpu not built (run __graft_entry__.build())"
    p = subprocess.run([CLI] + args, stdin=subprocess.DEVNULL, capture_output=True, cwd=str(cwd), timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


@pytest.mark.parametrize("args,code,stderr", EARLY, ids=[" ".join(c[0]) or "none" for c in EARLY])
def test_early_exits(args, code, stderr, tmp_path):
    assert run(args, tmp_path) == (code, b"", stderr)


@pytest.mark.parametrize("args,before", NEED_DEVICE, ids=[" ".join(c[0]) or "plain" for c in NEED_DEVICE])
def test_no_device_is_exit_1_with_the_library_message(fmd, args, before, tmp_path):
    code, stdout, stderr = run(["-o", str(tmp_path / "out")] + args + [os.devnull], tmp_path)
    if fmd.device_count() > 0:                               # with a device the empty capture is a run of no blocks
        assert code == 0 and "error" not in stderr and stderr.startswith(before)
    else:
        assert (code, stdout) == (1, b"") and stderr.startswith(before + NO_DEVICE)
        assert stderr.count("\n") == before.count("\n") + 1 and stderr.endswith("\n")
