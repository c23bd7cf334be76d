"""CPU check of fm_receiver_gpu's argument handling: the exit code and the stderr text of every path that returns before a device is
needed, and the no-device message.  The capture is os.devnull: no block is ever read."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "rtl-sdr-rs_amd", "fm_receiver_gpu")

USAGE = """usage: %s [-s rate] [-o prefix] -S off1,off2,... [-I] <capture.bin | ->
       (FM receiver: station k's stereo as s16 L/R at capture_rate / downsample / R to prefix.k.s16; -I: its RDS baseband to prefix.k.rds.cs16;
        stdout: offset_hz PI PS "radiotext" groups_ok blocks_bad of every station)
"""
NEED = "need -S off1,off2,... (and a non-zero -s rate)\n"
MISSING = "/nonexistent-dir/capture.bin"
NO_FILE = ": No such file or directory\n"
NO_DEVICE = "error: no usable gfx950 device: "             # fmd_strerror(FMD_ERR_NO_DEVICE); the runtime's own reason follows

# (arguments, exit code, stderr)
EARLY = [
    (["-h"], 0, USAGE % CLI),
    (["--help"], 0, USAGE % CLI),
    ([], 2, NEED),
    ([os.devnull], 2, NEED),
    (["-I", "-o", "x", os.devnull], 2, NEED),
    (["-s", "0", "-S", "1000", os.devnull], 2, NEED),
    (["-S", "150000"], 2, "missing input file (use - for stdin)\n"),
    (["-S", "150000", MISSING], 2, MISSING + NO_FILE),
    (["-S", "x", os.devnull], 2, "bad -S list: x\n"),
    (["-S", "150000,x", os.devnull], 2, "bad -S list: 150000,x\n"),
    (["-S", "150000,x", MISSING], 2, "bad -S list: 150000,x\n"),
    (["-S", "", os.devnull], 2, "bad -S list: \n"),
]

# arguments in front of the capture that pass every check of the program itself
NEED_DEVICE = [["-S", "150000"], ["-S", "150000,-300000", "-I"], ["-s", "170000", "-S", "0"]]


def run(args, cwd):
    assert os.path.exists(CLI), "fm_receiver_gpu not built (run __graft_entry__.build())"
    p = subprocess.run([CLI] + args, stdin=subprocess.DEVNULL, capture_output=True, cwd=str(cwd), timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


@pytest.mark.parametrize("args,code,stderr", EARLY, ids=[" ".join(c[0]) or "none" for c in EARLY])
def test_early_exits(args, code, stderr, tmp_path):
    assert run(args, tmp_path) == (code, b"", stderr)
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("args", NEED_DEVICE, ids=[" ".join(c) for c in NEED_DEVICE])
def test_no_device_is_exit_1_with_the_library_message(fmd, args, tmp_path):
    code, stdout, stderr = run(["-o", str(tmp_path / "out")] + args + [os.devnull], tmp_path)
    if fmd.device_count() > 0:                               # with a device the empty capture is a run of no blocks: nothing decoded
        assert code == 0 and "error" not in stderr and "stereo audio: " in stderr and "RDS baseband: " in stderr
        lines = stdout.decode().splitlines()
        assert lines and all(ln.split(" ", 1)[1] == '0000          "" 0 0' for ln in lines)
    else:
        assert (code, stdout) == (1, b"") and stderr.startswith(NO_DEVICE)
        assert stderr.count("\n") == 1 and stderr.endswith("\n")
        assert list(tmp_path.iterdir()) == []                # no output file is created before the device is there
