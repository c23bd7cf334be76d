"""band_plan_gpu on the MI355X: a synthetic capture of about 1 MB through the program; its per-channel files and the activity lines
on stdout equal what the Python handle returns for the same bytes cut into the program's calls, and the definition agrees."""
import os
import subprocess

import numpy as np
import pytest

import bandplan_ref as br
import narrow_ref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rtl-sdr-rs_amd", "band_plan_gpu")
FS, N, HOP, P, R = 2400000, 96, 48, 8, 4


def _capture(n):
    off = lambda k: (k if 2 * k < N else k - N) * FS / N
    z = nr.am(n, FS, off(37), 20, 1000.0, 0.5) + nr.carrier(n, FS, off(90), 60)
    return nr.to_u8(z, noise=1.0, seed=3)


@pytest.mark.parametrize("mode,ext", [("am", "s16"), ("iq", "cs16")])
def test_cli_writes_what_the_python_handle_returns(fmd, tmp_path, mode, ext):
    sel = [5, 37, 38, 90]
    iq = np.concatenate([_capture(499968), np.zeros(10, np.uint8)])     # 10416 hops (1 MB) and 10 bytes that fill no hop
    (tmp_path / "cap.bin").write_bytes(iq.tobytes())
    p = subprocess.run([EXE, "-s", str(FS), "-U", "%d:%d:%d" % (N, HOP, P), "-N", "%s:%d:-4000:4000" % (mode, R), "-q", "40", "-C",
                        ",".join(map(str, sel)), "-o", str(tmp_path / "ch"), str(tmp_path / "cap.bin")], capture_output=True, timeout=300)
    err = p.stderr.decode()
    assert p.returncode == 0, err
    assert "dropped 10 trailing bytes" in err and "output at 12500.0 Hz" in err and "4 of 96 channels" in err
    gr, gi = fmd.narrow_taps(FS / HOP, min(64, 8 * R), -4000, 4000)
    assert gi is None
    bank = fmd.BandPlanBank(fmd.uniform_taps(N, P), N, HOP, gr, R, mode=mode, channels=sel, block=256, squelch=40, gain=256, device_id=0)
    ref = br.BandPlanRef(fmd.uniform_taps(N, P), N, HOP, bank.shift, gr, None, bank.mode, R, bank.chan_shift, 256, 40, 256, channels=sel)
    frame = 2 * HOP
    step = fmd.DEFAULT_BUF_LENGTH // frame * frame            # the program's call size: whole hops
    whole = iq.size // frame * frame
    parts = [bank.run_batch(iq[None, a:min(a + step, whole)]) for a in range(0, whole, step)]
    want = np.concatenate(parts, axis=2)[0]
    exp = np.concatenate([ref.feed(iq[a:min(a + step, whole)]) for a in range(0, whole, step)], axis=1)
    assert np.array_equal(want, exp)
    for i, k in enumerate(sel):
        got = np.fromfile(str(tmp_path / ("ch.%d.%s" % (k, ext))), dtype=np.int16)
        assert got.size == want[i].size and np.array_equal(got, want[i].ravel()), k
    opn, rms = bank.levels()
    lines = p.stdout.decode().splitlines()
    offs = fmd.uniform_channel_offsets(FS, N)
    assert lines == ["%d %.1f %d %d" % (k, offs[k], opn[0, i], rms[0, i]) for i, k in enumerate(sel)]
    assert opn[0].tolist() == [False, True, False, True]      # the AM signal in 37 and the carrier in 90
    assert sorted(f.name for f in tmp_path.iterdir()) == ["cap.bin"] + sorted("ch.%d.%s" % (k, ext) for k in sel)
