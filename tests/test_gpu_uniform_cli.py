"""simple_fm_gpu -U (the uniform channelizer's file mode) on the MI355X: the selected channels' .cs16 files against the test-side
definition (tests/uniform_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import uniform_ref as ur

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_uniform_mode_writes_the_selected_channels(fmd, tmp_path):
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "simple_fm_gpu")
    N, hop, P, sel = 16, 8, 8, [2, 5]
    rng = np.random.default_rng(62)
    iq = rng.integers(0, 256, 2 * hop * 3000 + 6, dtype=np.uint8)            # 6 trailing bytes do not fill a hop
    (tmp_path / "cap.bin").write_bytes(iq.tobytes())
    p = subprocess.run([exe, "-s", "2400000", "-U", "%d:%d:%d" % (N, hop, P), "-C", ",".join(map(str, sel)), "-o", str(tmp_path / "ch"),
                        str(tmp_path / "cap.bin")], capture_output=True, timeout=300)
    err = p.stderr.decode()
    assert p.returncode == 0, err
    assert "dropped 6 trailing bytes" in err
    assert "channel 2 at +300000.0 Hz" in err and "channel 5 at +750000.0 Hz" in err and "output at 300000.0 Hz" in err
    h = ur.taps(N, P)
    exp = ur.UniformRef(h, N, hop, ur.min_shift(h, ur.channel_incs(N, sel)), channels=sel).feed(iq[:2 * hop * 3000])
    for i, k in enumerate(sel):
        got = np.fromfile(str(tmp_path / ("ch.%d.cs16" % k)), dtype=np.int16)
        assert got.size == 2 * (3000 - N * P // hop + 1) and np.array_equal(got, exp[i].ravel()), k
    assert sorted(f.name for f in tmp_path.iterdir()) == ["cap.bin", "ch.2.cs16", "ch.5.cs16"]
