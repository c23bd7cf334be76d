"""The pulse bank (include/fmd.h, fmd_pulses_*) on the MI355X: after every call the counts, the records of every stream and at the end
the totals, bit for bit against the definition (tests/pulses_ref.py) over the cases of tests/pulses_cases.py -- an edge on every side
of a tile's end at three boxes, pulses and gaps across whole tiles and calls, the edge a tile owes at its first definite sample,
overflow inside a tile and across tiles, three cuttings of one stream, stream counts around a wave -- and the other surfaces: reset,
empty calls, host against device input at three alignments, the selection of streams, the refusals of a call, the kernel names, and
sender, bank, slicer and command-line tool composed."""
import os
import subprocess

import numpy as np
import pytest

import pulses_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_LENGTH, CAPACITY = -1, -2, -5


def _bank(fmd, c, **over):
    cfg = dict(c.cfg, **over)
    return fmd.PulseBank(c.n_streams, cfg["W"], cfg["lo"], cfg["hi"], cfg["pulse_cap"], device_id=0)


def _same(bank, want, what=None):
    """counts and the records of every stream are the definition's (counts, kept records per stream)"""
    counts, recs = want
    got = bank.counts()
    assert got.tolist() == list(counts), (what, got.tolist(), list(counts))
    every = bank.pulses(np.arange(bank.n_streams))
    bad = [s for s in range(bank.n_streams) if every[s] != recs[s]]
    assert not bad, (what, bad[:8], every[bad[0]][:3], recs[bad[0]][:3])


@pytest.mark.parametrize("name", [n for n in pc.CASE_NAMES if n != "cuts_four"])
def test_case_matches_the_definition(fmd, name):
    c = pc.case(name)
    per_call, info = pc.expected(name)
    bank = _bank(fmd, c)
    for i, (iq, want) in enumerate(zip(c.calls, per_call)):
        bank.run(iq)
        _same(bank, want, (name, i))
    assert bank.info() == info
    bank.check()


def test_calls_of_four_samples_give_the_same_records(fmd):
    """Calls of 8 bytes, every one shorter than the box: the counts come back after each, the records where a call has some; in
    absolute positions the stream's records are those of one call, and the totals agree."""
    c = pc.case("cuts_four")
    per_call, info = pc.expected("cuts_four")
    want = pc.absolute(per_call, c.calls, 0)
    assert want == pc.absolute(pc.expected("cuts_one")[0], pc.case("cuts_one").calls, 0)
    bank = _bank(fmd, c)
    got, pos = [], 0
    for iq, (counts, recs) in zip(c.calls, per_call):
        bank.run(iq)
        n = bank.counts()
        assert n.tolist() == list(counts), pos
        if n[0]:
            got += [dict({k: v for k, v in r.items() if k != "k_rel"}, p=pos + r["k_rel"]) for r in bank.pulses([0])[0]]
        pos += iq.shape[1] // 2
    assert got == want and bank.info() == info


def test_reset_and_empty_calls(fmd):
    c = pc.case("cuts_random")
    per_call, info = pc.expected("cuts_random")
    bank = _bank(fmd, c)
    zero = {"samples": 0, "pulses": 0, "rises": 0, "state": 0, "run": 0}
    assert bank.counts().tolist() == [0] and bank.info() == [zero]
    for rounds in range(2):
        for iq, want in zip(c.calls, per_call):
            bank.run(iq)
            _same(bank, want)
            bank.run(iq[:, :0])                              # nbytes == 0: nothing launched, the results stay
            _same(bank, want)
        assert bank.info() == info
        bank.reset()
        assert bank.counts().tolist() == [0] and bank.info() == [zero]


@pytest.mark.parametrize("off", [0, 4, 8])
def test_device_input_matches_host_input(fmd, off):
    """run_device on rows cap_bytes apart, `off` bytes behind a 16-byte boundary and with a pitch that is no multiple of 16, with
    sentinels between the rows' valid bytes and behind the last: the same results as run_batch."""
    import torch
    c = pc.case("streams_3")
    per_call, info = pc.expected("streams_3")
    nbytes = c.calls[0].shape[1]
    cap_bytes = nbytes + (20 if off else 32)
    host = np.full(3 * cap_bytes + 32, 0xC8, np.uint8)       # (a sentinel that would read as a strong carrier)
    host[off:off + 3 * cap_bytes].reshape(3, cap_bytes)[:, :nbytes] = c.calls[0]
    d = torch.from_numpy(host).cuda()
    assert d.data_ptr() % 16 == 0
    bank = _bank(fmd, c)
    torch.cuda.synchronize()
    bank.run_device(d.data_ptr() + off, nbytes, cap_bytes)
    bank.check()
    _same(bank, per_call[0], off)
    assert bank.info() == info
    bank.reset()
    s = torch.cuda.Stream()
    bank.run_device(d.data_ptr() + off, nbytes, cap_bytes, stream=s.cuda_stream)
    bank.check()
    _same(bank, per_call[0], ("stream", off))
    assert np.array_equal(d.cpu().numpy(), host)             # the input is only read


def test_selection_of_streams_in_a_chosen_order(fmd):
    c = pc.case("streams_65")
    per_call, _ = pc.expected("streams_65")
    bank = _bank(fmd, c)
    bank.run(c.calls[0])
    counts, recs = per_call[0]
    order = [64, 0, 33, 3, 3, 1]
    assert bank.pulses(order) == [recs[s] for s in order]
    assert bank.pulses([]) == []
    raw = bank.records([3])[0]                               # zeros behind the stream's own records
    assert 0 < counts[3] < bank.pulse_cap and all(bytes(raw[k]) == bytes(16) for k in range(counts[3], bank.pulse_cap))
    with pytest.raises(fmd.FmdError) as ei:
        bank.pulses([0, 65])
    assert ei.value.status == INVALID_ARG


def test_refusals_of_a_call_and_kernel_names(fmd):
    import torch
    c = pc.case("streams_1")
    per_call, info = pc.expected("streams_1")
    bank = _bank(fmd, c)
    bank.run(c.calls[0])
    lib, iq = fmd.lib(), np.zeros(64, np.uint8)
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.fmd_pulses_run_batch(bank._h, iq.ctypes.data, 12, 16) == BAD_LENGTH
    assert lib.fmd_pulses_run_batch(bank._h, iq.ctypes.data, 24, 16) == CAPACITY
    assert lib.fmd_pulses_run_batch(bank._h, iq.ctypes.data, 8, 18) == INVALID_ARG
    assert lib.fmd_pulses_run_batch(bank._h, None, 8, 8) == INVALID_ARG
    assert lib.fmd_pulses_run_device(bank._h, d.data_ptr(), 12, 16, None) == BAD_LENGTH
    assert lib.fmd_pulses_run_device(bank._h, d.data_ptr(), 24, 16, None) == CAPACITY
    assert lib.fmd_pulses_run_device(bank._h, d.data_ptr() + 2, 8, 16, None) == INVALID_ARG
    assert lib.fmd_pulses_run_device(bank._h, None, 8, 16, None) == INVALID_ARG
    _same(bank, per_call[0])                                 # a refused call takes nothing
    assert bank.info() == info
    assert bank.kernel_name(0) == "fmd_pl::fmd_pulses_tile_kernel" and bank.kernel_name(1) == "fmd_pl::fmd_pulses_gather_kernel"
    with pytest.raises(fmd.FmdError):
        bank.kernel_name(2)


def _capture(fmd):
    """Noise of sigma 6 with a PWM package and, far behind it, a PPM package: (u8 IQ [2 n], the bits of each, their first samples)."""
    rng = np.random.default_rng(31)
    pwm_bits, ppm_bits = rng.integers(0, 2, 40).tolist(), rng.integers(0, 2, 24).tolist()
    n = 131072 + 6000
    x = rng.normal(127.5, 6.0, 2 * n)
    at = (3000, 131072 - 700)                                # the second package lies across the tool's first call
    for p, e in ((at[0], fmd.ook_encode(pwm_bits, "pwm", 20, 60, 150, amplitude=60)), (at[1], fmd.ook_encode(ppm_bits, "ppm", 30, 90, 25, amplitude=60))):
        x[2 * p:2 * p + e.size] += e.astype(np.float64) - 128.0
    return np.clip(np.rint(x), 0, 255).astype(np.uint8), pwm_bits, ppm_bits, at


def test_sender_bank_slicer_and_tool_give_the_sent_bits_back(fmd, tmp_path):
    iq, pwm_bits, ppm_bits, at = _capture(fmd)
    lo, hi = fmd.pulse_thresholds(iq[:4000], 8, 6.0)
    bank = fmd.PulseBank(1, 8, lo, hi, 256, device_id=0)
    slicers = {"pwm": fmd.PulseSlicer("pwm", 20, 60, 10, 300), "ppm": fmd.PulseSlicer("ppm", 30, 90, 10, 300)}
    found = {"pwm": [], "ppm": []}
    pos = 0
    for a in range(0, iq.size, 65536):
        call = iq[None, a:a + 65536]
        bank.run(call)
        recs, info = bank.pulses([0])[0], bank.info()[0]
        for m, s in slicers.items():
            s.push(recs, pos)
            s.idle(info["state"], info["run"])
            found[m] += [k for k in s.take() if not k["flags"] and k["n_bits"]]
        pos += call.shape[1] // 2
    for s in slicers.values():
        s.idle(0, 300)
    assert [fmd.package_bits(k) for k in found["pwm"]] == [pwm_bits] and abs(found["pwm"][0]["start"] - at[0]) <= 8
    assert [fmd.package_bits(k) for k in found["ppm"]] == [ppm_bits] and abs(found["ppm"][0]["start"] - at[1]) <= 8

    path = tmp_path / "capture.bin"
    path.write_bytes(iq.tobytes())
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "ook_gpu")
    hexof = lambda bits: np.packbits(np.array(bits, np.uint8)).tobytes().hex().upper()
    common = ["-W", "8", "-l", str(lo), "-h", str(hi), "-t", "10", "-R", "300"]
    p = subprocess.run([exe] + common + ["-m", "pwm", "-S", "20", "-L", "60", str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [l.split() for l in p.stdout.splitlines()]
    assert [l[1:] for l in lines] == [["40", hexof(pwm_bits)]] and abs(int(lines[0][0]) - at[0]) <= 8
    assert p.stderr.split()[:2] == ["samples", str(iq.size // 2)] and "dropped 0" in p.stderr
    p = subprocess.run([exe] + common + ["-m", "ppm", "-S", "30", "-L", "90", str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [l.split() for l in p.stdout.splitlines()]
    assert [l[1:] for l in lines] == [["24", hexof(ppm_bits)]] and abs(int(lines[0][0]) - at[1]) <= 8
    assert subprocess.run([exe, "-W", "65"] + common[2:] + ["-m", "pwm", "-S", "20", "-L", "60", str(path)], capture_output=True).returncode == 1
