"""The package bank (include/fmd.h, fmd_packages_*) on the MI355X: after every call the counts, the packages of every stream and the
totals, bit for bit against the definition (tests/packages_ref.py) over the cases of tests/packages_cases.py -- packages that end on
every side of a chunk of 64 records, boundaries and bad records at the chunk's edges with and without a carried package, the windows'
edges, truncation at 256 bits, a close on every record at four capacities, the reading limits, the idle test and flush, min_bits,
start, stream counts around a workgroup and a wave -- and the other surfaces: reset, empty calls, the selection of streams, the
refusals of a call, rows against the C slicer, the pulse bank and the package bank composed on the device at three cuttings, and the
command-line tool with and without -G."""
import os
import subprocess

import numpy as np
import pytest

import packages_cases as kc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED, BAD_STATE = -1, -6, -7


def _bank(fmd, c, **over):
    g = dict(c.cfg, **over)
    return fmd.PackageBank(c.n_streams, g["modulation"], g["short"], g["long"], g["tol"], g["reset"], g["min_bits"], g["pkg_cap"], device_id=0)


def _feed(bank, call):
    if call.flush:
        bank.flush()
    else:
        bank.run_batch(call.counts, call.recs, call.totals, call.n_samples)


def _same(bank, want, what=None):
    """counts and the packages of every stream are the definition's (counts, kept packages per stream)"""
    counts, pkgs = want
    got = bank.counts()
    assert got.tolist() == list(counts), (what, got.tolist(), list(counts))
    every = bank.packages(np.arange(bank.n_streams))
    bad = [s for s in range(bank.n_streams) if every[s] != pkgs[s]]
    assert not bad, (what, bad[:8], [(a, b) for a, b in zip(every[bad[0]], pkgs[bad[0]]) if a != b][:2])


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_case_matches_the_definition(fmd, name):
    c = kc.case(name)
    per_call, info = kc.expected(name)
    bank = _bank(fmd, c)
    ref_bank, lib_infos = kc.ref_bank(c), []
    for i, (call, want) in enumerate(zip(c.calls, per_call)):
        _feed(bank, call)
        _same(bank, want, (name, i))
        lib_infos.append(bank.info())
    # the totals after every call, not only at the end
    for call, got in zip(c.calls, lib_infos):
        if call.flush:
            ref_bank.flush()
        else:
            ref_bank.run(call.counts, [kc.rows_of(call, s) for s in range(c.n_streams)], call.recs.shape[1], call.totals, call.n_samples)
        assert got == ref_bank.info
    assert lib_infos[-1] == info
    bank.check()


def test_reset_and_calls_of_no_samples(fmd):
    c = kc.case("streams_3")
    per_call, info = kc.expected("streams_3")
    bank = _bank(fmd, c)
    assert bank.counts().tolist() == [0] * 3 and bank.info() == [kc.ref.ZERO] * 3
    for rounds in range(2):
        for call, want in zip(c.calls, per_call):
            _feed(bank, call)
            _same(bank, want)
            bank.run_batch(call.counts, call.recs, call.totals, 0)      # n_samples == 0: nothing launched, the results stay
            _same(bank, want)
        assert bank.info() == info and any(i["open"] for i in info)
        bank.reset()
        assert bank.counts().tolist() == [0] * 3 and bank.info() == [kc.ref.ZERO] * 3
        assert bank.packages([0, 1, 2]) == [[], [], []]


def test_selection_of_streams_in_a_chosen_order(fmd):
    c = kc.case("streams_65")
    per_call, _ = kc.expected("streams_65")
    bank = _bank(fmd, c)
    _feed(bank, c.calls[0])
    counts, pkgs = per_call[0]
    order = [64, 0, 33, 3, 3, 2]
    assert bank.packages(order) == [pkgs[s] for s in order] and any(pkgs[s] for s in order)
    assert bank.packages([]) == []
    s = int(np.argmax(counts))
    raw = bank.records([s])[0]                               # zeros behind the stream's own packages
    assert 0 < counts[s] < bank.pkg_cap and all(bytes(raw[k]) == bytes(56) for k in range(counts[s], bank.pkg_cap))
    with pytest.raises(fmd.FmdError) as ei:
        bank.packages([0, 65])
    assert ei.value.status == INVALID_ARG


def test_refusals_of_a_call_and_the_kernel_name(fmd):
    c = kc.case("streams_1")
    per_call, info = kc.expected("streams_1")
    bank = _bank(fmd, c)
    _feed(bank, c.calls[0])
    lib, call = fmd.lib(), c.calls[0]
    tot = (fmd.pulses.PulsesTotals * 1)()
    cnt, recs = np.zeros(1, np.uint32), np.zeros((1, 1025, 4), np.uint32)
    for rec_cap in (0, 1025):
        assert lib.fmd_packages_run_batch(bank._h, cnt.ctypes.data, recs.ctypes.data, rec_cap, tot, 8) == UNSUPPORTED
        assert lib.fmd_last_error().decode() == "need 1 <= rec_cap <= 1024"
    assert lib.fmd_packages_run_batch(bank._h, None, recs.ctypes.data, 4, tot, 8) == INVALID_ARG
    assert lib.fmd_packages_run_batch(bank._h, cnt.ctypes.data, None, 4, tot, 8) == INVALID_ARG
    assert lib.fmd_packages_run_batch(bank._h, cnt.ctypes.data, recs.ctypes.data, 4, None, 8) == INVALID_ARG
    assert lib.fmd_packages_run_bank(bank._h, None, None) == INVALID_ARG
    other, fresh = fmd.PulseBank(2, 1, 1000, 5000, 8, device_id=0), fmd.PulseBank(1, 1, 1000, 5000, 8, device_id=0)
    assert lib.fmd_packages_run_bank(bank._h, other._h, None) == INVALID_ARG          # another n_streams
    assert lib.fmd_packages_run_bank(bank._h, fresh._h, None) == BAD_STATE           # has not launched
    fresh.run(np.full((1, 16), 128, np.uint8))
    fresh.reset()
    assert lib.fmd_packages_run_bank(bank._h, fresh._h, None) == BAD_STATE           # nor since its reset
    _same(bank, per_call[0])                                 # a refused call takes nothing
    first = kc.ref_bank(c)
    first.run(call.counts, [kc.rows_of(call, 0)], call.recs.shape[1], call.totals, call.n_samples)
    assert bank.info() == first.info
    bank.check()
    assert bank.kernel_name() == "fmd_pk::fmd_packages_kernel"
    for call, want in list(zip(c.calls, per_call))[1:]:
        _feed(bank, call)
        _same(bank, want)
    assert bank.info() == info


@pytest.mark.parametrize("name", ["host_rows", "host_rows_ppm"])
def test_rows_match_the_c_slicer(fmd, name):
    """No call closes more than 64 packages, so a C fmd_pulse_slicer per stream, emptied after every call, holds them all."""
    c = kc.case(name)
    g = c.cfg
    bank = _bank(fmd, c)
    slicers = [fmd.PulseSlicer(g["modulation"], g["short"], g["long"], g["tol"], g["reset"]) for _ in range(c.n_streams)]
    total = 0
    for call in c.calls:
        _feed(bank, call)
        got = bank.packages(np.arange(c.n_streams))
        for s, sl in enumerate(slicers):
            n = min(call.counts[s], call.recs.shape[1])
            sl.push(kc.rows_of(call, s)[:n], call.totals[s]["samples"] - call.n_samples)
            sl.idle(call.totals[s]["state"], call.totals[s]["run"])
            want = sl.take()
            assert got[s] == want and len(want) < 64, (s, got[s][:2], want[:2])
            total += len(want)
    assert total >= 10


def _ook_stream(fmd):
    """Four PWM packages of 12 ... 70 bits on a quiet stream: (u8 IQ [2 n] with n % 4 == 0, the bits of each)."""
    rng = np.random.default_rng(17)
    bits = [rng.integers(0, 2, n).tolist() for n in (12, 70, 1, 33)]
    parts = [fmd.ook_encode(b, "pwm", 4, 9, 5, lead=60, trail=3) for b in bits]
    iq = np.concatenate(parts + [np.full(2 * 80, 128, np.uint8)])
    return iq[:iq.size // 8 * 8], bits


@pytest.fixture(scope="module")
def ook_want(fmd):
    """What PulseSlicer gives behind PulseBank.pulses for the stream as one call: computed once, shared, left unchanged."""
    iq, bits = _ook_stream(fmd)
    bank, slicer = fmd.PulseBank(1, 1, 1000, 5000, 512, device_id=0), fmd.PulseSlicer("pwm", 4, 9, 1, 40)
    bank.run(iq[None])
    info = bank.info()[0]
    slicer.push(bank.pulses([0])[0], 0)
    slicer.idle(info["state"], info["run"])
    want = slicer.take()
    assert [fmd.package_bits(k) for k in want] == bits and not any(k["flags"] for k in want)
    return want


@pytest.mark.parametrize("how", ["one", "random", "four"])
def test_pulse_bank_and_package_bank_composed_on_the_device(fmd, ook_want, how):
    """PulseBank.run_device then run_bank on one stream, nothing visiting the host between them: whatever the cutting, the packages
    in total are those of the host slicer behind the pulse bank."""
    import torch
    iq, _ = _ook_stream(fmd)
    n = iq.size // 2
    if how == "one":
        cuts = []
    elif how == "random":
        cuts = sorted(set((np.random.default_rng(5).integers(1, n // 4, 12) * 4).tolist()))
    else:
        cuts = list(range(4, n, 4))
    d = torch.from_numpy(iq).cuda()
    stream = torch.cuda.Stream()
    pulses = fmd.PulseBank(1, 1, 1000, 5000, 512, device_id=0)
    bank = fmd.sliced(pulses, "pwm", 4, 9, 1, 40, device_id=0)
    assert bank.pkg_cap == 513 and bank.n_streams == 1
    torch.cuda.synchronize()
    got = []
    for a, b in zip([0] + cuts, cuts + [n]):
        pulses.run_device(d.data_ptr() + 2 * a, 2 * (b - a), 2 * (b - a), stream=stream.cuda_stream)
        bank.run_bank(pulses, stream=stream.cuda_stream)
        if bank.counts()[0]:
            got += bank.packages([0])[0]
    bank.flush(stream=stream.cuda_stream)
    got += bank.packages([0])[0]
    bank.check()
    assert got == ook_want
    info = bank.info()[0]
    assert info["records"] == pulses.info()[0]["pulses"] == sum(k["n_pulses"] for k in got) and info["packages"] == 4 and not info["open"]


def test_tool_prints_the_same_with_the_device_bank(fmd, tmp_path):
    """ook_gpu -G (packages from the device bank: run_bank per call, flush at the end) prints what ook_gpu prints."""
    rng = np.random.default_rng(31)
    n = 131072 + 6000
    x = rng.normal(127.5, 6.0, 2 * n)
    bits = [rng.integers(0, 2, 40).tolist(), rng.integers(0, 2, 24).tolist()]
    for p, b in zip((3000, 131072 - 700), bits):             # the second package lies across the tool's first call
        e = fmd.ook_encode(b, "pwm", 20, 60, 150, amplitude=60)
        x[2 * p:2 * p + e.size] += e.astype(np.float64) - 128.0
    iq = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    lo, hi = fmd.pulse_thresholds(iq[:4000], 8, 6.0)
    path = tmp_path / "capture.bin"
    path.write_bytes(iq.tobytes())
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "ook_gpu")
    args = ["-W", "8", "-l", str(lo), "-h", str(hi), "-t", "10", "-R", "300", "-m", "pwm", "-S", "20", "-L", "60"]
    outs = []
    for extra in ([], ["-G"], ["-v"], ["-v", "-G"]):
        p = subprocess.run([exe] + args + extra + [str(path)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        outs.append((p.stdout, p.stderr))
    assert outs[0] == outs[1] and outs[2] == outs[3]
    hexof = lambda b: np.packbits(np.array(b, np.uint8)).tobytes().hex().upper()
    assert [l.split()[1:] for l in outs[1][0].splitlines()] == [["40", hexof(bits[0])], ["24", hexof(bits[1])]]
    assert len(outs[3][0].splitlines()) >= 2
