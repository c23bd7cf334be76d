"""The Mode S bank (include/fmd.h, fmd_modes_*) on the MI355X: after every call the counts, the records of every stream and at the end
the counters, bit for bit against the definition (tests/modes_ref.py) over the cases of tests/modes_cases.py -- a message on every
side of a tile's end, three cuttings of one stream, stream counts around a wave, overflow inside a tile and across tiles, the fix,
min_power -- and the other surfaces: reset, empty calls, host against device input at both alignments, the selection of streams, the
refusals of a call, the kernel names and the command-line tool."""
import os
import subprocess

import numpy as np
import pytest

import modes_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_LENGTH, CAPACITY = -1, -2, -5


def _bank(fmd, c, **over):
    cfg = dict(c.cfg, **over)
    return fmd.ModeSBank(c.n_streams, cfg["min_power"], cfg["fix_errors"], cfg["df11"], cfg["msg_cap"], device_id=0)


def _same(bank, want, what=None):
    """counts and the records of every stream are the definition's (counts, kept records per stream)"""
    counts, recs = want
    got = bank.counts()
    assert got.tolist() == list(counts), (what, got.tolist(), list(counts))
    every = bank.messages(np.arange(bank.n_streams))
    bad = [s for s in range(bank.n_streams) if every[s] != recs[s]]
    assert not bad, (what, bad[:8], every[bad[0]][:2], recs[bad[0]][:2])


@pytest.mark.parametrize("name", [n for n in mc.CASE_NAMES if n != "cuts_four"])
def test_case_matches_the_definition(fmd, name):
    c = mc.case(name)
    per_call, info = mc.expected(name)
    bank = _bank(fmd, c)
    for i, (iq, want) in enumerate(zip(c.calls, per_call)):
        bank.run(iq)
        _same(bank, want, (name, i))
    assert bank.info() == info
    bank.check()


def test_calls_of_four_samples_give_the_same_records(fmd):
    """4096 calls of 8 bytes: the counts come back after each, the records where a call has some; in absolute positions the stream's
    records are those of one call, and the counters agree."""
    c = mc.case("cuts_four")
    per_call, info = mc.expected("cuts_four")
    want = mc.absolute(per_call, c.calls, 0)
    assert want == mc.absolute(mc.expected("cuts_one")[0], mc.case("cuts_one").calls, 0)
    bank = _bank(fmd, c)
    got, pos = [], 0
    for iq, (counts, recs) in zip(c.calls, per_call):
        bank.run(iq)
        n = bank.counts()
        assert n.tolist() == list(counts), pos
        if n[0]:
            got += [dict({k: v for k, v in r.items() if k != "k_rel"}, p=pos + r["k_rel"]) for r in bank.messages([0])[0]]
        pos += iq.shape[1] // 2
    assert got == want and bank.info() == info


def test_reset_empty_calls_and_short_calls(fmd):
    c = mc.case("cuts_random")
    per_call, info = mc.expected("cuts_random")
    bank = _bank(fmd, c)
    assert bank.counts().tolist() == [0] and bank.info() == [{"samples": 0, "candidates": 0, "messages": 0, "fixed": 0}]
    for rounds in range(2):
        last = None
        for iq, want in zip(c.calls, per_call):
            bank.run(iq)
            _same(bank, want)
            bank.run(iq[:, :0])                              # nbytes == 0: nothing launched, the results stay
            _same(bank, want)
            last = want
        assert bank.info() == info and last is not None
        bank.reset()
        assert bank.counts().tolist() == [0] and bank.info()[0]["samples"] == 0


@pytest.mark.parametrize("off", [0, 4, 8])
def test_device_input_matches_host_input(fmd, off):
    """run_device on rows cap_bytes apart, `off` bytes behind a 16-byte boundary and with a pitch that is no multiple of 16, with
    sentinels between the rows' valid bytes: the same results as run_batch."""
    import torch
    c = mc.case("streams_3")
    per_call, info = mc.expected("streams_3")
    nbytes = c.calls[0].shape[1]
    cap_bytes = nbytes + (20 if off else 32)
    host = np.full(3 * cap_bytes + 32, 0xC8, np.uint8)       # (a sentinel that would decode as pulses if it were read)
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


def test_selection_of_streams_in_a_chosen_order(fmd):
    c = mc.case("streams_65")
    per_call, _ = mc.expected("streams_65")
    bank = _bank(fmd, c)
    bank.run(c.calls[0])
    counts, recs = per_call[0]
    order = [64, 0, 33, 2, 2, 1]
    assert bank.messages(order) == [recs[s] for s in order]
    assert bank.messages([]) == []
    raw = bank.records([2])[0]                               # zeros behind the stream's own records
    assert counts[2] < bank.msg_cap and all(bytes(raw[k]) == bytes(32) for k in range(counts[2], bank.msg_cap))
    with pytest.raises(fmd.FmdError) as ei:
        bank.messages([0, 65])
    assert ei.value.status == INVALID_ARG


def test_refusals_of_a_call_and_kernel_names(fmd):
    import torch
    c = mc.case("min_power_at")
    per_call, info = mc.expected("min_power_at")
    bank = _bank(fmd, c)
    bank.run(c.calls[0])
    lib, iq = fmd.lib(), np.zeros(64, np.uint8)
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.fmd_modes_run_batch(bank._h, iq.ctypes.data, 12, 16) == BAD_LENGTH
    assert lib.fmd_modes_run_batch(bank._h, iq.ctypes.data, 24, 16) == CAPACITY
    assert lib.fmd_modes_run_batch(bank._h, iq.ctypes.data, 8, 18) == INVALID_ARG
    assert lib.fmd_modes_run_batch(bank._h, None, 8, 8) == INVALID_ARG
    assert lib.fmd_modes_run_device(bank._h, d.data_ptr(), 12, 16, None) == BAD_LENGTH
    assert lib.fmd_modes_run_device(bank._h, d.data_ptr(), 24, 16, None) == CAPACITY
    assert lib.fmd_modes_run_device(bank._h, d.data_ptr() + 2, 8, 16, None) == INVALID_ARG
    assert lib.fmd_modes_run_device(bank._h, None, 8, 16, None) == INVALID_ARG
    _same(bank, per_call[0])                                 # a refused call takes nothing
    assert bank.info() == info
    assert bank.kernel_name(0) == "fmd_ms::fmd_modes_tile_kernel" and bank.kernel_name(1) == "fmd_ms::fmd_modes_gather_kernel"
    with pytest.raises(fmd.FmdError):
        bank.kernel_name(2)


def test_cli_prints_rtl_adsb_lines(fmd, tmp_path):
    """adsb_gpu on a synthetic capture over two calls: one `*HEX;` line per message, the damaged one only with -e, the short one only
    with -S, and the counters on stderr."""
    n = 131072 + 4000
    iq = mc.noise(1, n, 77)
    msgs = [(500, mc.LONG[0]), (131072 - 100, mc.LONG[1]), (131072 + 900, mc.flip(mc.LONG[2], 50)), (131072 + 1500, mc.short_msg(3)),
            (131072 + 2500, mc.LONG[3])]
    for p, m in msgs:
        mc.place(iq, 0, p, m)
    path = tmp_path / "capture.bin"
    path.write_bytes(iq.tobytes())
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "adsb_gpu")
    line = lambda m: "*%s;" % m.hex().upper()
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.split() == [line(mc.LONG[0]), line(mc.LONG[1]), line(mc.LONG[3])]
    assert p.stderr.split()[:2] == ["samples", str(n)] and "messages 3 fixed 0" in p.stderr
    p = subprocess.run([exe, "-e", "-S", "-v", str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    out = p.stdout.splitlines()
    assert [l for l in out if l.startswith("*")] == [line(mc.LONG[0]), line(mc.LONG[1]), line(mc.LONG[2]), line(mc.short_msg(3)), line(mc.LONG[3])]
    assert any("callsign KLM1023" in l for l in out) and any("altitude 38000 ft" in l and "fixed bit 50" in l for l in out)
    assert any("speed 159 kt track 183 deg vrate -832 ft/min" in l for l in out)
