"""The pulse bank on the MI355X over the cases of tests/pulses_domain_cases.py, bit for bit against the definition (tests/pulses_ref.py):
after every call the counts and the records of every stream, at the end the totals.  130 tiles in one call and in three, with pulses,
gaps, keep tiles and owed edges on the seams between the batches of 64 summaries; boxes of 2 ... 63 samples with and without
hysteresis; the thresholds at both ends of their domain; and, over a constant device buffer of 2^30 samples taken five times, a gap, a
width and a run beyond 2^32 samples."""
import numpy as np
import pytest

import pulses_cases as pc
import pulses_domain_cases as dc

pytestmark = pytest.mark.gpu


def _bank(fmd, c):
    g = c.cfg
    return fmd.PulseBank(c.n_streams, g["W"], g["lo"], g["hi"], g["pulse_cap"], device_id=0)


def _same(bank, want, what=None):
    """counts and the records of every stream are the definition's (counts, kept records per stream)"""
    counts, recs = want
    got = bank.counts()
    assert got.tolist() == list(counts), (what, got.tolist(), list(counts))
    every = bank.pulses(np.arange(bank.n_streams))
    bad = [s for s in range(bank.n_streams) if every[s] != recs[s]]
    assert not bad, (what, bad[:8], every[bad[0]][:3], recs[bad[0]][:3])


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_case_matches_the_definition(fmd, name):
    c = dc.case(name)
    per_call, info = dc.expected(name)
    assert dc.tile() == fmd.pulses_tile()
    bank = _bank(fmd, c)
    for i, (iq, want) in enumerate(zip(c.calls, per_call)):
        bank.run(iq)
        _same(bank, want, (name, i))
    assert bank.info() == info
    bank.check()


def test_gap_width_and_run_beyond_2_32_samples(fmd):
    """The script of pulses_domain_cases.saturation_script on one stream, every call from device memory: a pulse, five calls over 2^30
    quiet samples, a pulse whose gap saturates, a rise, five calls over 2^30 strong samples, a fall whose width saturates.  After
    every call the count, the records and the totals are the definition's; `run` passes 2^32 exactly."""
    import torch
    import big_cases as bc
    import big_gpu
    big_gpu.need(torch, 6 * bc.GiB)
    want = dc.check_saturation()
    g = dc.SAT_CFG
    buf = torch.full((2 * dc.STRETCH,), pc.QUIET, dtype=torch.uint8, device="cuda")
    bank = fmd.PulseBank(1, g["W"], g["lo"], g["hi"], g["pulse_cap"], device_id=0)
    held = pc.QUIET
    for i, ((kind, x), (count, recs, info)) in enumerate(zip(dc.saturation_script(), want)):
        if kind == "bytes":
            d = torch.from_numpy(x[0]).cuda()
            nbytes = x.shape[1]
        else:
            if x != held:                                    # I = x, Q = 128 in every sample, as one 16-bit fill
                buf.view(torch.int16).fill_((128 << 8 | x) - 65536)
                held = x
            d, nbytes = buf, 2 * dc.STRETCH
        torch.cuda.synchronize()
        bank.run_device(d.data_ptr(), nbytes, nbytes)
        bank.check()
        assert bank.counts().tolist() == [count] and bank.pulses([0])[0] == recs, (i, bank.counts().tolist(), bank.pulses([0])[0], recs)
        assert bank.info()[0] == info, (i, bank.info()[0], info)
    assert bank.info()[0]["run"] < 200 and want[11][2]["run"] > 1 << 32
    del buf
    torch.cuda.empty_cache()
