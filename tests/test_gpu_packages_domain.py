"""The package bank on the MI355X over the cases of tests/packages_domain_cases.py, bit for bit against the definitions: a run of 1 ...
64 bits appended to a carried package at every kind of bit offset, with truncation on either side of 256 bits; and the pulse bank and
the package bank composed on the device over 1, 4, 5 and 65 streams at a pulse_cap of 16, PWM and PPM, with silent streams and one
whose pulse count is far above pulse_cap."""
import numpy as np
import pytest

import packages_cases as kc
import packages_domain_cases as dc

pytestmark = pytest.mark.gpu


def _same(bank, counts, pkgs, what):
    got = bank.counts()
    assert got.tolist() == list(counts), (what, got.tolist(), list(counts))
    every = bank.packages(np.arange(bank.n_streams))
    bad = [s for s in range(bank.n_streams) if every[s] != pkgs[s]]
    assert not bad, (what, bad[:8], [(a, b) for a, b in zip(every[bad[0]], pkgs[bad[0]]) if a != b][:2])


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_case_matches_the_definition(fmd, name):
    c = dc.case(name)
    per_call, info = dc.expected(name)
    g = c.cfg
    bank = fmd.PackageBank(c.n_streams, g["modulation"], g["short"], g["long"], g["tol"], g["reset"], g["min_bits"], g["pkg_cap"], device_id=0)
    ref_bank = kc.ref_bank(c)
    for i, (call, (counts, pkgs)) in enumerate(zip(c.calls, per_call)):
        bank.run_batch(call.counts, call.recs, call.totals, call.n_samples)
        _same(bank, counts, pkgs, (name, i))
        ref_bank.run(call.counts, [kc.rows_of(call, s) for s in range(c.n_streams)], call.recs.shape[1], call.totals, call.n_samples)
        assert bank.info() == ref_bank.info, (name, i)
    assert bank.info() == info
    bank.check()


@pytest.mark.parametrize("m", ["pwm", "ppm"])
@pytest.mark.parametrize("n_streams", dc.COMPOSED_STREAMS)
def test_pulse_bank_and_package_bank_composed_on_many_streams(fmd, n_streams, m):
    """PulseBank.run_device then run_bank, three calls and a flush, nothing read to the host between the two banks: after every call
    the pulse counts, the package counts, the packages and the totals are those of the two definitions chained."""
    import torch
    c, want = dc.composed_case(n_streams, m), dc.composed_expected(n_streams, m)
    g = dc.PULSE_CFG
    d = torch.from_numpy(c.iq).cuda()
    stream = torch.cuda.Stream()
    pulses = fmd.PulseBank(n_streams, g["W"], g["lo"], g["hi"], g["pulse_cap"], device_id=0)
    bank = fmd.sliced(pulses, m, dc.SHORT, dc.LONG, dc.TOL, dc.RESET_GAP, device_id=0)
    assert bank.pkg_cap == g["pulse_cap"] + 1 and d.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    for k, (p_counts, counts, pkgs, info) in enumerate(want[:3]):
        pulses.run_device(d.data_ptr() + 2 * dc.CALL * k, 2 * dc.CALL, c.iq.shape[1], stream=stream.cuda_stream)
        bank.run_bank(pulses, stream=stream.cuda_stream)
        _same(bank, counts, pkgs, (c.name, k))
        assert bank.info() == info, (c.name, k)
        assert pulses.counts().tolist() == p_counts
    _, counts, pkgs, info = want[3]
    bank.flush(stream=stream.cuda_stream)
    _same(bank, counts, pkgs, (c.name, "flush"))
    assert bank.info() == info
    bank.check()
    pulses.check()
