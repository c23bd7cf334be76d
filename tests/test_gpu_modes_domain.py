"""The Mode S bank on the MI355X over the cases of tests/modes_domain_cases.py, bit for bit against the definition (tests/modes_ref.py):
after every call the counts and the records of every stream, at the end the counters.  A candidate queue of more than two waves'
length with acceptances on every side of its chunks, the single-bit fix at each of the 112 bits and double flips across the seam of
its ballots, every downlink format on either side of the selection, msg_cap cut inside a tile and over the sum of many, 130 tiles in
one call and in two, full-scale samples and a message at absolute position 0."""
import numpy as np
import pytest

import modes_domain_cases as dc

pytestmark = pytest.mark.gpu


def _bank(fmd, c):
    g = c.cfg
    return fmd.ModeSBank(c.n_streams, g["min_power"], g["fix_errors"], g["df11"], g["msg_cap"], device_id=0)


def _same(bank, want, what=None):
    """counts and the records of every stream are the definition's (counts, kept records per stream)"""
    counts, recs = want
    got = bank.counts()
    assert got.tolist() == list(counts), (what, got.tolist(), list(counts))
    every = bank.messages(np.arange(bank.n_streams))
    bad = [s for s in range(bank.n_streams) if every[s] != recs[s]]
    assert not bad, (what, bad[:8], every[bad[0]][:2], recs[bad[0]][:2])


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_case_matches_the_definition(fmd, name):
    c = dc.case(name)
    per_call, info = dc.expected(name)
    assert c.cfg["msg_cap"] <= 256 and dc.tile() == fmd.modes_tile()
    bank = _bank(fmd, c)
    for i, (iq, want) in enumerate(zip(c.calls, per_call)):
        bank.run(iq)
        _same(bank, want, (name, i))
    assert bank.info() == info
    bank.check()
