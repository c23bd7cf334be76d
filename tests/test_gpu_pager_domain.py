"""The page bank (include/fmd.h, fmd_pager_*) on the MI355X over the cases of tests/pager_domain_cases.py (what each reaches and which
wrong kernel it tells: tests/test_pager_domain.py): after every call the counts, every byte of every row's records, info() and
inputs() against tests/pager_ref.py, as tests/test_gpu_pager.py's `_same` compares them.  The bank is integer-exact: no tolerances.

    A  every rate of pager_cases.RATES and the two whose carry sum passes 2^32, over clean and flipped pages and noise
    B  sample numbers beyond 2^32: the position brought to 2^32 - L by sixteen calls of zeros from one constant device buffer
    C  a call edge on every sample of a line, and calls of one sample
    D  a message of every word count, a short message behind a long one in the same handle, and the short one alone after reset()
    E  lanes of a wave closing on the same sample at different slots, at every msg_cap
    F  the record rules at their edges
    G  40000 rows, a sample of them against the definition"""
import numpy as np
import pytest

import big_cases as bc
import big_gpu
import pager_cases as pc
import pager_domain_cases as dc
from test_gpu_pager import _call, _feed, _pager, _records, _ref, _same

pytestmark = pytest.mark.gpu

T32 = 1 << 32


# ---- A ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dc.RATES))
def test_every_rate_over_clean_and_flipped_pages_and_noise(fmd, name):
    rate = dc.RATES[name]
    x, hits = dc.rate_rows(name)
    pg = _pager(fmd, rate, rows=5)
    total = _feed(fmd, pg, _ref(rate, rows=5), x, hits, [])
    assert total >= 8 and [i["messages"] for i in pg.info()[:2]] == [4, 4] and min(i["batches"] for i in pg.info()) >= 1
    pg.reset()
    assert _feed(fmd, pg, _ref(rate, rows=5), x, hits, dc.CUTS, batch=True) == total


# ---- B ------------------------------------------------------------------------------------------------------------------------------------
IDLE_CAP = 1 << 28


@pytest.fixture(scope="module")
def zeros():
    """three rows of 2^28 zero samples on the device, and a call's counts and records of none"""
    import torch
    big_gpu.need(torch, 4 * bc.GiB)
    buf = torch.zeros(3 * IDLE_CAP, dtype=torch.int16, device="cuda")
    none = torch.zeros(3 * 16 * 4 + 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    yield buf, none
    del buf, none
    torch.cuda.empty_cache()


@pytest.mark.parametrize("run", dc.beyond_runs(), ids=[r[0] for r in dc.beyond_runs()])
def test_sample_numbers_beyond_2_to_the_32(fmd, zeros, run):
    name, L, cuts = run
    buf, none = zeros
    x, hits = dc.beyond_rows()
    pg, ref = _pager(fmd, dc.B_RATE, rows=3), _ref(dc.B_RATE, rows=3)
    for m in [IDLE_CAP] * 15 + [IDLE_CAP - L]:
        pg.run_device(buf.data_ptr(), m, IDLE_CAP, none.data_ptr(), none.data_ptr() + 16, 16)
        pg.check()
        dc.skip(ref, m)
        _same(fmd, pg, ref, m)
    assert ref.pos == T32 - L
    at0 = _ref(dc.B_RATE, rows=3).run(x, *pc.pack(hits, 0, x.shape[1]))[2]
    got = [[] for _ in range(3)]
    lo = 0
    for m in cuts + [x.shape[1]]:
        part = np.ascontiguousarray(x[:, lo:lo + m])
        _call(fmd, pg, ref, part, *pc.pack(hits, lo, part.shape[1]), what=(name, lo))
        for r in range(3):
            got[r] += ref.last[2][r]
        lo += part.shape[1]
    assert ref.pos > T32 and [len(g) for g in got] == [3, 3, 0]
    assert all(m["end_sample"] > T32 for g in got for m in g)
    assert [[dict(m, end_sample=m["end_sample"] - (T32 - L)) for m in g] for g in got] == at0
    assert not bool(buf.any()) and not bool(none.any())      # the constant input, once, on the device
    pg.close()


# ---- C ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.C_RATES)
def test_a_call_edge_on_every_sample_of_a_line(fmd, name):
    rate = dc.RATES[name]
    x, hits, cuts = dc.edge_rows(name)
    pg, ref = _pager(fmd, rate, rows=2 * dc.S), _ref(rate, rows=2 * dc.S)
    assert _feed(fmd, pg, ref, x, hits, cuts, batch=name == "5") == dc.S * (18 + 2)
    assert [i["batches"] for i in pg.info()] == [3] * (2 * dc.S)


def test_calls_of_one_sample_behind_the_first_record(fmd):
    rate = dc.RATES["2"]
    x, hits, cuts = dc.edge_rows_single()
    pg, ref = _pager(fmd, rate, rows=2), _ref(rate, rows=2)
    assert _feed(fmd, pg, ref, x, hits, cuts) == 18 + 2


# ---- D ------------------------------------------------------------------------------------------------------------------------------------
def test_every_message_length_and_a_short_message_behind_a_long_one(fmd):
    (x1, h1, c1), (x2, h2, c2) = dc.length_rows(), dc.short_rows()
    rows = len(dc.D_WORDS)
    pg, ref = _pager(fmd, dc.D_RATE, rows=rows), _ref(dc.D_RATE, rows=rows)
    assert _feed(fmd, pg, ref, x1, h1, c1) == rows
    assert [i["locked"] + i["searching"] for i in pg.info()] == [0] * rows
    assert _feed(fmd, pg, ref, x2, h2, c2) == rows           # the same handle, no reset: the rows' kept bytes are the long message's
    behind = _records(fmd, pg, np.arange(rows)).copy()
    assert [int(m["n_bits"]) for m in behind[:, 0]] == [20 * ((w + 1) % 4) for w in dc.D_WORDS]
    pg.reset()
    assert _feed(fmd, pg, _ref(dc.D_RATE, rows=rows), x2, h2, c2) == rows
    alone = _records(fmd, pg, np.arange(rows)).copy()
    assert (alone["end_sample"][:, 0] + x1.shape[1] == behind["end_sample"][:, 0]).all()
    behind["end_sample"], alone["end_sample"] = 0, 0
    assert behind.tobytes() == alone.tobytes()


# ---- E ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", range(1, 17))
def test_lanes_closing_on_one_sample_at_different_slots(fmd, cap):
    x, hits = dc.closing_rows(cap)
    pg, ref = _pager(fmd, dc.E_RATE, cap=cap, rows=dc.E_ROWS), _ref(dc.E_RATE, cap=cap, rows=dc.E_ROWS)
    _feed(fmd, pg, ref, x, hits, [])
    assert pg.counts().tolist() == [j % (cap + 2) + 1 for j in range(dc.E_ROWS)]
    assert len({e[-1]["end_sample"] for e in ref.last[2]}) == 1
    assert [len(m) for m in pg.msgs(range(dc.E_ROWS))] == [min(j % (cap + 2) + 1, cap) for j in range(dc.E_ROWS)]
    if cap == 4:                                             # once more across two calls: the slot is the call's own count
        pg.reset()
        ref = _ref(dc.E_RATE, cap=cap, rows=dc.E_ROWS)
        _feed(fmd, pg, ref, x, hits, [hits[0][0][0] + dc.E_CUT])
        assert sorted(set(pg.counts().tolist())) == [1, 2, 3]


# ---- F ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.F_RATES)
def test_the_record_rules_at_their_edges(fmd, name):
    rate = dc.RATES[name]
    x, hits = dc.rule_rows(name)
    pg, ref = _pager(fmd, rate, rows=len(hits)), _ref(rate, rows=len(hits))
    _feed(fmd, pg, ref, x, hits, [])
    assert [(i["batches"], i["locked"], i["messages"]) for i in pg.info()] == dc.RULES[name]


# ---- G ------------------------------------------------------------------------------------------------------------------------------------
def test_40000_rows_sampled(fmd):
    x, calls = dc.many_rows()
    sample = dc.many_sample()
    sel = np.array(sample)
    pg, ref = _pager(fmd, dc.G_RATE, rows=dc.G_ROWS), _ref(dc.G_RATE, rows=len(sample))
    for lo, m, counts, rec in calls:
        part = np.ascontiguousarray(x[:, lo:lo + m])
        pg.run_batch(part, counts, rec)
        want, records, every = ref.run(part[sel], counts[sel], rec[sel])
        assert np.array_equal(pg.counts()[sel], want) and _records(fmd, pg, sel).tobytes() == records.tobytes(), lo
        info = pg.info()
        assert [info[r] for r in sample] == ref.info() and pg.inputs() == ref.pos
        assert pg.msgs(sample) == [e[:pg.msg_cap] for e in every]
    pages = [r for r in range(dc.G_ROWS) if dc.many_kind(r) in ("page", "inverted")]
    assert all(info[r]["messages"] == 1 and info[r]["batches"] == 1 for r in pages) and len(pages) > dc.G_ROWS // 2
    assert all(info[r]["messages"] == 0 and info[r]["batches"] == 0 for r in range(dc.G_ROWS) if dc.many_kind(r) == "idle")
    pg.close()
