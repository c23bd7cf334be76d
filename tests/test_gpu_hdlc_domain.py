"""The frame bank (include/fmd.h, fmd_hdlc_*) over its domain on the MI355X: the case tables of tests/digital_cases.py through the handle,
after every call the counts, every byte of every record, the counters and inputs() against the test-side definition (tests/hdlc_ref.py
over tests/ax25_ref.py).  tests/test_digital_cases.py shows without a GPU what each case reaches: every line of `cases()` in either
polarity beside idle and noise rows at three clocks, every frame length from 15 to 512 bytes and the two outside, lanes that close on one
sample at and below their cap, a call edge on every sample of a frame (and which lost state field it tells), the clock on either side of
its switch to 64 bits, and the rows."""
import numpy as np
import pytest

import digital_cases as dg
from test_gpu_hdlc import _feed, _records

pytestmark = pytest.mark.gpu


def _framer(fmd, c):
    return fmd.Ax25Framer(c.num, c.den, c.baud, c.cap, n_rows=c.rows, device_id=0)


def _run(fmd, c, run, fr=None, snaps=None, **kw):
    """run `run` of the case through a fresh (or the reset) handle against the definition's snapshots; the handle and the snapshots"""
    fr = _framer(fmd, c) if fr is None else fr
    snaps = dg.hd_reference(c, run) if snaps is None else snaps
    ref = dg.Replay(snaps)
    _feed(fmd, fr, ref, c.x, c.runs[run] if len(snaps) > 1 else [], **kw)
    assert ref.i == len(snaps) - 1
    return fr, snaps


# ---- 1a: every line of cases() ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", sorted(dg.HD_CLOCKS))
def test_every_line_in_either_polarity_beside_idle_and_noise_rows(fmd, clock):
    c = dg.hd_lines(clock)
    fr, snaps = _run(fmd, c, 1, odd=True)                    # 1 | 7 | 1000 | 333 | rest
    info = fr.info()
    for name, rows in c.claim.where.items():
        for r in rows:
            assert name not in dg.WANT or (info[r]["frames_ok"], info[r]["bad_fcs"], info[r]["aborts"]) == dg.WANT[name], (name, r)
    fr.reset()
    _run(fmd, c, 0, fr, [dg.merged(snaps, c.cap)])           # and in one call
    got = fr.frames([c.claim.where["ff-514"][0]])[0]
    assert [f["data"] for f in got] == [b"\xff" * 512]


# ---- 1b: every frame length ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", range(len(dg.HD_LENGTH_GROUPS)))
def test_every_frame_length_is_delivered_whole(fmd, g):
    c = dg.hd_lengths(g)
    fr, _ = _run(fmd, c, 0, batch=True)
    rec = _records(fmd, fr, np.arange(c.rows))
    for r, d in enumerate(c.claim.bodies):
        assert rec[r, 0]["len"] == len(d) and bytes(rec[r, 0]["data"][:len(d)]) == d and not rec[r, 0]["data"][len(d):].any(), (r, len(d))
    assert fr.counts()[-1] == 0 and fr.info()[-1]["bad_fcs"] == len(c.claim.outside) and fr.info()[-1]["frames_ok"] == 0
    fr.reset()
    _run(fmd, c, 1, fr, odd=True, off=3)


# ---- 1c: frames that close together ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,rows", dg.HD_CLOSE)
def test_lanes_that_close_on_one_sample_at_and_below_their_cap(fmd, cap, rows):
    c = dg.hd_close(cap, rows)
    fr, snaps = _run(fmd, c, 0)
    counts = fr.counts()
    assert counts.tolist() == [k + 1 for k in c.claim.prior]
    got = fr.frames(list(range(rows)))
    for r in range(rows):
        assert [f["data"] for f in got[r]] == c.claim.bodies[r][:cap]


# ---- 1d: every call edge inside a frame ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes,rate", dg.HD_EDGES)
def test_a_call_edge_on_every_sample_of_a_frame(fmd, nbytes, rate):
    c = dg.hd_edges(nbytes, rate)
    fr, _ = _run(fmd, c, 0)
    assert [i["frames_ok"] for i in fr.info()] == [1] * c.rows


def test_call_edges_in_the_last_bytes_and_the_closing_flag_of_the_longest_frame(fmd):
    c = dg.hd_long_edges()
    fr, _ = _run(fmd, c, 0, odd=True)
    assert [i["frames_ok"] for i in fr.info()] == [1] * c.rows


# ---- 1e: the clock switch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod,k", dg.HD_SWITCH)
def test_the_clock_on_either_side_of_its_switch(fmd, mod, k):
    c = dg.hd_switch(mod, k)
    fr, _ = _run(fmd, c, 0)
    assert [i["frames_ok"] for i in fr.info()] == [2, 2, 0]
    fr.reset()
    _run(fmd, c, 1, fr, odd=True)


# ---- 1f: rows -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", dg.HD_ROWS)
def test_row_counts_around_two_waves(fmd, rows):
    c = dg.hd_rows(rows)
    fr, _ = _run(fmd, c, 0, batch=rows % 2 == 0)
    assert [f[0]["data"] for f in fr.frames(list(range(rows)))] == c.claim.bodies


def test_40000_rows_sampled(fmd):
    c = dg.hd_rows(dg.HD_MANY)
    snaps = dg.hd_reference(c, 0, c.sample)
    fr = _framer(fmd, c)
    sel = np.array(c.sample)
    lo = 0
    for snap, m in zip(snaps, c.runs[0] + [c.x.shape[1]]):
        fr.run_batch(np.ascontiguousarray(c.x[:, lo:lo + m]))
        lo += m
        counts, rec, every = snap.last
        assert np.array_equal(fr.counts()[sel], counts) and _records(fmd, fr, sel).tobytes() == rec.tobytes()
        info = fr.info()
        assert [info[r] for r in c.sample] == snap.info and fr.inputs() == snap.pos
        assert fr.frames(c.sample) == [e[:c.cap] for e in every]
    assert all(i["frames_ok"] == 1 and i["bad_fcs"] == 0 for i in info)     # every row of the 40000 delivered its frame
