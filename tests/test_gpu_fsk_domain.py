"""FSK front end of the pager decoder (include/fmd.h, fmd_fsk_*) over its domain on the MI355X: the case tables of tests/digital_cases.py
through the handle, every output, count and record and counts() bit for bit against the test-side definition (tests/fsk_ref.py) after
every call.  tests/test_digital_cases.py shows without a GPU what each case reaches: all 1024 (D, W), every residue of the carries and
every row offset, a stream across box 65536, the rule's equalities, every shift on both rails, the records' lanes and caps, and the
rows."""
import numpy as np
import pytest

import digital_cases as dg
from rows_gpu import call, call_at
from test_gpu_fsk import _demod, _hits_equal

pytestmark = pytest.mark.gpu


def _run(fmd, c, run, rows=None):
    """run `run` of the case on a fresh handle, call by call against the definition (over the rows `rows` where given); the handle"""
    r = c.runs[run]
    dem = _demod(fmd, c.cfg, c.rows)
    for i, (lo, hi, want, counts, rec, total) in enumerate(dg.fk_reference(c, run, rows)):
        piece = np.ascontiguousarray(c.x[:, lo:hi, None])
        got = (call(dem, piece) if r.offs is None else call_at(dem, piece, *r.offs[i]))[:, :, 0]
        if rows is None:
            assert got.shape == want.shape and np.array_equal(got, want), (c.name, lo, hi)
            assert _hits_equal(dem, counts, rec), (c.name, lo, hi)
        else:
            n, records = dem.hits()
            assert np.array_equal(got[rows], want) and np.array_equal(n[rows], counts) and np.array_equal(dem.hit_counts()[rows], counts)
            assert np.array_equal(records[rows].view(np.uint32), rec.view(np.uint32)), (c.name, lo, hi)
        assert dem.counts() == total
    return dem


@pytest.mark.parametrize("W", range(1, 17))
def test_every_box_and_filter_length(fmd, W):
    for D in range(1, 65):
        c = dg.fk_every_shape(D, W)
        _run(fmd, c, 0)
        _run(fmd, c, 1)


@pytest.mark.parametrize("D,W,last", dg.FK_CARRY)
def test_every_residue_of_the_carries_and_every_row_offset(fmd, D, W, last):
    _run(fmd, dg.fk_carries(D, W, last), 0)


@pytest.mark.parametrize("D", [1, 3])
def test_a_stream_across_box_65536(fmd, D):
    c = dg.fk_line(D)
    _run(fmd, c, 0)
    _run(fmd, c, 1)


def test_the_equalities_of_the_rule(fmd):
    for c, variant, hits in dg.fk_equalities():
        dem = _run(fmd, c, 0)
        n, rec = dem.hits()
        assert bool([h for h in rec[0, :n[0]] if h["k_rel"] == 31]) == hits, c.name
    for sync in (0, 0xFFFFFFFF):
        c = dg.fk_top(sync)
        dem = _run(fmd, c, 0)
        n, rec = dem.hits()
        assert n[0] == 46 and (rec[0, :46]["corr"] == (-1 if sync else 1) << 20).all()
        _run(fmd, c, 1)


@pytest.mark.parametrize("D,W,shift", dg.FK_SHIFTS)
def test_every_shift_on_both_rails(fmd, D, W, shift):
    _run(fmd, dg.fk_shift(D, W, shift), 0)


@pytest.mark.parametrize("hit_cap", dg.FK_CAPS)
def test_records_lanes_and_caps(fmd, hit_cap):
    c = dg.fk_records(hit_cap)
    _run(fmd, c, 0)
    _run(fmd, c, 1)


@pytest.mark.parametrize("rows", dg.FK_ROWS)
def test_row_counts_around_the_tile(fmd, rows):
    _run(fmd, dg.fk_rows(rows), 0)


def test_40000_rows_sampled(fmd):
    c = dg.fk_rows(dg.FK_MANY)
    _run(fmd, c, 0, c.sample)
