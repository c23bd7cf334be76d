"""Tone-pair demodulator (include/fmd.h, fmd_afsk_*) on the MI355X where tests/test_gpu_afsk.py does not reach: every window and
stride of the domain (1551 pairs) with a carried history of every reachable length and a second tile behind it; every history
length against every input row offset (all 64 origins of the LDS plane) in calls of one tile and of two; rows too short for a whole
16-byte chunk at every alignment, with a refused piece in front; every pre_shift against every out_shift, and full-scale windows at
T = 64 under every pre_shift; tile counts against row counts around 256; 40000 rows.  Outputs and counts() against the test-side
definition (tests/afsk_ref.py), bit for bit, after every call; rows_gpu's call and call_at check that nothing beyond the outputs is
written and that the input stays as it was.  The cases come from tests/packet_cases.py; tests/test_packet_cases.py shows without a
GPU what each of them reaches.  FMD_FUZZ_SEED reseeds them."""
import numpy as np
import pytest

import afsk_ref as ar
import packet_cases as pc
from rows_gpu import TOO_SHORT, call, call_at

pytestmark = pytest.mark.gpu


def _handle(fmd, c):
    return fmd.AfskDemod(c.tab, c.D, c.pre, c.out, n_rows=c.rows, device_id=0)


def _feed(fmd, c, runs=None, h=None, rows=None):
    """The case's runs through one handle, reset between them (`h`; a fresh one per run where None): every piece against the
    definition over the run's stream (`rows`: only these rows are compared), outputs and counts() after every call; the refused
    pieces are the ones the counting rule names, are FMD_ERR_TOO_SHORT and change nothing."""
    for r in runs or c.runs:
        dm = _handle(fmd, c) if h is None else h
        dm.reset()
        pieces = pc.af_pieces(c, r)
        n = max(hi for _, hi, _, _, _ in pieces)
        xs = c.x if rows is None else c.x[rows]
        whole = ar.demod(xs[:, :n], c.tab, c.D, c.pre, c.out)
        for lo, hi, refused, in_cap, _ in pieces:
            piece = c.x[:, lo:hi, None]
            feed = (lambda: call_at(dm, piece, r.off_in, r.off_out, out_pad=3)) if r.mode == "at" else (lambda: call(dm, piece, in_cap, out_pad=3))
            if refused:
                before = dm.counts()
                with pytest.raises(fmd.FmdError) as e:
                    feed()
                assert e.value.status == TOO_SHORT and dm.counts() == before, (c.name, r.cuts, lo, hi)
                continue
            got = feed()[:, :, 0]
            o0, o1 = ar.outputs(c.T, c.D, lo), ar.outputs(c.T, c.D, hi)
            assert got.shape == (c.rows, o1 - o0), (c.name, r.cuts, lo, hi)
            assert np.array_equal(got if rows is None else got[rows], whole[:, o0:o1]), (c.name, r.cuts, r.mode, r.off_in, r.off_out, lo, hi)
            assert dm.counts() == (hi, o1), (c.name, r.cuts, lo, hi)


@pytest.mark.parametrize("g", range(len(pc.SHAPE_GROUPS)), ids=["T%d-%d" % (g[0], g[-1]) for g in pc.SHAPE_GROUPS])
def test_every_window_and_stride(fmd, g):
    """Every D of nine T per test: the cut T + 3 D + r | rest (the second call carries h = T - D + r and has a second tile), then the
    stream uncut on a fresh handle."""
    for c in pc.af_every_shape(pc.SHAPE_GROUPS[g]):
        _feed(fmd, c)


@pytest.mark.parametrize("T,D", pc.HIST_PAIRS)
def test_every_history_length_at_every_row_offset(fmd, T, D):
    c = pc.af_history_alignment(T, D)
    _feed(fmd, c, h=_handle(fmd, c))


@pytest.mark.parametrize("T,D", pc.SHORT_PAIRS)
def test_rows_shorter_than_a_chunk_at_every_alignment(fmd, T, D):
    c = pc.af_short_rows(T, D)
    _feed(fmd, c, h=_handle(fmd, c))


def test_every_pre_shift_against_every_out_shift(fmd):
    for c in pc.af_every_shift():
        _feed(fmd, c)


def test_full_scale_windows_under_every_pre_shift(fmd):
    for c in pc.af_full_scale():
        _feed(fmd, c)


@pytest.mark.parametrize("rows", pc.TILE_ROWS)
def test_tile_counts_against_row_counts(fmd, rows):
    for c in pc.af_tiles_and_rows(rows):
        _feed(fmd, c)


def test_40000_rows(fmd):
    c = pc.af_many_rows()
    _feed(fmd, c, rows=c.sample)
