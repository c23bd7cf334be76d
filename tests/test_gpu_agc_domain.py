"""Automatic gain control (include/fmd.h, fmd_agc_*) on the MI355X where tests/test_gpu_agc.py does not reach: every (P, width) cell
from P = 16 to 4096 -- each has its own number of blocks per LDS segment -- with one call over three segments and calls that emit
one block less than, exactly and one block more than a segment; every carried history length around P modulo the 16-byte chunk;
every input row offset against every output row offset; the whole cross of the configuration's corners at both widths at P = 32 (two blocks
per wave and turn in the peak pass) and P = 2048; 40000 rows.  Outputs, counts() and every row's gain() against the test-side definition
(tests/agc_ref.py), bit for bit, after every call.  The cases come from tests/rows_cases.py; tests/test_rows_cases.py shows without
a GPU what each of them reaches.  FMD_FUZZ_SEED reseeds them."""
import numpy as np
import pytest

import agc_ref as ar
import rows_cases as rc
from rows_gpu import call, call_at

pytestmark = pytest.mark.gpu


def _agc(fmd, c):
    cfg = c.cfg
    return fmd.Agc(n_rows=c.rows, width=c.width, target=cfg.target, block=cfg.block, hang=cfg.hang, decay=cfg.decay, gain_max=cfg.gain_max,
                   device_id=0)


def _odd(n):
    return n + 1 + n % 2


def _feed(fmd, c, ag=None):
    """The case's calls against the definition, call by call (odd in_cap, odd out_cap): the outputs, counts() and every row's
    (G, h).  Returns the outputs."""
    ag = _agc(fmd, c) if ag is None else ag
    ref = ar.Agc(c.cfg)
    outs = []
    for lo, hi, emits in rc.ag_pieces(c):
        piece = c.x[:, lo:hi]
        exp = ref.push(piece) if hi > lo else np.zeros((c.rows, 0, c.width), np.int16)
        got = call(ag, piece, _odd(hi - lo))
        assert got.shape == exp.shape and exp.shape[1] == emits * c.cfg.block and np.array_equal(got, exp), (c.name, lo, hi)
        assert ag.counts() == (ref.N, ar.outputs(ref.N, ref.P)), (c.name, lo, hi)
        assert all(ag.gain(r) == ref.gain(r) for r in range(c.rows)), (c.name, lo, hi)
        outs.append(got)
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("P", rc.AG_P)
def test_every_cell_over_its_segments(fmd, P, width):
    """One call of 2 sb + 2 blocks (three segments, the last one short), and a stream whose calls emit sb - 1, sb, sb + 1 and 1."""
    for c in rc.ag_cells(P, width):
        _feed(fmd, c)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("P", [32, 512])
def test_every_carried_history_length(fmd, P, width):
    cases = rc.ag_history(P, width)
    ag = _agc(fmd, cases[0])
    for c in cases:
        ag.reset()
        _feed(fmd, c, ag)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("P", [16, 64])
def test_alignment_matrix(fmd, P, width):
    """Every input row offset against every output row offset within 16 bytes, for calls of 3 blocks: the first from an empty
    history, the second with P + 3 carried samples; nothing outside the outputs is written."""
    c = rc.ag_align(P, width)
    ref = ar.Agc(c.cfg)
    cut = c.cuts[0]
    first, second = ref.push(c.x[:, :cut]), ref.push(c.x[:, cut:])
    assert first.shape[1] == second.shape[1] == 3 * P
    ag = _agc(fmd, c)
    offs = range(8 // width)
    for oi in offs:
        for oo in offs:
            ag.reset()
            assert np.array_equal(call_at(ag, c.x[:, :cut], oi, oo), first), (oi, oo)
            assert np.array_equal(call_at(ag, c.x[:, cut:], oi, oo), second), (oi, oo)
            assert ag.counts() == (ref.N, 6 * P) and all(ag.gain(r) == ref.gain(r) for r in range(c.rows)), (oi, oo)


@pytest.mark.parametrize("P", [32, 2048])
def test_the_configurations_corners(fmd, P):
    for c in rc.ag_corners(P):
        y = _feed(fmd, c)
        assert np.abs(y.astype(np.int64)).max() <= c.cfg.target, c.name
        assert np.abs(ar.agc_all(c.x, c.cfg).astype(np.int64)).max() <= c.cfg.target


def test_40000_rows(fmd):
    c = rc.ag_many_rows()
    rows = rc.sampled_rows(np.random.default_rng(c.seed), c.rows)
    ag, ref = _agc(fmd, c), ar.Agc(c.cfg)
    for lo, hi, emits in rc.ag_pieces(c):
        got = call(ag, c.x[:, lo:hi], _odd(hi - lo))
        exp = ref.push(c.x[rows, lo:hi])
        assert got.shape[1] == emits * 16 and np.array_equal(got[rows], exp), (lo, hi)
        assert ag.counts() == (ref.N, ar.outputs(ref.N, 16)) and all(ag.gain(r) == ref.gain(i) for i, r in enumerate(rows))
