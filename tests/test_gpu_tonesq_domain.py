"""Tone squelch (include/fmd.h, fmd_tonesq_*) on the MI355X where tests/test_gpu_tonesq.py does not reach: every F = 1 ... 64 (some
wave's number of tone-row groups changes behind every multiple of 4) with every tone winning in turn on a row of its own; P in
{128, 512, 1024, 2048, 8192} with F = 3 and 32, the corner F P = 262144 included; every ramp 1 ... P at P = 256; 31, 32, 33, 64 and 65
rows around the tile of 32; every input row offset against every output row offset, out of place and in place, for a call that
starts and ends inside a chunk; the decision's interior (a runner-up exactly guard and guard + 1 tones away, W >> dom_shift one
below, at and one above `rest`, ties); 40000 rows.  Outputs, counts() and status() against the test-side definition
(tests/tonesq_ref.py), bit for bit, after every call.  The cases come from tests/rows_cases.py; tests/test_rows_cases.py shows
without a GPU what each of them reaches.  FMD_FUZZ_SEED reseeds them."""
import numpy as np
import pytest

import rows_cases as rc
from rows_gpu import call, call_at
import tonesq_ref as tr

pytestmark = pytest.mark.gpu


def _sq(fmd, c):
    cfg = c.cfg
    return fmd.ToneSquelch(c.tab, n_rows=c.rows, width=c.width, accept=cfg.accept, guard=cfg.guard, dom_shift=cfg.dom_shift,
                           min_power=cfg.min_power, confirm=cfg.confirm, hang=cfg.hang, ramp=cfg.ramp, device_id=0)


def _odd(n):
    return n + 1 + n % 2


def _status_equal(sq, ref, rows=None):
    tone, power, gate = sq.status()
    rt, rp, rg = ref.status()
    pick = range(len(rt)) if rows is None else rows
    return [int(tone[r]) for r in pick] == rt and [int(power[r]) for r in pick] == rp and [bool(gate[r]) for r in pick] == rg


def _feed(fmd, c):
    """The case's calls against the definition, call by call (odd in_cap, odd out_cap): the outputs, counts() and every row's status.
    Returns the outputs and the reference."""
    sq, ref = _sq(fmd, c), tr.ToneSquelch(c.tab, c.cfg)
    outs, lo = [], 0
    for n in c.cuts + [c.x.shape[1]]:
        hi = min(c.x.shape[1], lo + n)
        exp = ref.push(c.x[:, lo:hi])
        got = call(sq, c.x[:, lo:hi], _odd(hi - lo))
        assert got.shape == exp.shape and np.array_equal(got, exp), (c.name, lo, hi)
        assert sq.counts() == (ref.N, ref.N) and _status_equal(sq, ref), (c.name, lo, hi)
        outs.append(got)
        lo = hi
    return np.concatenate(outs, axis=1), ref


@pytest.mark.parametrize("lo", [1, 17, 33, 49])
def test_every_tone_count_and_every_tone_wins(fmd, lo):
    """F = lo ... lo + 15 at P = 64, the widths in turn, F + 1 rows: row f carries tone f of the table, the last row nothing."""
    for F in range(lo, lo + 16):
        c = rc.tq_each_tone(F)
        _, ref = _feed(fmd, c)
        assert all(hit == (row if row < F else tr.NONE) for _, row, hit in ref.hits)


@pytest.mark.parametrize("P,F", rc.TQ_PS)
def test_block_sweep(fmd, P, F):
    _feed(fmd, rc.tq_p_sweep(P, F))


def test_every_ramp(fmd):
    for c in rc.tq_ramps():
        y, _ = _feed(fmd, c)
        assert y[0, 2 * 256:3 * 256].all() and not y[:, 4 * 256:].any()


@pytest.mark.parametrize("rows", [31, 32, 33, 64, 65])
def test_rows_around_the_tile(fmd, rows):
    _feed(fmd, rc.tq_rows(rows))


@pytest.mark.parametrize("width", [1, 2])
def test_alignment_matrix(fmd, width):
    """A call that starts 21 samples into a chunk and ends 57 samples into a later one, at every input row offset against every
    output row offset within 16 bytes, and in place at every offset; the calls before and behind it are plain.  Nothing outside the
    outputs is written, and the block the call leaves open completes with the right power."""
    c = rc.tq_align(width)
    a, b = c.cuts[0], c.cuts[0] + c.cuts[1]
    ref = tr.ToneSquelch(c.tab, c.cfg)
    exp = [ref.push(c.x[:, :a]), ref.push(c.x[:, a:b]), ref.push(c.x[:, b:])]
    sq = _sq(fmd, c)
    offs = list(range(8 // width))
    for oi, oo in [(i, o) for i in offs for o in offs] + [(i, None) for i in offs]:
        sq.reset()
        assert np.array_equal(call(sq, c.x[:, :a], _odd(a)), exp[0])
        got = call_at(sq, c.x[:, a:b], oi, oo or 0, in_place=oo is None)
        assert np.array_equal(got, exp[1]), (oi, oo)
        assert np.array_equal(call(sq, c.x[:, b:]), exp[2]), (oi, oo)
        assert sq.counts() == (ref.N, ref.N) and _status_equal(sq, ref), (oi, oo)


@pytest.mark.parametrize("guard,dom", rc.TQ_INTERIOR)
def test_decision_interior(fmd, guard, dom):
    c = rc.tq_interior(guard, dom)
    _, ref = _feed(fmd, c)
    for e, (_, row, hit) in zip(c.claim.expect, ref.hits):
        assert hit == e.hit, row


def test_40000_rows(fmd):
    c = rc.tq_many_rows()
    rows = rc.sampled_rows(np.random.default_rng(c.seed), c.rows)
    sq, ref = _sq(fmd, c), tr.ToneSquelch(c.tab, c.cfg)
    lo = 0
    for n in c.cuts + [c.x.shape[1]]:
        hi = min(c.x.shape[1], lo + n)
        got = call(sq, c.x[:, lo:hi], _odd(hi - lo))
        assert np.array_equal(got[rows], ref.push(c.x[rows, lo:hi])), (lo, hi)
        assert sq.counts() == (ref.N, ref.N) and _status_equal(sq, ref, rows), (lo, hi)
        lo = hi
