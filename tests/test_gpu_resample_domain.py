"""Rational resampler (include/fmd.h, fmd_resample_*) on the MI355X where tests/test_gpu_resample.py does not reach: odd tap counts
(a last tap pair of one tap and a padding zero) and every parity of the dwords per phase, in the whole-table and the lane-order
form; the ratios at the domain's edges (L around the tile of 256, L = 8 M, M = 32 L with and without skip-ahead, L T = 16384,
1023 / 1024 and back); every shift 0 ... 24 with the rails and negative sums; every input row offset against every output row
offset; every carried history length; calls that end around a tile's last input in lane order; 40000 rows.  Outputs and counts()
against the test-side definition (tests/resample_ref.py), bit for bit, after every call, and each stream once more uncut on a fresh
handle (the history cases share one stream per ratio and width, which runs uncut once).  The cases come from tests/rows_cases.py;
tests/test_rows_cases.py shows without a GPU what each of them reaches.  FMD_FUZZ_SEED reseeds them."""
import numpy as np
import pytest

import resample_ref as rr
import rows_cases as rc
from rows_gpu import TOO_SHORT, call, call_at

pytestmark = pytest.mark.gpu


def _rs(fmd, c):
    return fmd.Resampler(c.g, c.L, c.M, c.shift, n_rows=c.rows, width=c.width, device_id=0)


def _feed(fmd, c, uncut=True):
    """The case's calls against the definition, call by call (odd in_cap on every second call, odd out_cap): outputs and counts();
    the refused calls are the ones the case names, and change nothing.  Then the whole stream in one call on a fresh handle."""
    rs, ref = _rs(fmd, c), rr.Resampler(c.g, c.L, c.M, c.shift)
    outs, refused = [], 0
    for lo, hi, no in rc.rs_pieces(c):
        piece = c.x[:, lo:hi]
        in_cap = piece.shape[1] + (0 if len(outs) % 2 == 0 else 2 + piece.shape[1] % 2)
        if no:
            before = rs.counts()
            with pytest.raises(fmd.FmdError) as e:
                call(rs, piece, in_cap, out_pad=3)
            assert e.value.status == TOO_SHORT and rs.counts() == before, (c.name, lo, hi)
            refused += 1
            continue
        exp = ref.push(piece)
        got = call(rs, piece, in_cap, out_pad=3)
        assert got.shape == exp.shape and np.array_equal(got, exp), (c.name, lo, hi)
        assert rs.counts() == (ref.N, rr.outputs(ref.N, c.L, c.M, c.T)), (c.name, lo, hi)
        outs.append(got)
    assert refused == c.refused and ref.N == c.x.shape[1], c.name
    whole = np.concatenate(outs, axis=1)
    if uncut:
        one = _rs(fmd, c)
        assert np.array_equal(call(one, c.x, c.x.shape[1] + 1, out_pad=3), whole), c.name
        assert one.counts() == rs.counts()
    return whole


@pytest.mark.parametrize("width", [1, 2])
def test_tap_count_sweep(fmd, width):
    """T in {1, 2, 3, 5, 7, 31, 33, 63, 65, 127, 255, 256} at 3 / 4 (the whole table in LDS) and T <= 63 at 257 / 256 (lane order)."""
    for c in rc.rs_t_sweep(width):
        _feed(fmd, c)


@pytest.mark.parametrize("width", [1, 2])
def test_ratio_edges(fmd, width):
    for c in rc.rs_ratio_edges(width):
        _feed(fmd, c)


def test_every_shift(fmd):
    for c in rc.rs_shifts():
        y = _feed(fmd, c)
        assert (y < 0).any() and (not c.claim.rails or ((y == 32767).any() and (y == -32768).any()))


@pytest.mark.parametrize("width", [1, 2])
def test_alignment_matrix(fmd, width):
    """Every input row offset against every output row offset within 16 bytes, as a first call and as a second call that carries
    history; nothing outside the outputs is written."""
    c = rc.rs_align(width)
    ref = rr.Resampler(c.g, c.L, c.M, c.shift)
    cut = c.cuts[0]
    first, second = ref.push(c.x[:, :cut]), ref.push(c.x[:, cut:])
    rs = _rs(fmd, c)
    offs = range(8 // width)
    for oi in offs:
        for oo in offs:
            rs.reset()
            assert np.array_equal(call_at(rs, c.x[:, :cut], oi, oo), first), (oi, oo)
            assert np.array_equal(call_at(rs, c.x[:, cut:], oi, oo), second), (oi, oo)
            assert rs.counts() == (ref.N, first.shape[1] + second.shape[1])


def test_every_history_length(fmd):
    """The cases of a ratio and width are one stream with different first calls: the uncut call runs with the last of them."""
    for c in rc.rs_history():
        _feed(fmd, c, uncut=c.claim.first == 20)


@pytest.mark.parametrize("width", [1, 2])
def test_calls_around_a_tiles_last_input_in_lane_order(fmd, width):
    for c in rc.rs_tile_edges(width):
        _feed(fmd, c)


def test_40000_rows(fmd):
    c = rc.rs_many_rows()
    rows = rc.sampled_rows(np.random.default_rng(c.seed), c.rows)
    rs, ref = _rs(fmd, c), rr.Resampler(c.g, c.L, c.M, c.shift)
    for lo, hi, no in rc.rs_pieces(c):
        assert not no
        got = call(rs, c.x[:, lo:hi], out_pad=3)
        assert np.array_equal(got[rows], ref.push(c.x[rows, lo:hi])), (lo, hi)
        assert rs.counts() == (ref.N, rr.outputs(ref.N, c.L, c.M, c.T))
