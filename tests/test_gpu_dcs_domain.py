"""Code squelch (include/fmd.h, fmd_dcs_*) over its domain on the MI355X: the case tables of tests/digital_cases.py through the handle,
every output, the counters and every row's status bit for bit against the test-side definition (tests/dcs_ref.py) after every call.
tests/test_digital_cases.py shows without a GPU what each case reaches: B in {2, 4, 16, 32} with calls from every offset of a chunk and
both outcomes of the search trigger, tap[22] on either side of every size of the soft ring with the box index passing 1024, every T, ties
of the block-end argmax inside a lane and across lanes, in-place calls on unaligned rows, and the confirm counter at its cap."""
import numpy as np
import pytest

import dcs_ref as dr
import digital_cases as dg
from rows_gpu import call, call_at
from test_gpu_dcs import _odd, _sq

pytestmark = pytest.mark.gpu


def _run(fmd, c, run):
    """run `run` of the case on a fresh handle, call by call against the definition; the handle"""
    calls, ref = dg.dc_reference(c, run)
    r = c.runs[run]
    sq = _sq(fmd, c.words, c.cfg, c.rows, c.width)
    for lo, hi, exp, N, status in calls:
        piece = np.ascontiguousarray(c.x[:, lo:hi])
        got = call(sq, piece, _odd(hi - lo)) if r.mode == "call" else call_at(sq, piece, r.off_in, r.off_out, in_place=r.in_place)
        assert got.shape == exp.shape and np.array_equal(got, exp), (c.name, lo, hi, [q for q in range(c.rows) if not np.array_equal(got[q], exp[q])])
        code, hits, gate = sq.status()
        assert sq.counts() == (N, N) and (code.tolist(), [int(h) for h in hits], gate.tolist()) == status, (c.name, lo, hi)
    return sq


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("P", dg.DC_BOX_BLOCKS)
@pytest.mark.parametrize("B", dg.DC_BOXES)
def test_boxes_of_2_4_16_32_from_every_offset_of_a_chunk(fmd, B, P, width):
    _run(fmd, dg.dc_boxes(B, P, width), 0)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("last", dg.DC_RING_TAPS)
def test_the_soft_ring_on_either_side_of_its_sizes_and_the_box_index_past_1024(fmd, last, width):
    c = dg.dc_ring(last, width)
    _run(fmd, c, 0)
    _run(fmd, c, 1)


@pytest.mark.parametrize("width", [1, 2])
def test_every_T(fmd, width):
    for T in range(1, 65):
        _run(fmd, dg.dc_taps_T(T, width), 0)


@pytest.mark.parametrize("pair", dg.DC_TIES, ids=["%d-%d" % p for p in dg.DC_TIES])
def test_ties_of_the_argmax_inside_a_lane_and_across_lanes(fmd, pair):
    for width in (1, 2):
        for swapped in (False, True):
            for min_hits, code in ((32, pair[0]), (33, dr.NONE)):
                sq = _run(fmd, dg.dc_tie(pair, swapped, min_hits, width), 0)
                assert sq.status()[0].tolist() == [code] and sq.status()[1].tolist() == [32]


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("off", [1, 3, 7])
def test_in_place_on_unaligned_rows(fmd, off, width):
    _run(fmd, dg.dc_in_place(off, width), 0)


def test_the_confirm_counter_stays_at_its_cap(fmd):
    c, exp, status = dg.dc_confirm_cap()
    sq = _sq(fmd, c.words, c.cfg, 1, 1)
    got = call(sq, c.x)
    assert np.array_equal(got, exp) and got[0, -1, 0] == 1234
    code, hits, gate = sq.status()
    assert (code.tolist(), [int(h) for h in hits], gate.tolist()) == status and sq.counts() == (c.x.shape[1],) * 2
