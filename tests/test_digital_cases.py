"""What the case tables of tests/digital_cases.py reach, shown without a GPU from the test-side definitions alone: for the frame bank
the counters of every line, every delivered length, the lanes that close together at and below their cap, the call edges that tell
a dropped state field, the clock's range on either side of its switch and the rows; for the pager front end and the code squelch the
residues, offsets, trigger outcomes and hit counts their cases claim."""
import numpy as np
import pytest

import ax25_ref as xr
import dcs_ref as dr
import digital_cases as dg


# ---- the frame bank ------------------------------------------------------------------------------------------------------------------
def _totals(snaps, r):
    return [f for s in snaps for f in s.last[2][r]]


@pytest.mark.parametrize("clock", sorted(dg.HD_CLOCKS))
def test_hd_lines_every_line_keeps_its_counters_in_either_polarity(clock):
    c = dg.hd_lines(clock)
    assert c.rows >= 70 and set(c.claim.where) == set(dg.CASES) >= set(dg.WANT) and len(dg.WANT) == 20
    snaps = dg.hd_reference(c, 1)
    assert len(snaps) == 5 and snaps[-1].pos == c.x.shape[1]
    info = snaps[-1].info
    for name, rows in c.claim.where.items():
        for r in rows:
            assert name not in dg.WANT or (info[r]["frames_ok"], info[r]["bad_fcs"], info[r]["aborts"]) == dg.WANT[name], (name, r, info[r])
        assert _totals(snaps, rows[0]) == _totals(snaps, rows[1])
    both = [r for rows in c.claim.where.values() for r in rows]
    assert min(both) < 64 <= max(both)                       # lines in both waves
    others = sorted(set(range(c.rows)) - set(both))
    assert sum(info[r]["bad_fcs"] + info[r]["aborts"] for r in others) > 10 and not any(info[r]["frames_ok"] for r in others)
    r = c.claim.where["ff-514"][0]
    assert [f["data"] for f in _totals(snaps, r)] == [b"\xff" * 512]
    one = dg.merged(snaps, c.cap)                            # the one call the cuts add up to
    assert one.last[0].tolist() == [len(_totals(snaps, r)) for r in range(c.rows)] and one.last[0].sum() >= 30


def test_hd_merged_calls_equal_the_one_call():
    c = dg.hd_close(1, 64)
    c.runs = [[], [3000, 1, 7000]]
    one, cut = dg.hd_reference(c, 0), dg.hd_reference(c, 1)
    m = dg.merged(cut, c.cap)
    assert len(one) == 1 and len(cut) == 4 and m.info == one[0].info and m.pos == one[0].pos
    assert m.last[2] == one[0].last[2] and np.array_equal(m.last[0], one[0].last[0]) and m.last[1].tobytes() == one[0].last[1].tobytes()


def test_hd_lengths_all_498_are_delivered_and_the_two_outside_are_not():
    seen = []
    for g in range(len(dg.HD_LENGTH_GROUPS)):
        c = dg.hd_lengths(g)
        for run in (0, 1):
            snaps = dg.hd_reference(c, run)
            for r, d in enumerate(c.claim.bodies):
                assert [f["data"] for f in _totals(snaps, r)] == [d], (g, r)
            last = snaps[-1].info[c.rows - 1]
            assert (last["frames_ok"], last["bad_fcs"]) == (0, len(c.claim.outside)) and not _totals(snaps, c.rows - 1)
        one = dg.hd_reference(c, 0)[0].last[1]
        for r, d in enumerate(c.claim.bodies):               # the record: len, the body, zeros behind it
            assert one[r, 0]["len"] == len(d) and bytes(one[r, 0]["data"][:len(d)]) == d and not one[r, 0]["data"][len(d):].any()
        seen += [len(d) for d in c.claim.bodies]
        assert [len(d) for d in c.claim.outside] == ([14, 513] if g == 7 else [14])
    assert seen == list(range(15, 513)) and len(seen) == 498
    assert {n % 8 for n in seen} == set(range(8)) and {(n - 1) // 8 for n in seen} == set(range(1, 64))      # the copy's last lane with data


@pytest.mark.parametrize("cap,rows", dg.HD_CLOSE)
def test_hd_close_the_last_frames_close_on_one_sample_at_and_below_the_cap(cap, rows):
    c = dg.hd_close(cap, rows)
    snap = dg.hd_reference(c, 0)[0]
    counts, rec, every = snap.last
    ends = {e[-1]["end_sample"] for e in every}
    assert len(ends) == 1 and all(len(e) == k + 1 for e, k in zip(every, c.claim.prior))
    assert all(e[-1]["data"] == b[-1] for e, b in zip(every, c.claim.bodies))
    for n in dg.HD_CLOSE_LENS:                               # every length both delivered and only counted
        ks = {k for k, b in zip(c.claim.prior, c.claim.bodies) if len(b[-1]) == n}
        assert min(ks) < cap <= max(ks), (n, ks)
    assert rows >= 64 and (rows == 64 or cap > 1)


FIELDS = sorted(dg.Model.FIELDS)


def _model_row(c, r, cut, field=None):
    """row r of the case through the Model in the calls cut | rest, `field` lost at the cut: (frames, info, whether it held a value)"""
    m = dg.Model(c.num, c.den, c.baud)
    frames = m.push(c.x[r, :cut])
    held = m.drop(field) if field else False
    frames += m.push(c.x[r, cut:])
    return frames, m.info(), held


def test_hd_edges_between_them_tell_every_dropped_field():
    told = {e: _told(*e) for e in dg.HD_EDGES}
    assert set().union(*told.values()) == set(FIELDS)
    assert told[(15, 6000)] == set(FIELDS) - {"ones", "prev"} and told[(40, 6000)] == set(FIELDS) - {"prev"} and "prev" in told[(15, 4800)]


def _told(nbytes, rate):
    """the state fields whose loss at the call edge changes some row's frames or counters"""
    c = dg.hd_edges(nbytes, rate)
    L = c.claim.L
    assert c.rows == L and c.runs == [[L, 1]] and 600 <= L <= 1800
    snaps = dg.hd_reference(c, 0)
    assert len(snaps) == 3 and all([f["data"] for f in _totals(snaps, r)] == [c.claim.data] for r in range(L))
    # row r's call edge lies L - r samples into the line: every sample of the line, so every phase and every bit of the frame
    assert sorted(L - r for r in range(L)) == list(range(1, L + 1))
    assert (len(xr.stuffed_bits(xr.with_fcs(c.claim.data))) == 8 * (nbytes + 2)) == (nbytes == 15)     # the longer one has a stuffed bit
    told = {}
    for field in FIELDS:
        for r in list(range(7, L, 41)) + list(range(min(L, 200))):     # a few rows across the frame first, then the edges in the last 200 samples
            want = (_totals(snaps, r), snaps[-1].info[r])
            assert _model_row(c, r, L)[:2] == want
            frames, info, held = _model_row(c, r, L, field)
            if (frames, info) != want:
                assert held
                told[field] = r
                break
    return set(told)


def test_hd_long_edges_cross_a_call_beyond_4096_bits():
    c = dg.hd_long_edges()
    snaps = dg.hd_reference(c, 0)
    assert all([f["data"] for f in _totals(snaps, r)] == [c.claim.data] for r in range(c.rows))
    nbits, in_flag = [], 0
    for r in range(c.rows):
        m = dg.Model(c.num)
        m.push(c.x[r, :c.claim.c])
        assert m.in_frame == 1
        nbits.append(m.nbits)
        in_flag += m.nbits > 514 * 8
    assert sum(n > 4096 for n in nbits) >= 6 and in_flag >= 2 and len({n >> 3 for n in nbits if n > 4096}) >= 3, nbits
    for field in ("nbits", "crc", "hist"):
        assert any(_model_row(c, r, c.claim.c, field)[0] != _totals(snaps, r) for r in range(c.rows)), field


@pytest.mark.parametrize("mod,k", dg.HD_SWITCH)
def test_hd_switch_the_clock_on_either_side(mod, k):
    """At the switch itself ph + step stays below 2^32 on either side (ph < mod and step <= mod / 4), so what the cases tell apart
    is the choice of the path and each path's arithmetic next to it: on the framed rows the sum needs 32 bits on either side, which a
    signed 32-bit compare would get wrong.  The top of the domain, where the sum passes 2^32, is
    the `wide` clock of the lines."""
    c = dg.hd_switch(mod, k)
    assert (c.mod, c.step) == (mod, mod // 4 if k == 4 else -(-mod // 64)) and 4 * c.step <= c.mod <= 64 * c.step
    assert k == 64 or 4 * (c.step + 1) > c.mod
    assert k == 4 or 64 * (c.step - 1) < c.mod
    for run in (0, 1):
        snaps = dg.hd_reference(c, run)
        for r in (0, 1):
            assert [f["data"] for f in _totals(snaps, r)] == c.claim.bodies
        assert snaps[-1].info[2]["frames_ok"] == 0
    peaks = [dg.clock_peak(c.x[r], c.mod, c.step) for r in range(3)]
    assert all(p < 1 << 32 for p in peaks) and all(p >= 1 << 31 for p in peaks[:2]), peaks


def test_hd_wide_clock_passes_2_to_the_32():
    c = dg.hd_lines("wide")
    r = c.claim.where["bytes-17"][0]
    assert dg.clock_peak(c.x[r, :4000], c.mod, c.step) >= 1 << 32 and c.mod >= 1 << 31
    for name in ("6000", "11025-2"):
        assert dg.HD_CLOCKS[name][0] < 1 << 31


@pytest.mark.parametrize("rows", dg.HD_ROWS + (dg.HD_MANY,))
def test_hd_rows_every_sampled_row_delivers_its_frame(rows):
    c = dg.hd_rows(rows)
    assert c.x.shape[0] == rows and 900 <= c.x.shape[1] <= 1200 and len(c.sample) == (16 if rows > 1000 else rows)
    snaps = dg.hd_reference(c, 0, c.sample)
    assert len(snaps) == 2
    for i, r in enumerate(c.sample):
        assert [f["data"] for f in _totals(snaps, i)] == [c.line_bodies[c.which[r]]]
    if rows > 1000:
        assert {0, 32767, 32768, rows - 1} <= set(c.sample) and len({tuple(c.x[r]) for r in c.sample}) == 16


# ---- the code squelch ----------------------------------------------------------------------------------------------------------------

def _opens(c, run=0):
    """the definition over the run: some block hit, some did not have to, and the output is not all zero"""
    calls, ref = dg.dc_reference(c, run)
    assert any(h[2] != dr.NONE for h in ref.hits), c.name
    assert any(exp.any() for _, _, exp, _, _ in calls), c.name
    return calls, ref


@pytest.mark.parametrize("B", dg.DC_BOXES)
def test_dc_boxes_reach_both_outcomes_of_the_search_trigger(B):
    full_by_P = {}
    for P in dg.DC_BOX_BLOCKS:
        seen = []
        for width in (1, 2):
            c = dg.dc_boxes(B, P, width)
            assert (c.cfg.block, c.cfg.box, c.rows) == (P, B, 3)
            pieces = dg.dc_pieces(c, c.runs[0])
            assert sorted({lo % 64 for lo, _ in pieces[:64]}) == list(range(64)) and len(pieces) == 65
            seen = [s for lo, hi in pieces for s in dg.dc_searches(P, B, lo, hi - lo)]
            _opens(c)
        # the trigger where neither a block's nor the call's end asks for the search anyway
        full_by_P[P] = {full for np_, NB, block_end, call_end, full in seen if not block_end and not call_end}
        waits = {np_ for np_, NB, block_end, call_end, full in seen if block_end or call_end or full}
        assert any(w % 2 for w in waits) and all(NB == 64 // B for _, NB, _, _, _ in seen), (P, sorted(waits))
        assert max(waits) <= 64
    # at P = 64 and 192 a block ends before 64 boxes wait unless B = 2 and P = 192; the block of 65 chunks reaches it at every B
    assert full_by_P[4160] == {True, False}
    assert full_by_P[64] <= {False} and full_by_P[192] == ({True, False} if B == 2 else {False})


def test_dc_ring_sizes_and_the_box_index_wrap():
    sizes = {}
    for last in dg.DC_RING_TAPS:
        for width in (1, 2):
            c = dg.dc_ring(last, width)
            assert c.cfg.tap[22] == last and len(c.cfg.lp) == 64 and c.cfg.box == 1 and c.x.shape[1] > 1100
            assert [lo for lo, _ in dg.dc_pieces(c, c.runs[0])] == [0, 1023, 1024, 1025]
            _opens(c, 0)
            whole, _ = _opens(c, 1)
            assert np.array_equal(np.concatenate([e for _, _, e, _, _ in dg.dc_reference(c, 0)[0]], axis=1), whole[0][2])
        sizes[last] = c.claim.sring
        assert c.claim.sring >= last + 64 and (c.claim.sring == 128 or c.claim.sring // 2 < last + 64)
    assert [sizes[t] for t in dg.DC_RING_TAPS] == [128, 128, 256, 256, 256, 512, 512, 512, 1024, 1024]


def test_dc_every_T():
    for T in range(1, 65):
        for width in (1, 2):
            c = dg.dc_taps_T(T, width)
            assert len(c.cfg.lp) == T and c.width == width and c.cfg.box == 8
            _opens(c)


@pytest.mark.parametrize("pair", dg.DC_TIES)
def test_dc_ties_the_first_index_wins(pair):
    assert pair[0] < pair[1] and {p % 16 for p in dg.DC_TIES[0]} == {3} and [p % 16 for p in dg.DC_TIES[1]] == [15, 0]
    for swapped in (False, True):
        for min_hits, code in ((32, pair[0]), (33, dr.NONE)):
            c = dg.dc_tie(pair, swapped, min_hits, 1)
            calls, ref = dg.dc_reference(c, 0)
            assert [h[2:] for h in ref.hits] == [(code, pair[0], 32)] * 2
            assert ref.status() == ([code], [32], [code != dr.NONE]) and calls[-1][2].any() == (code != dr.NONE)


def test_dc_in_place_offsets_and_calls_inside_a_chunk():
    for off in (1, 3, 7):
        for width in (1, 2):
            c = dg.dc_in_place(off, width)
            r = c.runs[0]
            assert (r.mode, r.off_in, r.in_place, c.rows) == ("at", off, True, 35)
            assert [lo % 64 != 0 and lo % c.cfg.box != 0 for lo, _ in dg.dc_pieces(c, r)[1:]] == [True] * 3
            _opens(c)


def test_dc_confirm_cap_expectation_is_the_definitions():
    c, exp, status = dg.dc_confirm_cap()
    assert c.claim.opens == 254 and c.claim.state == (1, 1, 65535, 0) and dg.DC_CAP_BLOCKS > 65536
    assert not exp[0, :255 * 64].any() and (exp[0, 255 * 64:, 0] == 1234).all()
    ref = dr.CodeSquelch(c.words, c.cfg)
    n = 300 * 64
    assert np.array_equal(ref.push(c.x[:, :n]), exp[:, :n])
    assert [h[2:] for h in ref.hits] == [(1, 1, 42)] + [(1, 1, 64)] * 299 and ref.status() == status


# ---- the pager front end -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", range(1, 17))
def test_fk_every_shape_hits_cut_and_uncut(W):
    for D in range(1, 65):
        c = dg.fk_every_shape(D, W)
        assert (c.cfg.D, c.cfg.W, int(c.cfg.tap[31]), c.rows) == (D, W, 255, 3) and 0 <= c.claim.r < D
        assert c.x.shape[1] == 389 * D + c.claim.r and c.runs[0].cuts == [258 * D + c.claim.r]
        cut, one = dg.fk_reference(c, 0), dg.fk_reference(c, 1)
        assert len(cut) == 2 and cut[1][2].shape[1] > 64 and cut[1][5] == one[0][5] == (c.x.shape[1], 389)
        assert np.array_equal(np.concatenate([cut[0][2], cut[1][2]], axis=1), one[0][2])
        assert one[0][3].sum() >= 3 and cut[0][3].sum() + cut[1][3].sum() == one[0][3].sum(), c.name


@pytest.mark.parametrize("D,W,last", dg.FK_CARRY)
def test_fk_carries_reach_every_residue_and_offset(D, W, last):
    c = dg.fk_carries(D, W, last)
    pieces = dg.fk_pieces(c, c.runs[0])
    assert len(pieces) == 25 == len(c.runs[0].offs)
    first = [lo // D for lo, _ in pieces]
    assert {k % 16 for k in first} == set(range(16))                                        # the b carry's index
    assert {lo % D for lo, _ in pieces} >= set(range(min(D, 8)))                           # pos_r: the open box's samples
    for m in (128, 256, 512):                                # a call whose boxes cross a multiple of each ring size
        assert any(lo // D < m <= (hi - 1) // D for lo, hi in pieces), m
    assert {o[0] for o in c.runs[0].offs} == set(range(8)) and {o[1] for o in c.runs[0].offs} == {0, 3, 5}
    assert len(set(c.runs[0].offs[:24])) == 24
    assert sum(int(p[3].sum()) for p in dg.fk_reference(c, 0)) >= 3


@pytest.mark.parametrize("D", [1, 3])
def test_fk_line_hits_on_both_sides_of_box_65536_and_across_it(D):
    c = dg.fk_line(D)
    L, t31 = dg.FK_LINE, int(c.cfg.tap[31])
    pieces = dg.fk_pieces(c, c.runs[0])
    assert [(lo // D, hi // D) for lo, hi in pieces] == [(0, L - 100), (L - 100, L + 100), (L + 100, L + 330)] and t31 == 155
    for run in (0, 1):
        hits = dg.fk_hits(c, run)
        for r in (0, 1):
            ks = [k for row, k, d, C, thr in hits if row == r]
            assert all(any(abs(k - at) <= 1 for k in ks) for at in c.claim.ats), (r, ks)
            assert any(k < L for k in ks) and any(k - t31 < L <= k for k in ks) and any(k - t31 >= L for k in ks)
        assert all((d >> 31) == row for row, k, d, C, thr in hits)
    assert sorted(dg.fk_hits(c, 0)) == sorted(dg.fk_hits(c, 1))


def test_fk_equalities_each_tell_the_exchanged_comparison():
    told = set()
    for c, variant, hits in dg.fk_equalities():
        got = [h for h in dg.fk_hits(c, 0) if h[1] == 31]
        plain = [h for h in dg.fk_rule(c.x[0], c.cfg) if h[0] == 31]
        assert [h[1:] for h in got] == plain and bool(got) == hits, c.name
        if variant:
            assert [h for h in dg.fk_rule(c.x[0], c.cfg, variant) if h[0] == 31] != plain, c.name
            told.add(variant)
    assert told == {"bit", "tol", "inv", "corr"}
    names = [c.name for c, _, _ in dg.fk_equalities()]
    assert len(set(names)) == len(names) == 17
    for sync, inverted in ((0, 0), (0xFFFFFFFF, 1)):
        c = dg.fk_top(sync)
        for run in (0, 1):
            hits = dg.fk_hits(c, run)
            assert [h[1] for h in hits] == list(range(34, 80)) and len(hits) == 46
            assert all(h[2] == (32 if inverted else 0) | inverted << 31 and h[3] == (-1 if inverted else 1) << 20 for h in hits)
        assert dg.fk_rule(c.x[0], c.cfg, "corr") == [] and c.cfg.min_corr == 1 << 20


@pytest.mark.parametrize("D,W,shift", dg.FK_SHIFTS)
def test_fk_shifts_reach_both_rails(D, W, shift):
    c = dg.fk_shift(D, W, shift)
    assert c.cfg.shift == shift <= 10 and D * W <= 1 << shift
    calls = dg.fk_reference(c, 0)
    out = np.concatenate([p[2] for p in calls], axis=1)
    if D * W == 1 << shift:
        assert out.min() == -32768 and out.max() == 32767 and (out == -1).any()          # (a stretch of -1 comes out as -1)
    else:
        assert out.min() == (-32768 * D * W) >> shift and out.max() == (32767 * D * W) >> shift
    assert calls[1][0] % D != 0 or D == 1                    # the second call begins inside a box


@pytest.mark.parametrize("hit_cap", dg.FK_CAPS)
def test_fk_records_lanes_caps_and_k_rel(hit_cap):
    c = dg.fk_records(hit_cap)
    (lo, hi, out, counts, rec, _), = dg.fk_reference(c, 0)
    assert counts.tolist() == [200 - 31, 2, 0] and rec[1, :min(2, hit_cap)]["k_rel"].tolist() == [63, 64][:hit_cap]
    # row 0 hits at every k from 31 on: all 64 lanes of chunk 1 and 2, and its count passes hit_cap inside a chunk
    assert rec[0, :hit_cap]["k_rel"].tolist() == list(range(31, 31 + hit_cap)) and (31 + hit_cap) % 64 != 0 and out.shape[1] == 200
    a, b = dg.fk_reference(c, 1)
    assert b[0] == 122 and b[0] % 3 == 2 and a[3].tolist() == [40 - 31, 0, 0] and b[3].tolist() == [160, 2, 0]
    assert b[4][1, :min(2, hit_cap)]["k_rel"].tolist() == [23, 24][:hit_cap] and b[4][0, 0]["k_rel"] == 0


@pytest.mark.parametrize("rows", dg.FK_ROWS + (dg.FK_MANY,))
def test_fk_rows(rows):
    c = dg.fk_rows(rows)
    assert c.x.shape == (rows, 801) and len(c.sample) == min(rows, 16)
    calls = dg.fk_reference(c, 0, c.sample)
    assert sum(int(p[3].sum()) for p in calls) >= len(c.sample) and len(calls) == 2
