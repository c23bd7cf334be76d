"""The case generators of the *_domain GPU tests (tests/domain_cases.py) against the references alone, without a GPU: every case
reaches what it claims.  The first-pass tile is 64 G outputs (64 G - 1 in the stereo bank), G the largest of 4, 3, 2, 1 with
raw + 2048 + 256 K G <= 40960 bytes of LDS, raw = max(12 + 6 D + 8 D (16 G - 1) + 64 nkc, 12 + 2 D (64 G - 1) + 2 T + 15) rounded
up to 16 and nkc = ceil((12 + 2 T) / 64) (st_lds, nb_lds, ch_lds): dc.groups is the test-side copy.

For the RDS bank the file also shows, still without a GPU, that the cases can tell a wrong kernel from a right one: each of five
deliberately wrong variants of the definition (small subclasses of rds_ref.RdsRef below) gives, on the family of cases built for
it, a result that differs from the definition's."""
import numpy as np
import pytest

import domain_cases as dc
import narrow_ref as nr
import rds_ref as rr
import stereo_ref as st


def test_groups_formula_examples():
    for T in (1, 64, 256):
        assert [dc.groups(10, T, K) for K in (1, 8, 32)] == [4, 4, 4]
        assert dc.groups(30, T, 24) == 3 and dc.groups(64, T, 8) == 3
        assert dc.groups(64, T, 24) == 2 and dc.groups(64, T, 32) == 2
    assert all(dc.groups(D, T, K) >= 2 for D in range(2, 65, 2) for T in (1, 256) for K in (1, 32))


def _edges_both_forms(cases):
    seen = set()
    for c in cases:
        assert dc.digits_of(c.h, c.incs) == c.digits, c.i
        assert dc.groups(c.D, c.T, c.K) == c.G
        seen.add((c.K, c.digits))
    assert seen >= set(dc.K_EDGES), set(dc.K_EDGES) - seen
    assert {c.G for c in cases} >= {2, 3, 4}
    assert {c.D for c in cases} >= set(dc.DECIMS)


def test_stereo_sweep_covers_the_shapes():
    cases = list(dc.stereo_sweep())
    assert len(cases) >= 16
    assert {c.R for c in cases} == set(range(1, 33))
    _edges_both_forms(cases)
    assert {c.Ta for c in cases} >= set(dc.ST_TA) and {c.P for c in cases} == set(dc.ST_BLOCKS)
    assert {c.pilot_min for c in cases} >= {0, 1, 16384} and any(1 < c.pilot_min < 16384 for c in cases)
    assert {c.audio_shift for c in cases} >= {0, 16} or len({c.audio_shift for c in cases}) >= 10
    assert any(c.na < 256 for c in cases) and any(c.na == 48 for c in cases)
    many_tiles = [c for c in cases if c.na < 256 and c.long_tiles and any(nE - nS > 3 * c.na for _, _, nS, nE in dc.plan(c))]
    assert len(many_tiles) >= 2
    for c in cases:
        p = dc.plan(c)
        assert p and c.na == dc.stereo_na(c.Ta, c.R) and c.R * c.na + 2 * c.Ta <= 2048
        assert max(mE for _, mE, _, _ in p) > c.P, c.i             # a block completes, so an estimate is used
    # tiles of 64 G - 1 at G < 4 run through a block edge in one call
    assert any(c.G < 4 and any(mE - mS > 4 * (64 * c.G - 1) and mS // c.P != (mE - 1) // c.P for mS, mE, _, _ in dc.plan(c)) for c in cases)


@pytest.mark.parametrize("P", [1024, 4096])
def test_stereo_block_edges(P):
    c = dc.stereo_edges(P)
    p = dc.plan(c)
    assert [mE for _, mE, _, _ in p] == c.ends                     # no call is refused
    f = dc.edge_facts([(mS, mE) for mS, mE, _, _ in p], P)
    assert f.rel == {-1, 0, 1} and f.open_calls >= 3 and f.whole >= 4 and f.starts_on_edge
    assert dc.straddles(c) == (True, True)
    refs = dc.stereo_refs(c, st, check=[0])
    present = set()
    for data in dc.calls(c):
        refs[0].feed(data[0])
        present.add(refs[0].pilot(0)[0])
    assert True in present and refs[0].kc_max > 0


@pytest.mark.parametrize("R", [1, 3])
def test_stereo_short_calls(R):
    c = dc.stereo_short(R)
    p = dc.plan(c)
    assert [mE for _, mE, _, _ in p] == c.ends
    assert {mE - mS for mS, mE, _, _ in p} >= {1, 2, c.Ta - 2, c.Ta - 1, c.Ta} and p[-1][1] - p[-1][0] == 3000


def test_stereo_threshold_is_exact_equality():
    c = dc.stereo_threshold()
    assert st.pilot_inc(c.rate, c.D) == 1 << 29
    got = {}
    for pm in (7, 8, 9):
        ref = dc.stereo_refs(c, st, pilot_min=pm)[0]
        outs = [ref.feed(d[0]) for d in dc.calls(c)]
        I, Q = ref.block_iq(0, 0)
        assert (I, Q) == (1 << 26, 0) and I * I + Q * Q == (8 * c.P * 8192) ** 2
        got[pm] = np.concatenate(outs, axis=1)[0, :2 * c.P - c.Ta + 1]     # the audio whose windows lie in blocks 0 and 1
    assert np.array_equal(got[7], got[8]) and not np.array_equal(got[8], got[9])
    assert np.array_equal(got[9][:, 0], got[9][:, 1]) and not np.array_equal(got[8][:, 0], got[8][:, 1])


@pytest.mark.parametrize("limit,sign", [(16384, 1), (256, -1), (256, 0)])
def test_stereo_extremes(limit, sign):
    c = dc.stereo_extreme(limit, sign)
    assert int(np.abs(c.g.astype(np.int64)).sum()) == 16383 and c.audio_shift == 0
    assert dc.y_bound(c.h, c.incs, c.shift) <= limit < dc.y_bound(c.h, c.incs, c.shift - 1)
    ref = dc.stereo_refs(c, st)[0]
    out = np.concatenate([ref.feed(d[0]) for d in dc.calls(c)], axis=1)
    assert ref.kc_max >= 32000 and ref.corr_max > (1 << 23)
    for ch in (0, 1):
        assert out[..., ch].min() == -32768 and out[..., ch].max() == 32767
    assert ref.ms_max < (1 << 31)
    if limit == 16384:
        # |x| <= 16384 + 4096 (the quotient of the discriminator stays within 4096 whether or not its products wrap) and
        # |kc| <= 32768, so |s| = |x kc| >> 14 ends near 32768, not at the kernel's loose bound of 65540
        assert ref.s_max >= 30000 and ref.ms_max > (1 << 27)


def test_narrow_sweep_covers_the_shapes():
    cases = list(dc.narrow_sweep())
    for R in range(1, 33):
        mine = [c for c in cases if c.R == R]
        assert {-(-c.Ta // R) % 4 for c in mine} == {0, 1, 2, 3}, R
        assert any(c.Ta < R or c.Ta == 256 for c in mine) or R == 1
    assert any(c.Ta < c.R for c in cases) and any(c.Ta == 256 for c in cases)
    heavy = [c for c in cases if (c.K, c.digits) in dc.K_EDGES]
    _edges_both_forms(heavy)
    for c in cases:
        assert dc.digits_of(c.h, c.incs) == c.digits and c.Q == dc.narrow_q(c.Ta, c.R) and c.Q % 4 == 0
        assert c.R * ((c.na + c.Q) | 1) <= 6144 and dc.plan(c), c.i
    assert {(c.mode, c.cplx) for c in cases} == {(m, x) for m in range(4) for x in (False, True)}
    assert {c.P for c in cases} == set(dc.NB_BLOCKS)
    assert any(c.na < 256 for c in cases)
    many = [c for c in cases if c.R >= 24 and any(nE - nS > 3 * c.na for _, _, nS, nE in dc.plan(c))]
    assert len(many) >= 4


@pytest.mark.parametrize("P,mode", [(16, nr.AM), (16, nr.FM), (4096, nr.AM), (4096, nr.IQ)])
def test_narrow_block_edges(P, mode):
    c = dc.narrow_edges(P, mode)
    p = dc.plan(c)
    assert [nE for _, _, _, nE in p] == c.ends
    f = dc.edge_facts([(nS, nE) for _, _, nS, nE in p], P)
    assert f.rel == {-1, 0, 1} and f.starts_on_edge
    if P == 16:
        assert c.na == 256 and any(nS % P and nE - nS >= 256 for _, _, nS, nE in p)   # 17 blocks in a tile
    else:
        assert f.open_calls >= 4
    c.squelch = dc.probe_squelch(c, nr, c.data[0])
    assert c.squelch > 0
    ref = dc.narrow_refs(c, nr, check=[0])[0]
    levels = []
    for d in dc.calls(c):
        ref.feed(d[0])
        levels.append(ref.level(0)[0])
    opens = [ref.estimate(0, j) for j in range(ref.n_next // P)]
    assert {o for o, _ in opens} == {True, False}
    assert True in levels and False in levels                      # the state differs across call boundaries
    if P == 16:                                                    # and toggles inside one tile of one call
        assert any(opens[j][0] != opens[j + 1][0] and any(nS <= j * P and (j + 2) * P <= nE and (j * P - nS) // 256 == ((j + 2) * P - 1 - nS) // 256
                                                            for _, _, nS, nE in p) for j in range(len(opens) - 1))
    if mode == nr.AM:                                              # a call that starts on an edge applies the dc of the block before
        assert any(nS % P == 0 and nS > 0 and ref.estimate(0, nS // P - 1)[1] > 0 and ref.estimate(0, nS // P - 1)[0] for _, _, nS, _ in p)


@pytest.mark.parametrize("R", [1, 5])
def test_narrow_short_calls(R):
    c = dc.narrow_short(R)
    p = dc.plan(c)
    assert [mE for _, mE, _, _ in p] == c.ends
    assert {mE - mS for mS, mE, _, _ in p} >= {1, c.Ta - 1, c.Ta}


@pytest.mark.parametrize("mode", [nr.IQ, nr.AM])
def test_narrow_threshold_is_exact_equality(mode):
    c = dc.narrow_threshold(mode)
    ref = dc.narrow_refs(c, nr, z=None)[0]
    for d in dc.calls(c):
        ref.feed(d[0])
    E = [ref.block(0, j)[0] for j in range(len(c.kinds))]
    assert E == [400 + kd for kd in c.kinds] and 400 == c.squelch ** 2 * c.P
    assert [ref.estimate(0, j)[0] for j in range(len(c.kinds))] == c.want_open
    assert [ref.block(1, j)[0] for j in range(len(c.kinds))] == E   # the half-turn station: the same energies


def test_narrow_extremes():
    c = dc.narrow_extreme(nr.FM)
    ref = dc.narrow_refs(c, nr)[0]
    out = np.concatenate([ref.feed(d[0]) for d in dc.calls(c)], axis=1)
    assert out.min() == -32768 and out.max() == 32767 and ref.v_max > (1 << 28)
    c = dc.narrow_extreme(nr.AM)
    ref = dc.narrow_refs(c, nr)[0]
    out = np.concatenate([ref.feed(d[0]) for d in dc.calls(c)], axis=1)
    # bytes are within [-127, 128] of the centre, so each component of y reaches half of its bound (16384 counts I and Q taps
    # together): both at once give a = sqrt 2 * 8187
    assert ref.a_max >= 11500 and out.min() == -32768 and out.max() == 32767


def test_channelizer_sweep_covers_the_shapes():
    cases = list(dc.channelizer_sweep())
    _edges_both_forms(cases)
    assert {c.T for c in cases} == set(dc.TAPS)
    assert all(max(c.sizes) // 2 >= c.T + c.D * 64 * c.G * 3 for c in cases)          # a call of several tiles


# ---- RDS bank ------------------------------------------------------------------------------------------------------------------

def _rds_run(c, cls=None, stations=None, stream=0):
    """Per accepted call of stream `stream`: (u, [pilot(k) for every k]), by the definition or a variant of it."""
    ref = dc.rds_refs(c, rr, check=[stream], cls=cls, stations=stations)[stream]
    out = []
    for d in dc.calls(c):
        if ref.completes(d.shape[1]) < 1:
            continue
        u = ref.feed(d[stream])
        out.append((u, [ref.pilot(k) for k in range(ref.K)]))
    return ref, out


def _differs(a, b, what):
    assert len(a) == len(b)
    if what == "output":
        return any(not np.array_equal(x[0], y[0]) for x, y in zip(a, b))
    return any(x[1] != y[1] for x, y in zip(a, b))


class CarrierRestarts(rr.RdsRef):
    """Wrong: the 57 kHz carrier starts at phase 0 in every call."""

    def carrier_index(self, m0):
        return 0


class ShiftTruncates(rr.RdsRef):
    """Wrong: v >> rds_shift rounds toward zero."""

    def shifted(self, v):
        return np.sign(v) * (np.abs(v) >> self.rds_shift)


class HistoryForgotten(rr.RdsRef):
    """Wrong: a call of fewer than Ta - 1 MPX samples builds the filter history from its own samples alone."""

    def window(self, q, lo, hi, m0):
        w = q[lo:hi].copy()
        if q.size - m0 < self.Ta - 1:
            w[:max(0, m0 - lo)] = 0
        return w


class PartialSumsDropped(rr.RdsRef):
    """Wrong: a block that straddles calls counts only the samples of the call that completes it."""

    def block_span(self, j):
        a, b = j * self.P, (j + 1) * self.P
        return max([a] + [m for m in self.cuts if m < b]), b


class EdgeBlockUnreported(rr.RdsRef):
    """Wrong: a block that ends exactly at the call's end is not reported until the next call."""

    def blocks_done(self, m):
        return (m - 1) // self.P if m else 0


def test_rds_helpers():
    assert [dc.rds_na(Ta, R) for Ta, R in ((1, 1), (256, 6), (256, 7), (256, 8), (256, 32), (1, 8))] == [256, 256, 246, 216, 54, 247]
    assert dc.rds_shift_for([16383]) == 14 and dc.rds_shift_for([1]) == 1 and dc.rds_shift_for([-8191, 8192]) == 14
    for gs in (1, 3, 100, 8191, 8192, 16383):
        s = dc.rds_shift_for([gs])
        assert -(-32768 * gs >> s) <= 32767 < -(-32768 * gs >> (s - 1))


def test_rds_sweep_covers_the_shapes():
    cases = list(dc.rds_sweep())
    assert len(cases) >= 32
    assert {c.R for c in cases} == set(range(1, 33))
    _edges_both_forms(cases)
    assert {c.Ta for c in cases} >= {1, 2, 63, 64, 255, 256} and any(c.Ta < c.R for c in cases)
    assert {c.P for c in cases} == set(dc.ST_BLOCKS)
    assert {c.pilot_min for c in cases} >= {0, 1, 16384} and any(1 < c.pilot_min < 16384 for c in cases)
    assert any(c.P == 16384 for c in cases) and any(c.pilot_min == 0 for c in cases) and any(c.pilot_min == 16384 for c in cases)
    assert any(c.na < 256 for c in cases) and any(c.na == 54 for c in cases)
    small = [c for c in cases if c.rds_shift == c.rds_shift_min]
    assert len(small) >= 8 and len(cases) - len(small) >= 8 and max(c.rds_shift for c in cases) >= 20
    assert {c.long_tiles for c in small} == {False, True} == {c.long_tiles for c in cases if c.rds_shift > c.rds_shift_min}
    many = [c for c in cases if any(nE - nS > 3 * c.na for _, _, nS, nE in dc.plan(c))]
    assert len(many) >= 8 and sum(c.na < 256 for c in many) >= 4
    assert sum((c.g < 0).any() and (c.g > 0).any() for c in cases) >= len(cases) // 2   # random signs
    refused = 0
    for c in cases:
        p = dc.plan(c)
        total = int(np.abs(c.g.astype(np.int64)).sum())
        assert max(c.Ta, 8000) <= total <= 16383
        assert c.rds_shift_min == dc.rds_shift_for(c.g) <= c.rds_shift <= 24
        assert c.rate >= 120000 * c.D and c.na == dc.rds_na(c.Ta, c.R) and c.R * c.na + c.Ta <= 1984
        assert p and any(mE // c.P > mS // c.P for mS, mE, _, _ in p), c.i       # a pilot block completes
        assert any(mE - mS > c.P for mS, mE, _, _ in p), c.i
        refused += len(c.sizes) - len(p)
    assert refused >= len(cases) // 2


def test_rds_sweep_tells_a_restarting_carrier():
    """Every case of the sweep, station 0 of stream 0 only (the carrier does not depend on the station)."""
    for c in dc.rds_sweep():
        _, good = _rds_run(c, stations=[0])
        ref, bad = _rds_run(c, cls=CarrierRestarts, stations=[0])
        assert _differs(good, bad, "output"), c.i
        assert ref.x[0].size > c.P and good[-1][1] == bad[-1][1]


@pytest.mark.parametrize("R", [8, 16, 32])
def test_rds_full_tiles(R):
    c = dc.rds_full_tiles(R)
    assert c.Ta == 256 and c.R * c.na + c.Ta == 1984 and c.na < 256
    p = dc.plan(c)
    assert [mE for _, mE, _, _ in p] == c.ends
    for mS, mE, nS, nE in p[:2]:
        assert nE - nS == 2 * c.na and (mE - c.Ta) % c.R == c.R - 1
        # the last of the two tiles: from its first window to the call's end, the largest span there is
        assert mE - c.R * (nS + c.na) == c.R * c.na + c.Ta - 1 == 1983
    assert p[1][0] - c.R * p[1][2] == c.Ta - 1                     # the second call's first window starts Ta - 1 samples back
    assert 1982 + (1982 >> 5) == 2043


@pytest.mark.parametrize("R", [1, 3, 32])
def test_rds_short_calls(R):
    c = dc.rds_short(R)
    p = dc.plan(c)
    assert [mE for _, mE, _, _ in p] == c.ends
    Ms = [mE - mS for mS, mE, _, _ in p]
    want = [1, 2, c.Ta - 2, c.Ta - 1, c.Ta, 1, c.Ta - 1, 2]
    it = iter(Ms)
    assert all(any(m == w for m in it) for w in want), Ms          # the listed M occur, in order
    assert Ms[-1] == 3000
    _, good = _rds_run(c, stations=[0])
    _, bad = _rds_run(c, cls=HistoryForgotten, stations=[0])
    assert _differs(good, bad, "output")
    wrong = [i for i, (a, b) in enumerate(zip(good, bad)) if not np.array_equal(a[0], b[0])]
    assert set(wrong) <= {i for i, m in enumerate(Ms) if m < c.Ta - 1} and {Ms[i] for i in wrong} >= {1, 2}


@pytest.mark.parametrize("P", [1024, 4096])
def test_rds_block_edges(P):
    c = dc.rds_edges(P)
    p = dc.plan(c)
    assert (c.Ta, c.R) == (9, 1) and c.ends == dc.stereo_edges(P).ends
    assert [mE for _, mE, _, _ in p] == c.ends                     # no call is refused
    f = dc.edge_facts([(mS, mE) for mS, mE, _, _ in p], P)
    assert f.rel == {-1, 0, 1} and f.open_calls >= 4 and f.whole >= 4 and f.starts_on_edge
    for s in (0, 1):
        ref, good = _rds_run(c, stream=s)
        for k in (0, 1) if s == 0 else (1, 2):                     # the two stations that are there
            reports = [pl[k] for _, pl in good]
            assert len(set(reports)) >= 3 and {pr for pr, _ in reports} == {False, True}, (s, k, reports)
            assert max(lv for _, lv in reports) > 4 * c.pilot_min > 0
        _, bad = _rds_run(c, cls=PartialSumsDropped, stream=s)
        assert _differs(good, bad, "pilot") and not _differs(good, bad, "output")
        _, bad = _rds_run(c, cls=EdgeBlockUnreported, stream=s)
        assert _differs(good, bad, "pilot") and not _differs(good, bad, "output")


@pytest.mark.parametrize("g,rds_shift", dc.RDS_EXTREMES)
def test_rds_extremes(g, rds_shift):
    c = dc.rds_extreme(g, rds_shift)
    e = dc.narrow_extreme(nr.FM)
    assert (c.D, c.T, c.R, c.rate) == (2, 16, 1, 304000) and (c.h == 2047).all() and not c.incs.any()
    assert np.array_equal(c.data, e.data) and c.shift == e.shift
    assert dc.y_bound(c.h, c.incs, c.shift) <= 16384 < dc.y_bound(c.h, c.incs, c.shift - 1)
    assert int(np.abs(c.g.astype(np.int64)).sum()) == 16383 and dc.rds_shift_for(c.g) == 14 <= c.rds_shift
    ref, good = _rds_run(c)
    u = np.concatenate([a for a, _ in good], axis=1)
    assert ref.x_max == 16384 and ref.q_max == 16384               # a half turn; never the header's 32768
    if c.Ta == 1:
        assert ref.v_max == 16384 * 16383 == 268419072
        assert u.min() == -16383 and u.max() == 16383
    else:
        assert c.Ta == 256 and (c.g > 0).all() and (1 << 20) < ref.v_max < (1 << 24)   # the carrier turns under the taps
    if rds_shift == 24:
        assert set(np.unique(u).tolist()) == {-1, 0}               # |v| < 2^24: the sign of v is all that is left
        _, bad = _rds_run(c, cls=ShiftTruncates)
        assert _differs(good, bad, "output")
