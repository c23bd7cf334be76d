"""The case generators of the *_domain GPU tests (tests/domain_cases.py) against the references alone, without a GPU: every case
reaches what it claims.  The first-pass tile is 64 G outputs (64 G - 1 in the stereo bank), G the largest of 4, 3, 2, 1 with
raw + 2048 + 256 K G <= 40960 bytes of LDS, raw = max(12 + 6 D + 8 D (16 G - 1) + 64 nkc, 12 + 2 D (64 G - 1) + 2 T + 15) rounded
up to 16 and nkc = ceil((12 + 2 T) / 64) (st_lds, nb_lds, ch_lds): dc.groups is the test-side copy.

For the uniform channelizer and the band-plan bank dc.uniform_plan, dc.bp_cpr and dc.bp_pitch are the test-side copies of the host
plans, checked here at the points worked out by hand; the GPU files hold every case to the kernel name its
plan claims.

For the RDS bank the file also shows, still without a GPU, that the cases can tell a wrong kernel from a right one: each of five
deliberately wrong variants of the definition (small subclasses of rds_ref.RdsRef below) gives, on the family of cases built for
it, a result that differs from the definition's.

For the receiver bank dc.receiver_plan counts both second stages of every call and says which calls are refused and what they
would have completed; the tile counts of the two sides of its one second-pass grid follow from dc.stereo_na and
dc.rds_na."""
import numpy as np
import pytest

import domain_cases as dc
import narrow_ref as nr
import rds_ref as rr
import receiver_ref as rxr
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


# ---- receiver bank -------------------------------------------------------------------------------------------------------------

def _rx_run(c, stream=0, pilot_min=None):
    """The definition of one stream over the case's calls: (ref, [(audio, rds, [pilot(k) for every k]) per accepted call])."""
    ref = dc.receiver_refs(c, rxr, check=[stream], pilot_min=pilot_min)[stream]
    out = []
    for d in dc.calls(c):
        if min(ref.completes(d.shape[1])) < 1:
            continue
        a, u = ref.feed(d[stream])
        out.append((a, u, [ref.pilot(k) for k in range(ref.K)]))
    return ref, out


def test_receiver_sweep_covers_the_shapes():
    cases = list(dc.receiver_sweep())
    assert len(cases) >= 32
    assert {c.Ra for c in cases} == set(range(1, 33)) == {c.Rr for c in cases} and all(c.Ra != c.Rr for c in cases)
    _edges_both_forms(cases)
    assert {c.Ta_a for c in cases} >= set(dc.ST_TA) and {c.Ta_r for c in cases} >= set(dc.RX_TA_R)
    assert any(c.Ta_a < c.Ra for c in cases) and any(c.Ta_r < c.Rr for c in cases)
    assert {c.P for c in cases} == set(dc.ST_BLOCKS)
    assert {c.pilot_min for c in cases} >= {0, 1, 16384} and any(1 < c.pilot_min < 16384 for c in cases)
    assert any(c.na_a < 256 for c in cases) and any(c.na_r < 256 for c in cases)
    assert any(c.na_a == 48 for c in cases) and any(c.na_r == 54 for c in cases)
    small = [c for c in cases if c.rds_shift == c.rds_shift_min]
    assert len(small) >= 8 and len(cases) - len(small) >= 8 and max(c.rds_shift for c in cases) >= 20
    assert {c.long_tiles for c in small} == {False, True} == {c.long_tiles for c in cases if c.rds_shift > c.rds_shift_min}
    tiles, kinds, uneven_odd_rows = set(), set(), 0
    for c in cases:
        refused = []
        p = dc.receiver_plan(c, refused)
        kinds |= {k for _, k in refused}
        assert c.rate >= 120000 * c.D and 0 <= c.audio_shift <= 16 and dc.rds_shift_for(c.gr) == c.rds_shift_min <= c.rds_shift <= 24
        assert c.na_a == dc.stereo_na(c.Ta_a, c.Ra) and c.Ra * c.na_a + 2 * c.Ta_a <= 2048
        assert c.na_r == dc.rds_na(c.Ta_r, c.Rr) and c.Rr * c.na_r + c.Ta_r <= 1984
        for g in (c.ga, c.gr):
            assert max(g.size, 8000) <= int(np.abs(g.astype(np.int64)).sum()) <= 16383
        assert p and len(p) + len(refused) == len(c.sizes) == 7 and c.sizes[2] == 8 and max(c.Ra, c.Rr) >= 4
        # the 8-byte call after the first that completes both stages is refused in every case; a call refused although it completes
        # a stage is the receiver's own rule at work
        assert 2 in [i for i, _ in refused] and 1 not in [i for i, _ in refused] and 5 not in [i for i, _ in refused], (c.i, refused)
        assert max(mE - mS for mS, mE, _, _ in p) > c.P and any(mE // c.P > mS // c.P for mS, mE, _, _ in p), c.i
        nts = [dc.receiver_tiles(c, call) for call in p]
        tiles |= {(a > 1, r > 1) for a, r in nts}
        spans = sorted((c.Ra * c.na_a, c.Rr * c.na_r))
        if c.long_tiles:                                           # more than three tiles of the side with the smaller tile
            assert any(mE - mS > 3 * spans[0] for mS, mE, _, _ in p), c.i
        uneven_odd_rows += (c.S * c.K) % 2 == 1 and any(a > 1 and r > 1 and a != r for a, r in nts)
    assert tiles == {(False, False), (False, True), (True, False), (True, True)}
    assert uneven_odd_rows >= 4
    assert sum(c.long_tiles for c in cases) >= len(cases) // 4
    assert kinds == {"audio", "rds", "neither"}


def test_receiver_full_tiles():
    c = dc.receiver_full_tiles()
    assert (c.Ta_a, c.Ra, c.na_a) == (256, 6, 256) and c.Ra * c.na_a + 2 * c.Ta_a == 2048
    assert (c.Ta_r, c.Rr, c.na_r) == (256, 8, 216) and c.Rr * c.na_r + c.Ta_r == 1984
    p = dc.receiver_plan(c)
    assert [mE for _, mE, _, _ in p] == c.ends == [14079, 27903, 27975]
    assert [dc.receiver_tiles(c, call) for call in p] == [(9, 8), (9, 8), (1, 1)]
    three = 0
    for mS, mE, (aS, aE), (rS, rE) in p[:2]:
        assert (aE - aS, rE - rS) == (9 * c.na_a, 8 * c.na_r) and (mE - 256) % 24 == 23
        # the last tile of either side: from its first window to the call's end, the largest span there is
        assert mE - c.Ra * (aS + 8 * c.na_a) == c.Ra * c.na_a + c.Ta_a - 1 == 1791
        assert mE - c.Rr * (rS + 7 * c.na_r) == c.Rr * c.na_r + c.Ta_r - 1 == 1983
        for t in range(9):                                         # the call's own samples that audio tile t stages
            lo = max(c.Ra * (aS + t * c.na_a), mS)
            hi = mE if t == 8 else c.Ra * (aS + (t + 1) * c.na_a - 1) + c.Ta_a
            three += (hi - 1) // c.P - lo // c.P + 1 == 3
    assert three >= 1
    mS, _, (aS, _), (rS, _) = p[1]                                 # the second call's first windows start Ta - 1 samples back
    assert mS - c.Ra * aS == c.Ta_a - 1 and mS - c.Rr * rS == c.Ta_r - 1
    assert 1982 + (1982 >> 5) == 2043


@pytest.mark.parametrize("Ra,Rr", dc.RX_SHORT)
def test_receiver_short_calls(Ra, Rr):
    c = dc.receiver_short(Ra, Rr)
    refused = []
    p = dc.receiver_plan(c, refused)
    assert refused == c.refused and len(p) + len(refused) == len(c.spans)
    # the byte ranges are what the bank's position makes of them: an accepted call starts where the last accepted one ended, and a
    # refused call's bytes are the head of the next call, which is accepted
    pos, ref_idx = 0, {i for i, _ in refused}
    for i, (a, b) in enumerate(c.spans):
        assert a == pos and b > a
        if i in ref_idx:
            assert i + 1 not in ref_idx and c.spans[i + 1][0] == a and c.spans[i + 1][1] > b
        else:
            pos = b
    assert pos == c.data.shape[1]
    Ms = [mE - mS for mS, mE, _, _ in p]
    assert set(Ms) >= {1, 2, c.Ta_r - 2, c.Ta_r - 1, c.Ta_r, c.Ta_a - 2, c.Ta_a - 1, c.Ta_a} and Ms[-1] == 3000
    assert all(aE > aS and rE > rS for _, _, (aS, aE), (rS, rE) in p)
    # the kinds of refusal the strides allow: a side at stride 1 completes an output with every sample
    allowed = {"audio", "rds", "neither"} - ({"audio", "neither"} if Rr == 1 else set()) - ({"rds", "neither"} if Ra == 1 else set())
    assert {k for _, k in refused} == allowed and ((Ra, Rr) != (3, 5) or len(allowed) == 3)
    # a refusal comes before accepted calls of 2 and of Ta - 2 ... Ta samples
    after = {c.sizes[i + 1] // 8 for i, _ in refused}               # D = 4: 8 bytes a multiplex sample
    assert after >= {2, 254, 255, 256}
    # call-cut invariance of the definition: the uncut bytes give the concatenation of the accepted calls
    _, cut = _rx_run(c)
    whole = dc.receiver_refs(c, rxr, check=[0])[0]
    a, u = whole.feed(c.data[0])
    assert np.array_equal(a, np.concatenate([x[0] for x in cut], axis=1)) and np.array_equal(u, np.concatenate([x[1] for x in cut], axis=1))
    assert [whole.pilot(k) for k in range(c.K)] == cut[-1][2]


@pytest.mark.parametrize("P", [1024, 4096])
def test_receiver_block_edges(P):
    c = dc.receiver_edges(P)
    e = dc.rds_edges(P)
    assert c.ends == dc.stereo_edges(P).ends and np.array_equal(c.data, e.data) and np.array_equal(c.incs, e.incs)
    assert (c.Ta_a, c.Ra, c.Ta_r, c.Rr) == (9, 1, 9, 1) and c.pilot_min == dc.default_pilot_min(c.rate, c.D) > 0
    p = dc.receiver_plan(c)
    assert [mE for _, mE, _, _ in p] == c.ends                     # no call is refused
    f = dc.edge_facts([(mS, mE) for mS, mE, _, _ in p], P)
    assert f.rel == {-1, 0, 1} and f.open_calls >= 4 and f.whole >= 4 and f.starts_on_edge
    for s in (0, 1):
        ref, got = _rx_run(c, stream=s)
        for k in (0, 1) if s == 0 else (1, 2):                     # the two stations that are there: a pilot appears or vanishes
            reports = [pl[k] for _, _, pl in got]
            assert len(set(reports)) >= 3 and {pr for pr, _ in reports} == {False, True}, (s, k, reports)
        assert ref.stereo.kc_max > 0                               # the audio was stereo somewhere


def test_receiver_threshold_is_exact_equality():
    c, t = dc.receiver_threshold(), dc.stereo_threshold()
    assert np.array_equal(c.data, t.data) and c.sizes == t.sizes and c.rate == t.rate >= 120000 * c.D
    assert st.pilot_inc(c.rate, c.D) == 1 << 29
    audio, base = {}, {}
    for pm in (7, 8, 9):
        ref, got = _rx_run(c, pilot_min=pm)
        assert len(got) == len(c.sizes)
        I, Q = ref.stereo.block_iq(0, 0)
        assert (I, Q) == (1 << 26, 0) and I * I + Q * Q == (8 * c.P * 8192) ** 2
        audio[pm] = np.concatenate([a for a, _, _ in got], axis=1)[0, :2 * c.P - c.Ta_a + 1]
        base[pm] = np.concatenate([u for _, u, _ in got], axis=1)
    assert np.array_equal(audio[7], audio[8]) and not np.array_equal(audio[8], audio[9])
    assert np.array_equal(audio[9][:, 0], audio[9][:, 1]) and not np.array_equal(audio[8][:, 0], audio[8][:, 1])
    assert np.array_equal(base[7], base[8]) and np.array_equal(base[8], base[9]) and base[8].any()


@pytest.mark.parametrize("which", dc.RX_EXTREMES)
def test_receiver_extremes(which):
    c = dc.receiver_extreme(which)
    ref, got = _rx_run(c)
    assert len(got) == len(c.sizes)
    a = np.concatenate([x[0] for x in got], axis=1)
    u = np.concatenate([x[1] for x in got], axis=1)
    for ch in (0, 1):                                              # the audio at both rails in both channels
        assert a[..., ch].min() == -32768 and a[..., ch].max() == 32767
    assert int(np.abs(c.gr.astype(np.int64)).sum()) == 16383 and dc.rds_shift_for(c.gr) == 14 and c.audio_shift == 0
    if which == "stereo":
        e = dc.stereo_extreme(16384, 1)
        assert np.array_equal(c.data, e.data) and np.array_equal(c.ga, e.g) and c.shift == e.shift and c.rds_shift == 14
        assert ref.stereo.kc_max >= 32000 and ref.stereo.corr_max > (1 << 23) and ref.rds.v_max > (1 << 24)
    else:
        e = dc.rds_extreme(*{"rds-plus": ("plus", 14), "rds-256": ("256", 24)}[which])
        assert np.array_equal(c.data, e.data) and np.array_equal(c.gr, e.g) and (c.shift, c.rds_shift) == (e.shift, e.rds_shift)
        assert c.ga.tolist() == [16383]
        if c.Ta_r == 1:                                            # what tests/test_gpu_rds_domain.py asserts of the RDS bank's output
            assert ref.rds.v_max == 16384 * 16383 and u.min() == -16383 and u.max() == 16383
        if c.rds_shift == 24:
            assert set(np.unique(u).tolist()) == {-1, 0}


# ---- uniform channelizer and band-plan bank -----------------------------------------------------------------------------------------

def test_uniform_plan_copy():
    """The test-side plan (dc.uniform_plan, dc.bp_cpr, dc.bp_pitch) at the points worked out by hand."""
    Ts = range(1, 2049)
    for hop, T in dc.UV_G_EDGES:                                   # the two G edges, 64 KiB exactly on their G = 8 side
        _, G, _, _, lds = dc.uniform_plan(1, 2, hop, T)
        assert (G, lds == 65536) == ((8, True) if T in (1248, 224) else (4, False)), (hop, T)
    assert [min(T for T in Ts if dc.uniform_plan(1, 2, hop, T)[1] == 4) for hop in (240, 248)] == [1249, 225]
    assert all(dc.uniform_plan(1, 2, hop, T)[1] == (4 if T >= e else 8) for hop, e in ((240, 1249), (248, 225)) for T in Ts)
    assert all(dc.uniform_plan(1, 2, 256, T)[1] == 4 for T in Ts)
    assert all(dc.uniform_plan(1, 2, hop, T)[1] == 8 for hop in dc.UV_HOPS if hop <= 232 for T in Ts)
    assert all(dc.uniform_plan(K, d, hop, T)[4] <= 65536 for K in (1, 256) for d in (1, 2) for hop in dc.UV_HOPS for T in Ts)
    # R by the row tiles: 4 channels a tile with two-digit taps, 8 with one-digit taps
    assert [dc.uniform_plan(K, 2, 8, 8)[:3:2] for K in (1, 16, 17, 32, 33, 256)] == [(1, 1), (1, 4), (2, 5), (2, 8), (4, 9), (4, 64)]
    assert [dc.uniform_plan(K, 1, 8, 8)[:3:2] for K in (1, 32, 33, 64, 65, 256)] == [(1, 1), (1, 4), (2, 5), (2, 8), (4, 9), (4, 32)]
    assert [dc.uniform_plan(1, 2, 8, T)[3] for T in (1, 32, 33, 2047, 2048)] == [1, 1, 2, 64, 64]
    # pass 2: R rows of `pitch` dwords fit the 2176 staged dwords, and a row holds the tile's cells plus the padded taps' reach
    for R in range(1, 9):
        for Ta in range(1, 65):
            for cplx in (False, True):
                cpr, pitch = dc.bp_cpr(Ta, R, cplx), dc.bp_pitch(Ta, R, cplx)
                tpc = 4 if cplx else 8
                assert (cpr - 1) * tpc < -(-Ta // R) <= cpr * tpc and pitch % 2 == 1 and pitch >= dc.BP_TILE + cpr * tpc
                assert pitch * R <= 2176, (R, Ta, cplx)
    assert dc.bp_pitch(64, 8, False) * 8 == 2120 and dc.bp_pitch(64, 1, True) == 321


def _uniform_cases():
    if not hasattr(_uniform_cases, "cases"):
        _uniform_cases.cases = list(dc.uniform_sweep())
    return _uniform_cases.cases


def _bandplan_cases():
    if not hasattr(_bandplan_cases, "cases"):
        _bandplan_cases.cases = list(dc.bandplan_sweep())
    return _bandplan_cases.cases


def test_uniform_sweep_claims():
    import uniform_ref as ur
    for c in _uniform_cases():
        incs = ur.channel_incs(c.N, c.sel)
        assert len(incs) == c.K and (c.sel is None) == (c.K == c.N)
        assert ur.digits(c.h, incs) == c.digits, c.i
        assert dc.y_bound(c.h, incs, c.shift) <= c.limit and c.shift <= 24, c.i
        assert c.shift == 0 or dc.y_bound(c.h, incs, c.shift - 1) > c.limit, c.i
        assert c.shift >= ur.min_shift(c.h, incs) and (c.shift == ur.min_shift(c.h, incs)) == (c.limit == 16384), c.i
        assert (c.R, c.G, c.nrt, c.nkc, c.lds_bytes) == dc.uniform_plan(c.K, c.digits, c.hop, c.T), c.i
    shifts = [c.limit for c in _uniform_cases()]
    assert set(shifts) == {256, 2048, 16384} and all(a != b for a, b in zip(shifts[:-1], shifts[1:]))


def test_uniform_sweep_covers_the_kernel():
    cases = _uniform_cases()
    cell = lambda c: (c.R, c.G)
    assert {(cell(c), c.digits) for c in cases} == {(x, d) for x in dc.UV_CELLS for d in (1, 2)}
    assert {(c.K, c.digits) for c in cases} >= set(dc.UV_K_EDGES)
    # batching: a partial last batch of 1 and of 3 row tiles at R = 4, of 1 at R = 2; K that does not fill its last row tile
    assert {c.nrt % 4 for c in cases if c.R == 4} >= {1, 3} and {c.nrt % 2 for c in cases if c.R == 2} >= {1}
    assert any(c.R > 1 and c.digits == 2 and c.K % 4 for c in cases) and any(c.R > 1 and c.digits == 1 and c.K % 2 for c in cases)
    assert any(-(-c.nrt // c.R) > 4 and c.nrt % c.R for c in cases)                      # a wave takes a second batch, the last is partial
    assert any(c.nrt == 64 and c.N == 256 and c.digits == 2 for c in cases)
    # the G edge, at R = 2 or 4
    at = {(c.hop, c.T): c for c in cases}
    assert set(dc.UV_G_EDGES) <= set(at) and all(at[e].R in (2, 4) for e in dc.UV_G_EDGES)
    assert [(at[e].G, at[e].lds_bytes == 65536) for e in dc.UV_G_EDGES] == [(8, True), (4, False), (8, True), (4, False)]
    assert {at[e].R for e in dc.UV_G_EDGES if at[e].G == 4} == {2, 4}                     # G = 4 no longer with R = 1 alone
    # hops: all 32, and those that are no power of two in every R
    assert {c.hop for c in cases} == set(dc.UV_HOPS) and len(dc.UV_HOPS) == 32
    assert {c.R for c in cases if c.hop & (c.hop - 1)} == {1, 2, 4}
    # taps: the K-chunk edges, no history, exactly one hop, one more, whole hops
    assert {c.T for c in cases} >= {32, 33, 2047, 2048, 1}
    assert any(c.T < c.hop for c in cases) and any(c.T == c.hop for c in cases) and any(c.T == c.hop + 1 for c in cases)
    assert any(c.T % c.hop == 0 and c.T > c.hop for c in cases)
    # the device path: half of the cases, every cell
    dev = [c for c in cases if c.dev]
    assert 2 * len(dev) == len(cases) and {cell(c) for c in dev} == set(dc.UV_CELLS)
    assert max(c.S for c in cases) == 3 and min(c.S for c in cases) == 2


def test_uniform_sweep_calls():
    """By the definition's own counting: the first call is refused wherever a refusal exists (T > hop: a call is at least one hop,
    and one hop completes an output when T <= hop), three calls are accepted, the first of them spans more than three tiles and
    ends inside one, a single hop follows, then more than a tile."""
    import uniform_ref as ur
    for c in _uniform_cases():
        ref = ur.UniformRef(np.ones(c.T, np.int64), c.N, c.hop, 0, channels=[0])
        fed, spans = [], []
        for n in c.sizes:
            m = ref.outputs_after(n // 2) - ref.m_next
            fed.append(m >= 1)
            if m >= 1:
                spans.append(m)
                ref.m_next += m
                ref.pos += n // 2
        tile = 16 * c.G
        assert c.refuses == (c.T > c.hop) and fed == ([False] if c.refuses else []) + [True] * 3, c.i
        assert spans[0] > 3 * tile and spans[0] % tile and spans[1] == 1 and tile < spans[2] < 2 * tile, (c.i, spans)
        assert [b - a for a, b in dc.uniform_outputs(c)] == spans
        assert c.sizes[-2] == 2 * c.hop and all(n % (2 * c.hop) == 0 and n > 0 for n in c.sizes)
        assert sum(spans) <= 800                                   # a few hundred outputs per channel, not a workload
    assert sum(c.refuses for c in _uniform_cases()) >= 25


def test_bandplan_sweep_covers_the_second_pass():
    cases = _bandplan_cases()
    for R in range(1, 9):
        mine = [c for c in cases if c.R == R]
        qmax = -(-64 // R)
        for cplx in (True, False):
            want = {min(q, qmax) for q in dc.BP_Q_EDGES[cplx]}
            assert {c.q for c in mine if c.cplx == cplx} >= want, (R, cplx)
            assert want == set(dc.BP_Q_EDGES[cplx]) or qmax in want      # what Ta <= 64 cannot reach: the nearest edge there is
        assert any(c.Ta < R for c in mine) or R == 1
        assert any(c.Ta == 64 for c in mine) and {c.uv[:2] for c in mine} == set(dc.UV_CELLS), R
    assert {c.R for c in cases} == set(range(1, 9))
    # the chunk edges as the kernel sees them: 1 | 2 and 2 | 3 chunks a row in both tap kinds
    assert {(c.cplx, c.cpr) for c in cases} >= {(x, n) for x in (True, False) for n in (1, 2, 3)}
    for c in cases:
        assert 1 <= c.Ta <= 64 and c.q == -(-c.Ta // c.R) and c.cpr == dc.bp_cpr(c.Ta, c.R, c.cplx) and c.pitch * c.R <= 2176
        assert c.cplx == (c.gi is not None and bool(np.any(c.gi))), c.i
        total = int(np.abs(c.gr.astype(np.int64)).sum() + (0 if c.gi is None else np.abs(c.gi.astype(np.int64)).sum()))
        peak = max(int(np.abs(c.gr).max()), 0 if c.gi is None else int(np.abs(c.gi).max()))
        assert total <= 65535 and peak <= 16383
        if not c.rule:                                             # the edge taps
            assert peak == 16383 and (total == 65535 or c.Ta * (2 if c.cplx else 1) < 5), c.i
    assert {(c.rule, c.cplx) for c in cases} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {(c.mode, c.cplx) for c in cases} == {(m, x) for m in range(4) for x in (False, True)}
    assert {c.P for c in cases} == set(dc.BP_BLOCKS) and len(dc.BP_BLOCKS) == 9 and dc.BP_BLOCKS[0] == 16 and dc.BP_BLOCKS[-1] == 4096
    assert 3 * sum(c.use_squelch for c in cases) == 2 * len(cases)
    assert {c.P for c in cases if c.use_squelch} == set(dc.BP_BLOCKS) == {c.P for c in cases if not c.use_squelch}
    assert len({c.gain for c in cases}) > len(cases) // 2 and all(1 <= c.gain <= 65535 for c in cases)
    assert min(c.gain for c in cases) < 8192 and max(c.gain for c in cases) > 57344


def test_bandplan_sweep_shifts_and_stage_one():
    import bandplan_ref as br
    import uniform_ref as ur
    cases = _bandplan_cases()
    for c in cases:
        incs = ur.channel_incs(c.N, c.sel)
        assert ur.digits(c.h, incs) == c.digits and c.uv == dc.uniform_plan(c.K, c.digits, c.hop, c.T), c.i
        assert c.shift_min == ur.min_shift(c.h, incs) <= c.shift <= 24 and (c.shift == c.shift_min) == c.auto_shift, c.i
        assert c.chan_shift == br.min_chan_shift(c.h, c.N, c.shift, c.gr, c.gi, c.sel, limit=c.cs_limit) <= 30, c.i
        assert c.auto_chan_shift == (c.cs_limit == (256 if c.mode == br.FM else 16384))
    assert {c.cs_limit for c in cases} == {256, 4096, 16384}
    assert {c.cs_limit for c in cases if c.mode != br.FM} == {256, 4096, 16384}
    fm = [c for c in cases if c.mode == br.FM]
    assert 2 * sum(c.cs_limit == 256 for c in fm) >= len(fm) and any(c.cs_limit > 256 for c in fm)
    assert 3 * sum(not c.auto_shift for c in cases) == len(cases)
    assert {c.uv[:2] for c in cases} == set(dc.UV_CELLS) and all(c.K <= 33 for c in cases)


def test_bandplan_sweep_calls():
    """By the definition's own counting (completes): the first call is refused -- in some cases although it completes stage-one
    outputs -- and the other four are accepted: the first audio, more than three tiles of 256, a call of one or two stage-one
    outputs (fewer than Ta - 1 wherever Ta >= 4) that completes an audio sample, one more."""
    import bandplan_ref as br
    kinds = set()
    for c in _bandplan_cases():
        ref = br.BandPlanRef(np.ones(c.T, np.int64), c.N, c.hop, 0, c.gr, c.gi, c.mode, c.R, 0, c.P, 0, 256, channels=[0])
        done, ys = [], []
        for n in c.sizes:
            a = ref.completes(n)
            m = ref.ch.outputs_after(n // 2) - ref.ch.m_next
            if not done and not ys and a < 1:
                kinds.add(m > 0)
                ys.append(m)
                continue
            done.append(a)
            ys.append(m)
            ref.n_next += a
            ref.ch.m_next += m
            ref.ch.pos += n // 2
        assert len(c.sizes) == 5 and len(done) == 4 and min(done) >= 1, (c.i, done)
        assert ys[0] == c.refused_outputs < c.Ta and done[1] > 3 * dc.BP_TILE and done[1] % dc.BP_TILE and done[2] == 1, (c.i, ys, done)
        assert ys[3] in (1, 2) and (ys[3] < c.Ta - 1 or c.Ta < 4), (c.i, ys)
        assert [(mE - mS, nE - nS) for mS, mE, nS, nE in dc.bp_plan(c)] == list(zip(ys[1:], done)), c.i
        assert ref.ch.m_next == c.ms[-1] and all(n % (2 * c.hop) == 0 for n in c.sizes)
    assert kinds == {False, True}
    assert sum(c.Ta >= 4 for c in _bandplan_cases()) >= 50


@pytest.mark.parametrize("P,mode,off", [(16, nr.AM, 0), (16, nr.FM, 0), (256, nr.AM, 0), (256, nr.FM, 1), (256, nr.IQ, 1), (4096, nr.AM, 0),
                                        (4096, nr.SSB, 0)])
def test_bandplan_block_edges(P, mode, off):
    import bandplan_ref as br
    c = dc.bandplan_edges(P, mode, off)
    p = dc.bp_plan(c)
    assert [nE for _, _, _, nE in p] == c.ends and len(p) == len(c.sizes)          # no call is refused
    f = dc.edge_facts([(nS, nE) for _, _, nS, nE in p], P)
    assert f.rel == {-1, 0, 1}
    if P == 16:
        assert f.starts_on_edge and any(nS % P and nE - nS >= 256 for _, _, nS, nE in p)              # 17 blocks in a tile
    elif P == 256:
        tiles = [(nS + t, min(nS + t + 256, nE)) for _, _, nS, nE in p for t in range(0, nE - nS, 256)]
        whole = [a % P == 0 and b - a == P for a, b in tiles]
        split = [a % P == 1 and b - a == P for a, b in tiles]      # the last sample of a block and 255 of the next
        assert (sum(whole) >= 6 and not any(split[:3])) if off == 0 else (sum(split) >= 5 and sum(whole) <= 1), (whole, split)
    else:
        assert f.open_calls >= 4
    c.squelch = dc.bandplan_probe_squelch(c, br, c.data[0])
    assert c.squelch > 0
    ref = dc.bandplan_refs(c, br, check=[0])[0]
    for d in dc.calls(c):
        ref.feed(d[0])
    opens = [ref.estimate(0, j)[0] for j in range(ref.n_next // P)]
    assert {o for o in opens} == {True, False}


@pytest.mark.parametrize("mode", [nr.IQ, nr.FM, nr.AM, nr.SSB])
def test_bandplan_threshold_is_exact_equality(mode):
    import bandplan_ref as br
    import uniform_ref as ur
    c = dc.bandplan_threshold(mode)
    assert ur.channel_incs(2) == [0, 1 << 31] and (c.N, c.hop, c.T, c.Ta, c.P, c.squelch, c.shift, c.chan_shift) == (2, 8, 1, 1, 16, 5, 0, 0)
    t = dc.narrow_threshold(mode)
    assert np.array_equal(c.data.reshape(-1, 16)[:, :2], t.data.reshape(-1, 4)[:, :2]) and c.kinds == t.kinds
    ref = dc.bandplan_refs(c, br)[0]
    out = np.concatenate([ref.feed(d[0]) for d in dc.calls(c)], axis=1)
    E = [ref.block(0, j)[0] for j in range(len(c.kinds))]
    assert E == [400 + kd for kd in c.kinds] and 400 == c.squelch ** 2 * c.P
    assert [ref.block(1, j)[0] for j in range(len(c.kinds))] == E    # the half-turn channel: the same energies
    assert [ref.estimate(0, j)[0] for j in range(len(c.kinds))] == c.want_open == [e >= 400 for e in E]
    if mode != nr.AM:                                              # (AM: a - dc is 5 - 5 in most open blocks)
        for k in (0, 1):
            loud = [bool(out[k, j * c.P:(j + 1) * c.P].any()) for j in range(len(c.kinds))]
            assert loud == [False] + c.want_open[:-1], (k, loud)    # a block sounds exactly when the block before had E >= 400


def test_bandplan_extremes():
    """What bytes can reach: a component of y, and of u, half of its bound of 16384 (8187 after the two floors), so
    a = isqrt(ur^2 + ui^2) stops at 11578 = floor(sqrt 2 * 8187), not at 23170, as in the narrow-band bank's case."""
    import bandplan_ref as br
    for mode in (nr.FM, nr.AM):
        c, e = dc.bandplan_extreme(mode), dc.narrow_extreme(mode)
        assert (c.N, c.hop, c.T, c.Ta, c.gain) == (2, 8, 16, 4, 65535) and (c.h == 2047).all() and (c.gr == 16383).all()
        assert np.array_equal(c.data, e.data) and (c.shift, c.chan_shift) == (e.shift, e.chan_shift)
        assert c.shift == br.ur.min_shift(c.h, [0]) and c.chan_shift == br.min_chan_shift(c.h, 2, c.shift, c.gr, None, [0])
        ref = dc.bandplan_refs(c, br)[0]
        out = np.concatenate([ref.feed(d[0]) for d in dc.calls(c)], axis=1)
        assert out.min() == -32768 and out.max() == 32767 and ref.v_max > (1 << 28)
        assert int(np.abs(ref.u[0]).max()) == 8187 and (mode == nr.FM or ref.a_max == 11578)
