"""The case generators of the packet demodulator's *_domain GPU test (tests/packet_cases.py), checked here without a GPU: the
test-side copy of the tone-pair kernel's plan at points worked out by hand, its closed-form staging against a sample-by-sample walk,
the plane's margin over the whole domain, and, on the reference alone (tests/afsk_ref.py), that every family reaches what it claims.

The file also shows that the cases can tell a wrong kernel from a right one: each deliberately wrong variant of the definition
(WRONG, below) gives, on the families built for it, a result that differs from the definition's.  A variant that does not differ
means the family is too weak."""
import numpy as np
import pytest

import afsk_ref as ar
import packet_cases as pc


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan

def test_af_plan_by_hand():
    """2 (255 D + T + 32 rounded up to 8) + 16 ceil(T / 2) bytes.  (10, 2): 552 samples, 5 pairs, 1104 + 80.
    (20, 4): 1072 samples, 10 pairs, 2144 + 160.  (64, 32): 8256 samples, 32 pairs, 16512 + 512.  (3, 3): 800 samples, 2 pairs."""
    assert pc.af_plan(10, 2) == (5, 552, 1184)
    assert pc.af_plan(20, 4) == (10, 1072, 2304)
    assert pc.af_plan(64, 32) == (32, 8256, 17024)
    assert pc.af_plan(3, 3) == (2, 800, 1632) and pc.af_plan(2, 1) == (1, 296, 608)
    assert len(pc.AF_SHAPES) == 1551 and all(pc.af_domain_ok(T, D) for T, D in pc.AF_SHAPES)
    assert max(pc.af_plan(T, D).lds for T, D in pc.AF_SHAPES) == 17024 and all(pc.af_plan(T, D).plane_len % 8 == 0 for T, D in pc.AF_SHAPES)
    assert pc.af_reachable_h(10, 2) == [0, 8, 9] and pc.af_reachable_h(9, 9) == list(range(9)) and pc.af_reachable_h(64, 32) == [0] + list(range(32, 64))
    for T, D in ((10, 2), (9, 9), (64, 32), (7, 3)):         # what the counting rule leaves behind a call, at every stream length
        assert {N - ar.outputs(T, D, N) * D for N in range(T, T + 5 * D)} | {0} == set(pc.af_reachable_h(T, D))


def test_af_stage_by_hand():
    """(10, 2), 8 carried samples, 300 new ones, the row 3 samples behind a boundary: 150 outputs.  One tile: hh = 8, the call's
    samples [0, 300), koff = 3, kc = 8 + 3 = 11, the chunk at LDS 8.  The tile's chunks are 0 ... 37 (samples 3 ... 302 of the
    boundary's count end in chunk 37); chunk 0 starts in front of the row and chunk 37 ends behind it, so 1 ... 36 go whole.  The
    last sample is written to 11 + 299 = 310; lane 149 starts at 3 + 298 = 301 and reads dwords 150 ... 155, samples up to 311."""
    s = pc.af_stage(10, 2, 8, 300, 3, 0)
    assert (s.n_out, s.ntiles, s.no, s.hh, s.ja, s.jb, s.koff, s.kc, s.k_lo, s.nchunks) == (150, 1, 150, 8, 0, 300, 3, 11, 8, 38)
    assert (s.whole_lo, s.whole_hi, s.head_whole, s.tail_whole, s.min_written, s.max_written, s.kn0, s.max_read) == (1, 36, False, False, 3, 310, 3, 311)
    # the same call of 309 samples: 154 outputs, the window's last sample is 307 + 9 - 8 = 308 of the call, and chunk 38 holds
    # the boundary's samples 304 ... 311, all inside the row: the last chunk goes whole, up to LDS 8 + 39 * 8 - 1
    s = pc.af_stage(10, 2, 8, 309, 3, 0)
    assert (s.n_out, s.jb, s.nchunks, s.whole_hi, s.tail_whole, s.max_written) == (154, 308, 39, 38, True, 319)
    # a second tile: no history, ja = 512 - 8, koff = (3 + 504) & 7 = 3
    s = pc.af_stage(10, 2, 8, 1000, 3, 1)
    assert (s.n_out, s.ntiles, s.no, s.hh, s.ja, s.koff, s.kc, s.k_lo, s.head_whole) == (500, 2, 244, 0, 504, 3, 3, 0, True)


def test_the_closed_form_staging_equals_the_sample_by_sample_walk():
    rng = np.random.default_rng(pc.seed(4000))
    n = 0
    for T, D in [(2, 1), (3, 3), (9, 4), (10, 2), (64, 32), (63, 1)] + [pc.AF_SHAPES[int(i)] for i in rng.integers(0, 1551, 60)]:
        for h in pc.af_reachable_h(T, D)[:: max(1, D // 4)]:
            for _ in range(3):
                off = int(rng.integers(0, 8))
                n_in = T - h + int(rng.integers(0, [8, 40, 300 * D][int(rng.integers(0, 3))]))
                s0 = pc.af_stage(T, D, h, n_in, off, 0)
                for t in sorted({0, s0.ntiles - 1}):
                    s = pc.af_stage(T, D, h, n_in, off, t)
                    written, read = pc.stage_by_samples(T, D, h, n_in, off, t)
                    assert (min(written), max(written), max(read)) == (s.min_written, s.max_written, s.max_read), (T, D, h, n_in, off, t)
                    span = set(range(s.kn0, s.kn0 + (s.no - 1) * D + T))
                    assert span <= written and min(read) >= min(s.min_written, s.kn0 & ~1)        # every window is staged
                    n += 1
    assert n > 500


def test_the_plane_holds_every_index_over_the_whole_domain():
    """Every (T, D), every reachable h, every row offset, and the tile shapes: the call's only tile and its first of several
    (history in front), a middle tile and a last one (none), each with 1, 2, 3, 128, 255 and 256 outputs where it may, and every
    length of the call behind the last window (0 ... D - 1 samples: whole chunks reach up to 7 samples past what the tile needs).
    The largest index written or read stays below plane_len, and the smallest margin, plane_len - 1 - index, is 22 samples: at
    T = 3, D = 3, a full tile, the LDS origin shifted by 7.  (It is a lane's read one dword past its window that comes closest; a
    write comes no closer than 24.)  Every pair (hh & 7, koff) occurs."""
    worst_r, worst_w, pairs = (1 << 30,), (1 << 30,), set()
    no = np.array([1, 2, 3, 128, 255, 256])[:, None, None, None]
    off = np.arange(8)[None, :, None, None]
    for T, D in pc.AF_SHAPES:
        hs = np.array(pc.af_reachable_h(T, D))[None, None, :, None]
        e = np.arange(D)[None, None, None, :]
        plane = pc.af_plan(T, D).plane_len
        for t, more in ((0, 0), (0, 300), (1, 300), (1, 0), (2, 0)):      # `more`: outputs behind this tile (then it is a full one)
            n_out = t * 256 + (256 if more else no) + more
            n_in = (n_out - 1) * D + T - hs + e
            s = pc.stage_arrays(T, D, hs, n_in, off, t)
            assert (s.n_out == n_out).all() and (s.no == (256 if more else no)).all() and (s.min_written >= 0).all() and (s.k_lo >= 0).all()
            assert (s.hh == (hs if t == 0 else 0)).all() and ((s.kc - s.koff) % 8 == 0).all() and (s.kc - s.hh < 8).all()
            mr, mw = plane - 1 - s.max_read, plane - 1 - s.max_written
            i = np.unravel_index(mr.argmin(), mr.shape)
            worst_r = min(worst_r, (int(mr.min()), T, D, int(np.broadcast_to(s.kn0, mr.shape)[i])))
            worst_w = min(worst_w, (int(mw.min()), T, D))
            pairs |= set(zip((np.broadcast_to(s.hh, mr.shape) & 7).ravel().tolist(), np.broadcast_to(s.koff, mr.shape).ravel().tolist()))
    assert worst_r == (22, 3, 3, 7) and worst_w[0] == 24 and len(pairs) == 64
    # the bound behind it: the origin shift is at most 7, a window reads at most T + 2 samples from an even index (an odd T's pad
    # and the loop's last dword), a whole chunk at most 7 samples behind the span
    assert all(pc.af_plan(T, D).plane_len - (7 + 255 * D + T + 3) >= 22 for T, D in pc.AF_SHAPES)


# ---------------------------------------------------------------------------------------------------------------------------------
# wrong variants

WRONG = ["pre_trunc", "out_trunc", "energy_first", "sq_i32", "odd_drop", "odd_pad", "no_parity", "hist_zero", "hist_stale", "tab_swap",
         "tile_255", "row_hist", "rails"]
"""pre_trunc / out_trunc: the shift truncates toward zero.  energy_first: each energy is shifted before the subtraction.  sq_i32:
every square wraps to i32.  odd_drop: an odd T's last tap is lost.  odd_pad: an odd T's padding tap is 1 and reads the next sample.
no_parity: a lane ignores its window's parity in the plane (sh = 0) and starts one sample early where it is odd.  hist_zero: the
carried samples read as zero.  hist_stale: the carried samples are the ones that ended one sample earlier.  tab_swap: table rows 1
and 2 change places.  tile_255: the call's second and later tiles start at output 255 t.  row_hist: a row reads its neighbour's
carried samples.  rails: saturation at +-32767."""


# the variants each family is there to catch, as its test asserts them
CATCHES = {
    "af_every_shape": ["pre_trunc", "energy_first", "tab_swap", "hist_zero", "hist_stale", "row_hist", "tile_255", "no_parity", "odd_drop", "odd_pad"],
    "af_history_alignment": ["hist_zero", "hist_stale", "row_hist", "no_parity", "tile_255"],
    "af_short_rows": ["hist_zero", "hist_stale", "no_parity"],
    "af_every_shift": ["pre_trunc", "out_trunc", "energy_first", "rails"],
    "af_full_scale": ["sq_i32", "rails"],
    "af_tiles_and_rows": ["tile_255", "row_hist", "hist_stale"],
    "af_many_rows": ["hist_zero", "row_hist", "tile_255"],
}


def test_every_variant_has_a_family():
    assert sorted(set(sum(CATCHES.values(), []))) == sorted(WRONG) and len(WRONG) == 13 and all(hasattr(pc, f) for f in CATCHES)


def _trunc_shift(v, s):
    return np.where(v < 0, -((-v) >> s), v >> s)


def ref_call(c, r, lo, hi, in_cap, h, wrong=None):
    """The outputs [rows, n_out] of the call x[:, lo:hi] behind h carried samples: the definition, or one wrong variant of it."""
    T, D = c.T, c.D
    x = c.x.astype(np.int64)
    hist = x[:, lo - h:lo]
    if wrong == "hist_zero":
        hist = np.zeros_like(hist)
    elif wrong == "hist_stale" and h:
        hist = x[:, lo - h - 1:lo - 1]
    elif wrong == "row_hist":
        hist = np.roll(hist, -1, axis=0)
    virt = np.concatenate([np.zeros((c.rows, 1), np.int64), hist, x[:, lo:hi], np.zeros((c.rows, 1), np.int64)], axis=1)   # virtual sample v at v + 1
    n_out = (h + hi - lo - T) // D + 1
    o = np.arange(n_out)
    start = np.broadcast_to(o * D, (c.rows, n_out))
    if wrong == "tile_255":
        start = np.broadcast_to((o - o // 256) * D, (c.rows, n_out))
    if wrong == "no_parity":
        kn0 = np.array([[pc.af_stage(T, D, h, hi - lo, off, t).kn0 for t in range(-(-n_out // 256))] for off in pc.row_offsets(c, r, in_cap)])
        start = start - ((kn0[:, o // 256] + (o % 256) * D) & 1)
    tab = c.tab.astype(np.int64)
    if wrong == "odd_drop" and T % 2:
        tab = tab.copy()
        tab[:, -1] = 0
    if wrong == "tab_swap":
        tab = tab[[0, 2, 1, 3]]
    if wrong == "odd_pad" and T % 2:
        tab = np.concatenate([tab, np.ones((4, 1), np.int64)], axis=1)
    idx = start[:, :, None] + 1 + np.arange(tab.shape[1])[None, None, :]
    assert idx.min() >= 0 and idx.max() < virt.shape[1]
    S = np.take_along_axis(virt[:, None, :], idx, axis=2) @ tab.T
    A = _trunc_shift(S, c.pre) if wrong == "pre_trunc" else S >> c.pre
    sq = A * A
    if wrong == "sq_i32":
        sq = ((sq + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    Em, Es = sq[..., 0] + sq[..., 1], sq[..., 2] + sq[..., 3]
    if wrong == "energy_first":
        v = (Em >> c.out) - (Es >> c.out)
    elif wrong == "out_trunc":
        v = _trunc_shift(Em - Es, c.out)
    else:
        v = (Em - Es) >> c.out
    return np.clip(v, -32767 if wrong == "rails" else -32768, 32767).astype(np.int16)


def ref_runs(c, wrong=None, runs=None):
    """[[outputs per accepted call] per run]"""
    return [[ref_call(c, r, lo, hi, cap, h, wrong) for lo, hi, refused, cap, h in pc.af_pieces(c, r) if not refused] for r in (runs or c.runs)]


def differs(c, wrong, good=None, runs=None):
    good = ref_runs(c, None, runs) if good is None else good
    return any(not np.array_equal(a, b) for ra, rb in zip(good, ref_runs(c, wrong, runs)) for a, b in zip(ra, rb))


def common(c, runs=None):
    """Every run of the case equals the definition over its stream (tests/afsk_ref.py), call by call; the outputs per run."""
    good = ref_runs(c, None, runs)
    for r, outs in zip(runs or c.runs, good):
        n = max(hi for _, hi, _, _, _ in pc.af_pieces(c, r))
        assert np.array_equal(np.concatenate(outs, axis=1), ar.demod(c.x[:, :n], c.tab, c.D, c.pre, c.out)), c.name
    return good


# ---------------------------------------------------------------------------------------------------------------------------------
# the families

SHAPE_WRONG = CATCHES["af_every_shape"]


@pytest.mark.parametrize("g", range(7))
def test_every_shape_reaches_its_claims(g):
    """Per case: the cut leaves the claimed h (every reachable h > 0 of the pair's D occurs over the T that share it), the second
    call has a second tile behind history and the uncut one two tiles without; an odd T ends on a padded pair.  The variants a
    random draw cannot hide differ on every case, the carried samples wherever there are any; pre_shift's rounding, which out_shift
    can hide, on most cases and on every T."""
    Ts = pc.SHAPE_GROUPS[g]
    assert sorted(sum(pc.SHAPE_GROUPS, [])) == list(range(2, 65))
    cases = pc.af_every_shape(Ts)
    assert [(c.T, c.D) for c in cases] == [s for s in pc.AF_SHAPES if s[0] in Ts]
    seen = {w: {} for w in SHAPE_WRONG}
    for c in cases:
        good = common(c)
        cut, one = (pc.af_pieces(c, r) for r in c.runs)
        assert [p[2] for p in cut + one] == [False] * 3 and cut[1][4] == c.claim.h == c.T - c.D + (cut[0][1] - c.T) % c.D and one[0][3] % 2 == 1
        assert [o.shape[1] for o in good[0]] == [4, c.claim.second] and 257 <= c.claim.second <= 261 and good[1][0].shape[1] == 4 + c.claim.second
        assert 4 <= c.pre <= 9 and np.abs(c.tab.astype(np.int64)).max() == 1023 and c.tab.min() == -1023
        y = np.concatenate(good[0], axis=1).astype(np.int64)
        assert (np.abs(y) >= 32767).mean() < 0.25 and (c.out == 0 or (np.abs(y) > 8000).any())
        tiles = {(lo, t): s for r, lo, hi, row, t, s in pc.stages(c) if r is c.runs[0]}
        assert tiles[(cut[1][0], 0)].hh == c.claim.h and tiles[(cut[1][0], 1)].hh == 0 and tiles[(cut[1][0], 1)].no == c.claim.second - 256
        assert 2 * c.plan.npair - c.T == c.T % 2
        for w in SHAPE_WRONG:
            seen[w][(c.T, c.D)] = differs(c, w, good)
    for w in ("energy_first", "tab_swap", "tile_255", "no_parity"):
        assert all(seen[w].values()), (w, [k for k, v in seen[w].items() if not v])
    for w in ("odd_drop", "odd_pad"):
        assert all(v == (T % 2 == 1) for (T, D), v in seen[w].items()), w
    for w in ("hist_zero", "hist_stale", "row_hist"):                # (h = 0 behind the cut where D = T and r = 0)
        assert all(v == (c.claim.h > 0) for c, v in zip(cases, seen[w].values())), w
    hit = [k for k, v in seen["pre_trunc"].items() if v]             # out_shift hides a last bit of A in about one case of 20
    assert {T for T, _ in hit} == set(Ts) and len(hit) >= 0.8 * len(cases), (len(hit), len(cases))


@pytest.mark.parametrize("T,D", pc.HIST_PAIRS)
def test_history_alignment_reaches_its_claims(T, D):
    c = pc.af_history_alignment(T, D)
    hs = pc.af_reachable_h(T, D)
    assert c.claim.hs == hs and len(c.runs) == 16 * len(hs) and c.rows == 3
    assert sorted({(r.h, r.off_in, r.outs) for r in c.runs}) == [(h, off, n) for h in hs for off in range(8) for n in (3, 300)]
    assert {r.off_out for r in c.runs} == set(range(8))
    good = common(c)
    pairs, parity = set(), set()
    for r, lo, hi, row, t, s in pc.stages(c):
        if hi == sum(r.cuts):                                # the call under test
            assert (s.hh if t == 0 else 0, s.n_out) == (r.h if t == 0 else 0, r.outs)
            pairs.add((s.hh & 7, s.koff))
            if t == 1:
                parity.add(s.kn0 & 1)
    want = {(h & 7, off) for h in hs for off in range(8)} | {(0, (off - h) & 7) for h in hs for off in range(8)}
    assert pairs == want and parity == {0, 1}
    if (T, D) == (64, 32):
        assert len(pairs) == 64
    for r, outs in zip(c.runs, good):
        assert outs[-1].shape[1] == r.outs
        for w in ("hist_zero", "hist_stale", "row_hist"):
            assert differs(c, w, [outs], [r]) == (r.h > 0), (c.name, w, r.h, r.off_in, r.outs)
    assert differs(c, "no_parity", good) and differs(c, "tile_255", good)


def test_history_alignment_reaches_all_64_origins():
    """Over the four pairs: every (hh & 7, koff); (64, 32) alone gives them all, the smaller pairs give them at other plane lengths."""
    pairs = set()
    for T, D in pc.HIST_PAIRS:
        pairs |= {(h & 7, off) for h in pc.af_reachable_h(T, D) for off in range(8)}
    assert len(pairs) == 64 and pc.HIST_PAIRS == [(64, 32), (15, 8), (9, 9), (10, 2)]


@pytest.mark.parametrize("T,D", pc.SHORT_PAIRS)
def test_short_rows_reach_their_claims(T, D):
    """Calls with no whole chunk, with exactly one, and with a partial head and tail around whole ones; the refused piece in front
    where the shortest call is longer than one sample."""
    c = pc.af_short_rows(T, D)
    hs = [h for h in pc.af_reachable_h(T, D) if h]
    assert sorted({(r.h, r.n) for r in c.runs}) == [(h, n) for h in hs for n in range(T - h, 25)] and c.rows == 3
    good = common(c)
    kinds, offs = set(), set()
    for r in c.runs:
        p = pc.af_pieces(c, r)
        assert [q[2] for q in p] == ([False, True, False] if T - r.h > 1 else [False, False]) and p[-1][1] - p[-1][0] == r.n and p[-1][4] == r.h
        assert r.mode == "at" or (p[-1][3] % 2 == 1 and p[-1][3] > r.n)
    for r, lo, hi, row, t, s in pc.stages(c):
        if lo:
            nw = max(0, s.whole_hi - s.whole_lo + 1)
            kinds.add((min(nw, 2), s.head_whole, s.tail_whole))
            offs.add((hi - lo, s.koff))
            assert s.ntiles == 1 and s.hh == r.h
    assert {k[0] for k in kinds} == {0, 1, 2} and (1, False, False) in kinds and (2, False, False) in kinds and (0, False, False) in kinds
    assert {(n, k) for n in range(max(1, T - hs[-1]), 8) for k in range(8)} <= offs          # fewer than 8 samples, at every alignment
    for w in ("hist_zero", "hist_stale", "no_parity"):
        assert differs(c, w, good), w


def test_every_shift_separates_the_truncating_variants_per_value():
    """All 17 x 49 pairs.  Not every pair can show a difference (at (16, 48) every output is 0 or -1 whatever the rounding), so the
    condition is per value: every pre_shift >= 1 separates the variant that truncates it toward zero at some out_shift, every
    out_shift >= 1 separates its own at some pre_shift, and likewise the variant that shifts the energies before it subtracts."""
    cases = pc.af_every_shift()
    assert [(c.pre, c.out) for c in cases] == pc.SHIFTS and len(cases) == 17 * 49 and (cases[0].T, cases[0].D, cases[0].rows) == (7, 3, 16)
    x = cases[0].x.astype(np.int64)
    assert [int(np.abs(x[k]).max()) for k in range(15)] == [1 << k for k in range(15)] and x[15].min() == -32768 and x[15].max() == 32767
    sep = {w: set() for w in ("pre_trunc", "out_trunc", "energy_first", "rails")}
    for c in cases:
        good = common(c)
        y = np.concatenate(good[0], axis=1).astype(np.int64)
        if 2 * c.pre + c.out <= 48:                          # some row's value off the rails and away from 0 and -1 (the largest
            assert ((y > 0) & (y < 32767)).any() or ((y < -1) & (y > -32768)).any(), c.name    # |E_m - E_s| is about 2^56 / 4^pre_shift)
        for w in sep:
            if differs(c, w, good):
                sep[w].add((c.pre, c.out))
    assert {p for p, _ in sep["pre_trunc"]} == set(range(1, 17)) and not any(p == 0 for p, _ in sep["pre_trunc"])
    assert {o for _, o in sep["out_trunc"]} == set(range(1, 49)) and {o for _, o in sep["energy_first"]} == set(range(1, 49))
    assert not any(o == 0 for _, o in sep["out_trunc"] | sep["energy_first"])
    assert {p for p, _ in sep["out_trunc"]} == set(range(17)) and sep["rails"]


def test_full_scale_reaches_the_bound_the_rails_and_the_i32_wrap():
    cases = pc.af_full_scale()
    assert sorted({(c.pre, c.out) for c in cases}) == [(p, o) for p in range(17) for o in pc.FULL_OUT] and all(c.T == 64 for c in cases)
    S = 64 * 32768 * 1023
    wrap = set()
    for c in cases:
        good = common(c)
        y = np.concatenate(good[0], axis=1).astype(np.int64)
        if c.name.startswith("bound"):
            mark = c.tab[0, 0] == 1023
            want = (2 * (S >> c.pre) ** 2) >> c.out if mark else (-2 * (-S >> c.pre) ** 2) >> c.out
            assert y[0, 0] == max(-32768, min(32767, want)) and (c.out == 31) == (not mark), c.name
        else:
            assert len(good[0]) == 2 and y.shape == (4, 300) and (y < 0).any()
            assert c.out or ((y == 32767).any() and (y == -32768).any() and (np.abs(y) < 32767).any()), c.name
        if differs(c, "sq_i32", good):
            wrap.add(c.pre)
    assert wrap >= set(range(16))                            # (at pre_shift 16 |A| < 2^15 and a square fits i32)
    assert any(differs(c, "rails") for c in cases if c.out == 0)


@pytest.mark.parametrize("rows", pc.TILE_ROWS)
def test_tiles_and_rows_reach_their_claims(rows):
    cases = pc.af_tiles_and_rows(rows)
    assert [c.claim.n_out for c in cases] == list(pc.TILE_OUTS) and all((c.T, c.D, c.rows) == (5, 1, rows) for c in cases)
    for c in cases:
        good = common(c)
        n = c.claim.n_out
        assert [o.shape[1] for o in good[0]] == [n, n]
        tiles = [s for r, lo, hi, row, t, s in pc.stages(c) if row == 0]
        assert [s.no for s in tiles] == 2 * ([256] * (n // 256) + ([n % 256] if n % 256 else []))
        assert {s.hh for s in tiles} == {0, 4} and len(np.unique(c.x, axis=0)) == rows
        assert differs(c, "tile_255", good) == (n > 256), c.name
        assert differs(c, "row_hist", good) == (rows > 1) and differs(c, "hist_stale", good), c.name
    assert [-(-n // 256) * rows for n in (255, 257)] == [rows, 2 * rows]


def test_many_rows():
    c = pc.af_many_rows()
    assert (c.rows, c.T, c.D, c.x.shape) == (40000, 10, 2, (40000, 530))
    p = pc.af_pieces(c, c.runs[0])
    assert [(lo, hi, ref, h) for lo, hi, ref, _, h in p] == [(0, 522, False, 0), (522, 530, False, 8)]
    assert [ar.outputs(10, 2, n) for n in (522, 530)] == [257, 261] and pc.af_stage(10, 2, 0, 522, 0, 0).ntiles == 2
    assert len(set(c.sample)) == 16 and set(c.sample) >= {0, 32767, 32768, 39999}
    small = pc._case("many16", 7300, 10, 2, c.tab, c.pre, c.out, c.x[c.sample], c.runs)
    good = common(small)
    assert all(differs(small, w, good) for w in ("hist_zero", "row_hist", "tile_255"))
    y = np.concatenate(good[0], axis=1).astype(np.int64)
    assert (np.abs(y) >= 32767).mean() < 0.25


# ---------------------------------------------------------------------------------------------------------------------------------
# the designer

def test_the_designed_table_tells_mark_from_space_at_every_window(fmd):
    """T = 4 ... 64 at rate = 1200 T (a window of one bit): a full window of the mark tone at amplitude 1024 gives a positive output,
    one of the space tone a negative one, and out_shift is the smallest that keeps both inside int16."""
    for T in range(4, 65):
        rate = 1200 * T
        tab, pre, out = fmd.afsk_table(rate)
        assert tab.shape == (4, T) and pre == 8
        raw = []
        for f in (1200, 2200):
            x = [round(1024 * np.cos(2 * np.pi * f * t / rate)) for t in range(T)]
            A = [sum(int(tab[q, t]) * x[t] for t in range(T)) >> pre for q in range(4)]
            raw.append(A[0] ** 2 + A[1] ** 2 - A[2] ** 2 - A[3] ** 2)
            assert ar.afsk_row(x, tab, 1, pre, out) == [raw[-1] >> out]
        assert raw[0] > 0 > raw[1], (T, raw)
        assert all(-32768 <= v >> out <= 32767 for v in raw) and (raw[0] >> out) > 0 > (raw[1] >> out), (T, out, raw)
        assert out == 0 or any(not -32768 <= v >> (out - 1) <= 32767 for v in raw), (T, out, raw)
