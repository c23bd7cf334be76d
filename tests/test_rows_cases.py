"""The case generators of the row processors' *_domain GPU tests (tests/rows_cases.py), checked here without a GPU: the test-side
copies of the three launch plans at points worked out by hand, the resampler's tile of 256 over the whole domain, and, on the
references alone, that every family reaches what it claims -- history lengths, segments, tiles, refused calls, rails, winners, the gate.

The file also shows that the cases can tell a wrong kernel from a right one: each deliberately wrong variant of a definition (small
subclasses of the references below) gives, on the family built for it, a result that differs from the definition's.  A variant that
does not differ means the family is too weak."""
import numpy as np
import pytest

import agc_ref as ar
import resample_ref as rr
import rows_cases as rc
import tonesq_ref as tr


# ---------------------------------------------------------------------------------------------------------------------------------
# the plans

def test_agc_plan_table():
    """16 KiB of int16 are 8192 samples at width 1 and 4096 at width 2; two blocks exceed that from P = 4096 (width 1: exactly two
    blocks) and P = 2048 (width 2: exactly two blocks, and four blocks of bytes at P = 4096)."""
    assert [rc.agc_plan(P, 1)[1] for P in rc.AG_P] == [511, 255, 127, 63, 31, 15, 7, 3, 1]
    assert [rc.agc_plan(P, 2)[1] for P in rc.AG_P] == [255, 127, 63, 31, 15, 7, 3, 1, 1]
    assert rc.agc_plan(16, 1)[0] == 8192 and rc.agc_plan(4096, 1)[0] == 8192 and rc.agc_plan(4096, 2)[0] == 8192 and rc.agc_plan(16, 2)[0] == 4096
    assert len({rc.agc_plan(P, w)[1] for P in rc.AG_P for w in (1, 2)}) == 9


def test_tq_nj_by_hand():
    """2 F tone rows; wave w starts at row 8 w and strides 32."""
    assert [rc.tq_nj(F) for F in (4, 5, 16, 17, 38, 64)] == [(1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 1, 1), (2, 1, 1, 1), (3, 3, 2, 2), (4, 4, 4, 4)]
    edges = [F for F in range(1, 64) if rc.tq_nj(F) != rc.tq_nj(F + 1)]
    assert edges == list(range(4, 64, 4))                    # some wave's nj changes behind every multiple of 4
    assert all(sum(rc.tq_nj(F)) * 8 >= 2 * F for F in range(1, 65))


def test_rs_plan_by_hand():
    """15 / 16 at T = 32: output 255 starts ceil(255 16 / 15) = 272 samples in, span 304, plane 336; 16 pairs, 17 dwords; the whole
    table, 15 phases.  441 / 512 at T = 24: ceil(255 512 / 441) = 297, span 321, plane 360; 12 pairs, 13 dwords; 256 lanes' phases.
    64 / 1023 at T = 256, width 2: ceil(255 1023 / 64) = 4077, span 4333, plane 4368; 128 pairs, 129 dwords; 64 phases."""
    assert rc.rs_plan(15, 16, 32, 1) == (256, True, 16, 17, 336, 2 * 336 + 4 * 15 * 17)
    assert rc.rs_plan(15, 16, 32, 2) == (256, True, 16, 17, 336, 4 * 336 + 4 * 15 * 17)
    assert rc.rs_plan(441, 512, 24, 1) == (256, False, 12, 13, 360, 2 * 360 + 4 * 256 * 13)
    assert rc.rs_plan(441, 512, 24, 2) == (256, False, 12, 13, 360, 4 * 360 + 4 * 256 * 13)
    assert rc.rs_plan(64, 1023, 256, 2) == (256, True, 128, 129, 4368, 50496)
    # an odd T > 1 ends on a pair of one tap and a padding zero; npair | 1 adds a dword for some T and not for others
    assert [(rc.rs_plan(3, 4, T, 1).npair, rc.rs_plan(3, 4, T, 1).tdw) for T in (1, 2, 3, 5, 7, 255, 256)] == \
        [(1, 1), (1, 1), (2, 3), (3, 3), (4, 5), (128, 129), (128, 129)]


def test_the_resamplers_tile_is_256_over_the_whole_domain():
    """The LDS of a tile is 2 width plane_len + 4 min(L, tile) tdw bytes.  plane_len grows with the span ceil((tile - 1) M / L) + T,
    so with M and with T; tdw grows with T; neither falls.  For a given L the largest admissible M (min(1024, 32 L)) and T
    (min(256, 16384 // L)) therefore bound every plan of that L, and the 1024 values of L are the whole domain.  Each of them fits
    the budget at the tile of 256: the shrink branch of the plan is unreachable in today's domain.  This test fails when a wider
    domain, a larger slack or a smaller budget makes it reachable -- and its path is then one that no GPU test has run."""
    worst = {}
    for width in (1, 2):
        for L in range(1, 1025):
            M, T = min(1024, 32 * L), min(256, 16384 // L)
            assert rc.rs_domain_ok(L, M, T) and not rc.rs_domain_ok(L, M + 1, T) and not rc.rs_domain_ok(L, M, T + 1)
            p = rc.rs_plan(L, M, T, width)
            assert p.tile == 256 and p.lds <= rc.RS_BUDGET, (L, M, T, width)
            worst[width] = max(worst.get(width, (0,)), (p.lds, L, M, T))
        for L in (255, 256, 257):                            # around the switch of the table's form
            for M in (L - 1, L + 1):
                p = rc.rs_plan(L, M, 16384 // L, width)
                assert p.tile == 256 and p.whole == (L <= 256)
    assert worst[2][:2] == (50496, 64) and worst[1][0] < worst[2][0]
    assert rc.rs_plan(64, 1023, 256, 2).lds == worst[2][0]
    # monotone in M and in T, on a sample of the domain
    rng = np.random.default_rng(5)
    for _ in range(300):
        L = int(rng.integers(1, 1025))
        M, T = int(rng.integers(max(1, -(-L // 8)), min(1024, 32 * L))), int(rng.integers(1, min(256, 16384 // L) + 1))
        a = rc.rs_plan(L, M, T, 2).lds
        assert rc.rs_plan(L, M + 1, T, 2).lds >= a and (L * (T + 1) > 16384 or T == 256 or rc.rs_plan(L, M, T + 1, 2).lds >= a)


# ---------------------------------------------------------------------------------------------------------------------------------
# resampler: wrong variants and the families

class RsWrong(rr.Resampler):
    """The definition with one fault.  `drop_last`: tap T - 1 of an odd T > 1 (the tap next to the padding zero) is lost.  `no_mod`:
    in lane order (L > 256) lane j of a tile reads phase p0 + j M without the reduction mod L, and what lies behind the table is
    zero.  `oldest`: the oldest carried sample is lost.  `sat_first`: the sum saturates before the shift."""

    def __init__(self, g, L, M, shift, wrong):
        super().__init__(g, L, M, shift)
        self.wrong = wrong
        if wrong == "drop_last" and self.T % 2 == 1 and self.T > 1:
            self.g = self.g.copy()
            self.g[:, -1] = 0

    def push(self, x):
        x = np.asarray(x, dtype=np.int16)
        n_in = x.shape[-2]
        o0, o1 = rr.outputs(self.N, self.L, self.M, self.T), rr.outputs(self.N + n_in, self.L, self.M, self.T)
        if o1 == o0:
            raise rr.TooShort()
        virt = x if self.hist is None else np.concatenate([self.hist, x], axis=-2)
        base = self.N - (0 if self.hist is None else self.hist.shape[-2])
        if self.wrong == "oldest" and self.hist is not None and self.hist.shape[-2] > 0:
            virt = virt.copy()
            virt[..., 0, :] = 0
        n = np.arange(o0, o1, dtype=np.int64)
        i, p = (n * self.M) // self.L - base, (n * self.M) % self.L
        g = self.g[p]
        if self.wrong == "no_mod" and not rc.rs_plan(self.L, self.M, self.T, x.shape[-1]).whole:
            j = (n - o0) % rc.RS_TILE
            pu = ((n - j) * self.M) % self.L + j * self.M
            g = np.where((pu < self.L)[:, None], self.g[np.minimum(pu, self.L - 1)], 0)
        idx = i[:, None] + np.arange(self.T)[None, :]
        v = (virt.astype(np.int64)[..., idx, :] * g[:, :, None]).sum(axis=-2)
        self.N += n_in
        hn = self.history()
        self.hist = virt[..., virt.shape[-2] - hn:, :].copy()
        if self.wrong == "sat_first":
            v = np.clip(v, -32768, 32767)
        return np.clip(v >> self.shift, -32768, 32767).astype(np.int16)


def _rs_run(c, ref=None):
    """The case through a reference call by call: (outputs per accepted call, history lengths behind them, refusals)."""
    ref = rr.Resampler(c.g, c.L, c.M, c.shift) if ref is None else ref
    outs, hist, refused = [], [], 0
    for lo, hi, no in rc.rs_pieces(c):
        if no:
            with pytest.raises(rr.TooShort):
                ref.push(c.x[:, lo:hi])
            refused += 1
            continue
        outs.append(ref.push(c.x[:, lo:hi]))
        hist.append(ref.history())
    return outs, hist, refused


def _rs_differs(c, wrong):
    good, _, _ = _rs_run(c)
    bad, _, _ = _rs_run(c, RsWrong(c.g, c.L, c.M, c.shift, wrong))
    return any(not np.array_equal(a, b) for a, b in zip(good, bad))


def _rs_common(c, min_calls=4):
    outs, hist, refused = _rs_run(c)
    assert refused == c.refused, c.name                      # the refused calls the case names, none more
    assert len(outs) >= min_calls and np.array_equal(np.concatenate(outs, axis=1), rr.resample_all(c.x, c.g, c.L, c.M, c.shift)), c.name
    assert c.plan.tile == 256 and max(hist) <= c.T - 1
    return outs, hist


@pytest.mark.parametrize("width", [1, 2])
def test_resampler_t_sweep_reaches_its_claims(width):
    cases = rc.rs_t_sweep(width)
    assert [c.T for c in cases if c.L == 3] == list(rc.RS_T) and [c.T for c in cases if c.L == 257] == [T for T in rc.RS_T if T <= 63]
    for c in cases:
        outs, hist = _rs_common(c)
        assert c.plan.whole == c.claim.whole == (c.L == 3)
        assert c.claim.odd_pair == (2 * c.plan.npair == c.T + 1 and c.T > 1)
        total = sum(o.shape[1] for o in outs)
        assert rc.rs_tiles(total) == (2, True) and rc.rs_tiles(outs[0].shape[1])[0] == 1       # the uncut call: a full and a partial tile
        if c.claim.odd_pair:
            assert _rs_differs(c, "drop_last"), c.name
        assert _rs_differs(c, "no_mod") == (not c.plan.whole), c.name
        assert c.T == 1 or (max(hist[:-1]) > 0 and _rs_differs(c, "oldest")), c.name


@pytest.mark.parametrize("width", [1, 2])
def test_resampler_ratio_edges_reach_their_claims(width):
    cases = rc.rs_ratio_edges(width)
    assert {(c.L, c.M) for c in cases} >= {(255, 254), (255, 256), (256, 255), (256, 257), (257, 256), (257, 258), (8, 1), (1024, 128), (1, 32),
                                           (32, 1024), (1023, 1024), (1024, 1023)}
    assert {(c.L, c.T) for c in cases if c.L * c.T == 16384} == {(64, 256), (1024, 16)}
    assert sum(c.refused for c in cases) == 2
    for c in cases:
        outs, hist = _rs_common(c, 3)
        assert c.plan.whole == c.claim.whole
        assert rc.rs_tiles(sum(o.shape[1] for o in outs))[0] >= 2
        if c.claim.skip:                                     # the next output starts beyond what has arrived
            assert hist[0] == 0 and rr.outputs(5, c.L, c.M, c.T) * c.M // c.L > 5
        if not c.plan.whole:
            assert _rs_differs(c, "no_mod"), c.name


def test_resampler_shifts_reach_the_rails_and_negative_sums():
    cases = rc.rs_shifts()
    assert [c.shift for c in cases] == list(range(25))
    for c in cases:
        outs, _ = _rs_common(c)
        y = np.concatenate(outs, axis=1)
        assert (y < 0).any() and (y == -1).any() and (y > 0).any(), c.name
        if c.claim.rails:
            assert (y == 32767).any() and (y == -32768).any() and ((y > -32768) & (y < 32767)).any(), c.name
        assert _rs_differs(c, "sat_first") == (c.shift > 0), c.name
    assert sum(c.claim.rails for c in cases) == rc.RS_SHIFT_RAILS + 1


def test_resampler_history_lengths():
    cases = rc.rs_history()
    seen = {}
    for c in cases:
        outs, hist = _rs_common(c, 2)
        assert c.cuts == [c.claim.first]
        seen.setdefault((c.L, c.M, c.width), []).append(hist[0])
        if hist[0] > 0:
            assert _rs_differs(c, "oldest"), c.name
    for width in (1, 2):
        assert seen[(1, 12, width)] == list(range(9))        # every carried length 0 ... T - 1
        assert seen[(3, 2, width)] == [8] * 12             # interpolating: always T - 1, whatever the length


@pytest.mark.parametrize("width", [1, 2])
def test_resampler_tile_edges_in_lane_order(width):
    L, M, T = 441, 512, 24
    assert 255 * M // L + T == 320 and 511 * M // L + T == 617
    assert [rr.outputs(n, L, M, T) for n in (319, 320, 321, 616, 617, 618)] == [255, 256, 257, 511, 512, 513]
    cases = rc.rs_tile_edges(width)
    assert len(cases) == 12
    for c in cases:
        outs, _ = _rs_common(c, 2)
        assert not c.plan.whole and outs[0].shape[1] == rr.outputs(c.claim.first, L, M, T)
        assert rc.rs_tiles(outs[0].shape[1]) == {319: (1, True), 320: (1, False), 321: (2, True), 616: (2, True), 617: (2, False),
                                                  618: (3, True)}[c.claim.first]
        assert _rs_differs(c, "no_mod")


def test_resampler_many_rows_and_alignment_shapes():
    c = rc.rs_many_rows()
    assert (c.rows, c.width, c.x.shape[1]) == (40000, 2, 40) and rc.rs_pieces(c) == [(0, 25, False), (25, 40, False)]
    rows = rc.sampled_rows(np.random.default_rng(c.seed), c.rows)
    assert len(set(rows)) == 16 and set(rows) >= {0, 32767, 32768, 39999}
    for width in (1, 2):
        a = rc.rs_align(width)
        outs, hist = _rs_common(a, 2)
        assert hist[0] == 6 and a.T == 7 and outs[0].shape[1] > 256 and outs[1].shape[1] > 256


# ---------------------------------------------------------------------------------------------------------------------------------
# AGC

class AgWrong(ar.Agc):
    """The definition with one fault, over calls walked in segments of agc_plan's sb blocks.  `seg_ramp`: the first block of a
    call's second and later segments ramps from its own G instead of the block before's.  `seg_peak`: that block forgets its own
    peak, which was the look-ahead peak of the segment before.  `short_hist`: at most P - 1 carried samples are kept; the older ones
    read as zero.  `hang_call`: the hang counter steps once per call instead of once per block."""

    def __init__(self, cfg, wrong):
        super().__init__(cfg)
        self.wrong = wrong

    def push(self, x):
        x = np.asarray(x, dtype=np.int16)
        c, P, wrong = self.cfg, self.P, self.wrong
        sb = rc.agc_plan(P, x.shape[2])[1]
        hist = self.hist
        if wrong == "short_hist" and hist is not None and hist.shape[1] > P - 1:
            hist = hist.copy()
            hist[:, :hist.shape[1] - (P - 1)] = 0
        virt = x if hist is None else np.concatenate([hist, x], axis=1)
        B0, self.N = ar.outputs(self.N, P) // P, self.N + x.shape[1]
        nb = ar.outputs(self.N, P) // P - B0
        if self.G is None:
            self.G, self.h = np.full(x.shape[0], c.gain_max, np.int64), np.zeros(x.shape[0], np.int64)
        v = virt.astype(np.int64)
        p = np.abs(v[:, :(nb + 1) * P]).reshape(x.shape[0], nb + 1, P * x.shape[2]).max(axis=2) if nb else None
        Gs = np.empty((x.shape[0], nb + 1), np.int64)
        Gs[:, 0] = self.G
        for k in range(nb):
            G, h = self.G, self.h
            own = p[:, k] * (0 if wrong == "seg_peak" and k and k % sb == 0 else 1)
            e = np.maximum(own, p[:, k + 1])
            d = np.minimum(c.gain_max, (c.target * 1024) // np.maximum(e, 1))
            live = e > 0
            attack = live & (d <= G)
            hang = live & ~attack & (h > 0)
            release = live & ~attack & ~hang
            up = np.minimum(d, G + np.maximum(1, ((d - G) * c.decay) >> 8))
            self.G = np.where(attack, d, np.where(release, up, G))
            self.h = np.where(attack, c.hang, np.where(hang & (wrong != "hang_call" or k == 0), h - 1, h))
            Gs[:, k + 1] = self.G
        if nb and B0 == 0:
            Gs[:, 0] = Gs[:, 1]
        prev = Gs[:, :-1].copy()
        if wrong == "seg_ramp":
            for k in range(sb, nb, sb):
                prev[:, k] = Gs[:, k + 1]
        r1 = np.arange(1, P + 1, dtype=np.int64)
        g = prev[:, :, None] + (((Gs[:, 1:] - prev)[:, :, None] * r1) >> self.lg)
        prod = v[:, :nb * P] * g.reshape(x.shape[0], nb * P)[:, :, None]
        self.hist = virt[:, nb * P:].copy()
        return (prod >> 10).astype(np.int16)


def _ag_run(c, ref=None):
    """The case through a reference call by call: (outputs, (G, h) of every row) per call, and the history lengths."""
    ref = ar.Agc(c.cfg) if ref is None else ref
    res, hist = [], []
    for lo, hi, _ in rc.ag_pieces(c):
        y = ref.push(c.x[:, lo:hi]) if hi > lo else np.zeros((c.rows, 0, c.width), np.int16)
        res.append((y, [ref.gain(r) for r in range(c.rows)]))
        hist.append(ref.history())
    return res, hist


def _ag_differs(c, wrong):
    good, _ = _ag_run(c)
    bad, _ = _ag_run(c, AgWrong(c.cfg, wrong))
    return any(not np.array_equal(a[0], b[0]) or a[1] != b[1] for a, b in zip(good, bad))


def _ag_common(c):
    res, hist = _ag_run(c)
    y = np.concatenate([r[0] for r in res], axis=1)
    assert np.array_equal(y, ar.agc_all(c.x, c.cfg)), c.name
    assert [r[0].shape[1] // c.cfg.block for r in res] == [e for _, _, e in rc.ag_pieces(c)]
    return res, hist, y


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("P", rc.AG_P)
def test_agc_cells_reach_their_segments(P, width):
    sb = rc.agc_plan(P, width)[1]
    one, cut = rc.ag_cells(P, width)
    assert one.x.shape[1] <= 29000 and cut.x.shape[1] <= 29000 and one.rows == cut.rows == 2
    res, _, y = _ag_common(one)
    assert [r[0].shape[1] // P for r in res] == one.claim.emits == [2 * sb + 2]
    assert rc.agc_segments(2 * sb + 2, sb) == ((3, 2) if sb > 2 else (4, 1))      # three segments, the last one short
    res, hist, _ = _ag_common(cut)
    assert [r[0].shape[1] // P for r in res] == cut.claim.emits == [sb - 1, sb, sb + 1, 1, 0]
    assert [rc.agc_segments(e, sb)[0] for e in cut.claim.emits[:4]] == [1 if sb > 1 else 0, 1, 2, 1]
    assert hist[0] == P + 5 and all(P <= h < 2 * P for h in hist)
    assert (one.claim.at, cut.claim.at) == (sb, 3 * sb - 1)  # a later segment's first block: in the one call, in the third call
    for c in (one, cut):                                     # full scale with -32768, a level of 3, a silent block
        k = c.claim.at
        assert c.x.min() == -32768 and not c.x[1, (k + 2) * P:(k + 3) * P].any()
        assert np.abs(c.x[1, (k - 1) * P:k * P].astype(np.int64)).max() == 3
        for wrong in ("seg_ramp", "seg_peak"):
            assert _ag_differs(c, wrong), (c.name, wrong)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("P", [32, 512])
def test_agc_carried_history_lengths(P, width):
    cases = rc.ag_history(P, width)
    hs = [c.claim.h for c in cases]
    chunk = 8 // width                                       # samples of a 16-byte chunk
    assert set(hs) >= {0, P - 1, P, P + 1, 2 * P - 1}
    assert {h % chunk for h in hs if h < P} == {h % chunk for h in hs if h >= P} == set(range(chunk))
    for c in cases:
        res, hist, _ = _ag_common(c)
        assert hist[0] == c.claim.h and res[0][0].shape[1] == 0 and res[1][0].shape[1] >= 2 * P
        assert _ag_differs(c, "short_hist") == (c.claim.h >= P), c.name


@pytest.mark.parametrize("P", [32, 2048])
def test_agc_corners_stay_under_the_target(P):
    cases = rc.ag_corners(P)
    assert {(c.cfg.target, c.cfg.gain_max) for c in cases} == {(1, 1), (1, 262144), (32767, 1), (32767, 262144)}
    assert {(c.cfg.hang, c.cfg.decay, c.width) for c in cases} == {(h, d, w) for h in (0, 1, 65535) for d in (1, 255, 256) for w in (1, 2)}
    assert len(cases) == len({c.cfg + (c.width,) for c in cases}) == 72
    moved = 0
    for c in cases:
        _, _, y = _ag_common(c)
        assert c.x.min() == -32768 and np.abs(y.astype(np.int64)).max() <= c.claim.target == c.cfg.target
        if c.cfg.hang == 1 and c.cfg.gain_max > 1:
            assert _ag_differs(c, "hang_call"), c.name
            moved += 1
    assert moved == 12


def test_agc_many_rows_and_alignment_shapes():
    c = rc.ag_many_rows()
    assert (c.rows, c.width, c.cfg.block) == (40000, 1, 16) and [e for _, _, e in rc.ag_pieces(c)] == c.claim.emits == [1, 4]
    for P in (16, 64):
        for width in (1, 2):
            a = rc.ag_align(P, width)
            res, hist, _ = _ag_common(a)
            assert [r[0].shape[1] for r in res] == [3 * P, 3 * P] and hist[0] == P + 3


# ---------------------------------------------------------------------------------------------------------------------------------
# tone squelch

class TqWrong(tr.ToneSquelch):
    """The definition with one fault.  ("rows", k, w): wave w does not run its tone rows 8 w + 32 k ... + 7, so their sums stay
    zero.  `tie_high`: of equal powers the larger index wins.  `stale`: a call's last, partial chunk of 64 is not cleared, so the
    samples of the chunk before it, where the call had one, are added again at the positions the call did not reach.  `ramp`: the
    gate ramps with r instead of min(r, Q - 1)."""

    def __init__(self, tab, cfg, wrong):
        super().__init__(tab, cfg)
        self.wrong = wrong

    def _decide(self, W):
        if self.wrong != "tie_high":
            return tr.decide(W, self.cfg)
        fs = max(range(len(W)), key=lambda f: (W[f], f))
        rest = max([W[f] for f in range(len(W)) if abs(f - fs) > self.cfg.guard], default=0)
        return (fs if W[fs] >= self.cfg.min_power and (W[fs] >> self.cfg.dom_shift) >= rest else tr.NONE), fs, W[fs]

    def push(self, x):
        x = np.asarray(x, dtype=np.int16)
        rows, n, _ = x.shape
        self._start(rows)
        xi = x.astype(np.int64)
        m = tr.mono(xi).astype(np.float64)
        out = np.empty_like(xi)
        start, lo = self.N, 0
        lg = self.cfg.ramp.bit_length() - 1
        dead = range(0)
        if isinstance(self.wrong, tuple):
            _, k, w = self.wrong
            assert rc.tq_nj(self.F)[w] > k                   # the wave the plan says should run them
            dead = range(8 * w + 32 * k, min(2 * self.F, 8 * w + 32 * k + 8))
        while lo < n:
            r0 = self.N % self.P
            hi = min(n, lo + self.P - r0)
            r = np.arange(r0, r0 + hi - lo, dtype=np.int64)
            if self.wrong == "ramp":
                g = self.sp[:, None] + (((self.sc - self.sp)[:, None] * (r[None, :] + 1)) >> lg)
            else:
                g = self.sp[:, None] + tr.gains(0, (self.sc - self.sp)[:, None], r[None, :], self.cfg)
            out[:, lo:hi] = (xi[:, lo:hi] * g[:, :, None]) >> 8
            self.sums += (m[:, lo:hi] @ self.mat[r0:r0 + hi - lo]).astype(np.int64)
            self.N += hi - lo
            lo = hi
            if self.N % self.P == 0:
                for row in range(rows):
                    ab = [0 if q in dead else int(v) >> 14 for q, v in enumerate(self.sums[row])]
                    W = [ab[2 * f] ** 2 + ab[2 * f + 1] ** 2 for f in range(self.F)]
                    hit, _, w_ = self._decide(W)
                    self.state[row], s = tr.step(self.state[row], hit, self.cfg)
                    self.sp[row], self.sc[row] = self.sc[row], s
                    self.power[row] = w_
                    self.hits.append((self.N // self.P - 1, row, hit))
                self.sums[:] = 0
        c0 = self.N - self.N % 64
        if self.wrong == "stale" and self.N % 64 and c0 - 64 >= start - 63:
            pos = np.arange(self.N, c0 + 64)
            pos = pos[pos - 64 >= start]
            self.sums += (m[:, pos - 64 - start] @ self.mat[pos % self.P]).astype(np.int64)
        return out.astype(np.int16)


def _tq_run(c, ref=None):
    """The case through a reference call by call: (outputs, status) per call, and the reference."""
    ref = tr.ToneSquelch(c.tab, c.cfg) if ref is None else ref
    res, lo = [], 0
    for n in c.cuts + [c.x.shape[1]]:
        hi = min(c.x.shape[1], lo + n)
        res.append((ref.push(c.x[:, lo:hi]), ref.status()))
        lo = hi
    return res, ref


def _tq_differs(c, wrong):
    good, _ = _tq_run(c)
    bad, _ = _tq_run(c, TqWrong(c.tab, c.cfg, wrong))
    return any(not np.array_equal(a[0], b[0]) or a[1] != b[1] for a, b in zip(good, bad))


def _tq_common(c):
    res, ref = _tq_run(c)
    y = np.concatenate([r[0] for r in res], axis=1)
    assert np.array_equal(y, tr.tonesq_all(c.x, c.tab, c.cfg)), c.name
    return res, ref, y


def test_sine_table_separates_64_tones_at_a_block_of_64():
    """A row that carries tone f alone (16 x its cosine row, no noise) leaves every other tone below half of tone f's power, with
    room for the family's noise; the Hann-windowed designer of the product does not, at the same frequencies."""
    t = rc.sine_table(64).astype(np.int64)
    assert np.abs(t).max() == 1023 and t.shape == (64, 64, 2)

    def worst(tab):
        m = 16 * tab[:, :, 0]
        W = ((m @ tab[:, :, 0].T) >> 14) ** 2 + ((m @ tab[:, :, 1].T) >> 14) ** 2
        rival = W - np.diag(np.diag(W))
        return (rival.max(axis=1) / np.diag(W)).max()
    assert worst(t) < 0.42
    r = np.arange(64)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * (r + 0.5) / 64)
    a = 2 * np.pi * (0.25 + 0.5 * np.arange(64))[:, None] * r[None, :] / 64
    assert worst(np.stack([np.rint(1023 * hann * np.cos(a)), np.rint(-1023 * hann * np.sin(a))], axis=2).astype(np.int64)) > 0.5


@pytest.mark.parametrize("lo", [1, 17, 33, 49])
def test_tone_squelch_every_tone_wins_in_turn(lo):
    for F in range(lo, lo + 16):
        c = rc.tq_each_tone(F)
        assert (c.F, c.cfg.block, c.rows, c.width, c.x.shape[1]) == (F, 64, F + 1, 2 - F % 2, 4 * 64 + 37)
        assert c.cuts == [213] and 213 // 64 == 3 and 213 % 64 and c.claim.nj == rc.tq_nj(F)
        assert (c.cfg.guard, c.cfg.dom_shift, c.cfg.confirm) == (0, 1, 1) and c.cfg.accept & 3 == 1 and c.cfg.accept == (c.cfg.accept << 2 | 1) & rc.ALL
        res, ref, y = _tq_common(c)
        assert len(ref.hits) == 4 * (F + 1)
        assert all(hit == (row if row < F else tr.NONE) for _, row, hit in ref.hits), c.name
        tone, power, gate = res[-1][1]
        assert tone == list(range(F)) + [tr.NONE] and gate == [f % 2 == 0 for f in range(F)] + [False] and min(power[:F]) > 10 ** 8
        assert _tq_differs(c, "stale"), c.name
        if F > 1:
            assert np.abs(c.x[:F, :, 0].astype(np.int64)).max() > 16000 and not c.x[F].any()


def test_tone_squelch_a_wave_that_drops_a_group_is_told_apart():
    """For every group k = 1, 2, 3 and wave w: at the smallest F at which the plan gives wave w that group, at the next F, and at
    F = 64, the variant in which the wave does not run it differs from the definition on the every-tone family."""
    n = 0
    for k in (1, 2, 3):
        for w in range(4):
            first = min(F for F in range(1, 65) if rc.tq_nj(F)[w] > k)
            assert first == 16 * k + 4 * w + 1 and rc.tq_nj(first - 1)[w] == k
            for F in sorted({first, first + 1, 64}):
                assert _tq_differs(rc.tq_each_tone(F), ("rows", k, w)), (k, w, F)
                n += 1
    assert n >= 33


@pytest.mark.parametrize("P,F", rc.TQ_PS)
def test_tone_squelch_p_sweep(P, F):
    c = rc.tq_p_sweep(P, F)
    assert (c.rows, c.cfg.block, c.F) == (33, P, F) and 2 * P < c.x.shape[1] < 3 * P and c.cuts == [7, P + 1]
    res, ref, y = _tq_common(c)
    assert len(ref.hits) == 2 * 33 and len({h for _, _, h in ref.hits}) > 1
    assert not y[:, :P].any() and c.x.min() == -32768            # closed before the first decision
    opened = {row for b, row, h in ref.hits if b == 0 and h != tr.NONE and (c.cfg.accept >> h) & 1}
    assert opened and all(y[row, P:2 * P].any() for row in opened if c.x[row, P + 64:2 * P].any())


def test_tone_squelch_p_sweep_covers_both_corners():
    assert (32, 8192) in [(F, P) for P, F in rc.TQ_PS] and all(F * P <= 262144 for P, F in rc.TQ_PS) and 32 * 8192 == 262144
    assert {rc.tq_p_sweep(P, F).width for P, F in rc.TQ_PS} == {1, 2}


def test_tone_squelch_ramps_open_and_close():
    cases = rc.tq_ramps()
    assert [c.claim.Q for c in cases] == [1 << i for i in range(9)] and {c.width for c in cases} == {1, 2}
    for c in cases:
        P, Q = 256, c.claim.Q
        res, ref, y = _tq_common(c)
        assert c.cfg.ramp == Q
        assert [h for b, row, h in ref.hits if row == 0] == [0, 0, tr.NONE, tr.NONE, tr.NONE]
        # closed, ramping up, open, ramping down, closed
        assert not y[:, :P].any() and np.array_equal(y[0::2, P + Q - 1:3 * P], c.x[0::2, P + Q - 1:3 * P]) and y[0, P + Q:3 * P].all()
        assert not y[:, 3 * P + Q - 1:].any() and not y[1::2].any()
        if Q > 2:
            assert not np.array_equal(y[0, P:P + Q - 1], c.x[0, P:P + Q - 1]) and y[0, 3 * P:3 * P + Q - 2].any()
        assert _tq_differs(c, "ramp") == (Q < P), c.name


def test_tone_squelch_row_counts_and_many_rows():
    for rows in (31, 32, 33, 64, 65):
        c = rc.tq_rows(rows)
        res, ref, y = _tq_common(c)
        assert c.rows == rows and len(ref.hits) == 3 * rows and y.any()
    c = rc.tq_many_rows()
    assert (c.rows, c.F, c.cfg.block, c.x.shape[1], c.width, c.cuts) == (40000, 2, 64, 130, 1, [70])
    for width in (1, 2):
        a = rc.tq_align(width)
        assert a.cuts == [21, 100] and a.x.shape[1] == 151 and 21 % 64 and 121 % 64 and 21 < 64 < 121 < 128 < 151
        assert _tq_differs(a, "stale")


@pytest.mark.parametrize("guard,dom", rc.TQ_INTERIOR)
def test_tone_squelch_decision_interior(guard, dom):
    c = rc.tq_interior(guard, dom)
    res, ref, y = _tq_common(c)
    exp = c.claim.expect
    assert len(exp) == c.rows == 13 and {e.fs for e in exp if not e.tie and e.W} == {0, 13, 31}
    assert sorted(e.rel for e in exp if not e.tie and e.W) == [-1] * 3 + [0] * 3 + [1] * 3
    tab = c.tab.astype(np.int64)
    for row, e in enumerate(exp):
        m = tr.mono(c.x[row, :64].astype(np.int64))
        W = [int((tab[f, :, 0] @ m) >> 14) ** 2 + int((tab[f, :, 1] @ m) >> 14) ** 2 for f in range(c.F)]
        hit, fs, w = tr.decide(W, c.cfg)
        assert (hit, w) == (e.hit, e.W) and all(h == e.hit for _, r, h in ref.hits if r == row), (row, e)
        if e.W and not e.tie:
            rest = max(W[f] for f in range(c.F) if abs(f - fs) > guard)
            near = [W[f] for f in range(c.F) if abs(f - fs) == guard and W[f]]
            assert fs == e.fs and rest == e.rest and (w >> dom) - rest == e.rel          # one below, at, one above
            assert len(near) == 1 and (w >> dom) < near[0] < w                          # the runner-up at distance guard would refuse it
            assert [f for f in range(c.F) if W[f] == rest] == [fs + (guard + 1) * (1 if fs + guard + 1 < c.F else -1)]
        if e.tie:
            assert sorted(f for f in range(c.F) if W[f] == w) == [e.fs, e.fs + guard] and hit == e.fs
    assert len(ref.hits) == 3 * 13
    assert _tq_differs(c, "tie_high")
