"""Case generators of the *_domain GPU tests of the three int16 row processors -- the rational resampler, the AGC and the tone
squelch -- in plain numpy, with test-side copies of their launch plans written from DESIGN.md (9j, 9k, 9l) and the kernel headers'
prose, so that a case can say which kernel path it reaches.  tests/test_rows_cases.py runs the cases against the references alone
(tests/resample_ref.py, tests/agc_ref.py, tests/tonesq_ref.py) and asserts what each case claims; the GPU files feed the same cases
to the handles.  Every case carries its seed, its calls (`cuts`: the lengths of the pieces; the rest of the stream follows them) and
what it claims to reach.  FMD_FUZZ_SEED moves every seed; what a case claims is built into it and does not hang on the draw."""
import os
from collections import namedtuple
from types import SimpleNamespace as NS

import numpy as np

import agc_ref as ar
import resample_ref as rr
import tonesq_ref as tr

ALL = (1 << 64) - 1
SAMPLED = 16                                                       # rows compared in the many-rows cases


def seed(offset):
    return int(os.environ.get("FMD_FUZZ_SEED", "20260101")) + offset


def sampled_rows(rng, rows):
    """16 rows of a many-rows case: the first, the two around 2^15, the last, and 12 drawn ones."""
    fixed = [0, 32767, 32768, rows - 1]
    return fixed + sorted(int(r) for r in rng.choice(np.setdiff1d(np.arange(rows), fixed), SAMPLED - len(fixed), replace=False))


# ---------------------------------------------------------------------------------------------------------------------------------
# the plans

RsPlan = namedtuple("RsPlan", "tile whole npair tdw plane_len lds")
RS_BUDGET, RS_SLACK, RS_TILE = 61440, 32, 256


def rs_plan(L, M, T, width):
    """The resampler's tile plan: taps are held as dwords of two, every phase padded to an ODD number of dwords; a
    plane holds the tile's input span -- the last output of the tile starts ceil((tile - 1) M / L) samples behind the first and reads
    T -- plus 32 samples of slack, rounded up to a multiple of 8; the table is whole in LDS when L <= tile, else the tile's own
    phases, one per lane.  The tile is the largest power of two <= 256 whose planes and taps fit 60 KiB; 32 is taken as it is."""
    npair = -(-T // 2)
    tdw = npair if npair % 2 else npair + 1
    tile = RS_TILE
    while True:
        span = -(-(tile - 1) * M // L) + T
        plane_len = -(-(span + RS_SLACK) // 8) * 8
        whole = L <= tile
        lds = width * plane_len * 2 + (L if whole else tile) * tdw * 4
        if lds <= RS_BUDGET or tile == 32:
            return RsPlan(tile, whole, npair, tdw, plane_len, lds)
        tile //= 2


def rs_domain_ok(L, M, T):
    return 1 <= L <= 1024 and 1 <= M <= 1024 and M <= 32 * L and L <= 8 * M and 1 <= T <= 256 and L * T <= 16384


def rs_tiles(n_out, tile=RS_TILE):
    """(tiles of a call of n_out outputs, whether the last one is partial)"""
    return -(-n_out // tile), n_out % tile != 0


def agc_plan(P, width):
    """(ring, sb) of the AGC: the ring holds 16 KiB of samples, or two blocks where they are larger, and a segment
    emits one block less than the ring holds."""
    ring = max(16384, 2 * P * 2 * width) // (2 * width)
    return ring, ring // P - 1


def agc_segments(nb, sb):
    """(segments of a call that emits nb blocks, the blocks of the last one)"""
    segs = -(-nb // sb)
    return segs, nb - (segs - 1) * sb


def tq_nj(F):
    """The tone-row groups each of the four waves runs: thread (qg = tid >> 3) owns the tone rows qg + 32 j, a wave's
    smallest qg is 8 w, and it runs the j with 8 w + 32 j < 2 F."""
    return tuple(min(4, max(0, -(-(2 * F - 8 * w) // 32))) for w in range(4))


# ---------------------------------------------------------------------------------------------------------------------------------
# resampler

def taps(rng, L, T, mag=32767):
    """random taps of both signs, every phase with sum |g| <= mag and one phase with exactly mag"""
    g = rng.integers(-(mag // T), mag // T + 1, (L, T))
    p = int(rng.integers(0, L))
    g[p, 0] += (mag - np.abs(g[p]).sum()) * (1 if g[p, 0] >= 0 else -1)
    assert np.abs(g).sum(axis=1).max() == mag
    return g.astype(np.int16)


def _rs_case(name, sd, L, M, T, width, rows, N, cuts, shift=None, refused=0, g=None, x=None, **claim):
    assert rs_domain_ok(L, M, T), name
    rng = np.random.default_rng(seed(sd))
    g = taps(rng, L, T) if g is None else g
    shift = int(rng.integers(12, 17)) if shift is None else shift
    x = rng.integers(-32768, 32768, (rows, N, width)).astype(np.int16) if x is None else x
    return NS(name=name, seed=seed(sd), L=L, M=M, T=T, width=width, rows=rows, g=g, shift=shift, x=x, cuts=list(cuts), refused=refused,
              plan=rs_plan(L, M, T, width), claim=NS(**claim))


def rs_pieces(c):
    """The case's calls as the reference takes them: (lo, hi, refused) per handed-over piece; a refused piece is handed over again
    in front of the next one."""
    out, lo, pos = [], 0, 0
    for n in c.cuts + [c.x.shape[1]]:
        pos = min(c.x.shape[1], pos + n)
        if pos == lo:
            continue
        o0, o1 = rr.outputs(lo, c.L, c.M, c.T), rr.outputs(pos, c.L, c.M, c.T)
        out.append((lo, pos, o1 == o0))
        if o1 > o0:
            lo = pos
    return out


RS_T = (1, 2, 3, 5, 7, 31, 33, 63, 65, 127, 255, 256)


def rs_t_sweep(width):
    """Every T of RS_T at the whole-table ratio 3 / 4 and, for T <= 63 (L T <= 16384), at the lane-order ratio 257 / 256: 3 rows,
    two tiles, the cuts T + 40 | 150 | 77 | rest.  An odd T > 1 ends on a tap pair of one tap and a padding zero."""
    out = []
    for L, M in ((3, 4), (257, 256)):
        for T in RS_T:
            if L * T > 16384:
                continue
            N = T + 500
            out.append(_rs_case("T%d-%d/%d-w%d" % (T, L, M, width), 1000 * L + 10 * T + width, L, M, T, width, 3, N, [T + 40, 150, 77],
                                odd_pair=T % 2 == 1 and T > 1, whole=L <= 256))
    return out


RS_RATIOS = [(255, 254, 9), (255, 256, 9), (256, 255, 9), (256, 257, 9), (257, 256, 9), (257, 258, 9),     # L around the tile
             (8, 1, 16), (1024, 128, 16),                                                                  # L = 8 M
             (1, 32, 1), (1, 32, 40), (32, 1024, 1), (32, 1024, 40),                                       # M = 32 L
             (64, 63, 256), (1024, 999, 16),                                                               # L T = 16384
             (1023, 1024, 16), (1024, 1023, 16)]


def rs_ratio_edges(width):
    """The ratios at the domain's edges, 2 rows, more than one tile each, cut T + 8 | a third of the rest | a third | rest.  Where
    M = 32 L the pieces are 5 | 2 M / L + T | 5 M / L | rest: at T = 1 the first piece completes output 0 and the next output starts
    beyond what has arrived (skip-ahead); at T = 40 it completes nothing and is the one refused call."""
    out = []
    for L, M, T in RS_RATIOS:
        n_out = 300 if M > L else 520
        N = n_out * M // L + T
        deep = M == 32 * L
        cuts = [5, 2 * M // L + T, 5 * M // L] if deep else [T + 8, (N - T - 8) // 3, (N - T - 8) // 3]
        out.append(_rs_case("%d/%d-T%d-w%d" % (L, M, T, width), 7000 + 3 * L + 5 * M + T + width, L, M, T, width, 2, N, cuts,
                            refused=1 if deep and T == 40 else 0, whole=L <= 256, skip=deep and T == 1))
    return out


RS_SHIFT_RAILS = 12                                                # shifts up to here reach both rails


def rs_shifts():
    """Every shift 0 ... 24 at 3 / 2, T = 4, width 2, on phases with sum |g| = 32767: full-scale runs of both signs drive |v| to
    32767 * 32768 (the rails at every shift <= 15, claimed up to 12), and samples of -1 under positive taps give sums in [-2^shift,
    0) whose arithmetic shift is -1 at every shift."""
    g = np.array([[32767, 0, 0, 0], [16384, -16383, 0, 0], [-8192, 8192, -8192, 8191]], np.int16)
    out = []
    for shift in range(25):
        rng = np.random.default_rng(seed(300 + shift))
        x = rng.choice(np.array([-32768, 32767, -32768, 32767, 5, -1], np.int16), (2, 700, 2))
        x[0, :40] = -32768
        x[0, 40:80:2] = 32767
        x[1, 100:140] = -1
        out.append(_rs_case("shift%d" % shift, 300 + shift, 3, 2, 4, 2, 2, 700, [50, 300, 101], shift=shift, g=g, x=x,
                            rails=shift <= RS_SHIFT_RAILS))
    return out


def rs_align(width):
    """The shape of the alignment matrix: 15 / 16 at T = 7, 3 rows, a first call and a second one that carries history."""
    return _rs_case("align-w%d" % width, 400 + width, 15, 16, 7, width, 3, 700, [333], shift=13)


def rs_history():
    """T = 9: at 3 / 2 a first call of every length 9 ... 20 and then the rest (interpolating, the next output starts at most one
    sample behind the last one, so the carried history is T - 1 = 8 samples whatever the length); at 1 / 12 the lengths 12 ... 20, which
    leave h = 0 ... 8 in turn, and then the rest."""
    out = []
    for L, M, lens in ((3, 2, range(9, 21)), (1, 12, range(12, 21))):
        for n in lens:
            for width in (1, 2):
                out.append(_rs_case("hist-%d/%d-n%d-w%d" % (L, M, n, width), 500 + L, L, M, 9, width, 2, 400 if L == 3 else 4000, [n],
                                    shift=14, first=n))
    return out


def rs_tile_edges(width):
    """441 / 512 at T = 24, the lane-order path: output 255 reads x[296 ... 319] and output 511 x[593 ... 616]; first calls of 319,
    320, 321, 616, 617 and 618 samples end one input before, on and one after them; then the rest."""
    return [_rs_case("tile-n%d-r%d-w%d" % (n, rows, width), 600 + width, 441, 512, 24, width, rows, 1200, [n], shift=14, first=n)
            for rows in (2, 3) for n in (319, 320, 321, 616, 617, 618)]


def rs_many_rows():
    """40000 rows of 40 inputs at width 2, 3 / 4 at T = 8, cut 25 | 15."""
    return _rs_case("many", 700, 3, 4, 8, 2, 40000, 40, [25], shift=14)


# ---------------------------------------------------------------------------------------------------------------------------------
# AGC

AG_P = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
AG_AMPS = [900, 0, 32768, 40, 0, 0, 32767, 3, 0, 0, 0, 0, 0, 32768, 32768, 900, 40, 3, 3, 3, 3, 40, 3, 3, 3, 3, 3, 3, 900, 0, 3, 3]


def agc_stream(rng, rows, blocks, P, width, tail, levels=(0, 3, 40, 900, 32767, 32768)):
    """ar.envelope with a given length: `blocks` blocks and `tail` samples (< P) per row."""
    x = ar.envelope(rng, rows, blocks, P, width, levels)
    keep = x[:, :blocks * P + tail]
    return np.concatenate([keep, rng.integers(-40, 41, (rows, blocks * P + tail - keep.shape[1], width)).astype(np.int16)], axis=1)


def _ag_case(name, sd, cfg, width, x, cuts, **claim):
    return NS(name=name, seed=seed(sd), cfg=ar.Cfg(*cfg), width=width, rows=x.shape[0], x=x, cuts=list(cuts), claim=NS(**claim))


def ag_pieces(c):
    """(lo, hi, blocks emitted) per call of the case"""
    P, out, lo = c.cfg.block, [], 0
    for n in c.cuts + [c.x.shape[1]]:
        hi = min(c.x.shape[1], lo + n)
        out.append((lo, hi, (ar.outputs(hi, P) - ar.outputs(lo, P)) // P))
        lo = hi
    return out


def ag_cells(P, width):
    """One (P, width) cell: a stream of 3 sb + 2 blocks and 11 samples, 2 rows.  `one`: its first 2 sb + 3 blocks in one call, which
    emits 2 sb + 2 blocks in three segments, the last of two blocks (four segments of one block where sb = 1).  `cut`: calls that
    emit sb - 1, sb, sb + 1 and 1 blocks (the first one ends 5 samples into a block), and the rest, which emits none.  Block sb is
    the second segment's first block in `one`, block 3 sb - 1 in the third call of `cut`; around each of them row 0 has the peaks
    40, 40, 32768 (the gain falls inside that block, so its ramp starts at the block before's G) and row 1 has 3, 900, 3, 0 (that
    block's own peak, the look-ahead peak of the segment before, decides its gain).  Where sb = 1 the two places overlap, and `cut`
    is a copy of the stream with the peaks around its own block.  hang is 0, so that a wrong gain shows at once."""
    sb = agc_plan(P, width)[1]
    rng = np.random.default_rng(seed(2000 + 4 * P + width))
    cfg = ar.Cfg(P, 12000, 262144, 0, 64)

    def plant(x, k):
        x[0, (k - 1) * P:(k + 2) * P] = ar.from_peaks(rng, [40, 40, 32768], P, width)
        x[1, (k - 1) * P:(k + 3) * P] = ar.from_peaks(rng, [3, 900, 3, 0], P, width)
    x = agc_stream(rng, 2, 3 * sb + 2, P, width, 11)
    plant(x, sb)
    one = _ag_case("one-P%d-w%d" % (P, width), 2000 + 4 * P + width, cfg, width, x[:, :(2 * sb + 3) * P].copy(), [], sb=sb, at=sb,
                   emits=[2 * sb + 2])
    plant(x, 3 * sb - 1)
    cut = _ag_case("cut-P%d-w%d" % (P, width), 2000 + 4 * P + width, cfg, width, x, [sb * P + 5, sb * P, (sb + 1) * P, P], sb=sb,
                   at=3 * sb - 1, emits=[sb - 1, sb, sb + 1, 1, 0])
    return one, cut


def ag_history(P, width):
    """First calls that leave h = 0 ... 8, P - 1, P, P + 1, P + 3 ... P + 10 and 2 P - 1 carried samples -- every residue class
    modulo the 16-byte chunk on both sides of P -- and then a call of 3 P + 5 samples, which emits."""
    hs = sorted(set(range(9)) | {P - 1, P, P + 1, 2 * P - 1} | set(range(P + 3, P + 11)))
    rng = np.random.default_rng(seed(2500 + P + width))
    x = agc_stream(rng, 2, 6, P, width, 4, levels=(40, 900, 32767, 32768))      # (no silent block: every carried sample counts)
    return [_ag_case("hist-P%d-w%d-h%d" % (P, width, h), 2500 + P + width, (P, 9000, 65536, 2, 128), width, x[:, :h + 3 * P + 5], [h], h=h)
            for h in hs]


def ag_align(P, width):
    """The shape of the alignment matrix: calls that emit 3 blocks each, the second with a carried history of P + 3 samples."""
    rng = np.random.default_rng(seed(2600 + P + width))
    return _ag_case("align-P%d-w%d" % (P, width), 2600 + P + width, (P, 12000, 262144, 1, 64), width, agc_stream(rng, 3, 7, P, width, 3 + P // 2),
                    [4 * P + 3], emits=[3, 3])


AG_CORNERS = [(t, g, h, d) for t in (1, 32767) for g in (1, 262144) for h in (0, 1, 65535) for d in (1, 255, 256)]


def ag_corners(P):
    """target in {1, 32767} x gain_max in {1, 262144} x hang in {0, 1, 65535} x decay in {1, 255, 256}, each at both widths: zero
    runs of 1, 2 and 5 blocks, a full-scale block (-32768 included) behind each, a long quiet stretch."""
    out = []
    for width in (1, 2):
        rng = np.random.default_rng(seed(2700 + P + width))
        x = np.stack([ar.from_peaks(rng, AG_AMPS, P, width, 5), ar.from_peaks(rng, AG_AMPS[::-1], P, width, 5)])
        for target, gain_max, hang, decay in AG_CORNERS:
            out.append(_ag_case("corner-P%d-w%d-t%d-g%d-h%d-d%d" % (P, width, target, gain_max, hang, decay), 2700 + P + width,
                                (P, target, gain_max, hang, decay), width, x, [3 * P + 1, 9 * P], target=target))
    return out


def ag_many_rows():
    """40000 rows at P = 16, width 1: 6 blocks and 7 samples, 5 blocks emitted over the cut 40 | rest."""
    rng = np.random.default_rng(seed(2800))
    x = rng.integers(-32768, 32768, (40000, 6 * 16 + 7, 1)).astype(np.int64)
    scale = np.concatenate([rng.choice([1, 64, 4096, 32768], (40000, 6)).repeat(16, axis=1), np.ones((40000, 7), np.int64)], axis=1)
    x = (x * scale[:, :, None]) >> 15                              # every block at a level of its own
    return _ag_case("many", 2800, (16, 12000, 262144, 1, 64), 1, x.astype(np.int16), [40], emits=[1, 4])


# ---------------------------------------------------------------------------------------------------------------------------------
# tone squelch

def tq_table(rng, F, P):
    t = rng.integers(-1023, 1024, (F, P, 2)).astype(np.int16)
    t[0, :2] = [[1023, -1023], [-1023, 1023]]
    return t


def tq_audio(rng, rows, n, width):
    """Rows at different levels, full scale among them, with -32768 and a silent stretch."""
    x = rng.integers(-32768, 32768, (rows, n, width)).astype(np.int64)
    x = (x * rng.choice([1, 64, 4096, 32768], (rows, 1, 1))) >> 15
    x[:, n // 3] = -32768
    x[rows // 2, n // 2:n // 2 + n // 5] = 0
    return x.astype(np.int16)


def tq_loose(P, rng):
    """A configuration under which noise opens and closes the gate: any strongest tone is a hit, about half of the tones open."""
    return tr.Cfg(P, 0, 0, 1, int(rng.integers(0, 2)), min(P, 64), 1, int(rng.integers(1, 1 << 62)) | 1)


def _tq_case(name, sd, tab, cfg, width, x, cuts, **claim):
    return NS(name=name, seed=seed(sd), tab=tab, cfg=tr.Cfg(*cfg), width=width, rows=x.shape[0], x=x, cuts=list(cuts), F=tab.shape[0],
              claim=NS(**claim))


def sine_table(F, P=64):
    """The test-side designer for the every-tone family: tone f is an un-windowed sinusoid of 0.25 + 0.5 f cycles per block,
    (c_f[r], s_f[r]) = rint(1023 cos(a)), rint(-1023 sin(a)) with a = 2 pi (0.25 + 0.5 f) r / P.  At P = 64 the 64 tones lie half a
    cycle per block apart and are not orthogonal, but a row that carries tone f leaves the strongest other tone at 0.39 of the
    winner's power, below the 0.5 that dom_shift = 1 allows, so every tone wins on its own row.  fmd.tone_table's Hann-windowed rows
    do not separate 64 tones at P = 64: the window's main lobe covers the neighbouring tones."""
    a = 2 * np.pi * (0.25 + 0.5 * np.arange(F))[:, None] * np.arange(P)[None, :] / P
    return np.stack([np.rint(1023 * np.cos(a)), np.rint(-1023 * np.sin(a))], axis=2).astype(np.int16)


TQ_EACH_ACCEPT = 0x5555555555555555


def tq_each_tone(F):
    """F tones at P = 64, width 1 for odd F and 2 for even F, F + 1 rows: row f carries 16 x the table's cosine row f (half scale)
    plus noise within +-8, the same in both components; the last row is silent.  guard 0, dom_shift 1, confirm 1, accept the even
    tones.  4 blocks and 37 samples in two calls cut at 213, inside a chunk of the last whole block, whose power status() reports
    behind the second call: sums that the first call's partial chunk left wrong show there.  Every completed block's hit of row f is f."""
    P, width = 64, 2 - F % 2
    rng = np.random.default_rng(seed(3000 + F))
    tab = sine_table(F, P)
    n = 4 * P + 37
    x = np.zeros((F + 1, n, width), np.int64)
    reps = -(-n // P)
    x[:F] = (16 * np.tile(tab[:, :, 0].astype(np.int64), (1, reps))[:, :n] + rng.integers(-8, 9, (F, n)))[:, :, None]
    return _tq_case("each-F%d" % F, 3000 + F, tab, (P, 0, 1, 1, 0, 8, 1, TQ_EACH_ACCEPT), width, x.astype(np.int16), [3 * P + 21], nj=tq_nj(F))


TQ_PS = [(P, F) for P in (128, 512, 1024, 2048, 8192) for F in (3, 32)]


def tq_p_sweep(P, F):
    """Random tables and rows, 33 rows, 2 blocks and a remainder, cut 7 | P + 1 | rest; the widths in turn."""
    assert F * P <= 262144
    rng = np.random.default_rng(seed(3100 + P + F))
    i = TQ_PS.index((P, F))
    width = 1 + (i // 2 + i) % 2
    return _tq_case("P%d-F%d" % (P, F), 3100 + P + F, tq_table(rng, F, P), tq_loose(P, rng), width,
                    tq_audio(rng, 33, 2 * P + int(rng.integers(1, P)), width), [7, P + 1])


def tq_open_close(rng, rows, P, width, n):
    """One tone row of all +1023: every second row carries a positive signal in blocks 0 and 1 and a zero-mean one behind them, so
    those rows come out closed, ramping up, open, ramping down and closed."""
    tab = np.zeros((1, P, 2), np.int16)
    tab[0, :, 0] = 1023
    x = np.zeros((rows, n, width), np.int16)
    k = (rows + 1) // 2
    sig = rng.integers(1, 32768, (k, n, width)).astype(np.int16)
    sig[:, 2 * P:] = 0
    sig[:, 2 * P:, 0] = np.where(np.arange(n - 2 * P) % 2 == 0, 12345, -12345)
    if width == 2:
        sig[:, 2 * P:, 1] = sig[:, 2 * P:, 0]
    x[0::2] = sig
    return tab, x


def tq_ramps():
    """Every ramp 1, 2, 4 ... 256 at P = 256 on the open / close signal, 5 rows, the widths in turn, cut Q / 2 samples into the rising
    ramp and 3 + Q / 2 samples into the block of the falling one."""
    out = []
    for i in range(9):
        Q, width = 1 << i, 1 + i % 2
        rng = np.random.default_rng(seed(3200 + i))
        tab, x = tq_open_close(rng, 5, 256, width, 5 * 256 + 9)
        out.append(_tq_case("ramp%d" % Q, 3200 + i, tab, (256, 0, 0, 1, 0, Q, 1, 1), width, x, [256 + max(1, Q // 2), 2 * 256 + 3], Q=Q))
    return out


def tq_rows(rows):
    """31, 32, 33, 64 and 65 rows, the edges of the tile of 32: F = 3, P = 64, random table and rows, 3 blocks and 21 samples."""
    rng = np.random.default_rng(seed(3300 + rows))
    width = 1 + rows % 2
    return _tq_case("rows%d" % rows, 3300 + rows, tq_table(rng, 3, 64), tq_loose(64, rng), width, tq_audio(rng, rows, 3 * 64 + 21, width), [50])


def tq_align(width):
    """The shape of the alignment matrix: F = 5, P = 64, 3 rows; a first call of 21 samples, then the call under test, 100 samples
    from inside chunk 0 over a block end to inside chunk 1 of the next block, then 30 samples that complete that block, so that
    status() reports the power of the block whose partial chunk the call under test left behind."""
    rng = np.random.default_rng(seed(3400 + width))
    return _tq_case("align-w%d" % width, 3400 + width, tq_table(rng, 5, 64), tq_loose(64, rng), width, tq_audio(rng, 3, 151, width), [21, 100])


def _two_squares(lo, hi):
    """{W: (a, b)} of the sums of two squares a^2 + b^2 = W in [lo, hi] with 0 <= a, b <= 2045"""
    out = {}
    for a in range(0, min(2045, int(hi ** 0.5)) + 1):
        b0 = max(0, int(max(0, lo - a * a) ** 0.5) - 1)
        for b in range(b0, 2046):
            W = a * a + b * b
            if W > hi:
                break
            if W >= lo:
                out.setdefault(W, (a, b))
    return out


def tq_interior_powers(dom):
    """(rest R = c^2, {-1, 0, +1: W with (W >> dom) - R equal to it}, the near tone's power), all sums of two squares: the smallest
    c >= 30 for which the three W exist.  The near tone's power lies between W >> dom and W for each of the three."""
    for c in range(30, 200):
        R = c * c
        sq = _two_squares((R - 1) << dom, ((R + 2) << dom) - 1)
        Ws = {}
        for rel in (-1, 0, 1):
            cand = [W for W in sq if (W >> dom) - R == rel]
            if cand:
                Ws[rel] = min(cand)
        if len(Ws) == 3:
            near = int((min(Ws.values()) - 1) ** 0.5) ** 2
            assert all((W >> dom) < near < W for W in Ws.values()) and near > R
            return R, {rel: (W,) + sq[W] for rel, W in Ws.items()}, near
    raise AssertionError("no powers for dom_shift %d" % dom)


TQ_INTERIOR = [(g, d) for g in (1, 5) for d in (1, 4, 9)]


def tq_interior(guard, dom):
    """F = 32 at P = 64 with a one-hot table: the cosine row of tone f is 1023 at r = f, its sine row 1023 at r = 32 + f, so a row's
    sample m[f] sets A_f = (1023 m[f]) >> 14 and m[32 + f] sets B_f, each to any value in 0 ... 2045, and W_f = A_f^2 + B_f^2 is set
    exactly.  Per winner f* in {0, 13, F - 1} and relation in {-1, 0, +1}: the winner at W with (W >> dom_shift) - rest equal to the
    relation, a runner-up exactly `guard` tones away (outside `rest`; its power is above W >> dom_shift, so counting it would refuse
    the block) and the tone that is `rest`, guard + 1 away.  Per winner also a tie: the tone `guard` away at the winner's own power;
    the smaller index wins.  The last row is silent.  Every block of a row is the same, 3 blocks and 9 samples, cut at 70."""
    F, P = 32, 64
    tab = np.zeros((F, P, 2), np.int16)
    tab[np.arange(F), np.arange(F), 0] = 1023
    tab[np.arange(F), 32 + np.arange(F), 1] = 1023
    R, Ws, near = tq_interior_powers(dom)
    c, nr = int(R ** 0.5), int(near ** 0.5)

    def m_for(a):
        m = -(-a * 16384 // 1023)
        assert (1023 * m) >> 14 == a and m <= 32767
        return m
    rows, expect = [], []
    for fs in (0, 13, F - 1):
        sgn = 1 if fs + guard + 1 < F else -1
        for rel in (-1, 0, 1, "tie"):
            W, a, b = Ws[0 if rel == "tie" else rel]
            blk = np.zeros(P, np.int64)
            blk[fs], blk[32 + fs] = m_for(a), m_for(b)
            if rel == "tie":
                blk[fs + sgn * guard], blk[32 + fs + sgn * guard] = m_for(b), m_for(a)     # the same power, the squares swapped
            else:
                blk[fs + sgn * guard] = m_for(nr)
            blk[32 + fs + sgn * (guard + 1)] = m_for(c)
            rows.append(blk)
            first = min(fs, fs + sgn * guard) if rel == "tie" else fs
            expect.append(NS(fs=first, W=W, rest=R, rel=0 if rel == "tie" else rel, tie=rel == "tie",
                             hit=tr.NONE if rel == -1 else first))
    rows.append(np.zeros(P, np.int64))
    expect.append(NS(fs=0, W=0, rest=0, rel=0, tie=False, hit=tr.NONE))
    n = 3 * P + 9
    x = np.tile(np.stack(rows), (1, 4))[:, :n, None].astype(np.int16)
    return _tq_case("interior-g%d-d%d" % (guard, dom), 3500, tab, (P, guard, dom, 1, 0, 1, 1, ALL), 1, x, [70], expect=expect)


def tq_many_rows():
    """40000 rows, F = 2, P = 64, 130 samples at width 1, cut 70 | rest."""
    rng = np.random.default_rng(seed(3600))
    x = rng.integers(-32768, 32768, (40000, 130, 1)).astype(np.int64)
    x = ((x * rng.choice([1, 64, 4096, 32768], (40000, 1, 1))) >> 15).astype(np.int16)
    return _tq_case("many", 3600, tq_table(rng, 2, 64), tq_loose(64, rng), 1, x, [70])
