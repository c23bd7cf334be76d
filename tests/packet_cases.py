"""Case generators of the packet demodulator's *_domain GPU test (tests/test_gpu_afsk_domain.py) in plain numpy, with a test-side
copy of the tone-pair kernel's launch plan and LDS staging written from DESIGN.md 9m and the kernel header's prose, so that a case
can say which path it reaches.  tests/test_packet_cases.py runs the cases against the reference alone (tests/afsk_ref.py) and asserts
what each case claims; the GPU file feeds the same cases to the handle.  Every case carries its seed, its runs (a run starts at a
fresh or reset handle; its `cuts` are the lengths of the pieces, and a piece that completes no output is refused and handed over
again in front of the next one) and what it claims to reach.  FMD_FUZZ_SEED moves every seed; what a case claims is built into it
and does not hang on the draw."""
from collections import namedtuple
from types import SimpleNamespace as NS

import numpy as np

import afsk_ref as ar
from rows_cases import sampled_rows, seed

AF_TILE, AF_SLACK = 256, 32

# ---------------------------------------------------------------------------------------------------------------------------------
# the plan

AfPlan = namedtuple("AfPlan", "npair plane_len lds")


def af_plan(T, D):
    """The tone-pair kernel's LDS: the taps as ceil(T / 2) pairs of 16 bytes (four rows' dwords); a plane of the
    tile's span 255 D + T plus 32 samples of slack, rounded up to a multiple of 8 int16."""
    npair = -(-T // 2)
    plane_len = -(-((AF_TILE - 1) * D + T + AF_SLACK) // 8) * 8
    return AfPlan(npair, plane_len, 2 * plane_len + 16 * npair)


def af_domain_ok(T, D):
    return 2 <= T <= 64 and 1 <= D <= min(T, 32)


AF_SHAPES = [(T, D) for T in range(2, 65) for D in range(1, min(T, 32) + 1)]


def af_reachable_h(T, D):
    """The carried history lengths a call can meet: none at the first call; behind a call that ended with N samples in all,
    N - outputs(N) D = T - D + (N - T) mod D."""
    return sorted({0} | set(range(T - D, T)))


STAGE_FIELDS = "n_out ntiles no hh ja jb koff kc k_lo nchunks whole_lo whole_hi head_whole tail_whole min_written max_written max_read kn0"
AfStage = namedtuple("AfStage", STAGE_FIELDS)


def stage_arrays(T, D, h, n_in, row_offset, tile):
    """af_stage on int64 arrays that broadcast against each other (the domain sweep of tests/test_packet_cases.py); closed-form
    arithmetic only.  Samples are counted from the 16-byte boundary in front of the row: the row's sample j is at row_offset + j,
    and chunk c holds the samples [8 c, 8 c + 8)."""
    T, D, h, n_in, off, t = (np.asarray(v, np.int64) for v in (T, D, h, n_in, row_offset, tile))
    npair = (T + 1) // 2
    n_out = (h + n_in - T) // D + 1                           # the call's outputs: virtual samples are the h carried, then the call's
    ntiles = (n_out + AF_TILE - 1) // AF_TILE
    no = np.minimum(n_out - t * AF_TILE, AF_TILE)
    va = t * AF_TILE * D                                      # the tile stages the virtual samples [va, vb)
    vb = va + (no - 1) * D + T
    hh = np.maximum(h - va, 0)                                # of them history
    ja, jb = np.maximum(va - h, 0), vb - h                    # and the call's samples [ja, jb)
    koff = (off + ja) & 7                                     # ja's place in its chunk
    kc = hh + ((koff + 8 - (hh & 7)) & 7)                     # the LDS index of sample ja: behind the history, kc = koff mod 8
    k_lo = kc - koff                                          # the LDS index of chunk c_lo's first sample
    c_lo, c_hi = (off + ja) // 8, (off + jb + 7) // 8
    nchunks = c_hi - c_lo
    w_lo, w_hi = (off + 7) // 8, (off + n_in) // 8 - 1        # the chunks whole inside the row's valid samples
    whole_lo, whole_hi = np.maximum(w_lo, c_lo) - c_lo, np.minimum(w_hi, c_hi - 1) - c_lo     # as indexes of the tile's chunks
    any_whole = whole_lo <= whole_hi
    head_whole, tail_whole = any_whole & (whole_lo == 0), any_whole & (whole_hi == nchunks - 1)
    max_written = np.where(tail_whole, k_lo + 8 * nchunks - 1, kc + (jb - ja) - 1)
    min_written = np.where(hh > 0, kc - hh, np.where(head_whole, k_lo, kc))
    kn0 = kc - hh                                             # lane 0's window; lane j's starts j D behind it
    max_read = 2 * (((kn0 + (no - 1) * D) >> 1) + npair) + 1  # per tap pair one dword, and one more in front of the loop's end
    return AfStage(n_out, ntiles, no, hh, ja, jb, koff, kc, k_lo, nchunks, whole_lo, whole_hi, head_whole, tail_whole, min_written,
                   max_written, max_read, kn0)


def af_stage(T, D, h, n_in, row_offset, tile):
    """What the kernel's staging computes for tile `tile` of a call of n_in samples per row behind h carried ones, for a row that
    starts row_offset samples (0 ... 7) behind a 16-byte boundary: the tile's outputs `no`, the history hh and the call's samples
    [ja, jb) it stages, ja's offset koff in its 16-byte chunk, the LDS index kc of sample ja and k_lo of its chunk's first sample,
    the tile's chunks 0 ... nchunks - 1 of which whole_lo ... whole_hi (none when whole_lo > whole_hi) go as one 16-byte load and the
    others by elements, the smallest and largest LDS index written, the largest a lane reads, and lane 0's window start kn0."""
    assert af_domain_ok(T, D) and h in af_reachable_h(T, D) and 0 <= row_offset < 8 and h + n_in >= T
    s = stage_arrays(T, D, h, n_in, row_offset, tile)
    assert 0 <= tile < s.ntiles
    return AfStage(*(bool(v) if v.dtype == bool else int(v) for v in s))


def stage_by_samples(T, D, h, n_in, row_offset, tile):
    """The same staging walked sample by sample, as the kernel's loops do it: (LDS indexes written, LDS indexes read).  Slow; the
    CPU test compares it with af_stage at drawn points."""
    n_out = (h + n_in - T) // D + 1
    no = min(n_out - tile * AF_TILE, AF_TILE)
    va = tile * AF_TILE * D
    vb = va + (no - 1) * D + T
    hh = max(h - va, 0)
    ja, jb = max(va - h, 0), vb - h
    R, Rend = 2 * row_offset, 2 * (row_offset + n_in)         # byte addresses from the boundary
    a0, a1 = R + 2 * ja, R + 2 * jb
    c_lo, c_hi = a0 >> 4, (a1 + 15) >> 4
    koff = (a0 & 15) >> 1
    kc = hh + ((koff + 8 - (hh & 7)) & 7)
    written = set()
    for i in range(c_hi - c_lo):
        ca, k = (c_lo + i) << 4, kc - koff + 8 * i
        if ca >= R and ca + 16 <= Rend:
            written |= set(range(k, k + 8))
        else:
            written |= {k + e for e in range(8) if a0 <= ca + 2 * e < a1}
    written |= {kc - hh + i for i in range(hh)}
    read = set()
    for lane in range(no):
        kn = kc - hh + lane * D
        for d in range((T + 1) // 2 + 1):
            read |= {2 * ((kn >> 1) + d), 2 * ((kn >> 1) + d) + 1}
    return written, read


# ---------------------------------------------------------------------------------------------------------------------------------
# cases

def table(rng, T):
    """a random table of both signs with +1023 and -1023 in it"""
    t = rng.integers(-1023, 1024, (4, T)).astype(np.int16)
    t[0, 0], t[3, -1] = 1023, -1023
    return t


def stream(rng, rows, n):
    x = rng.integers(-32768, 32768, (rows, n)).astype(np.int16)
    x[:, n // 3] = -32768
    return x


def quieter(x, lo, hi):
    """The samples [lo, hi) at an eighth of their level: the outputs whose windows lie in there stay far from the rails (at a
    64th of what out_shift was chosen for), so that a wrong carried sample cannot hide behind a saturated output."""
    x[:, max(0, lo):hi] >>= 3
    return x


def quarter_rule(x, tab, D, pre):
    """The smallest out_shift at which fewer than a quarter of the reference's outputs lie on the rails."""
    win = np.lib.stride_tricks.sliding_window_view(x.astype(np.int64), tab.shape[1], axis=1)[:, ::D]
    A = (win @ tab.astype(np.int64).T) >> pre
    v = A[..., 0] ** 2 + A[..., 1] ** 2 - A[..., 2] ** 2 - A[..., 3] ** 2
    return next(s for s in range(49) if (np.abs(np.clip(v >> s, -32768, 32767)) >= 32767).mean() < 0.25)


def run(cuts, mode="call", off_in=0, off_out=0, caps=None):
    """One run: the pieces `cuts` from the stream's start on a fresh (or reset) handle.  mode "call": rows_gpu.call with the
    in_cap of `caps` (per accepted call; n_in where None); "at": rows_gpu.call_at, every row off_in samples behind a 16-byte
    boundary and every output row off_out."""
    return NS(cuts=list(cuts), mode=mode, off_in=off_in, off_out=off_out, caps=caps)


def _case(name, sd, T, D, tab, pre, out, x, runs, **claim):
    assert af_domain_ok(T, D) and tab.shape == (4, T), name
    return NS(name=name, seed=seed(sd), T=T, D=D, tab=tab, pre=pre, out=out, rows=x.shape[0], x=x, runs=runs, plan=af_plan(T, D), claim=NS(**claim))


def af_pieces(c, r):
    """The run's calls: (lo, hi, refused, in_cap, h) per handed-over piece, h the history the handle carries in front of it; a
    refused piece is handed over again in front of the next one.  in_cap is what rows_gpu.call gets (odd and larger than n_in on
    every second accepted call unless the run names its own), or what rows_gpu.call_at makes of n_in."""
    out, lo, pos, calls = [], 0, 0, 0
    for n in r.cuts:
        pos = min(c.x.shape[1], pos + n)
        if pos == lo:
            continue
        o0, o1 = ar.outputs(c.T, c.D, lo), ar.outputs(c.T, c.D, pos)
        n_in = pos - lo
        if r.mode == "at":
            in_cap = (n_in + 15) // 8 * 8
        elif r.caps is not None:
            in_cap = r.caps[calls]
        else:
            in_cap = n_in + (0 if calls % 2 == 0 else 2 + n_in % 2)
        out.append((lo, pos, o1 == o0, in_cap, lo - o0 * c.D))
        if o1 > o0:
            lo = pos
            calls += 1
    return out


def row_offsets(c, r, in_cap):
    """The rows' offsets behind a 16-byte boundary: call's buffer starts on one and rows follow each other in_cap samples apart."""
    return [r.off_in] * c.rows if r.mode == "at" else [(k * in_cap) & 7 for k in range(c.rows)]


def stages(c):
    """(run, lo, hi, row, AfStage) of every row and tile of every accepted call of the case"""
    for r in c.runs:
        for lo, hi, refused, in_cap, h in af_pieces(c, r):
            if refused:
                continue
            for row, off in enumerate(row_offsets(c, r, in_cap)):
                nt = af_stage(c.T, c.D, h, hi - lo, off, 0).ntiles
                for t in range(nt):
                    yield r, lo, hi, row, t, af_stage(c.T, c.D, h, hi - lo, off, t)


SHAPE_GROUPS = [list(range(2 + 9 * g, 11 + 9 * g)) for g in range(7)]          # T = 2 ... 64 in 7 groups of 9


def af_every_shape(Ts=range(2, 65)):
    """Every (T, D) of the domain (1551 of them; `Ts` picks the T): 2 rows, a random table, pre_shift 4 ... 9, out_shift by the
    quarter rule.  The stream is cut T + 3 D + r | rest with r drawn in [0, D): the second call carries h = T - D + r samples, and
    the rest completes 257 + T % 5 outputs, a second tile behind the history.  Every window that touches a carried sample lies in
    a quieter stretch.  Then the stream uncut on a fresh handle: two tiles without history."""
    out = []
    for T in Ts:
        for D in range(1, min(T, 32) + 1):
            sd = 5000 + 100 * T + D
            rng = np.random.default_rng(seed(sd))
            r = int(rng.integers(0, D))
            n0 = T + 3 * D + r
            N = n0 + rest_len(T, D, r)
            x, tab, pre = quieter(stream(rng, 2, N), n0 - (T - D + r) - 1, n0 + T), table(rng, T), int(rng.integers(4, 10))
            out.append(_case("T%d-D%d" % (T, D), sd, T, D, tab, pre, quarter_rule(x, tab, D, pre), x, [run([n0, N]), run([N], caps=[N + 1 + N % 2])],
                             h=T - D + r, second=257 + T % 5))
    return out


def rest_len(T, D, r):
    """samples behind a first call of T + 3 D + r that complete exactly 257 + T % 5 outputs, and up to D - 1 - r more, here D - 1 - r
    on even T (the last window ends before the call does)"""
    return (257 + T % 5) * D - r + ((D - 1 - r) if T % 2 == 0 else 0)


HIST_PAIRS = [(64, 32), (15, 8), (9, 9), (10, 2)]


def af_history_alignment(T, D):
    """One of the pairs (64, 32), (15, 8), (9, 9), (10, 2): for every reachable history length h and every input row offset 0 ... 7
    (output offsets cycled), a first call of T + h - (T - D) samples that leaves h (none for h = 0 where T > D: the call under test is
    the first), then a call of 3 outputs, and in another run one of 300 outputs.  3 rows."""
    sd = 6000 + 100 * T + D
    rng = np.random.default_rng(seed(sd))
    tab, pre = table(rng, T), 8
    x = quieter(stream(rng, 3, 2 * T + 301 * D), 0, D + 2 * T)           # (every window that touches a carried sample)
    runs, k = [], 0
    for h in af_reachable_h(T, D):
        first = [] if h < T - D else [D + h]                 # one output, h = N - D behind it
        for off in range(8):
            for outs in (3, 300):
                e = k % D                                    # and up to D - 1 samples behind the last window
                n1 = (outs - 1) * D + T - h + e
                runs.append(run(first + [n1], "at", off, (3 * off + k) % 8))
                runs[-1].h, runs[-1].outs = h, outs
                k += 1
    return _case("hist-T%d-D%d" % (T, D), sd, T, D, tab, pre, quarter_rule(x, tab, D, pre), x, runs, hs=af_reachable_h(T, D))


SHORT_PAIRS = [(2, 1), (3, 2), (9, 4)]
SHORT_MAX = 24


def af_short_rows(T, D):
    """One of the pairs (2, 1), (3, 2), (9, 4), 3 rows: behind a first call that leaves h (every reachable h > 0), second calls of
    every n_in from the shortest that completes an output (T - h) to 24 samples, at all 8 row offsets and once more in a buffer
    with an odd in_cap (rows at three different offsets).  Where the shortest is more than one sample, a piece one sample shorter
    comes first, is refused, and is handed over again."""
    sd = 6500 + 100 * T + D
    rng = np.random.default_rng(seed(sd))
    tab, pre = table(rng, T), 6
    x = stream(rng, 3, T + D + SHORT_MAX)
    runs = []
    for h in af_reachable_h(T, D):
        if h == 0:
            continue
        n0, m = D + h, T - h
        for n in range(m, SHORT_MAX + 1):
            cuts = [n0] + ([m - 1] if m > 1 else []) + [n - (m - 1 if m > 1 else 0)]
            for off in range(8):
                runs.append(run(cuts, "at", off, (off + n) % 8))
            runs.append(run(cuts, "call", caps=[n0 + 1 + n0 % 2, n + 1 + n % 2]))
            for r in runs[-9:]:
                r.h, r.n = h, n
    return _case("short-T%d-D%d" % (T, D), sd, T, D, tab, pre, quarter_rule(x, tab, D, pre), x, runs)


SHIFT_SHAPE = (7, 3)
SHIFTS = [(p, o) for p in range(17) for o in range(49)]


def shift_inputs():
    """(table, x) of the every-shift family: 16 rows whose amplitudes form the ladder 2^0 ... 2^15 (row k is drawn from
    [-2^k, 2^k], clipped to int16, and holds both ends), 64 samples, T = 7, D = 3.  Row 0 is four lone samples of +-1 that meet
    the table's small middle tap alone, so that the lowest shifts have a value off the rails too."""
    rng = np.random.default_rng(seed(7000))
    amp = 1 << np.arange(16)
    x = np.clip(rng.integers(-amp[:, None], amp[:, None] + 1, (16, 64)), -32768, 32767).astype(np.int16)
    x[:, 5], x[:, 6] = -np.minimum(amp, 32768), np.minimum(amp, 32767)
    x[0] = 0
    x[0, [9, 18, 30, 45]] = [1, -1, 1, -1]                   # alone in the windows that start 3 samples before them
    tab = table(rng, SHIFT_SHAPE[0])
    tab[:, 3] = [3, -2, 1, 1]                                # there S = +-(3, -2, 1, 1): 11 at shifts (0, 0), 1 at (0, 3) and at (1, 1)
    return tab, x


def af_every_shift():
    """All 17 x 49 (pre_shift, out_shift) on T = 7, D = 3 with the ladder rows, cut 30 | rest."""
    tab, x = shift_inputs()
    return [_case("pre%d-out%d" % (p, o), 7000, 7, 3, tab, p, o, x, [run([30, 64])]) for p, o in SHIFTS]


FULL_OUT = (0, 31, 48)


def full_scale_inputs():
    """T = 64, D = 5, 4 rows of runs of -32768 and 32767 (and a stretch of small values) against a table of +-1023 in blocks: the
    mark rows see the window's first half, the space rows its second, so that |S| reaches 32 * 32768 * 1023 on either side and, where a
    run covers the whole window against row 0 or row 2 alone, both."""
    rng = np.random.default_rng(seed(7100))
    tab = np.zeros((4, 64), np.int16)
    tab[0, :32], tab[1, :32] = 1023, -1023
    tab[2, 32:], tab[3, 32:] = 1023, 1023
    tab[1, 7], tab[3, 40] = 1000, -1001                      # (not all the same magnitude)
    n = 64 + 5 * 299
    x = np.empty((4, n), np.int16)
    for r in range(4):
        pos = 0
        while pos < n:
            ln = int(rng.integers(20, 120))
            kind = int(rng.integers(0, 4))
            x[r, pos:pos + ln] = (-32768, 32767, 0)[kind] if kind < 3 else rng.integers(-300, 301, min(ln, n - pos))
            pos += ln
    x[0, :64] = -32768                                       # the i32 bound itself: output 0 of row 0
    full = np.zeros((4, 64), np.int16)
    full[0], full[1] = 1023, -1023
    return tab, full, x


def af_full_scale():
    """Per pre_shift 0 ... 16 and out_shift 0, 31 and 48 two full-scale cases at T = 64, D = 5.  `full`: the block table over 4 rows
    of 300 outputs, cut 700 | rest (a second tile in the second call).  `bound`: all samples -32768 in output 0 of row 0 against
    rows of +1023 and -1023 on the mark side (on the space side at out_shift 31): |S| = 64 * 32768 * 1023, the largest an i32
    sum is asked for."""
    tab, full, x = full_scale_inputs()
    out = []
    for p in range(17):
        for o in FULL_OUT:
            out.append(_case("full-pre%d-out%d" % (p, o), 7100, 64, 5, tab, p, o, x, [run([700, x.shape[1]])]))
            out.append(_case("bound-pre%d-out%d" % (p, o), 7100, 64, 5, full if o != 31 else full[::-1].copy(), p, o, x[:2, :200], [run([200])]))
    return out


TILE_OUTS = (255, 256, 257, 511, 512, 513, 1025)
TILE_ROWS = (1, 2, 3, 255, 256, 257)


def af_tiles_and_rows(rows):
    """T = 5, D = 1 at `rows` rows: per outputs-per-call in {255, 256, 257, 511, 512, 513, 1025} a first call of that many outputs
    and a second one of as many, every row with data of its own."""
    T, D = 5, 1
    sd = 7200 + rows
    rng = np.random.default_rng(seed(sd))
    tab, pre = table(rng, T), 5
    out = []
    for n_out in TILE_OUTS:
        x = quieter(stream(rng, rows, T - 1 + 2 * n_out), n_out - 1, 2 * T - 1 + n_out)      # (around the cut)
        out.append(_case("tiles-r%d-o%d" % (rows, n_out), sd, T, D, tab, pre, quarter_rule(x[:8], tab, D, pre), x,
                         [run([T - 1 + n_out, x.shape[1]], caps=[T - 1 + n_out, n_out + 3])], n_out=n_out))
    return out


def af_many_rows():
    """40000 rows at (10, 2), 530 samples cut 522 | 8: 257 outputs in two tiles, then 4 outputs from 8 carried samples and 8 new
    ones.  16 sampled rows are compared."""
    rng = np.random.default_rng(seed(7300))
    x = rng.integers(-32768, 32768, (40000, 530), dtype=np.int16)
    tab = table(rng, 10)
    c = _case("many", 7300, 10, 2, tab, 8, quarter_rule(x[:64], tab, 2, 8), x, [run([522, 530])])
    c.sample = sampled_rows(np.random.default_rng(c.seed), 40000)
    return c
