"""Case generators of the *_domain GPU tests of the stereo bank, the RDS bank, the receiver bank, the narrow-band bank, the channelizer,
the uniform channelizer and the band-plan bank: shapes, tap sets and call-size sequences, in plain numpy, with the host-side plan arithmetic
(tile sizes, the uniform kernel's instantiation, the band-plan pass's tap chunks) copied from DESIGN.md so that a case can say
which kernel path it reaches.  tests/test_domain_cases.py runs these against the references alone and asserts what each case
claims; the GPU files feed the same cases to the handles."""
import os
from types import SimpleNamespace as NS

import numpy as np

import stations_ref as sr
import uniform_ref as ur

DECIMS = (2, 4, 6, 30, 62, 64)
TAPS = (1, 2, 26, 27, 58, 59, 250, 256)
K_TWO = (4, 5, 8, 9, 28, 29, 32)                                   # row tiles of 4 stations (two-digit taps)
K_ONE = (8, 9, 16, 17, 24, 25, 32)                                 # row tiles of 8 (one-digit taps)
K_EDGES = [(k, 2) for k in K_TWO] + [(k, 1) for k in K_ONE]


def fuzz(default, offset):
    n = max(default, int(os.environ.get("FMD_FUZZ_CASES", str(default))))
    return n, np.random.default_rng(int(os.environ.get("FMD_FUZZ_SEED", "20260101")) + offset)


def groups(D, T, K):
    """G, the 16-column MFMA groups per wave of the first pass (st_lds / nb_lds / ch_lds): the largest G in 4 ... 1 with
    raw + 2048 + 4 K 64 G <= 40960, raw = max(12 + 6 D + 8 D (16 G - 1) + 64 nkc, 12 + 2 D (64 G - 1) + 2 T + 15) rounded up to
    16, nkc = ceil((12 + 2 T) / 64)."""
    nkc = (12 + 2 * T + 63) // 64
    for G in (4, 3, 2, 1):
        reads = 12 + 6 * D + 8 * D * (16 * G - 1) + 64 * nkc
        staged = 12 + 2 * D * (64 * G - 1) + 2 * T + 15
        raw = (max(reads, staged) + 15) & ~15
        if raw + 2048 + 4 * K * 64 * G <= 40960 or G == 1:
            return G


def stereo_na(Ta, R):
    return min(256, (2048 - 2 * Ta) // R)


def narrow_q(Ta, R):
    return (-(-Ta // R) + 3) & ~3


def narrow_na(Ta, R):
    return min(256, ((6144 // R - 1) | 1) - narrow_q(Ta, R))


def incs(rng, S, K):
    """[S, K] phase_incs, every (stream, station) its own: an index slip between streams or stations cannot pass."""
    while True:
        v = rng.integers(0, 1 << 32, S * K, dtype=np.uint64)
        if np.unique(v).size == v.size:
            return v.reshape(S, K).astype(np.uint32)


def front(rng, T, S, K, digits):
    """Front-end taps and phase_incs of the wanted digit form: inc[0][0] = 0 makes that station's taps h itself."""
    if digits == 2:
        h = rng.integers(-2047, 2048, T).astype(np.int16)
        h[int(rng.integers(0, T))] = 2047 * int(rng.choice([-1, 1]))
    else:
        h = rng.integers(-127, 128, T).astype(np.int16)
    ii = incs(rng, S, K)
    ii[0, 0] = 0
    return h, ii


def digits_of(h, ii):
    w = [sr.complex_taps(h, int(x)) for x in np.asarray(ii).ravel()]
    return 1 if max(max(np.abs(a).max(), np.abs(b).max()) for a, b in w) <= 127 else 2


def shift_for(h, ii, limit):
    """The smallest shift with ceil(256 max_gain / 2^shift) <= limit."""
    g = sr.max_gain(h, np.unique(np.asarray(ii, dtype=np.uint64)))
    s = 0
    while -(-256 * g >> s) > limit:
        s += 1
    return s


def y_bound(h, ii, shift):
    return -(-256 * sr.max_gain(h, np.unique(np.asarray(ii, dtype=np.uint64))) >> shift)


def bytes_(rng, S, n):
    b = rng.integers(0, 256, (S, n), dtype=np.uint8)
    if n >= 64:                                                    # a full-scale stretch
        a = int(rng.integers(0, n - n // 4)) & ~1
        b[:, a:a + n // 4] = np.where(rng.random((S, n // 4)) < 0.5, 0, 255)
    return b


def loud_quiet(rng, S, n, run):
    """Random bytes in stretches of about `run` bytes, alternately full range and within 8 of the centre."""
    b = rng.integers(0, 256, (S, n), dtype=np.uint8)
    a, quiet = 0, False
    while a < n:
        e = a + 2 * int(rng.integers(run // 4, run))
        if quiet:
            b[:, a:e] = rng.integers(120, 136, b[:, a:e].shape, dtype=np.uint8)
        a, quiet = e, not quiet
    return b


def audio_taps(rng, Ta, total=16383, sign=0):
    """int16 taps with sum |g| == total exactly; sign +1 / -1: all of one sign, 0: random signs."""
    mag = rng.multinomial(total - min(Ta, total), np.ones(Ta) / Ta) + (np.arange(Ta) < total)
    sg = rng.choice([-1, 1], Ta) if sign == 0 else np.full(Ta, sign)
    g = (mag * sg).astype(np.int16)
    assert int(np.abs(g.astype(np.int64)).sum()) == total
    return g


def chan_taps(rng, Ta, cplx, peak=300):
    """Random channel taps scaled to the rule: sum |gr| + |gi| <= 65535, every tap within 16383."""
    gr = rng.integers(-peak, peak + 1, Ta).astype(np.int64)
    gi = rng.integers(-peak, peak + 1, Ta).astype(np.int64) if cplx else np.zeros(Ta, np.int64)
    gr[0] = gr[0] or 1
    if cplx:
        gi[-1] = gi[-1] or 1
    f = min(65535 / int(np.abs(gr).sum() + np.abs(gi).sum()), 16383 / int(max(np.abs(gr).max(), np.abs(gi).max())))
    if f < 1:
        gr, gi = np.trunc(gr * f).astype(np.int64), np.trunc(gi * f).astype(np.int64)
        gr[0] = gr[0] or 1
        if cplx:
            gi[-1] = gi[-1] or 1
    return gr.astype(np.int16), (gi.astype(np.int16) if cplx else None)


def chan_shift_for(h, ii, shift, gr, gi, limit):
    peak = y_bound(h, ii, shift) * int(np.abs(gr.astype(np.int64)).sum() + (0 if gi is None else np.abs(gi.astype(np.int64)).sum()))
    s = 0
    while -(-peak >> s) > limit:
        s += 1
    return s


def pos_for_outputs(T, D, m):
    """The smallest sample count, a multiple of 4 (nbytes % 8 == 0), after which exactly m front-end outputs exist (D >= 4)."""
    assert D >= 4 and m >= 1
    p = -(-(T + (m - 1) * D) // 4) * 4
    assert (p - T) // D + 1 == m
    return p


def sizes_for_outputs(T, D, ends):
    """Byte counts of consecutive calls after which the front end has produced ends[0], ends[1], ... outputs in all."""
    out, pos = [], 0
    for m in ends:
        p = pos_for_outputs(T, D, m)
        assert p > pos
        out.append(2 * (p - pos))
        pos = p
    return out


def y_for_audio(Ta, R, n):
    """The smallest count of second-stage inputs after which exactly n audio samples exist."""
    return Ta + (n - 1) * R


def short_ends(Ta, R, Ms):
    """Second-stage input counts after consecutive calls: a call of M inputs for every M in Ms, each completing audio (a call
    that re-aligns to one input before a completion comes first where needed), then a long call."""
    m = Ta + 40 * R + R - 1
    ends = [m]
    for M in Ms:
        if (m - Ta) % R != R - 1:
            m = Ta + ((m - Ta) // R + 2) * R - 1
            ends.append(m)
        m += M
        ends.append(m)
    return ends + [m + 3000]


# ---- stereo bank ---------------------------------------------------------------------------------------------------------------

ST_BLOCKS = (1024, 4096, 16384)
ST_TA = (1, 2, 63, 64, 255, 256)


def stereo_handle(c, fmd, S=None):
    return fmd.StereoBank(c.h, c.D, c.incs, c.rate, c.g, c.R, n_streams=c.S if S is None else S, block=c.P, pilot_min=c.pilot_min,
                          audio_shift=c.audio_shift, shift=c.shift, device_id=0)


def stereo_refs(c, st, check=None, z=sr.z_corr, pilot_min=None):
    return {s: st.StereoRef(c.h, c.D, c.incs[s], c.shift, c.rate, c.g, c.R, c.P, c.pilot_min if pilot_min is None else pilot_min,
                            c.audio_shift, z=z) for s in (range(c.S) if check is None else check)}


def default_pilot_min(rate, D):
    return (32768 * 6750 * D) // (4 * rate)


def stereo_sweep():
    """Every R in 1 ... 32 (case i has R = i % 32 + 1); Ta from ST_TA or chosen against R; D, K edges of both digit forms, P,
    pilot_min, audio_shift spread over the sweep; every fourth case a call of more than three audio tiles."""
    n_cases, rng = fuzz(32, 1101)
    for i in range(n_cases):
        R = i % 32 + 1
        K, digits = K_EDGES[i % 14] if i % 2 == 0 or i < 28 else (int(rng.integers(1, 4)), 2)
        D = DECIMS[(i + i // 6) % 6]
        if i % 16 == 7:
            D, K, digits = 64, 8, 2                                # G = 3
        if i % 16 == 15:
            D, K, digits = 64, (24, 28, 32)[(i // 16) % 3], 2      # G = 2
        T = TAPS[(3 * i + i // 8) % 8]
        Ta = (ST_TA + (R, R + 1, max(1, R - 1), min(256, 4 * R + 1), 256, 255))[(i + i // 12) % 12]
        if i % 8 == 3 or R == 32:
            Ta = 256                                               # na < 256 from R = 7 on
        S = 1 if K > 9 else 2
        h, ii = front(rng, T, S, K, digits)
        P = ST_BLOCKS[i % 3] if ST_BLOCKS[i % 3] * D <= 65536 else 1024
        rate = 106000 * D + int(rng.integers(0, 50000)) * D
        pm = (0, 1, None, 16384, 1, None)[i % 6]
        pm = default_pilot_min(rate, D) if pm is None else pm
        g = audio_taps(rng, Ta, int(rng.integers(max(Ta, 8000), 16384)) if Ta < 16383 else 16383)
        c = NS(kind="stereo", i=i, R=R, K=K, digits=digits, D=D, T=T, Ta=Ta, S=S, h=h, incs=ii, P=P, rate=rate, pilot_min=pm, g=g,
               audio_shift=int(rng.integers(0, 17)), shift=shift_for(h, ii, int(rng.choice([256, 2048, 16384]))),
               G=groups(D, T, K), na=stereo_na(Ta, R))
        first = 8 * -(-(T + D * (Ta + 2 * R)) // 4)                 # completes audio
        tiles = 3 * c.na + 5 if i % 4 == 3 else int(rng.integers(8, 200))
        c.long_tiles = tiles > 3 * c.na
        c.sizes = [8 * int(rng.integers(1, 30)), first, 8 * int(rng.integers(1, 3 + D * R // 4)), 8 * -(-D * R * tiles // 4),
                   8 * -(-D * (P + 300) // 4), 8 * int(rng.integers(1, 3 + D * R // 2))]
        c.seed = int(rng.integers(0, 1 << 31))
        yield c


def stereo_edges(P, D=4, T=27, Ta=9, R=1, K=3):
    """A call sequence whose MPX end lands on j P - 1, j P and j P + 1; block 1 stays open over 4 calls; one call holds 4 whole
    blocks; one starts exactly on an edge; first-pass tiles straddle an edge at their first and at their last column."""
    rng = np.random.default_rng(1202 + P)
    h, ii = front(rng, T, 2, K, 2)
    G = groups(D, T, K)
    tile = 64 * G - 1
    ends = [P - 1, P, P + 1, P + P // 3, P + 2 * (P // 3), 2 * P - 1, 2 * P, 6 * P, 6 * P + 1, 7 * P - tile + 1, 7 * P + 40, 8 * P - 1,
            8 * P + 1, 9 * P]
    rate = 110000 * D
    c = NS(kind="stereo", R=R, K=K, D=D, T=T, Ta=Ta, S=2, h=h, incs=ii, P=P, rate=rate, pilot_min=1, g=audio_taps(rng, Ta, 16000),
           audio_shift=9, shift=shift_for(h, ii, 256), G=G, tile=tile, ends=ends, sizes=sizes_for_outputs(T, D, ends),
           seed=int(rng.integers(0, 1 << 31)))
    return c


def stereo_short(R):
    """Ta = 256: calls that complete audio with 1, 2, Ta - 2, Ta - 1 and Ta MPX samples (the (x, s) history is rebuilt from old
    history plus new samples), then a long call."""
    rng = np.random.default_rng(1303 + R)
    D, T, Ta, K, P = 4, 26, 256, 5, 1024
    h, ii = front(rng, T, 2, K, 2)
    ends = short_ends(Ta, R, (1, 2, Ta - 2, Ta - 1, Ta, 1, Ta - 1, 2))
    c = NS(kind="stereo", R=R, K=K, D=D, T=T, Ta=Ta, S=2, h=h, incs=ii, P=P, rate=120000 * D, pilot_min=1, g=audio_taps(rng, Ta),
           audio_shift=8, shift=shift_for(h, ii, 2048), G=groups(D, T, K), ends=ends, sizes=sizes_for_outputs(T, D, ends),
           seed=int(rng.integers(0, 1 << 31)))
    return c


def stereo_threshold():
    """T = 1, h = [1], decim 2, inc = 0, shift 0: y is the centred byte pair of every second sample.  capture_rate = 8 * 19000 *
    decim makes the pilot step 2^29 exactly, so theta = 0 at every m = 8 i: cosq = 16384, sinq = 0.  y constant (100, 0) up to
    m = 7 and (100, 100) from m = 8 on gives x = 0 everywhere except x[8] = 4096 (a turn of 45 degrees, where the discriminator
    is exact), so block 0 has I = 2^26, Q = 0 and I^2 + Q^2 == (8 * 1024 * 8192)^2: exact equality at pilot_min = 8.  Random
    bytes follow, whose audio differs between L and R only where block 0 counted as present."""
    rng = np.random.default_rng(1404)
    P, D = 1024, 2
    b = np.empty(2 * D * P + 8 * 3000, np.uint8)
    b[0::2], b[1::2] = 227, 127
    b[2 * D * 8 + 1:2 * D * P:2] = 227
    b[2 * D * P:] = rng.integers(0, 256, b.size - 2 * D * P, dtype=np.uint8)
    ii = np.array([[0]], np.uint32)
    c = NS(kind="stereo", R=1, K=1, D=D, T=1, Ta=3, S=1, h=np.ones(1, np.int16), incs=ii, P=P, rate=8 * 19000 * D, pilot_min=8,
           g=np.array([5000, 6000, 5383], np.int16), audio_shift=6, shift=0, data=b[None, :],
           sizes=[2 * D * 600, 2 * D * 424, 8 * 3000])
    return c


def stereo_extreme(limit, sign):
    """sum |g| = 16383 over taps of one sign or of alternating signs, audio_shift 0, the front-end shift at `limit`; a strong
    synthetic station with pilot, then bytes at the rails."""
    import stereo_ref as st
    rng = np.random.default_rng(1505 + limit + sign)
    fs, D, T, Ta, R, P = 1200000, 4, 32, 8, 3, 1024
    h = st.lowpass(T, 130000 / fs)
    ii = np.array([[sr.phase_inc(200000, fs), sr.phase_inc(-310000, fs)]], np.uint32)
    g = audio_taps(rng, Ta, 16383, sign=sign)
    if sign == 0:
        g = (np.abs(g) * np.where(np.arange(Ta) % 2, -1, 1)).astype(np.int16)
    n = D * 3 * P
    tone = lambda t: 0.4 * np.sin(2 * np.pi * 1000 * t)
    other = lambda t: 0.3 * np.sin(2 * np.pi * 3100 * t)
    iq = st.synth_iq(n, fs, [(200000, tone, other, 0.7, True), (-310000, other, tone, 2.1, True)], amp=60.0, noise=1.0, seed=limit)
    rails = np.where(rng.random(8 * 2000) < 0.5, 0, 255).astype(np.uint8)
    data = np.concatenate([iq, rails])[None, :]
    return NS(kind="stereo", R=R, K=2, D=D, T=T, Ta=Ta, S=1, h=h, incs=ii, P=P, rate=fs, pilot_min=1 if limit == 16384 else default_pilot_min(fs, D),
              g=g, audio_shift=0, shift=shift_for(h, ii, limit), data=data, sizes=[2 * n // 2, 2 * n // 2, 8 * 2000], limit=limit)


# ---- RDS bank ------------------------------------------------------------------------------------------------------------------

def rds_na(Ta, R):
    """Outputs per tile of the baseband pass: R na + Ta <= 1984 staged pairs."""
    return min(256, (1984 - Ta) // R)


def rds_shift_for(g):
    """The smallest rds_shift with ceil(32768 sum |g| / 2^s) <= 32767."""
    total = 32768 * int(np.abs(np.asarray(g, dtype=np.int64)).sum())
    s = 0
    while -(-total >> s) > 32767:
        s += 1
    return s


def rds_handle(c, fmd):
    return fmd.RdsBank(c.h, c.D, c.incs, c.rate, c.g, c.R, n_streams=c.S, block=c.P, pilot_min=c.pilot_min, rds_shift=c.rds_shift,
                       shift=c.shift, device_id=0)


def rds_refs(c, rr, check=None, cls=None, stations=None):
    """The definition of the streams in `check` (all by default); `cls`: a variant of rr.RdsRef, `stations`: only these k."""
    pick = (lambda row: row) if stations is None else (lambda row: [row[k] for k in stations])
    return {s: (cls or rr.RdsRef)(c.h, c.D, pick(c.incs[s]), c.shift, c.rate, c.g, c.R, c.rds_shift, c.P, c.pilot_min, z=sr.z_corr)
            for s in (range(c.S) if check is None else check)}


def rds_sweep():
    """Every R in 1 ... 32 (case i has R = i % 32 + 1); Ta from the list below or chosen against R; D, K edges of both digit forms,
    P, pilot_min spread over the sweep; rds_shift alternately the smallest allowed and a value up to 24 (the alternation slips by
    one every four cases, so the cases with many tiles get both); every fourth case a call of more than three tiles; every case a
    call of more than P MPX samples."""
    n_cases, rng = fuzz(32, 4101)
    for i in range(n_cases):
        R = i % 32 + 1
        K, digits = K_EDGES[i % 14] if i % 2 == 0 or i < 28 else (int(rng.integers(1, 4)), 2)
        D = DECIMS[(i + i // 6) % 6]
        if i % 16 == 7:
            D, K, digits = 64, 8, 2                                # G = 3
        if i % 16 == 15:
            D, K, digits = 64, (24, 28, 32)[(i // 16) % 3], 2      # G = 2
        T = TAPS[(3 * i + i // 8) % 8]
        Ta = (1, 2, 63, 64, 255, 256, R, R + 1, max(1, R - 1), min(256, 4 * R + 1))[(i + i // 10) % 10]
        if i % 8 == 3 or R == 32:
            Ta = 256
        S = 1 if K > 9 else 2
        h, ii = front(rng, T, S, K, digits)
        P = ST_BLOCKS[i % 3] if ST_BLOCKS[i % 3] * D <= 65536 else 1024
        rate = 120000 * D + int(rng.integers(0, 50000)) * D
        pm = (0, 1, None, 16384, 1, None)[i % 6]
        pm = default_pilot_min(rate, D) if pm is None else pm
        g = audio_taps(rng, Ta, int(rng.integers(max(Ta, 8000), 16384)))
        smin = rds_shift_for(g)
        c = NS(kind="rds", i=i, R=R, K=K, digits=digits, D=D, T=T, Ta=Ta, S=S, h=h, incs=ii, P=P, rate=rate, pilot_min=pm, g=g,
               rds_shift=smin if (i + i // 4) % 2 == 0 else int(rng.integers(smin + 1, 25)), rds_shift_min=smin,
               shift=shift_for(h, ii, int(rng.choice([256, 2048, 16384]))), G=groups(D, T, K), na=rds_na(Ta, R))
        first = 8 * -(-(T + D * (Ta + 2 * R)) // 4)                 # completes an output
        c.long_tiles = i % 4 == 3
        outs = 3 * c.na + 5 if c.long_tiles else int(rng.integers(8, 200))
        if not c.long_tiles and D * R * outs > 200000:             # keeps the reference quick; the long calls stay whole
            outs = max(4, 200000 // (D * R))
        c.sizes = [8 * int(rng.integers(1, 30)), first, 8 * int(rng.integers(1, 3 + D * R // 4)), 8 * -(-D * R * outs // 4),
                   8 * -(-D * (P + 300) // 4), 8 * int(rng.integers(1, 3 + D * R // 2))]
        c.seed = int(rng.integers(0, 1 << 31))
        yield c


def rds_full_tiles(R):
    """Ta = 256 and R in (8, 16, 32): R na + Ta == 1984 exactly.  Two calls of 2 na outputs each, both ending one MPX sample before
    the next output would complete: the last tile then stages R na + Ta - 1 pairs, the most any tile can (its highest LDS slot is
    1982 + 61 = 2043), and the second call reads back all Ta - 1 pairs of the history the first one wrote.  A short third call
    reads the second one's."""
    rng = np.random.default_rng(4202 + R)
    D, T, Ta, K, P = 4, 26, 256, 5, 1024
    na = rds_na(Ta, R)
    h, ii = front(rng, T, 2, K, 2)
    g = audio_taps(rng, Ta)
    m1 = Ta + 2 * na * R - 1
    ends = [m1, m1 + 2 * na * R, m1 + 2 * na * R + 3 * R]
    return NS(kind="rds", R=R, K=K, D=D, T=T, Ta=Ta, S=2, h=h, incs=ii, P=P, rate=125000 * D, pilot_min=1, g=g,
              rds_shift=rds_shift_for(g), shift=shift_for(h, ii, 2048), G=groups(D, T, K), na=na, ends=ends,
              sizes=sizes_for_outputs(T, D, ends), seed=int(rng.integers(0, 1 << 31)))


def rds_short(R):
    """Ta = 256: calls that complete outputs with 1, 2, Ta - 2, Ta - 1 and Ta MPX samples (the (qr, qi) history is rebuilt from
    old history plus new samples), then a long call."""
    rng = np.random.default_rng(4303 + R)
    D, T, Ta, K, P = 4, 26, 256, 5, 1024
    h, ii = front(rng, T, 2, K, 2)
    g = audio_taps(rng, Ta)
    ends = short_ends(Ta, R, (1, 2, Ta - 2, Ta - 1, Ta, 1, Ta - 1, 2))
    return NS(kind="rds", R=R, K=K, D=D, T=T, Ta=Ta, S=2, h=h, incs=ii, P=P, rate=125000 * D, pilot_min=1, g=g,
              rds_shift=rds_shift_for(g), shift=shift_for(h, ii, 2048), G=groups(D, T, K), na=rds_na(Ta, R), ends=ends,
              sizes=sizes_for_outputs(T, D, ends), seed=int(rng.integers(0, 1 << 31)))


def rds_edges(P):
    """The call ends of stereo_edges (MPX ends on j P - 1, j P, j P + 1; a block open over four calls; four whole blocks in one
    call; a call that starts on an edge) with Ta = 9, R = 1.  Two synthetic stations: the one at +110 kHz carries a pilot up to the
    middle of block 5 and none after, the one at -110 kHz the other way round; random bytes from block 8 on.  Station 2 tunes
    to nothing.  Stream 1 has the same bytes half a block later and the stations in another order."""
    import stereo_ref as st
    rng = np.random.default_rng(4404 + P)
    D, T, Ta, R, K = 4, 27, 9, 1, 3
    fs = 120000 * D
    e = stereo_edges(P, D=D, T=T, Ta=Ta, R=R, K=K)
    h = st.lowpass(T, 90000 / fs)
    a, b, x = sr.phase_inc(110000, fs), sr.phase_inc(-110000, fs), sr.phase_inc(5000, fs)
    ii = np.array([[a, b, x], [x, a, b]], np.uint32)
    n = sum(e.sizes) // 2
    cut, tail = D * (5 * P + P // 2), D * 8 * P
    tone = lambda t: 0.4 * np.sin(2 * np.pi * 1000 * t)
    other = lambda t: 0.3 * np.sin(2 * np.pi * 3100 * t)
    d0 = np.concatenate([st.synth_iq(cut, fs, [(110000, tone, other, 0.7, True), (-110000, other, tone, 2.1, False)], seed=P),
                         st.synth_iq(tail - cut, fs, [(110000, tone, other, 0.7, False), (-110000, other, tone, 2.1, True)], seed=P + 1),
                         rng.integers(0, 256, 2 * (n - tail), dtype=np.uint8)])
    g = audio_taps(rng, Ta, 16000)
    return NS(kind="rds", R=R, K=K, D=D, T=T, Ta=Ta, S=2, h=h, incs=ii, P=P, rate=fs, pilot_min=default_pilot_min(fs, D), g=g,
              rds_shift=rds_shift_for(g), shift=shift_for(h, ii, 256), G=e.G, tile=e.tile, na=rds_na(Ta, R), ends=e.ends, sizes=e.sizes,
              data=np.stack([d0, np.roll(d0, 2 * D * (P // 2))]))


RDS_EXTREMES = (("plus", 14), ("minus", 14), ("256", 14), ("256", 24))


def rds_extreme(g, rds_shift):
    """The front end and the bytes of narrow_extreme(FM): D = 2, T = 16, every tap 2047, inc 0, the front-end shift at limit
    16384, bytes at the rails.  `g`: "plus" = [16383], "minus" = [-16383], "256" = 256 taps of one sign with sum 16383.  The
    one-tap sets reach v = +-16384 * 16383, the largest |v| bytes can produce, and u = v >> 14 spans exactly -16383 ... 16383; at
    rds_shift 24 a small negative v must give u = -1, where a shift that truncates toward zero gives 0.

    |x| never exceeds 16384: the discriminator's range is +-16384 (a half turn), so |q| <= 16384 as well and the bound
    |q| <= 32768 of include/fmd.h (any int16 x) is never met through bytes."""
    e = narrow_extreme(1)
    rng = np.random.default_rng(4505)                              # the same 256 taps at both shifts
    taps = {"plus": np.array([16383], np.int16), "minus": np.array([-16383], np.int16)}
    gg = taps[g] if g in taps else audio_taps(rng, 256, 16383, sign=+1)
    return NS(kind="rds", R=1, K=1, D=e.D, T=e.T, Ta=gg.size, S=1, h=e.h, incs=e.incs, P=1024, rate=304000, pilot_min=1, g=gg,
              rds_shift=rds_shift, shift=e.shift, na=rds_na(gg.size, 1), data=e.data, sizes=e.sizes)


# ---- receiver bank -------------------------------------------------------------------------------------------------------------

RX_TA_R = (1, 2, 63, 64, 255, 256)                                 # the RDS sweep's fixed tap counts
RX_SHORT = ((3, 5), (32, 1), (1, 32))


def receiver_handle(c, fmd, pilot_min=None):
    return fmd.ReceiverBank(c.h, c.D, c.incs, c.rate, c.ga, c.Ra, c.gr, c.Rr, n_streams=c.S, block=c.P,
                            pilot_min=c.pilot_min if pilot_min is None else pilot_min, audio_shift=c.audio_shift, rds_shift=c.rds_shift,
                            shift=c.shift, device_id=0)


def receiver_refs(c, rxr, check=None, pilot_min=None):
    return {s: rxr.ReceiverRef(c.h, c.D, c.incs[s], c.shift, c.rate, c.ga, c.Ra, c.audio_shift, c.gr, c.Rr, c.rds_shift, c.P,
                               c.pilot_min if pilot_min is None else pilot_min, z=sr.z_corr) for s in (range(c.S) if check is None else check)}


def receiver_plan(c, refused=None):
    """(mS, mE, (nS, nE) of the audio stage, (nS, nE) of the RDS stage) of every accepted call of a receiver case, by the arithmetic
    of include/fmd.h alone.  A call that completes fewer than one output of either stage is refused and changes nothing; `refused`,
    a list, receives (index of the call, "audio" | "rds" | "neither": what the refused call would have completed)."""
    out_of = lambda p: (p - c.T) // c.D + 1 if p >= c.T else 0
    fir = lambda m, Ta, R: (m - Ta) // R + 1 if m >= Ta else 0
    pos, acc = 0, []
    for i, n in enumerate(c.sizes):
        mS, mE = out_of(pos), out_of(pos + n // 2)
        a = (fir(mS, c.Ta_a, c.Ra), fir(mE, c.Ta_a, c.Ra))
        r = (fir(mS, c.Ta_r, c.Rr), fir(mE, c.Ta_r, c.Rr))
        if a[1] - a[0] < 1 or r[1] - r[0] < 1:
            if refused is not None:
                refused.append((i, "audio" if a[1] > a[0] else "rds" if r[1] > r[0] else "neither"))
            continue
        acc.append((mS, mE, a, r))
        pos += n // 2
    return acc


def receiver_tiles(c, call):
    """Second-pass tiles per row of an accepted call of receiver_plan: (audio, RDS)."""
    _, _, (aS, aE), (rS, rE) = call
    return -(-(aE - aS) // c.na_a), -(-(rE - rS) // c.na_r)


def bytes_to_reach(T, D, pos, m):
    """The smallest byte count, a multiple of 8, of a call from sample `pos` (a multiple of 4) after which at least m front-end
    outputs exist."""
    p = max(pos + 4, -(-(T + (m - 1) * D) // 4) * 4)
    return 2 * (p - pos)


def receiver_sweep():
    """Case i has audio stride Ra = i % 32 + 1 and RDS stride Rr = (7 i + 3) % 32 + 1: every stride 1 ... 32 on each side, never
    the same on both (6 i = -3 mod 32 has no solution).  The tap counts come from the stereo and the RDS sweeps' lists, walked at
    different steps, and are 256 on either side where i % 8 == 3 or that side's stride is 32; D, T, K edges of both digit forms, the
    G = 2 and G = 3 overrides, P, pilot_min and the front-end limit as in stereo_sweep; rds_shift alternately the smallest and a
    larger one.  Calls: a short one; the first that completes both stages, ending on or one sample after an output of the side with
    the larger stride; 8 bytes, at most two multiplex samples, which that side (stride >= 4) cannot complete: refused; a few
    strides; a long one -- where i % 4 == 3 or S K is odd more than three tiles of the side whose tile spans fewer multiplex
    samples and more than one of the other; more than P multiplex samples; a short tail."""
    n_cases, rng = fuzz(32, 7101)
    for i in range(n_cases):
        Ra, Rr = i % 32 + 1, (7 * i + 3) % 32 + 1
        K, digits = K_EDGES[i % 14] if i % 2 == 0 or i < 28 else (int(rng.integers(1, 4)), 2)
        D = DECIMS[(i + i // 6) % 6]
        if i % 16 == 7:
            D, K, digits = 64, 8, 2                                # G = 3
        if i % 16 == 15:
            D, K, digits = 64, (24, 28, 32)[(i // 16) % 3], 2      # G = 2
        T = TAPS[(3 * i + i // 8) % 8]
        Ta_a = (ST_TA + (Ra, Ra + 1, max(1, Ra - 1), min(256, 4 * Ra + 1), 256, 255))[(i + i // 12) % 12]
        Ta_r = (RX_TA_R + (Rr, Rr + 1, max(1, Rr - 1), min(256, 4 * Rr + 1)))[(3 * i + i // 10) % 10]
        if i % 8 == 3 or Ra == 32:
            Ta_a = 256
        if i % 8 == 3 or Rr == 32:
            Ta_r = 256
        S = 1 if K > 9 else 2
        h, ii = front(rng, T, S, K, digits)
        P = ST_BLOCKS[i % 3] if ST_BLOCKS[i % 3] * D <= 65536 else 1024
        rate = 120000 * D + int(rng.integers(0, 50000)) * D
        pm = (0, 1, None, 16384, 1, None)[i % 6]
        pm = default_pilot_min(rate, D) if pm is None else pm
        ga = audio_taps(rng, Ta_a, int(rng.integers(max(Ta_a, 8000), 16384)))
        gr = audio_taps(rng, Ta_r, int(rng.integers(max(Ta_r, 8000), 16384)))
        smin = rds_shift_for(gr)
        c = NS(kind="receiver", i=i, Ra=Ra, Rr=Rr, K=K, digits=digits, D=D, T=T, Ta_a=Ta_a, Ta_r=Ta_r, S=S, h=h, incs=ii, P=P, rate=rate,
               pilot_min=pm, ga=ga, gr=gr, audio_shift=int(rng.integers(0, 17)),
               rds_shift=smin if (i + i // 4) % 2 == 0 else int(rng.integers(smin + 1, 25)), rds_shift_min=smin,
               shift=shift_for(h, ii, int(rng.choice([256, 2048, 16384]))), G=groups(D, T, K), na_a=stereo_na(Ta_a, Ra), na_r=rds_na(Ta_r, Rr))
        Rx, Tx = max((Ra, Ta_a), (Rr, Ta_r))                       # the side with the larger stride
        out_of = lambda p: (p - T) // D + 1 if p >= T else 0
        n0 = 8 * int(rng.integers(1, 30))
        m0 = out_of(n0 // 2)
        pos, m0 = (n0 // 2, m0) if (m0 >= Ta_a and m0 >= Ta_r) else (0, 0)   # a first call that completes both is accepted
        m1 = Tx + Rx * -(-(max(Ta_a, Ta_r, m0) + 2 * Rx - Tx) // Rx)   # an output of that side, two strides past the other's first
        first = bytes_to_reach(T, D, pos, m1)
        spans = sorted((Ra * c.na_a, Rr * c.na_r))                 # multiplex samples per tile of the two sides
        c.long_tiles = i % 4 == 3 or (S * K) % 2 == 1
        if c.long_tiles:
            mpx = max(3 * spans[0], spans[1]) + 5 * Rx
        else:
            mpx = Rx * int(rng.integers(8, 200))
            if D * mpx > 200000:                                   # keeps the reference quick; the long calls stay whole
                mpx = max(4 * Rx, 200000 // D)
        c.sizes = [n0, first, 8, 8 * int(rng.integers(1, 3 + D * Rx // 4)), 8 * -(-D * mpx // 4), 8 * -(-D * (P + 300) // 4),
                   8 * int(rng.integers(1, 3 + D * Rx // 2))]
        c.seed = int(rng.integers(0, 1 << 31))
        yield c


def receiver_full_tiles():
    """Audio Ta = 256, R = 6: na = 256 and R na + 2 Ta == 2048.  RDS Ta = 256, R = 8: na = 216 and R na + Ta == 1984.  Two calls of
    9 full audio tiles and 8 full RDS tiles per row, both ending one multiplex sample before the next output of BOTH stages
    ((m - 256) % 24 == 23), so both last tiles stage the most pairs they can and the second call reads back all 255 history pairs
    of both stages; a short third call reads the second one's."""
    rng = np.random.default_rng(7202)
    D, T, K, P, Ta = 4, 26, 5, 1024, 256
    h, ii = front(rng, T, 2, K, 2)
    ga, gr = audio_taps(rng, Ta), audio_taps(rng, Ta)
    ends = [14079, 14079 + 13824, 14079 + 13824 + 3 * 24]
    return NS(kind="receiver", Ra=6, Rr=8, K=K, D=D, T=T, Ta_a=Ta, Ta_r=Ta, S=2, h=h, incs=ii, P=P, rate=125000 * D, pilot_min=1, ga=ga,
              gr=gr, audio_shift=8, rds_shift=rds_shift_for(gr), shift=shift_for(h, ii, 2048), G=groups(D, T, K), na_a=stereo_na(Ta, 6),
              na_r=rds_na(Ta, 8), ends=ends, sizes=sizes_for_outputs(T, D, ends), seed=int(rng.integers(0, 1 << 31)))


def receiver_short(Ra, Rr):
    """Ta = 256 (audio) and 255 (RDS), D = 4, so that every multiplex count is a call end.  After a warm-up call: accepted calls of
    M = 1, 2, 253, 254, 255, 256, 1, 254, 2 multiplex samples, each completing an output of both stages (a call that re-aligns the
    start comes first where needed).  Before the calls of 253 samples and more comes a refused one over the head of the same bytes
    -- the longest that completes audio only, RDS only, or neither, walking through those of the three that the strides allow -- and
    before the accepted calls of 2 samples a refused call of their first sample where one exists.  A long call ends the sequence.
    c.spans are the byte ranges of the calls, c.sizes their lengths, c.refused the (index, kind) of the refused ones."""
    rng = np.random.default_rng(7303 + 100 * Ra + Rr)
    D, T, K, P, Ta_a, Ta_r = 4, 26, 5, 1024, 256, 255
    h, ii = front(rng, T, 2, K, 2)
    ga, gr = audio_taps(rng, Ta_a), audio_taps(rng, Ta_r)
    cnt = lambda m, Ta, R: (m - Ta) // R + 1 if m >= Ta else 0
    got = lambda a, b: (cnt(b, Ta_a, Ra) > cnt(a, Ta_a, Ra), cnt(b, Ta_r, Rr) > cnt(a, Ta_r, Rr))
    kind_of = {(True, False): "audio", (False, True): "rds", (False, False): "neither"}
    both = lambda a, b: got(a, b) == (True, True)
    m = Ta_a + 40 * max(Ra, Rr)
    mcalls, kinds, want = [(0, m)], ("audio", "rds", "neither"), 0  # (start, end) in multiplex samples

    def start_for(M, kind):
        """The nearest start s >= m of an accepted call of M samples (reached by an accepted call where s > m), and the lengths of the
        refused calls of `kind` (None: any) over its head; (s, []) of the nearest start if no start has such a refusal."""
        fallback = None
        for s in range(m, m + 4 * Ra * Rr + 1):
            if not both(s, s + M) or (s > m and not both(m, s)):
                continue
            ls = [L for L in range(1, M) if not both(s, s + L) and kind in (None, kind_of[got(s, s + L)])]
            if ls:
                return s, ls
            fallback = fallback or (s, [])
        return fallback

    for M in (1, 2, 253, 254, 255, 256, 1, 254, 2):
        if M >= 253:                                               # the next kind of refusal that the strides allow
            for _ in range(3):
                s, ls = start_for(M, kinds[want % 3])
                want += 1
                if ls:
                    break
        else:
            s, ls = start_for(M, None)
        if s > m:
            mcalls.append((m, s))
        if ls:
            mcalls.append((s, s + max(ls)))
        mcalls.append((s, s + M))
        m = s + M
    mcalls.append((m, m + 3000))
    at = lambda mm: 2 * pos_for_outputs(T, D, mm) if mm else 0
    c = NS(kind="receiver", Ra=Ra, Rr=Rr, K=K, D=D, T=T, Ta_a=Ta_a, Ta_r=Ta_r, S=2, h=h, incs=ii, P=P, rate=125000 * D, pilot_min=1, ga=ga,
           gr=gr, audio_shift=8, rds_shift=rds_shift_for(gr), shift=shift_for(h, ii, 2048), G=groups(D, T, K), na_a=stereo_na(Ta_a, Ra),
           na_r=rds_na(Ta_r, Rr), mcalls=mcalls, spans=[(at(a), at(b)) for a, b in mcalls])
    c.sizes = [b - a for a, b in c.spans]
    c.data = bytes_(rng, 2, at(m + 3000))
    c.refused = []
    receiver_plan(c, c.refused)
    return c


def receiver_edges(P):
    """The call ends of stereo_edges(P) and the bytes and front end of rds_edges(P) -- a pilot that stops mid-block on one station
    and starts on the other, a station tuned to nothing, stream 1 half a block later -- under 9 taps at stride 1 on both sides."""
    e = rds_edges(P)
    rng = np.random.default_rng(7404 + P)
    return NS(kind="receiver", Ra=1, Rr=1, K=e.K, D=e.D, T=e.T, Ta_a=9, Ta_r=9, S=2, h=e.h, incs=e.incs, P=P, rate=e.rate,
              pilot_min=default_pilot_min(e.rate, e.D), ga=audio_taps(rng, 9, 16000), gr=e.g, audio_shift=9, rds_shift=e.rds_shift,
              shift=e.shift, G=e.G, tile=e.tile, na_a=stereo_na(9, 1), na_r=rds_na(9, 1), ends=e.ends, sizes=e.sizes, data=e.data)


def receiver_threshold():
    """The bytes and the front end of stereo_threshold() -- I = 2^26, Q = 0 in block 0: exact equality at pilot_min 8 -- with its
    audio stage, and an RDS stage of 5 taps at stride 2.  capture_rate = 8 * 19000 * 2 = 304000 is above the receiver's floor of
    120000 * 2 as it stands, so the construction is untouched."""
    t = stereo_threshold()
    assert t.rate >= 120000 * t.D
    gr = audio_taps(np.random.default_rng(7505), 5)
    return NS(kind="receiver", Ra=t.R, Rr=2, K=1, D=t.D, T=t.T, Ta_a=t.Ta, Ta_r=5, S=1, h=t.h, incs=t.incs, P=t.P, rate=t.rate, pilot_min=8,
              ga=t.g, gr=gr, audio_shift=t.audio_shift, rds_shift=rds_shift_for(gr), shift=0, na_a=stereo_na(t.Ta, t.R), na_r=rds_na(5, 2),
              data=t.data, sizes=t.sizes)


RX_EXTREMES = ("stereo", "rds-plus", "rds-256")


def receiver_extreme(which):
    """"stereo": stereo_extreme(16384, 1) -- sum |ga| = 16383 of one sign, audio_shift 0, a strong station with pilot and then bytes
    at the rails -- and an RDS stage of 16 taps at stride 2 with sum |gr| = 16383 at the smallest rds_shift.  "rds-plus", "rds-256":
    rds_extreme("plus", 14) and rds_extreme("256", 24) -- bytes at the rails through maximal taps, the baseband at both ends of
    rds_shift -- and an audio stage of one tap 16383 at audio_shift 0."""
    if which == "stereo":
        e = stereo_extreme(16384, 1)
        gr = audio_taps(np.random.default_rng(7606), 16, 16383)
        return NS(kind="receiver", Ra=e.R, Rr=2, K=e.K, D=e.D, T=e.T, Ta_a=e.Ta, Ta_r=16, S=1, h=e.h, incs=e.incs, P=e.P, rate=e.rate,
                  pilot_min=e.pilot_min, ga=e.g, gr=gr, audio_shift=0, rds_shift=rds_shift_for(gr), shift=e.shift, na_a=stereo_na(e.Ta, e.R),
                  na_r=rds_na(16, 2), data=e.data, sizes=e.sizes)
    e = rds_extreme(*{"rds-plus": ("plus", 14), "rds-256": ("256", 24)}[which])
    return NS(kind="receiver", Ra=1, Rr=e.R, K=1, D=e.D, T=e.T, Ta_a=1, Ta_r=e.Ta, S=1, h=e.h, incs=e.incs, P=e.P, rate=e.rate,
              pilot_min=e.pilot_min, ga=np.array([16383], np.int16), gr=e.g, audio_shift=0, rds_shift=e.rds_shift, shift=e.shift,
              na_a=stereo_na(1, 1), na_r=e.na, data=e.data, sizes=e.sizes)


# ---- narrow-band bank ----------------------------------------------------------------------------------------------------------

NB_BLOCKS = (16, 64, 4096)


def narrow_handle(c, fmd, squelch=None):
    return fmd.NarrowBank(c.h, c.D, c.incs, (c.gr, c.gi), c.R, mode=c.mode, n_streams=c.S, block=c.P,
                          squelch=c.squelch if squelch is None else squelch, gain=c.gain, chan_shift=c.chan_shift, shift=c.shift,
                          device_id=0)


def narrow_refs(c, nr, check=None, z=sr.z_corr, squelch=None, mode=None):
    return {s: nr.NarrowRef(c.h, c.D, c.incs[s], c.shift, c.gr, c.gi, c.mode if mode is None else mode, c.R, c.chan_shift, c.P,
                            c.squelch if squelch is None else squelch, c.gain, z=z) for s in (range(c.S) if check is None else check)}


def probe_squelch(c, nr, data):
    """A squelch between the loud and the quiet block RMS of stream 0, station 0 (0 when fewer than two blocks complete)."""
    p = nr.NarrowRef(c.h, c.D, c.incs[0][:1], c.shift, c.gr, c.gi, nr.IQ, c.R, c.chan_shift, c.P, 0, 256, z=sr.z_corr)
    u = p.feed(data)[0]
    nblk = u.shape[0] // c.P
    if nblk < 2:
        return 0
    rms = np.sqrt((u[:nblk * c.P].astype(np.float64) ** 2).sum(axis=1).reshape(nblk, c.P).mean(axis=1))
    return min(23170, int(np.sqrt(max(1.0, rms.min()) * rms.max())))


def narrow_sweep():
    """For every R in 1 ... 32: four Ta with ceil(Ta / R) mod 4 = 0, 1, 2, 3 and a fifth that is below R or 256.  Modes, real and
    complex taps, D, K edges of both digit forms and P spread over the sweep; R >= 24 gets a call of more than three tiles."""
    _, rng = fuzz(160, 2101)
    i = 0
    for R in range(1, 33):
        for res in (0, 1, 2, 3, 4):
            if res < 4:
                qs = [q for q in range(1, -(-256 // R) + 1) if q % 4 == res]
                q = int(rng.choice(qs))
                Ta = int(rng.integers((q - 1) * R + 1, min(256, q * R) + 1))
            else:
                Ta = int(rng.integers(1, R)) if R % 2 == 0 else 256
            heavy = i % 5 == res % 5 and i < 5 * 28                # 28 cases with a K edge; the rest K = 1 ... 3
            K, digits = K_EDGES[(i // 5) % 14] if heavy else (int(rng.integers(1, 4)), 1 + i % 2)
            D = DECIMS[(i // 5 + i) % 6] if heavy else DECIMS[i % 4]
            if i in (33, 98):
                D, K, digits = 64, 8, 2                            # G = 3
            if i in (66, 131):
                D, K, digits = 64, 32, 1 + (i == 131)              # G = 2
            T = TAPS[(3 * i + i // 8) % 8]
            S = 1 if K > 5 else 2
            h, ii = front(rng, T, S, K, digits)
            mode, cplx = i % 4, (i // 4) % 2 == 1
            gr, gi = chan_taps(rng, Ta, cplx)
            shift = shift_for(h, ii, int(rng.choice([256, 2048, 16384])))
            P = NB_BLOCKS[i % 3]
            c = NS(kind="narrow", i=i, R=R, K=K, digits=digits, D=D, T=T, Ta=Ta, S=S, h=h, incs=ii, P=P, mode=mode, cplx=cplx, gr=gr,
                   gi=gi, shift=shift, chan_shift=chan_shift_for(h, ii, shift, gr, gi, int(rng.choice([256, 4096, 16384]))),
                   gain=int(rng.integers(1, 65536)), G=groups(D, T, K), na=narrow_na(Ta, R), Q=narrow_q(Ta, R), squelch=0)
            first = 8 * -(-(T + D * (Ta + 2 * R)) // 4)
            c.long_tiles = R >= 24 and res == 1
            aud = 3 * c.na + 7 if c.long_tiles else int(rng.integers(20, 300 if D > 6 else 700))
            if D * R * aud > 400000:
                aud = max(4, 400000 // (D * R))
            c.sizes = [8 * int(rng.integers(1, 20)), first, 8 * -(-D * R * aud // 4), 8 * int(rng.integers(1, 3 + D * R // 2)),
                       8 * -(-D * R * int(rng.integers(5, 80)) // 4)]
            c.seed = int(rng.integers(0, 1 << 31))
            c.use_squelch = i % 3 != 2
            i += 1
            yield c


def narrow_edges(P, mode):
    """Audio ends on j P - 1, j P, j P + 1.  P = 16: calls of several 256-sample tiles that start inside a block (17 blocks in a
    tile).  P = 4096: one block open across many calls.  Loud and quiet stretches around a squelch between them."""
    rng = np.random.default_rng(2202 + P + mode)
    D, T, Ta, R, K = 4, 27, 9, 2, 3
    h, ii = front(rng, T, 2, K, 2)
    if P == 16:
        ends = [P - 1, P, P + 1, 3 * P - 1, 3 * P + 5 + 3 * 256, 3 * P + 5 + 3 * 256 + 11, 64 * P, 64 * P + 1, 70 * P - 1, 70 * P + 600, 112 * P]
    else:
        ends = [300, 1000, 2000, 3000, P - 1, P, P + 1, P + 500, P + 2500, 2 * P - 1, 2 * P + 1, 3 * P, 3 * P + 700]
    gr, gi = chan_taps(rng, Ta, mode != 2)
    shift = shift_for(h, ii, 16384)
    ys = [y_for_audio(Ta, R, n) for n in ends]
    c = NS(kind="narrow", R=R, K=K, D=D, T=T, Ta=Ta, S=2, h=h, incs=ii, P=P, mode=mode, gr=gr, gi=gi, shift=shift,
           chan_shift=chan_shift_for(h, ii, shift, gr, gi, 16384), gain=300, G=groups(D, T, K), na=narrow_na(Ta, R), ends=ends,
           sizes=sizes_for_outputs(T, D, ys))
    c.data = loud_quiet(rng, 2, sum(c.sizes), 2 * D * R * (40 if P == 16 else 3000))
    c.data[1] = c.data[1][::-1]
    c.squelch = 0
    return c


def narrow_short(R):
    """Ta = 256: calls that complete audio with 1, Ta - 1 and Ta second-stage inputs, then a long call."""
    rng = np.random.default_rng(2303 + R)
    D, T, Ta, K, P = 4, 26, 256, 5, 16
    h, ii = front(rng, T, 2, K, 2)
    ends = short_ends(Ta, R, (1, Ta - 1, Ta, 1))
    gr, gi = chan_taps(rng, Ta, True)
    shift = shift_for(h, ii, 2048)
    return NS(kind="narrow", R=R, K=K, D=D, T=T, Ta=Ta, S=2, h=h, incs=ii, P=P, mode=1, gr=gr, gi=gi, shift=shift,
              chan_shift=chan_shift_for(h, ii, shift, gr, gi, 256), gain=256, squelch=0, ends=ends, sizes=sizes_for_outputs(T, D, ends),
              seed=int(rng.integers(0, 1 << 31)))


def narrow_threshold(mode):
    """T = 1, h = [1], decim 2, shift 0, one channel tap 1, chan_shift 0: u is the centred byte pair of every second sample.
    Blocks of 16 samples with |u|^2 = 25 each ((3, 4), (5, 0), (4, 3)) have E = 400 = 5^2 * 16: exact equality at squelch 5.  A
    block with (7, 0) and (0, 0) in place of two of them has E = 399, one with (5, 1) in place of one has E = 401."""
    rng = np.random.default_rng(2404 + mode)
    P = 16
    kinds = [0, -1, 1, 0, 0, 1, -1, -1, 0, 1, 1, 0]
    u = []
    for kd in kinds:
        blk = [[(3, 4), (5, 0), (4, 3), (0, 5), (-3, 4), (-5, 0), (4, -3)][int(x)] for x in rng.integers(0, 7, P)]
        if kd == -1:
            blk[3], blk[9] = (7, 0), (0, 0)
        if kd == 1:
            blk[6] = (5, 1)
        u += blk
    u = np.array(u)
    b = np.empty(4 * u.shape[0], np.uint8)
    b[0::4], b[1::4] = u[:, 0] + 127, u[:, 1] + 127
    b[2::4], b[3::4] = rng.integers(0, 256, u.shape[0]), rng.integers(0, 256, u.shape[0])       # never read: decim 2, one tap
    ii = np.array([[0, 1 << 31]], np.uint32)
    want = [kd >= 0 for kd in kinds]
    return NS(kind="narrow", R=1, K=2, D=2, T=1, Ta=1, S=1, h=np.ones(1, np.int16), incs=ii, P=P, mode=mode, gr=np.ones(1, np.int16),
              gi=None, shift=0, chan_shift=0, gain=4000, squelch=5, data=b[None, :], kinds=kinds, want_open=want,
              sizes=[4 * P * 2 + 8, 4 * P * 3 - 8, 4 * P * 4 + 16, 4 * P * 3 - 16])


def narrow_extreme(mode):
    """FM: gain 65535 and |u| up to 16384, where the discriminator's i32 arithmetic wraps and its i16 value takes every value,
    -32768 among them.  AM: full-scale bytes through maximal taps at the smallest shifts, a = isqrt(ur^2 + ui^2) near 23170."""
    rng = np.random.default_rng(2505 + mode)
    D, T, R, P = 2, 16, 1, 16
    h = np.full(T, 2047, np.int16)
    ii = np.zeros((1, 1), np.uint32)
    shift = shift_for(h, ii, 16384)
    gr = np.array([16383, 16383, 16383, 16383], np.int16)
    n = 8 * 6000
    b = np.empty((1, n), np.uint8)
    if mode == 2:
        r = np.repeat(np.where(rng.random(n // 128 + 1) < 0.5, 0, 255), 64)[:n // 2]
        b[0, 0::2], b[0, 1::2] = r, np.where(rng.random(n // 2) < 0.03, 255 - r, r)
    else:
        b[0, 0::2] = np.repeat(np.where(rng.random(n // 16 + 1) < 0.5, 0, 255), 8)[:n // 2]
        b[0, 1::2] = np.repeat(np.where(rng.random(n // 24 + 1) < 0.5, 0, 255), 12)[:n // 2]
    return NS(kind="narrow", R=R, K=1, D=D, T=T, Ta=4, S=1, h=h, incs=ii, P=P, mode=mode, gr=gr, gi=None, shift=shift,
              chan_shift=chan_shift_for(h, ii, shift, gr, None, 16384), gain=65535, squelch=0, data=b, sizes=[n // 2, n // 2])


# ---- channelizer ---------------------------------------------------------------------------------------------------------------

def channelizer_sweep():
    """The K edges x both digit forms, with D and T walking their lists so that G = 4, 3 and 2 all occur; one call of several
    tiles in every case."""
    n_cases, rng = fuzz(28, 3101)
    for i in range(n_cases):
        K, digits = K_EDGES[i % 14]
        D = DECIMS[(i + i // 14 + i // 6) % 6]
        T = TAPS[(3 * i + i // 8) % 8]
        if i % 14 == 2:
            D, K, digits = 64, 8, 1 + (i // 14) % 2                # G = 3
        if i % 14 == 13:
            D = 64                                                 # K = 32: G = 2
        S = 1 if K > 9 else 2
        h, ii = front(rng, T, S, K, digits)
        G = groups(D, T, K)
        c = NS(kind="channelizer", i=i, K=K, digits=digits, D=D, T=T, S=S, h=h, incs=ii, G=G,
               shift=shift_for(h, ii, 16384 if i % 3 else 2048))
        tiles = int(rng.integers(3, 7))
        c.sizes = [8 * int(rng.integers(1, (T + 2 * D) // 4 + 3)), 8 * -(-(T + D * (64 * G * tiles + int(rng.integers(1, 64)))) // 4),
                   8 * int(rng.integers(1, 40)), 8 * -(-D * (64 * G + int(rng.integers(1, 64))) // 4)]
        c.tiles = tiles
        c.seed = int(rng.integers(0, 1 << 31))
        yield c


# ---- uniform channelizer -------------------------------------------------------------------------------------------------------

UV_TABLE_BYTES = 2048                                              # the NCO table beside the staged bytes
UV_HOPS = tuple(range(8, 257, 8))
UV_CELLS = tuple((R, G) for G in (8, 4) for R in (1, 2, 4))
UV_K_EDGES = [(k, 2) for k in (16, 17, 32, 33)] + [(k, 1) for k in (32, 33, 64, 65)]
UV_G_EDGES = ((240, 1248), (240, 1249), (248, 224), (248, 225))    # hop, T: G = 8 | 4 on the two sides of each pair
UV_LIMITS = (16384, 2048, 256)


def uniform_plan(K, digits, hop, T):
    """(R, G, nrt, nkc, lds_bytes) of a uniform channelizer with K selected channels: row tiles of 4 channels with
    two-digit taps and of 8 with one-digit taps; R = 1, 2, 4 row tiles per batch for up to 4, up to 8, more row tiles; K chunks of
    64 bytes over the frame's 2 T; G = 8 column groups where the staged bytes of 16 G frames -- 2 hop (16 G - 1) + 64 nkc, in whole
    256-byte rows -- and the NCO table fit 64 KiB, else 4."""
    nrt = -(-K // (4 if digits == 2 else 8))
    nkc = -(-2 * T // 64)
    R = 4 if nrt > 8 else (2 if nrt > 4 else 1)
    raw = lambda G: (2 * hop * (16 * G - 1) + 64 * nkc + 255) & ~255
    G = 8 if raw(8) + UV_TABLE_BYTES <= 65536 else 4
    return R, G, nrt, nkc, raw(G) + UV_TABLE_BYTES


def uniform_taps(rng, T, digits):
    """Prototype taps of the wanted digit form for ANY selection: |h| <= 127 keeps every |W| <= 127; one tap at +-2047 puts the
    larger of |Wr|, |Wi| of every channel at 1447 or more."""
    if digits == 1:
        return rng.integers(-127, 128, T).astype(np.int16)
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    h[int(rng.integers(0, T))] = 2047 * int(rng.choice([-1, 1]))
    return h


def uniform_handle(c, fmd):
    """The handle of a uniform case; the smallest admissible shift is left to the handle to find."""
    return fmd.UniformChannelizer(c.h, c.N, c.hop, channels=c.sel, n_streams=c.S, shift=None if c.limit == 16384 else c.shift, device_id=0)


def uniform_refs(c, ur, check=None):
    return {s: ur.UniformRef(c.h, c.N, c.hop, c.shift, channels=c.sel, z=c.z) for s in (range(c.S) if check is None else check)}


def uniform_outputs(c):
    """(m before, m after) of every accepted call of a uniform case, by the arithmetic of include/fmd.h alone; a call that
    completes no output is refused and changes nothing."""
    out_of = lambda p: (p - c.T) // c.hop + 1 if p >= c.T else 0
    pos, acc = 0, []
    for n in c.sizes:
        if out_of(pos + n // 2) - out_of(pos) < 1:
            continue
        acc.append((out_of(pos), out_of(pos + n // 2)))
        pos += n // 2
    return acc


# hop: N, K, digits, T.  Every hop once; the rows marked G = 4 are the only ones where eight column groups do not fit.
UV_SHAPES = (
    (8, 256, 256, 2, 33),       # nrt = 64: the most row tiles
    (16, 64, 16, 2, 32),
    (24, 40, 17, 2, 24),        # T = hop; nrt = 5: R = 2 with a last batch of one
    (32, 64, 32, 2, 33),        # T = hop + 1
    (40, 96, 33, 2, 120),       # T = 3 hop; nrt = 9: R = 4 with a last batch of one
    (48, 64, 32, 1, 37),        # T < hop: no history
    (56, 100, 33, 1, 2047),
    (64, 128, 64, 1, 65),
    (72, 130, 65, 1, 72),
    (80, 256, 70, 2, 100),      # nrt = 18: five batches, wave 0 takes two, the last one holds two row tiles
    (88, 200, 85, 1, 300),      # nrt = 11: a last batch of three
    (96, 12, 12, 2, 2048),
    (104, 48, 21, 2, 416),
    (112, 96, 47, 1, 111),
    (120, 256, 130, 1, 121),    # nrt = 17: five batches, the last one holds one row tile
    (128, 2, 2, 2, 1),
    (136, 77, 18, 2, 700),
    (144, 150, 37, 2, 433),
    (152, 33, 33, 1, 152),
    (160, 256, 3, 1, 2048),
    (168, 90, 34, 2, 169),
    (176, 64, 40, 1, 1000),
    (184, 256, 66, 1, 185),
    (192, 20, 20, 2, 64),
    (200, 180, 35, 2, 400),
    (208, 97, 9, 1, 2047),
    (216, 50, 29, 2, 217),
    (224, 120, 45, 2, 96),
    (232, 255, 5, 2, 2048),     # the largest hop whose G is 8 at every T
    (240, 40, 17, 2, 1249),     # G = 4
    (240, 100, 33, 1, 1248),    # G = 8 with exactly 64 KiB of LDS
    (248, 60, 43, 2, 224),      # G = 8 with exactly 64 KiB of LDS; nrt = 11
    (248, 256, 65, 1, 225),     # G = 4
    (256, 80, 33, 2, 2048),     # G = 4 from here on
    (256, 64, 33, 1, 2047),
    (256, 32, 16, 2, 255),
    (256, 48, 32, 1, 257),
    (256, 7, 5, 2, 256),
)


def uniform_sweep():
    """One case per row of UV_SHAPES: all 32 hops, the six (R, G) cells in both digit forms, the K edges of both forms, partial
    last batches, the four shapes at the G edge, T at the chunk edges and around hop.  The shift is alternately the smallest
    admissible one (limit 16384) and a larger one (limits 2048, 256).  Calls: one shorter than T (refused; it exists only where
    T > hop, since a call is whole hops), one of three tiles and a part of a fourth, one of a single hop, one of a tile and a
    part.  Every second case, at least one of every cell among them, goes through the device path."""
    _, rng = fuzz(len(UV_SHAPES), 5101)
    for i, (hop, N, K, digits, T) in enumerate(UV_SHAPES):
        sel = None if K == N else np.sort(rng.choice(N, K, replace=False)).astype(np.uint32)
        h = uniform_taps(rng, T, digits)
        R, G, nrt, nkc, lds = uniform_plan(K, digits, hop, T)
        limit = UV_LIMITS[i % 3]
        tile, first = 16 * G, -(-T // hop)                         # hops of the stream's first output
        hops = ([first - 1] if T > hop else []) + [first - 1 + 3 * tile + int(rng.integers(1, tile)), 1, tile + int(rng.integers(1, tile))]
        yield NS(kind="uniform", i=i, N=N, hop=hop, T=T, K=K, sel=sel, digits=digits, h=h, S=3 if i % 5 == 0 and K <= 33 else 2,
                 limit=limit, shift=shift_for(h, ur.channel_incs(N, sel), limit), R=R, G=G, nrt=nrt, nkc=nkc, lds_bytes=lds, dev=i % 2 == 1,
                 refuses=T > hop, sizes=[2 * hop * n for n in hops], seed=int(rng.integers(0, 1 << 31)),
                 z=sr.z_direct)                                    # a few hundred outputs: the gather matrices are the quicker form


# ---- band-plan bank ------------------------------------------------------------------------------------------------------------

BP_BLOCKS = tuple(16 << i for i in range(9))                       # 16 ... 4096
BP_TILE = 256                                                      # audio samples per second-pass tile
BP_Q_EDGES = {True: (4, 5, 8, 9), False: (8, 9, 16, 17)}           # ceil(Ta / R) around the tap chunks: 4 complex or 8 real taps
# the stage-one shapes under the bank, one per instantiation: N, K, digits, hop, T (T > hop: a call of one hop is refused)
BP_STAGE1 = ((16, 3, 1, 8, 40), (40, 17, 2, 24, 50), (96, 33, 2, 48, 100), (8, 2, 1, 256, 257), (64, 17, 2, 256, 260), (80, 33, 2, 256, 257))


def bp_cpr(Ta, R, cplx):
    """Eight-dword tap chunks per polyphase row of the second pass: a row holds ceil(Ta / R) taps, a chunk four
    complex taps or eight real ones."""
    tpc = 4 if cplx else 8
    return -(-(-(-Ta // R)) // tpc)


def bp_pitch(Ta, R, cplx):
    """LDS row pitch in dwords: the tile's 256 cells and the padded taps' reach, odd."""
    return (BP_TILE + bp_cpr(Ta, R, cplx) * (4 if cplx else 8)) | 1


def bp_q_targets(R, cplx):
    """The ceil(Ta / R) a band-plan sweep takes at chan_decim R: the chunk edges, or the largest there is (Ta = 64) in place of
    those that Ta <= 64 cannot reach."""
    qmax = -(-64 // R)
    return sorted({min(q, qmax) for q in BP_Q_EDGES[cplx]})


def edge_taps(rng, Ta, cplx):
    """Taps at the edges of the rule: one component at +-16383 and sum |gr| + |gi| = 65535 exactly (every component at +-16383
    where fewer than five of them cannot reach that sum)."""
    cells = Ta * (2 if cplx else 1)
    if cells * 16383 <= 65535:
        mag = np.full(cells, 16383, np.int64)
    else:
        mag = rng.multinomial(65535 - 16383, np.ones(cells - 1) / (cells - 1)).astype(np.int64)
        mag = np.concatenate([[16383], np.minimum(mag, 16383)])
        while mag.sum() < 65535:                             # what the clip took goes to the smallest components
            i = int(np.argmin(mag))
            mag[i] += min(16383 - mag[i], 65535 - mag.sum())
        assert mag.sum() == 65535 and mag.max() == 16383
    g = (mag * rng.choice([-1, 1], cells))[rng.permutation(cells)]
    return g[:Ta].astype(np.int16), (g[Ta:].astype(np.int16) if cplx else None)


def bandplan_handle(c, fmd, squelch=None, S=None):
    """The bank of a band-plan case; a shift that the case claims to be the smallest legal one is left to the handle to find."""
    return fmd.BandPlanBank(c.h, c.N, c.hop, c.gr if c.gi is None else (c.gr, c.gi), c.R, mode=c.mode, channels=c.sel,
                            n_streams=c.S if S is None else S, block=c.P, squelch=c.squelch if squelch is None else squelch,
                            gain=c.gain, chan_shift=None if getattr(c, "auto_chan_shift", False) else c.chan_shift,
                            shift=None if getattr(c, "auto_shift", False) else c.shift, device_id=0)


def bandplan_refs(c, br, check=None, squelch=None, sel=None, mode=None, gain=None):
    return {s: br.BandPlanRef(c.h, c.N, c.hop, c.shift, c.gr, c.gi, c.mode if mode is None else mode, c.R, c.chan_shift, c.P,
                              c.squelch if squelch is None else squelch, c.gain if gain is None else gain,
                              channels=c.sel if sel is None else sel, z=getattr(c, "z", sr.z_corr))
            for s in (range(c.S) if check is None else check)}


def bandplan_probe_squelch(c, br, data):
    """A squelch between the loud and the quiet block RMS of the first selected channel over `data` (one stream); with fewer than
    two complete blocks, the RMS of all its samples."""
    first = [int(c.sel[0])] if c.sel is not None else [0]
    p = bandplan_refs(c, br, check=[0], squelch=0, sel=first, mode=br.IQ, gain=256)[0]
    u = p.feed(data)[0].astype(np.float64)
    e = (u ** 2).sum(axis=1)
    nblk = e.size // c.P
    if nblk < 2:
        return max(1, min(23170, int(np.sqrt(e.mean()))))
    rms = np.sqrt(e[:nblk * c.P].reshape(nblk, c.P).mean(axis=1))
    return max(1, min(23170, int(np.sqrt(max(1.0, rms.min()) * rms.max()))))


def bp_sizes(c, ms):
    """Byte counts of consecutive calls after which stage one has produced ms[0], ms[1], ... outputs in all (T > hop or ms[0] >= 1:
    output m completes with hop ceil(T / hop) + m hops)."""
    first = -(-c.T // c.hop)
    hops = [first - 1 + m for m in ms]
    assert hops[0] >= 1 and all(b > a for a, b in zip(hops[:-1], hops[1:]))
    return [2 * c.hop * (b - a) for a, b in zip([0] + hops[:-1], hops)]


def bandplan_sweep():
    """For every chan_decim R in 1 ... 8: complex and real tap counts with ceil(Ta / R) on both sides of the tap-chunk edges
    (bp_q_targets), one Ta below R (1 at R = 1) and Ta = 64; taps alternately filling the rule and at its edges; the four modes
    against both tap kinds; P walking 16 ... 4096; a random gain; chan_shift at the limits 256, 4096, 16384 (FM: 256 in every
    second FM case at least); the stage-one shift above its minimum in every third case; stage one cycling through the six
    instantiations of the uniform kernel.  Calls: a refused one (one hop, or -- every second case with Ta >= 2 -- Ta - 1 stage-one
    outputs, which complete no audio sample), the first that completes audio, one of more than three tiles of 256 audio samples,
    one of one or two stage-one outputs that completes an audio sample (fewer than Ta - 1 where Ta >= 4: the y history is rebuilt
    from old history plus new samples), one more."""
    _, rng = fuzz(80, 6101)
    i = 0
    for R in range(1, 9):
        specs = [(True, q) for q in bp_q_targets(R, True)] + [(False, q) for q in bp_q_targets(R, False)]
        specs += [(R % 2 == 1, "below"), (R % 2 == 0, 64)]
        for j, (cplx, q) in enumerate(specs):
            if q == "below":
                Ta = max(1, R - 1) if R < 4 else int(rng.integers(1, R))
            elif q == 64:
                Ta = 64
            else:
                Ta = int(rng.integers((q - 1) * R + 1, min(64, q * R) + 1))
            N, K, digits, hop, T = BP_STAGE1[i % 6]
            sel = np.sort(rng.choice(N, K, replace=False)).astype(np.uint32)
            h = uniform_taps(rng, T, digits)
            mode = (j + R) % 4
            rule = (j + j // 4 + R) % 2 == 0
            gr, gi = chan_taps(rng, Ta, cplx) if rule else edge_taps(rng, Ta, cplx)
            incs = ur.channel_incs(N, sel)
            raised = i % 3 == 1
            shift = shift_for(h, incs, int(rng.choice([256, 2048])) if raised else 16384)
            fm_keeps = mode == 1 and (i // 4) % 2 == 0
            cs_limit = 256 if fm_keeps else (256, 4096, 16384)[(i + i // 3) % 3]
            c = NS(kind="bandplan", i=i, j=j, R=R, Ta=Ta, cplx=cplx, q=-(-Ta // R), mode=mode, rule=rule, N=N, K=K, sel=sel, digits=digits,
                   hop=hop, T=T, h=h, gr=gr, gi=gi, S=2, P=BP_BLOCKS[i % 9], gain=int(rng.integers(1, 65536)), shift=shift,
                   shift_min=shift_for(h, incs, 16384), cs_limit=cs_limit, chan_shift=chan_shift_for(h, incs, shift, gr, gi, cs_limit),
                   uv=uniform_plan(K, digits, hop, T), cpr=bp_cpr(Ta, R, cplx), pitch=bp_pitch(Ta, R, cplx), squelch=0,
                   use_squelch=(i + i // 9) % 3 != 2, z=sr.z_direct, auto_shift=not raised,
                   auto_chan_shift=cs_limit == (256 if mode == 1 else 16384))
            e = 1 if R >= 2 and Ta >= 4 and i % 2 == 0 else 0      # the short call has 1 + e stage-one outputs
            m1 = Ta + R * int(rng.integers(0, 6)) + int(rng.integers(0, R))
            n2 = (m1 - Ta) // R + 1 + 3 * BP_TILE + int(rng.integers(1, BP_TILE))
            m2 = Ta + R * (n2 - 1) + R - 1 - e
            m3 = m2 + 1 + e
            m4 = m3 + R * int(rng.integers(5, 80)) + int(rng.integers(0, R))
            c.ms = [m1, m2, m3, m4]
            c.refused_outputs = Ta - 1 if Ta >= 2 and i % 2 == 1 else 0
            c.sizes = [2 * hop * (-(-T // hop) - 1 + c.refused_outputs)] + bp_sizes(c, c.ms)
            c.seed = int(rng.integers(0, 1 << 31))
            i += 1
            yield c


def bp_plan(c):
    """(mS, mE, nS, nE) of every accepted call of a band-plan case, as plan() gives them for the narrow-band bank."""
    return plan(NS(T=c.T, D=c.hop, Ta=c.Ta, R=c.R, sizes=c.sizes))


def bandplan_edges(P, mode, off=0):
    """Audio ends on j P - 1, j P and j P + 1, around a squelch between the loud and the quiet stretches of the bytes.  P = 16:
    calls of several tiles that start inside a block (17 blocks in a tile).  P = 256, the tile's length: with off = 0 the first
    calls end on block edges, so block and tile coincide; with off = 1 the first call ends one sample later, so every tile of the
    later calls holds the last sample of one block and 255 of the next.  P = 4096: one block open across many calls."""
    rng = np.random.default_rng(6202 + P + mode + 7 * off)
    N, hop, T, Ta, R = 16, 8, 27, 9, 2
    sel = np.array([0, 5, 11], np.uint32)
    h = uniform_taps(rng, T, 2)
    if P == 16:
        ends = [P - 1, P, P + 1, 3 * P - 1, 3 * P + 5 + 3 * 256, 3 * P + 5 + 3 * 256 + 11, 64 * P, 64 * P + 1, 70 * P - 1, 70 * P + 600, 112 * P]
    elif P == 256:
        ends = [P + off, 4 * P + off, 6 * P + off, 7 * P - 1, 7 * P, 7 * P + 1, 10 * P + 1, 12 * P]
    else:
        ends = [300, 1000, 2000, 3000, P - 1, P, P + 1, P + 500, P + 2500, 2 * P - 1, 2 * P + 1, 3 * P, 3 * P + 700]
    gr, gi = chan_taps(rng, Ta, mode != 2)
    incs = ur.channel_incs(N, sel)
    shift = shift_for(h, incs, 16384)
    c = NS(kind="bandplan", R=R, K=3, N=N, hop=hop, T=T, Ta=Ta, S=2, h=h, sel=sel, P=P, mode=mode, gr=gr, gi=gi, shift=shift,
           chan_shift=chan_shift_for(h, incs, shift, gr, gi, 16384), gain=300, ends=ends, off=off, squelch=0)
    c.sizes = bp_sizes(c, [y_for_audio(Ta, R, n) for n in ends])
    c.data = loud_quiet(rng, 2, sum(c.sizes), 2 * hop * R * {16: 40, 256: 300, 4096: 3000}[P])
    c.data[1] = c.data[1][::-1]
    return c


def bandplan_threshold(mode):
    """narrow_threshold on the band-plan bank: N = 2, hop 8, T = 1, h = [1], shift 0, one channel tap 1, chan_shift 0, so u is the
    centred first byte pair of every hop in both channels (inc 0 and 2^31: hop inc is a whole turn); the other 14 bytes of a hop
    are never read.  Blocks of 16 samples with E = 400 = 5^2 * 16, 399 and 401 against squelch 5."""
    t = narrow_threshold(mode)
    rng = np.random.default_rng(6404 + mode)
    pairs = t.data[0].reshape(-1, 4)[:, :2]
    b = rng.integers(0, 256, (pairs.shape[0], 16), dtype=np.uint8)
    b[:, :2] = pairs
    P = t.P
    return NS(kind="bandplan", R=1, K=2, N=2, hop=8, T=1, Ta=1, S=1, h=np.ones(1, np.int16), sel=None, P=P, mode=mode,
              gr=np.ones(1, np.int16), gi=None, shift=0, chan_shift=0, gain=4000, squelch=5, data=b.reshape(1, -1), kinds=t.kinds,
              want_open=t.want_open, sizes=[16 * (2 * P + 2), 16 * (3 * P - 2), 16 * (4 * P + 4), 16 * (3 * P - 4)])


def bandplan_extreme(mode):
    """narrow_extreme's front end and bytes (T = 16, every tap 2047, the smallest shifts, four channel taps of 16383, gain 65535,
    bytes at the rails) with hop 8 in place of decim 2, N = 2, channel 0 alone.  A byte lies within 128 of the centre and the
    shifts are sized for 256, so a component of y and of u reaches half of its bound of 16384: |ur|, |ui| <= 8188, and
    a = isqrt(ur^2 + ui^2) reaches sqrt 2 times that, not 23170.  FM at that |u|: the discriminator's i32 products wrap and the
    output takes both rails."""
    e = narrow_extreme(mode)
    sel = np.array([0], np.uint32)
    n = e.data.shape[1] // 16 * 16
    return NS(kind="bandplan", R=1, K=1, N=2, hop=8, T=e.T, Ta=4, S=1, h=e.h, sel=sel, P=16, mode=mode, gr=e.gr, gi=None, shift=e.shift,
              chan_shift=e.chan_shift, gain=65535, squelch=0, data=e.data[:, :n], sizes=[n // 2, n // 2])


# ---- what a case reaches -------------------------------------------------------------------------------------------------------

def calls(c):
    """The byte arrays [S, n] of the case's calls: slices of c.data where the case brings its own, seeded random bytes otherwise."""
    if hasattr(c, "spans"):                                        # a refused call's bytes come again as the head of the next call
        return [c.data[:, a:b] for a, b in c.spans]
    if hasattr(c, "data"):
        assert c.data.shape[1] == sum(c.sizes)
        cuts = np.cumsum([0] + list(c.sizes))
        return [c.data[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    rng = np.random.default_rng(c.seed)
    return [bytes_(rng, c.S, n) for n in c.sizes]


def plan(c):
    """(mS, mE, nS, nE) of every accepted call of a stereo or narrow case -- second-stage inputs and audio samples before and after
    it -- by the arithmetic of include/fmd.h alone; a call that completes no audio sample is refused and changes nothing."""
    out_of = lambda p: (p - c.T) // c.D + 1 if p >= c.T else 0
    aud_of = lambda m: (m - c.Ta) // c.R + 1 if m >= c.Ta else 0
    pos, acc = 0, []
    for n in c.sizes:
        mS, mE = out_of(pos), out_of(pos + n // 2)
        if aud_of(mE) - aud_of(mS) < 1:
            continue
        acc.append((mS, mE, aud_of(mS), aud_of(mE)))
        pos += n // 2
    return acc


def edge_facts(ends_pairs, P):
    """Of (start, end) counts per call: which of j P - 1, j P, j P + 1 the ends land on, the most calls that end inside one block,
    the most whole blocks in one call, whether a call starts exactly on an edge."""
    rel = {e - P * round(e / P) for _, e in ends_pairs if e >= P - 1 and abs(e - P * round(e / P)) <= 1}
    inside = {}
    for _, e in ends_pairs:
        if e % P:
            inside[e // P] = inside.get(e // P, 0) + 1
    whole = max(e // P - -(-s // P) for s, e in ends_pairs)
    return NS(rel=rel, open_calls=max(inside.values()), whole=whole, starts_on_edge=any(s % P == 0 and s > 0 for s, _ in ends_pairs))


def straddles(c):
    """(first, last): a first-pass tile of the stereo case c whose FIRST column is the last sample of a block, and a full tile
    whose LAST column is the first sample of a block."""
    first = last = False
    for mS, mE, _, _ in plan(c):
        for o0 in range(0, mE - mS, c.tile):
            no = min(c.tile, mE - mS - o0)
            first |= no >= 2 and (mS + o0) % c.P == c.P - 1
            last |= no == c.tile and (mS + o0 + no - 1) % c.P == 0
    return first, last
