"""The package bank's cases: the inputs of tests/test_gpu_packages.py on the record level, with what tests/packages_ref.py (the
definition) makes of them.  Every case says what it is there to exercise, and `check_case` holds the definition's result to that -- a
case that stopped exercising its edge fails on the CPU (tests/test_packages.py), not silently on the GPU.

The settings: short 10, long 30, tol 3, reset 100.  PWM judges the width (10: a 1, 30: a 0, 20: bad), PPM the gap (10: a 0, 30: a 1,
50: bad).  A gap of 200 opens a package.  A call has 100000 samples per stream; record i of a call falls at sample 50 (i + 1)."""
import functools
from collections import namedtuple

import numpy as np

import packages_ref as ref

N_SAMPLES = 100000
SHORT, LONG, TOL, RESET = 10, 30, 3, 100
OPENS = 200                                                  # a gap that opens a package
Case = namedtuple("Case", "name cfg n_streams calls want")
Call = namedtuple("Call", "counts recs totals n_samples flush")   # recs: uint32 [n_streams, rec_cap, 4]; totals: dicts per stream


def cfg(modulation="pwm", short=SHORT, long=LONG, tol=TOL, reset=RESET, min_bits=0, pkg_cap=1025):
    return {"modulation": modulation, "short": short, "long": long, "tol": tol, "reset": reset, "min_bits": min_bits, "pkg_cap": pkg_cap}


def pulses(modulation, bits, opens=True, width=5):
    """(width, gap) of the records that carry `bits`: PWM a record per bit, PPM one more in front.  The first has a gap of OPENS if
    `opens`, else one that continues the package (PPM: and carries the first bit then, so there is no extra record)."""
    if modulation == "pwm":
        out = [(SHORT if b else LONG, 20) for b in bits]
        if opens and out:
            out[0] = (out[0][0], OPENS)
        return out
    out = [(width, LONG if b else SHORT) for b in bits]
    return [(width, OPENS)] + out if opens else out


BAD_REC = {"pwm": (20, 20), "ppm": (5, 50)}                 # continues the package and fits neither window


def build(n_streams, rows, idle=None, samples=None, counts=None, rec_cap=None, behind=None, n_samples=N_SAMPLES):
    """One call.  rows: per stream a list of (width, gap); idle: per stream (state, run), default (1, 0): no close; samples: per stream
    the total after the call; counts: per stream, default len(row); behind: a (width, gap) that fills each row behind its records."""
    cap = rec_cap or max([1] + [len(r) for r in rows])
    recs = np.zeros((n_streams, cap, 4), np.uint32)
    if behind is not None:
        recs[:, :, 0], recs[:, :, 1], recs[:, :, 2] = 7, behind[0], behind[1]
    for s, row in enumerate(rows):
        for i, (w, g) in enumerate(row[:cap]):
            recs[s, i] = (50 * (i + 1), w, g, 0)
    idle = idle or [(1, 0)] * n_streams
    samples = samples or [n_samples] * n_streams
    totals = [{"samples": samples[s], "state": idle[s][0], "run": idle[s][1]} for s in range(n_streams)]
    return Call([len(r) for r in rows] if counts is None else list(counts), recs, totals, n_samples, False)


FLUSH = Call(None, None, None, 0, True)


def later(call, k):
    """`call` as the k-th call of its streams (k = 0: the first): the totals' samples move on."""
    return call._replace(totals=[dict(t, samples=t["samples"] + k * call.n_samples) for t in call.totals])


def rows_of(call, s):
    return [{"k_rel": int(r[0]), "width": int(r[1]), "gap": int(r[2]), "level": int(r[3])} for r in call.recs[s]]


EDGE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129)
BOUNDARY_AT = (0, 1, 63, 64, 127)


def _bits(n, seed):
    return np.random.default_rng(seed).integers(0, 2, n).tolist()


def _edges(modulation, how):
    """A package of exactly n pulses per stream, closed by the next record or by idle."""
    n_bits = lambda n: n if modulation == "pwm" else n - 1
    rows = [pulses(modulation, _bits(n_bits(n), n)) for n in EDGE_SIZES]
    if how == "next":
        rows = [r + [(SHORT, OPENS)] for r in rows]
    idle = [(0, RESET)] * len(rows) if how == "idle" else None
    want = {"count": [[1] * len(rows)], "n_pulses": list(EDGE_SIZES), "n_bits": [n_bits(n) for n in EDGE_SIZES], "open": int(how == "next")}
    return cfg(modulation), len(rows), [build(len(rows), rows, idle)], want


def _boundary(carried):
    """130 records with the one that opens a package at index b; with a package of 3 pulses carried in, or none."""
    rows = []
    for b in BOUNDARY_AT:
        w = pulses("pwm", _bits(130, b), opens=False)
        w[b] = (w[b][0], OPENS)
        rows.append(w)
    calls = [build(5, [pulses("pwm", [1, 0, 1])] * 5)] if carried else []
    calls.append(later(build(5, rows), len(calls)))
    # without a carry the boundary at 0 closes nothing; one at b > 0 closes the package that record 0 opened
    count = [1] * 5 if carried else [0, 1, 1, 1, 1]
    pulses_first = [3 + b for b in BOUNDARY_AT] if carried else [None] + list(BOUNDARY_AT[1:])
    return cfg(), 5, calls, {"count_last": count, "first_n_pulses": pulses_first}


def _bad():
    """Streams 0-2: a bad record at index 0, 63, 64 of a package of 130 PWM pulses that the next call's first record closes.  Stream
    3: a package goes BAD in call 0 and good records follow in call 1.  Stream 4: the package's first PWM record is bad."""
    rows0 = []
    for b in (0, 63, 64):
        w = pulses("pwm", [1] * 130)
        w[b] = (20, OPENS if b == 0 else 20)
        rows0.append(w)
    rows0.append(pulses("pwm", [1, 1, 0]) + [BAD_REC["pwm"]] + pulses("pwm", [1, 1], opens=False))
    rows0.append([(20, OPENS), (SHORT, 20)])
    rows1 = [[(SHORT, OPENS)]] * 3 + [pulses("pwm", [1] * 70, opens=False) + [(SHORT, OPENS)]] + [[(SHORT, OPENS)]]
    want = {"n_bits": [0, 63, 64, 3, 0], "n_pulses": [130, 130, 130, 76, 2], "flags": [ref.BAD] * 5}
    return cfg(), 5, [build(5, rows0), later(build(5, rows1), 1)], want


def _ppm_first():
    """A PPM package's first record has a gap that fits nothing: it only opens the package (not BAD).  Stream 1: the same record
    inside a package is BAD."""
    rows = [[(5, 50 + RESET)] + pulses("ppm", [1, 0, 1], opens=False), pulses("ppm", [1, 0]) + [BAD_REC["ppm"]] + pulses("ppm", [1], opens=False)]
    return cfg("ppm"), 2, [build(2, rows, [(0, RESET)] * 2)], {"flags": [0, ref.BAD], "n_bits": [3, 2], "n_pulses": [4, 5]}


def _tolerance(which):
    t = TOL
    if which == "edges":                                     # short -+ tol inside, -+ (tol + 1) outside; the same at long
        widths = [SHORT - t, SHORT + t, LONG - t, LONG + t, SHORT - t - 1]
        rows = [[(w, OPENS if i == 0 else 20) for i, w in enumerate(widths)], [(SHORT + t + 1, OPENS), (SHORT, 20)],
                [(LONG - t - 1, OPENS)], [(LONG + t + 1, OPENS)]]
        return cfg(), 4, [build(4, rows, [(0, RESET)] * 4)], {"n_bits": [4, 0, 0, 0], "flags": [ref.BAD] * 4, "bits0": [1, 1, 0, 0]}
    if which == "overlap":                                   # windows 5 ... 15 and 7 ... 17: short wins where both fit
        rows = [[(11, OPENS), (16, 20), (7, 20), (15, 20), (5, 20), (17, 20)]]
        return cfg(short=10, long=12, tol=5), 1, [build(1, rows, [(0, RESET)])], {"n_bits": [6], "flags": [0], "bits0": [1, 0, 1, 1, 1, 0]}
    if which == "zero":
        rows = [[(SHORT, OPENS), (LONG, 20), (SHORT + 1, 20), (SHORT, 20)]]
        return cfg(tol=0), 1, [build(1, rows, [(0, RESET)])], {"n_bits": [2], "flags": [ref.BAD], "bits0": [1, 0]}
    rows = [[(SHORT, 2 ** 32 - 1), (0, 20), (2 ** 32 - 1, 20), (LONG, 20)]]      # tol = 2^32 - 1: everything is near short
    return cfg(tol=2 ** 32 - 1), 1, [build(1, rows, [(0, RESET)])], {"n_bits": [4], "flags": [0], "bits0": [1, 1, 1, 1]}


TRUNC_SIZES = (255, 256, 257, 300)


def _truncation():
    """255, 256, 257 and 300 bits in one call (streams 0-3) and 300 as 200 + 100 across two calls (stream 4), PWM and PPM."""
    out = {}
    for m in ("pwm", "ppm"):
        bits = [_bits(n, 40 + n) for n in TRUNC_SIZES] + [_bits(300, 77)]
        rows0 = [pulses(m, b) for b in bits[:4]] + [pulses(m, bits[4][:200])]
        rows1 = [[]] * 4 + [pulses(m, bits[4][200:], opens=False)]
        calls = [build(5, rows0), later(build(5, rows1, [(0, RESET)] * 5), 1)]
        extra = 0 if m == "pwm" else 1
        want = {"n_bits": [255, 256, 256, 256, 256], "flags": [0, 0, ref.TRUNCATED, ref.TRUNCATED, ref.TRUNCATED],
                "n_pulses": [n + extra for n in TRUNC_SIZES + (300,)], "bits": [b[:256] for b in bits]}
        out[m] = (cfg(m), 5, calls, want)
    return out


def _every_record_closes(pkg_cap):
    """A one-pulse package carried in, then 64, 65 and 1024 records that each open a package: R closes, and one more by idle in the
    streams 3-5: R + 1 = packages_max(R)."""
    sizes = (64, 65, 1024) * 2
    rows = [[(SHORT if i % 3 else LONG, OPENS + i) for i in range(n)] for n in sizes]
    idle = [(1, 0)] * 3 + [(0, RESET)] * 3
    calls = [build(6, [[(LONG, OPENS)]] * 6), later(build(6, rows, idle), 1)]
    return cfg(pkg_cap=pkg_cap), 6, calls, {"count_last": [64, 65, 1024, 65, 66, 1025], "kept": pkg_cap}


def _reading_limits():
    """Stream 0: count 5000 at rec_cap 64 reads 64 records.  Stream 1: count 3, and behind the three records sentinels that would each
    open a package with a bad pulse if they were read."""
    rows = [pulses("pwm", _bits(64, 9)), pulses("pwm", [1, 0, 1])]
    call = build(2, rows, [(0, RESET)] * 2, counts=[5000, 3], rec_cap=64, behind=(20, OPENS))
    return cfg(), 2, [call], {"count": [[1, 1]], "n_pulses": [64, 3], "records": [64, 3]}


def _idle():
    """Streams: state 1 with a long run (stays open), state 0 at reset - 1 (stays open), state 0 at reset (closes), state 0 and a run
    beyond 2^32 (closes).  Then a call of no records that closes the first two, then nothing is open, then flush closes what a third
    call opened."""
    rows = [pulses("pwm", [1, 0])] * 4
    a = build(4, rows, [(1, 10 ** 6), (0, RESET - 1), (0, RESET), (0, 2 ** 32 + 5)])
    b = later(build(4, [[]] * 4, [(0, RESET), (0, 2 ** 40), (0, RESET), (1, 0)]), 1)
    c = later(build(4, [pulses("pwm", [1])] * 4, [(1, 0), (0, RESET - 1), (0, 0), (1, 5)]), 2)
    return cfg(), 4, [a, b, c, FLUSH, FLUSH], {"count": [[0, 0, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0]]}


def _min_bits(min_bits):
    """Packages of 0 (a bad first pulse), 1, 23, 24, 25, 256 and 300 bits, each closed by the next; the last by idle."""
    sizes = (0, 1, 23, 24, 25, 256, 300)
    row = []
    for n in sizes:
        row += pulses("pwm", _bits(n, n)) if n else [(20, OPENS)]
    kept = [n for n in sizes if min(n, 256) >= min_bits]
    want = {"count": [[len(kept)]], "n_bits_all": [min(n, 256) for n in kept], "skipped": len(sizes) - len(kept), "packages": len(sizes)}
    return cfg(min_bits=min_bits), 1, [build(1, [row], [(0, RESET)])], want


def _start():
    """Stream 0: a first pulse wider than its fall's position: start clamps to 0.  Stream 1: pos beyond 2^32.  Stream 2: pos + k_rel
    crosses 2^32."""
    rows = [[(80, OPENS), (SHORT, 20)], [(SHORT, OPENS)], [(SHORT, OPENS)]]
    samples = [N_SAMPLES, 2 ** 33 + 12345 + N_SAMPLES, 2 ** 32 - 20 + N_SAMPLES]
    want = {"start": [0, 2 ** 33 + 12345 + 50 - SHORT, 2 ** 32 - 20 + 50 - SHORT]}
    return cfg(), 3, [build(3, rows, [(0, RESET)] * 3, samples=samples)], want


def _random_rows(rng, n_streams, modulation, max_n, empty_every=3):
    rows = []
    for s in range(n_streams):
        n = 0 if s % empty_every == 1 else int(rng.integers(1, max_n + 1))
        pick = lambda: int(rng.choice([SHORT, LONG, SHORT + TOL, LONG - TOL, 20 if modulation == "pwm" else 50], p=[.35, .35, .1, .1, .1]))
        row = []
        for i in range(n):
            v, opens = pick(), rng.random() < 0.06
            row.append((v, OPENS if opens else 20) if modulation == "pwm" else (5, OPENS if opens else v))
        rows.append(row)
    return rows


def _streams(n_streams, modulation="pwm", n_calls=2, max_n=150, seed=None):
    """Different counts, every third stream empty, packages across the calls, some closed by idle."""
    rng = np.random.default_rng(1000 + n_streams if seed is None else seed)
    calls = []
    for k in range(n_calls):
        rows = _random_rows(rng, n_streams, modulation, max_n)
        idle = [(int(rng.integers(0, 2)), int(rng.choice([0, RESET - 1, RESET, 5000]))) for _ in range(n_streams)]
        calls.append(later(build(n_streams, rows, idle, rec_cap=max_n), k))
    return cfg(modulation, min_bits=2 if n_streams == 65 else 0), n_streams, calls, {"streams": n_streams}


def _table():
    t = {}
    for m in ("pwm", "ppm"):
        for how in ("next", "idle"):
            t["edges_%s_%s" % (m, how)] = _edges(m, how)
    t["boundary_fresh"], t["boundary_carried"] = _boundary(False), _boundary(True)
    t["bad"], t["ppm_first"] = _bad(), _ppm_first()
    for which in ("edges", "overlap", "zero", "max"):
        t["tol_" + which] = _tolerance(which)
    for m, c in _truncation().items():
        t["truncation_" + m] = c
    for cap in (1, 4, 64, 1025):
        t["closes_cap_%d" % cap] = _every_record_closes(cap)
    t["reading_limits"], t["idle"], t["start"] = _reading_limits(), _idle(), _start()
    for mb in (0, 1, 24, 256):
        t["min_bits_%d" % mb] = _min_bits(mb)
    for n in (1, 3, 64, 65, 257):
        t["streams_%d" % n] = _streams(n, "ppm" if n == 3 else "pwm")
    t["host_rows"] = _streams(5, "pwm", n_calls=6, max_n=40, seed=5)       # (no call closes more than 64: the C slicer's ring holds them)
    t["host_rows_ppm"] = _streams(5, "ppm", n_calls=6, max_n=40, seed=6)
    return t


CASE_NAMES = ["edges_pwm_next", "edges_pwm_idle", "edges_ppm_next", "edges_ppm_idle", "boundary_fresh", "boundary_carried", "bad", "ppm_first",
              "tol_edges", "tol_overlap", "tol_zero", "tol_max", "truncation_pwm", "truncation_ppm", "closes_cap_1", "closes_cap_4",
              "closes_cap_64", "closes_cap_1025", "reading_limits", "idle", "start", "min_bits_0", "min_bits_1", "min_bits_24", "min_bits_256",
              "streams_1", "streams_3", "streams_64", "streams_65", "streams_257", "host_rows", "host_rows_ppm"]


@functools.lru_cache(maxsize=None)
def _cases():
    return {name: Case(name, *c) for name, c in _table().items()}


def case(name):
    return _cases()[name]


def all_cases():
    return [_cases()[n] for n in _cases()]


def ref_bank(c):
    g = c.cfg
    return ref.Bank(c.n_streams, ref.PWM if g["modulation"] == "pwm" else ref.PPM, g["short"], g["long"], g["tol"], g["reset"], g["min_bits"], g["pkg_cap"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """([(counts, kept packages per stream) per call], info) of the definition; computed once and shared: do not change it."""
    c = case(name)
    bank = ref_bank(c)
    per_call = []
    for call in c.calls:
        if call.flush:
            per_call.append(bank.flush())
        else:
            per_call.append(bank.run(call.counts, [rows_of(call, s) for s in range(c.n_streams)], call.recs.shape[1], call.totals, call.n_samples))
    return per_call, bank.info


def bits_of(k):
    return np.unpackbits(np.frombuffer(k["bits"], np.uint8))[:k["n_bits"]].tolist()


def check_case(name):
    """The definition's result has what the case is there for."""
    c = case(name)
    per_call, info = expected(name)
    w = c.want
    for call, (counts, pkgs) in zip(c.calls, per_call):
        assert len(counts) == c.n_streams and all(len(p) == min(n, c.cfg["pkg_cap"]) for n, p in zip(counts, pkgs))
        if not call.flush:
            read = [min(n, call.recs.shape[1]) for n in call.counts]
            assert all(n <= ref.packages_max(r) for n, r in zip(counts, read)), "more than R + 1 packages"
        for p in pkgs:
            for k in p:
                assert len(k["bits"]) == 32 and k["bits"][(k["n_bits"] + 7) // 8:] == bytes(32 - (k["n_bits"] + 7) // 8) and k["n_bits"] >= c.cfg["min_bits"]
    firsts = [next((p[s][0] for _, p in per_call if p[s]), None) for s in range(c.n_streams)]
    if "count" in w:
        assert [list(n) for n, _ in per_call] == w["count"], [list(n) for n, _ in per_call]
    if "count_last" in w:
        assert list(per_call[-1][0]) == w["count_last"], per_call[-1][0]
    for key in ("n_pulses", "n_bits", "flags", "start"):
        if key in w:
            assert [k[key] for k in firsts] == w[key], (key, [k[key] for k in firsts])
    if "first_n_pulses" in w:
        assert [k["n_pulses"] if k else None for k in firsts] == w["first_n_pulses"]
    if "bits0" in w:
        assert bits_of(firsts[0]) == w["bits0"]
    if "bits" in w:
        assert [bits_of(k) for k in firsts] == w["bits"]
    if "open" in w:
        assert [i["open"] for i in info] == [w["open"]] * c.n_streams
    if "kept" in w:
        assert [len(p) for p in per_call[-1][1]] == [min(n, w["kept"]) for n in w["count_last"]]
        assert max(w["count_last"]) == ref.packages_max(1024) and info[5]["packages"] == 1025
    if "records" in w:
        assert [i["records"] for i in info] == w["records"] and all(not k["flags"] for k in firsts)
    if "n_bits_all" in w:
        assert [k["n_bits"] for k in per_call[0][1][0]] == w["n_bits_all"]
        assert info[0]["skipped"] == w["skipped"] and info[0]["packages"] == w["packages"] and info[0]["bad"] == 1
    if "streams" in w:
        counts = np.array([n for n, _ in per_call])
        assert counts.shape[1] == w["streams"] and counts.sum() > 0
        if w["streams"] >= 3:
            assert (counts.sum(axis=0) == 0).any() and len(set(c.calls[0].counts)) >= 3
            assert any(k["flags"] & ref.BAD for _, p in per_call for row in p for k in row) and any(i["open"] for i in info)
        if name.startswith("host_rows"):
            assert counts.max() <= 64 and counts.max() >= 2
    if name == "idle":
        assert [i["open"] for i in info] == [0] * 4
    if name == "bad":
        assert [i["bad"] for i in info] == [1] * 5
