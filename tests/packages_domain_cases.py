"""The package bank's domain cases: the inputs of tests/test_gpu_packages_domain.py with what the definitions make of them.

carry_grid, on the record level like tests/packages_cases.py: call 0 leaves a package of p bits open, call 1 appends n good records
and idle closes it -- one stream per (p, n), so that the carried 256 bits take a run of every length at every kind of bit offset: in
front of, on and behind each multiple of 32, and on either side of the end.  Some rows have a bad record right behind the n, and good
ones behind that, which give no bits.

composed, on the sample level: PulseBank.run_device then PackageBank.run_bank on many streams at a pulse_cap of 16 -- streams of
ook_encode packages of different lengths, one of which lies across the first cut, silent streams, and one stream with an edge on
every sample, whose count is far above pulse_cap.  The expectation chains tests/pulses_ref.py into tests/packages_ref.py.

`check_case` / `check_composed` hold the definitions' results to what the cases are there for (tests/test_packages_domain.py)."""
import functools
from collections import namedtuple

import numpy as np

import packages_ref as ref
import pulses_ref
from packages_cases import BAD_REC, RESET, Case, bits_of, build, cfg, later, pulses, ref_bank, rows_of

GRID_P = (0, 1, 5, 31, 32, 33, 63, 64, 65, 95, 97, 191, 223, 224, 225, 255, 256)
GRID_N = (1, 2, 31, 32, 33, 63, 64)
REC_CAP = 320
TRAILING = 3                                                 # good records behind a bad one


def grid_pairs():
    return [(p, n) for p in GRID_P for n in GRID_N]


def has_bad(p, n):
    return (GRID_P.index(p) + GRID_N.index(n)) % 3 == 0


def grid_bits(p, n):
    return np.random.default_rng([p, n]).integers(0, 2, p + n).tolist()


def _carry_grid(m):
    """PWM with p == 0 carries nothing in: a PWM package has a bit from its first pulse on, so call 1 opens the package itself."""
    rows0, rows1 = [], []
    for p, n in grid_pairs():
        bits = grid_bits(p, n)
        opened = m == "ppm" or p > 0
        rows0.append(pulses(m, bits[:p]) if opened else [])
        row = pulses(m, bits[p:], opens=not opened)
        if has_bad(p, n):
            row += [BAD_REC[m]] + pulses(m, [1] * TRAILING, opens=False)
        rows1.append(row)
    n_streams = len(rows0)
    calls = [build(n_streams, rows0, rec_cap=REC_CAP), later(build(n_streams, rows1, [(0, RESET)] * n_streams, rec_cap=REC_CAP), 1)]
    return Case("carry_grid_" + m, cfg(m), n_streams, calls, {"grid": m})


CASE_NAMES = ["carry_grid_pwm", "carry_grid_ppm"]


@functools.lru_cache(maxsize=None)
def case(name):
    assert name in CASE_NAMES, name
    return _carry_grid(name.rpartition("_")[2])


@functools.lru_cache(maxsize=None)
def expected(name):
    """([(counts, kept packages per stream) per call], info) of the definition; computed once and shared: do not change it."""
    c = case(name)
    bank = ref_bank(c)
    per_call = [bank.run(call.counts, [rows_of(call, s) for s in range(c.n_streams)], call.recs.shape[1], call.totals, call.n_samples)
                for call in c.calls]
    return per_call, bank.info


def check_case(name):
    c = case(name)
    per_call, info = expected(name)
    m = c.want["grid"]
    assert per_call[0][0] == [0] * c.n_streams and per_call[1][0] == [1] * c.n_streams and not any(i["open"] for i in info)
    assert max(len(rows_of(call, 0)) for call in c.calls) == REC_CAP >= max(max(call.counts) for call in c.calls)
    truncated = []
    for s, (p, n) in enumerate(grid_pairs()):
        k, bits, bad = per_call[1][1][s][0], grid_bits(p, n), has_bad(p, n)
        assert k["n_bits"] == min(p + n, 256), (name, p, n, k)
        assert k["flags"] == (ref.TRUNCATED if p + n > 256 else 0) | (ref.BAD if bad else 0), (name, p, n, k)
        assert bits_of(k) == bits[:256], (name, p, n)
        assert k["n_pulses"] == p + n + (1 if m == "ppm" else 0) + (1 + TRAILING if bad else 0), (name, p, n, k)
        assert c.calls[1].counts[s] == n + (1 + TRAILING if bad else 0)          # the n lie in one chunk of 64 records from lane 0 on
        if p + n > 256:
            truncated.append((p, n))
    assert truncated == [(p, n) for p, n in grid_pairs() if p + n > 256] and len(truncated) >= 12
    assert any(has_bad(p, n) for p, n in truncated) and any(has_bad(p, 64) for p in GRID_P) and any(not has_bad(p, 64) for p in GRID_P)
    return per_call, info


# ---- the kernel's placement of a run in the carried 256 bits, modelled -------------------------------------------------------------

def word_of(X, w, p, negative=True):
    """Big-endian word w of a 256-bit string that has X (a 64-bit number, its first bit at bit 63) at bit offset p."""
    d = 32 * w - p
    if d >= 0:
        return ((X << d) & (2 ** 64 - 1)) >> 32 if d < 64 else 0
    return (X >> -d) >> 32 if negative and d > -32 else 0


def appended(bits, p, negative=True):
    """The 256 bits after bits[:p] were there and bits[p:] (at most 64) are placed by word_of, as a list of 0 / 1."""
    words = [int("".join(map(str, (bits[:p] + [0] * 256)[32 * w:32 * w + 32])), 2) for w in range(8)]
    run = bits[p:]
    X = int("".join(map(str, run + [0] * (64 - len(run)))), 2)
    for w in range(8):
        words[w] |= word_of(X, w, p, negative)
    return [int(b) for w in words for b in format(w, "032b")]


# ---- composed on the device ------------------------------------------------------------------------------------------------------------

COMPOSED_STREAMS = (1, 4, 5, 65)
CALL = 2000                                                  # samples per call; three calls
PULSE_CFG = {"W": 1, "lo": 1000, "hi": 5000, "pulse_cap": 16}
SHORT, LONG, GAP, TOL, RESET_GAP = 4, 9, 5, 1, 40
Composed = namedtuple("Composed", "name modulation n_streams iq kinds")


@functools.lru_cache(maxsize=None)
def composed_case(n_streams, m):
    """uint8 [n_streams, 6 CALL].  Stream 2: an edge on every sample.  Streams 1, 5, 9 ...: silent.  The others: a package in every
    call, of 3 ... 11 bits, and one across the first cut; stream 0's package in the third call has 30 bits, more pulses than
    pulse_cap keeps."""
    import rtl_sdr_rs_amd as fmd
    iq = np.full((n_streams, 6 * CALL), 128, np.uint8)
    kinds = []
    rng = np.random.default_rng([n_streams, m == "ppm"])
    for s in range(n_streams):
        if n_streams >= 4 and s == 2:
            iq[s, 0::4] = 188
            kinds.append("edges")
        elif n_streams >= 4 and s % 4 == 1:
            kinds.append("silent")
        else:
            for k, at in enumerate((100 + 13 * s % 700, CALL - 12 - s % 8,2 * CALL - 400 + 7 * s % 300, 2 * CALL + 500 + s)):
                n = 30 if (s, k) == (0, 3) else 3 + (s + 2 * k) % 9
                e = fmd.ook_encode(rng.integers(0, 2, n).tolist(), m, SHORT, LONG, GAP)
                iq[s, 2 * at:2 * at + e.size] = e
            kinds.append("packages")
    return Composed("composed_%d_%s" % (n_streams, m), m, n_streams, iq, kinds)


@functools.lru_cache(maxsize=None)
def composed_expected(n_streams, m):
    """Per call (pulse counts, package counts, kept packages per stream, package info per stream), the last entry being the flush:
    tests/pulses_ref.py's streams chained into tests/packages_ref.py's bank with rec_cap = pulse_cap and the definition's own totals."""
    c = composed_case(n_streams, m)
    cap = PULSE_CFG["pulse_cap"]
    streams = [pulses_ref.Stream(PULSE_CFG["W"], PULSE_CFG["lo"], PULSE_CFG["hi"]) for _ in range(n_streams)]
    bank = ref.Bank(n_streams, ref.PWM if m == "pwm" else ref.PPM, SHORT, LONG, TOL, RESET_GAP, 0, cap + 1)
    out = []
    for k in range(3):
        res = [st.run(c.iq[s, 2 * CALL * k:2 * CALL * (k + 1)]) for s, st in enumerate(streams)]
        counts, recs = [n for n, _ in res], [r[:cap] for _, r in res]
        got = bank.run(counts, recs, cap, [dict(st.info) for st in streams], CALL)
        out.append((counts, got[0], got[1], bank.info))
    got = bank.flush()
    out.append((None, got[0], got[1], bank.info))
    return out


def check_composed(n_streams, m):
    c, out = composed_case(n_streams, m), composed_expected(n_streams, m)
    cap = PULSE_CFG["pulse_cap"]
    every = [[k for _, _, pkgs, _ in out for k in pkgs[s]] for s in range(n_streams)]
    crossing = [s for s in range(n_streams) if any(k["start"] < CALL and not k["flags"] for k in out[1][2][s])]      # closed by the second call
    assert crossing and all(c.kinds[s] == "packages" for s in crossing), (c.name, crossing)
    overflow = [s for s in range(n_streams) if any(counts[s] > cap for counts, _, _, _ in out[:3])]
    assert 0 in overflow and max(counts[0] for counts, _, _, _ in out[:3]) < 64
    for s, kind in enumerate(c.kinds):
        if kind == "silent":
            assert every[s] == [] and all(counts[s] == 0 for counts, _, _, _ in out[:3])
        elif kind == "edges":
            assert s in overflow and min(counts[s] for counts, _, _, _ in out[:3]) > 50 * cap
            assert out[3][3][s]["records"] == 3 * cap
        else:
            good = [k for k in every[s] if not k["flags"]]
            assert len(good) >= 3 and len({k["n_bits"] for k in good}) >= 2, (c.name, s, every[s])
    if n_streams >= 4:
        assert {"silent", "edges", "packages"} == set(c.kinds)
    assert not any(i["open"] for i in out[3][3])
    return out
