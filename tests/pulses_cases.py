"""The pulse bank's cases: the inputs of tests/test_gpu_pulses.py, built from seeds and levels, with what tests/pulses_ref.py (the
definition) makes of them.  Every case says what it is there to exercise, and `check_case` holds the definition's result to that -- a
case that stopped exercising its edge fails on the CPU (tests/test_pulses.py), not silently on the GPU.  T is the tile length the
library reports (positions per workgroup of the first pass).

Levels: a sample is quiet (I = Q = 128, m = 1), medium (I = 158, m = 1861) or strong (I = 188, m = 7321).  The settings are chosen so
that a box of strong samples is "set", a box of quiet ones "clear" and a box of medium ones "keep"."""
import functools
from collections import namedtuple

import numpy as np

import pulses_ref

QUIET, MEDIUM, STRONG = 128, 158, 188
M_QUIET, M_MEDIUM, M_STRONG = 1, 1861, 7321
SETTINGS = {1: (1, 1000, 5000), 8: (8, 10000, 30000), 64: (64, 100000, 400000)}      # W: (W, lo, hi); medium keeps at W = 1 and 8
NOISE_LEVEL = 400                                            # about the median of m under noise of sigma 12: lo == hi there

Case = namedtuple("Case", "name cfg n_streams calls want")   # calls: uint8 [n_streams, nbytes] each; want: what check_case asserts


def cfg(W=8, lo=None, hi=None, pulse_cap=64):
    return {"W": W, "lo": SETTINGS[W][1] if lo is None else lo, "hi": SETTINGS[W][2] if hi is None else hi, "pulse_cap": pulse_cap}


def tile():
    import rtl_sdr_rs_amd as fmd
    return fmd.pulses_tile()


def noise(n_streams, n, seed, sigma=12.0):
    """Seeded Gaussian noise of `sigma` LSB around 127.5 as u8 IQ [n_streams, 2 n]."""
    g = np.random.default_rng(seed).normal(127.5, sigma, (n_streams, 2 * n))
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def quiet(n_streams, n):
    return np.full((n_streams, 2 * n), QUIET, np.uint8)


def level(iq, s, a, b, i_value):
    """The samples [a, b) of stream s at the level i_value (Q stays 128)."""
    assert 0 <= a <= b <= iq.shape[1] // 2, "outside the stream"
    iq[s, 2 * a:2 * b:2] = i_value
    iq[s, 2 * a + 1:2 * b:2] = 128


def split(iq, cuts):
    """iq [n_streams, nbytes] as calls that end at the samples `cuts` (increasing; multiples of 4) and at the end."""
    edges = [0] + [2 * c for c in cuts] + [iq.shape[1]]
    assert all(e % 8 == 0 for e in edges) and edges == sorted(edges)
    return [iq[:, a:b] for a, b in zip(edges[:-1], edges[1:])]


@functools.lru_cache(maxsize=None)
def delays(W):
    """(rise, fall) of the definition behind the first and behind the last sample of a long strong pulse on a quiet stream."""
    iq = quiet(1, 600)
    level(iq, 0, 200, 400, STRONG)
    _, lo, hi = SETTINGS[W]
    count, recs = pulses_ref.Stream(W, lo, hi).run(iq[0])
    assert count == 1
    return recs[0]["k_rel"] - recs[0]["width"] - 200, recs[0]["k_rel"] - 400


def tile_edge_case(kind, W):
    """One stream per offset: the rise (or the fall) of a pulse of 300 samples at each of T - 66 ... T + 2, in one call of T + 1024
    samples, with a second pulse behind it whose gap crosses nothing."""
    T = tile()
    offs = list(range(T - 66, T + 3))
    iq = quiet(len(offs), T + 1024)
    dr, df = delays(W)
    at = []
    for s, d in enumerate(offs):
        a = d - dr if kind == "rise" else d - df - 300       # the pulse's first strong sample
        level(iq, s, a, a + 300, STRONG)
        level(iq, s, T + 700, T + 800, STRONG)
        at.append((s, d))
    return Case("tile_edges_%s_%d" % (kind, W), cfg(W), len(offs), [iq], {kind + "_at": at, "pulses": 2})


def long_stream():
    """A pulse and then a gap that each span three whole tiles of "keep": strong for 100 samples at T / 2, medium up to 4 T + 300
    (the tiles 1, 2 and 3 hold nothing definite), quiet for 100, medium up to 8 T + 200 (the tiles 5, 6 and 7), strong for 100."""
    T = tile()
    iq = quiet(1, 9 * T)
    level(iq, 0, T // 2, T // 2 + 100, STRONG)
    level(iq, 0, T // 2 + 100, 4 * T + 300, MEDIUM)
    level(iq, 0, 4 * T + 400, 8 * T + 200, MEDIUM)
    level(iq, 0, 8 * T + 200, 8 * T + 300, STRONG)
    return iq


def long_case(how):
    T = tile()
    iq = long_stream()
    calls = [iq] if how == "one" else split(iq, [T, 3 * T])  # the pulse opens in the first call and falls in the third
    return Case("long_" + how, cfg(8), 1, calls, {"long": 3 * T, "keep_tiles": [1, 2, 3, 5, 6, 7]})


OWED_AT = ("0", "1", "63", "64", "last")


def owed_case():
    """W = 1.  Stream 2 i: the state is 0 into the second tile, which is medium up to its position q and strong from there: a rise the
    tile cannot see.  Stream 2 i + 1: the state is 1 into it (strong, then medium from the first tile on), and quiet from q: a fall.
    q = 0, 1, 63, 64 and T - 1.  The last stream: a tile with nothing definite between two busy ones.  Every stream ends with a pulse
    of its own in the third tile, whose gap counts from the owed edge."""
    T = tile()
    qs = [0, 1, 63, 64, T - 1]
    iq = quiet(2 * len(qs) + 1, 3 * T)
    owed = []
    for i, q in enumerate(qs):
        level(iq, 2 * i, 100, 150, STRONG)                   # an earlier pulse, so that the owed rise has a gap
        level(iq, 2 * i, T - 50, T + q, MEDIUM)
        level(iq, 2 * i, T + q, 2 * T + 20, STRONG)
        owed.append((2 * i, T + q, 1))
        level(iq, 2 * i + 1, T - 90, T - 50, STRONG)
        level(iq, 2 * i + 1, T - 50, T + q, MEDIUM)
        owed.append((2 * i + 1, T + q, 0))
    for s in range(2 * len(qs)):
        level(iq, s, 2 * T + 500, 2 * T + 600, STRONG)
    s = 2 * len(qs)
    level(iq, s, T - 200, T - 100, STRONG)
    level(iq, s, T - 100, 2 * T + 10, MEDIUM)
    level(iq, s, 2 * T + 300, 2 * T + 400, STRONG)
    return Case("owed", cfg(1), 2 * len(qs) + 1, [iq], {"owed": owed, "keep_tile": (s, 1)})


def overflow_case(pulse_cap):
    """W = 1, lo == hi, four tiles.  Stream 0: noise, an edge on about every other sample.  1: on and off by turns, an edge on every
    sample.  2: one pulse per tile.  3: two pulses in the third tile.  4: silent.  5: 2, 0, 3 and 1 pulses in the four tiles.  6: four
    samples on, four off: 512 falls per tile."""
    T = tile()
    n = 4 * T
    iq = quiet(7, n)
    iq[0] = noise(1, n, 41)[0]
    iq[1, 0::4] = STRONG                                     # the I of every other sample
    for t in range(4):
        level(iq, 2, t * T + 100, t * T + 200, STRONG)
    level(iq, 3, 2 * T + 10, 2 * T + 20, STRONG)
    level(iq, 3, 2 * T + 50, 2 * T + 60, STRONG)
    for t, k in enumerate((2, 0, 3, 1)):
        for i in range(k):
            level(iq, 5, t * T + 300 * i + 7, t * T + 300 * i + 77, STRONG)
    on = (np.arange(n) % 8) < 4
    iq[6, 0::2] = np.where(on, STRONG, QUIET)
    return Case("overflow_%d" % pulse_cap, cfg(1, NOISE_LEVEL, NOISE_LEVEL, pulse_cap), 7, [iq],
                {"counts": {1: 2 * T, 2: 4, 3: 2, 4: 0, 5: 6, 6: 2 * T // 4}, "noisy": 0})


def traffic(n, seed, sigma=6.0):
    """One stream of n samples: noise of `sigma` with strong pulses and gaps of 5 ... 300 samples, a tone rather than a constant."""
    rng = np.random.default_rng(seed)
    env, p = np.zeros(n), 0
    while p < n:
        g, w = int(rng.integers(5, 300)), int(rng.integers(5, 300))
        env[p + g:p + g + w] = 1
        p += g + w
    ph = np.arange(n) * 0.3
    x = 127.5 + env[:, None] * 60 * np.stack([np.cos(ph), np.sin(ph)], 1) + rng.normal(0, sigma, (n, 2))
    return np.clip(np.rint(x), 0, 255).astype(np.uint8).reshape(1, -1)


def cuts_stream():
    T = tile()
    n = 2 * T + 1000
    iq = traffic(n, 21)
    rng = np.random.default_rng(22)
    cuts = sorted(set([4, 8, 60]) | set((rng.integers(1, n // 4, 14) * 4).tolist()))      # the first calls are shorter than W
    return iq, cuts


def cuts_case(how):
    iq, cuts = cuts_stream()
    n = iq.shape[1] // 2
    calls = {"one": [iq], "random": split(iq, cuts), "four": split(iq, list(range(4, n, 4)))}[how]
    return Case("cuts_" + how, cfg(8, pulse_cap=64), 1, calls, {"pulses_at_least": 15})


def streams_case(n_streams):
    """Traffic in every third stream, a silent stream (all 128) behind it and a saturated one (all 255) behind that: T + 1000 samples."""
    T = tile()
    n = T + 1000
    iq = quiet(n_streams, n)
    for s in range(n_streams):
        if s % 3 == 0:
            iq[s] = traffic(n, 100 + s)[0]
        elif s % 3 == 2:
            iq[s] = 255
    return Case("streams_%d" % n_streams, cfg(8), n_streams, [iq], {"thirds": True})


def all_cases():
    out = [tile_edge_case(k, W) for k in ("rise", "fall") for W in (1, 8, 64)]
    out += [long_case("one"), long_case("calls"), owed_case()]
    out += [overflow_case(c) for c in (1, 4, 1024)]
    out += [cuts_case(h) for h in ("one", "random", "four")]
    out += [streams_case(n) for n in (1, 3, 64, 65)]
    return out


CASE_NAMES = ["tile_edges_rise_1", "tile_edges_rise_8", "tile_edges_rise_64", "tile_edges_fall_1", "tile_edges_fall_8", "tile_edges_fall_64",
              "long_one", "long_calls", "owed", "overflow_1", "overflow_4", "overflow_1024", "cuts_one", "cuts_random", "cuts_four",
              "streams_1", "streams_3", "streams_64", "streams_65"]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "owed":
        return owed_case()
    kind, _, arg = name.rpartition("_")
    if kind in ("tile_edges_rise", "tile_edges_fall"):
        return tile_edge_case(kind[11:], int(arg))
    if kind == "long":
        return long_case(arg)
    if kind == "overflow":
        return overflow_case(int(arg))
    if kind == "cuts":
        return cuts_case(arg)
    assert kind == "streams", name
    return streams_case(int(arg))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The definition's result for the case: (per call (counts, kept records per stream), info per stream).  Computed once."""
    c = case(name)
    return pulses_ref.run_bank(c.cfg, c.calls, c.n_streams)


def absolute(per_call, calls, s):
    """Stream s's kept records of every call with "p", the fall's absolute position, in place of k_rel."""
    out, pos = [], 0
    for (counts, recs), iq in zip(per_call, calls):
        if iq.shape[1]:
            out += [dict({k: v for k, v in r.items() if k != "k_rel"}, p=pos + r["k_rel"]) for r in recs[s]]
        pos += iq.shape[1] // 2
    return out


def trace(c, s):
    """(definite, value, state) per sample of stream s of a case, by the definition over the whole stream at once."""
    b = np.concatenate([iq[s] for iq in c.calls])
    st = pulses_ref.Stream(c.cfg["W"], c.cfg["lo"], c.cfg["hi"])
    e = st.box(b)[0][1:]
    definite, value = (e >= st.hi) | (e < st.lo), e >= st.hi
    state, cur = np.zeros(e.size, bool), False
    for i in range(e.size):
        cur = value[i] if definite[i] else cur
        state[i] = cur
    return definite, value, state


def check_case(name):
    """The definition's result for the case shows what the case is there for."""
    c = case(name)
    per_call, info = expected(name)
    recs = [absolute(per_call, c.calls, s) for s in range(c.n_streams)]
    total = [sum(cnt[s] for (cnt, _), iq in zip(per_call, c.calls) if iq.shape[1]) for s in range(c.n_streams)]
    want, T, cap = c.want, tile(), c.cfg["pulse_cap"]
    for s, d in want.get("rise_at", []):
        assert total[s] == want["pulses"] and recs[s][0]["p"] - recs[s][0]["width"] == d, (name, s, d, recs[s])
        assert recs[s][0]["gap"] == 0 and recs[s][1]["gap"] == recs[s][1]["p"] - recs[s][1]["width"] - recs[s][0]["p"]
    for s, d in want.get("fall_at", []):
        dr, df = delays(c.cfg["W"])
        assert total[s] == want["pulses"] and recs[s][0]["p"] == d and recs[s][0]["width"] == 300 + df - dr, (name, s, d, recs[s])
        assert recs[s][0]["level"] >= c.cfg["lo"]            # (the box in front of a fall had not fallen yet)
    if "long" in want:
        assert total[0] == 2 and recs[0][0]["width"] > want["long"] and recs[0][1]["gap"] > want["long"], (name, recs[0])
        definite, _, _ = trace(c, 0)
        for t in want["keep_tiles"]:
            assert not definite[t * T:(t + 1) * T].any(), (name, t)
        if len(c.calls) > 1:
            assert [cnt[0] for cnt, _ in per_call] == [0, 0, 2]
    for s, at, polarity in want.get("owed", []):
        definite, value, state = trace(c, s)
        first = (at // T) * T + int(np.argmax(definite[(at // T) * T:(at // T + 1) * T]))
        assert first == at and bool(value[at]) == bool(polarity) and bool(state[first - (first % T) - 1]) != bool(polarity), (name, s, at)
        edges = [r["p"] for r in recs[s]] if not polarity else [r["p"] - r["width"] for r in recs[s]]
        assert at in edges, (name, s, at, recs[s])
        assert total[s] == (3 if polarity else 2) and recs[s][-1]["gap"] == 2 * T + 500 - recs[s][-2]["p"]
    if "keep_tile" in want:
        s, t = want["keep_tile"]
        definite, _, state = trace(c, s)
        assert not definite[t * T:(t + 1) * T].any() and state[t * T:(t + 1) * T].all() and total[s] == 2
        assert definite[(t - 1) * T:t * T].any() and recs[s][0]["p"] // T == t + 1
    if "counts" in want:
        for s, n in want["counts"].items():
            assert total[s] == n, (name, s, total[s])
        s = want["noisy"]
        assert T // 2 < total[s] < 2 * T and info[s]["rises"] - info[s]["pulses"] in (0, 1)
        for s in range(c.n_streams):
            assert len(recs[s]) == min(total[s], cap)
        tiles = [np.bincount([p // T for p in falls_of(c, s)], minlength=4) for s in range(c.n_streams)]
        per_tile = lambda s: tiles[s]
        inside = [s for s in range(c.n_streams) if per_tile(s)[0] > cap or (s == 3 and per_tile(s)[2] > cap)]
        across = [s for s in range(c.n_streams) if total[s] > cap and per_tile(s).max() <= cap]
        below = [s for s in range(c.n_streams) if 0 < total[s] <= cap]
        assert inside and across and (below or cap == 1), (name, inside, across, below)
    if "pulses_at_least" in want:
        assert info[0]["pulses"] >= want["pulses_at_least"] and all(cnt[0] <= cap for cnt, _ in per_call), name
        if name != "cuts_one":
            assert c.calls[0].shape[1] // 2 < c.cfg["W"]     # a call shorter than the box
    if want.get("thirds"):
        for s in range(c.n_streams):
            if s % 3 == 0:
                assert total[s] >= 5, (name, s)
            elif s % 3 == 1:
                assert info[s] == {"samples": T + 1000, "pulses": 0, "rises": 0, "state": 0, "run": T + 1000}
            else:
                assert info[s]["rises"] == 1 and info[s]["pulses"] == 0 and info[s]["state"] == 1 and info[s]["run"] > T
    return recs, info


def falls_of(c, s):
    """Every fall of stream s of a one-call case, uncapped, as absolute positions."""
    st = pulses_ref.Stream(c.cfg["W"], c.cfg["lo"], c.cfg["hi"])
    return [r["k_rel"] for r in st.run(c.calls[0][s])[1]]
