"""The pulse bank's domain cases: the inputs of tests/test_gpu_pulses_domain.py, built from seeds and levels, with what
tests/pulses_ref.py (the definition) makes of them.  They enter what the cases of tests/pulses_cases.py leave out: more than 64 tiles
in a call, with every kind of carried state across the seam between the summaries 63 and 64 (and 127 and 128); boxes that are no power
of two; the thresholds at the ends of their domain; and widths, gaps and a run beyond 2^32 samples.  `check_case` holds the
definition's result to what each case is there for, so a case that stopped reaching its path fails on the CPU
(tests/test_pulses_domain.py).  T is the tile length the library reports.

Levels and SETTINGS are those of tests/pulses_cases.py.  The boxes in between take the W = 8 setting per sample: lo = 1250 W, hi =
3750 W -- a box of quiet samples (W) is clear, of medium ones (1861 W) keep, of strong ones (7321 W) set."""
import functools
from collections import namedtuple

import numpy as np

import pulses_ref
from pulses_cases import M_MEDIUM, M_QUIET, M_STRONG, MEDIUM, QUIET, SETTINGS, STRONG, absolute, level, noise, quiet, split, tile, traffic

Case = namedtuple("Case", "name cfg n_streams calls want")   # calls: uint8 [n_streams, nbytes] each; want: what check_case asserts

E_MAX = 64 * 65025
SEAMS = (64, 128)                                            # the tiles that are the first of a batch of 64 summaries


def cfg(W, lo, hi, pulse_cap=64):
    return {"W": W, "lo": lo, "hi": hi, "pulse_cap": pulse_cap}


def scaled(W):
    return W, 1250 * W, 3750 * W


def trace(c, s):
    """(definite, value, state) per sample of stream s of a case, by the definition over the whole stream at once."""
    b = np.concatenate([iq[s] for iq in c.calls])
    st = pulses_ref.Stream(c.cfg["W"], c.cfg["lo"], c.cfg["hi"])
    e = st.box(b)[0][1:]
    definite, value = (e >= st.hi) | (e < st.lo), e >= st.hi
    last = np.maximum.accumulate(np.where(definite, np.arange(e.size), -1))
    return definite, value, np.where(last >= 0, value[np.maximum(last, 0)], False)


def lag(W, lo, hi, m_to):
    """How many samples behind the first sample of a new level a box of medium samples turns definite."""
    for k in range(1, W + 1):
        e = (W - k) * M_MEDIUM + k * m_to
        if e >= hi or e < lo:
            return k - 1
    raise AssertionError("the level never decides")


# ---- 7. more than 64 tiles --------------------------------------------------------------------------------------------------------------

def tiles_many_streams(W):
    """130 T samples, a stream per situation at the seams (tile 64 and tile 128):
    0  a pulse that rises in the tile in front of the seam and falls behind it;
    1  a gap the same way;
    2  the tile behind the seam holds nothing definite and is entered with state 1;
    3  an owed fall at the first sample behind the seam, with medium level ("keep") up to it;
    4  an owed rise there;
    5  a pulse open from tile 62 to tile 129 over medium level: 66 tiles with nothing definite;
    6  the same pulse at strong level: every tile is definite and has no edge;
    7  a gap from tile 0 to tile 129 over medium level."""
    T = tile()
    _, lo, hi = SETTINGS[W]
    iq = quiet(8, 130 * T)
    owed, keep = [], []
    level(iq, 4, 1000, 1100, STRONG)                         # an earlier pulse, so that the owed rise has a gap
    for t in SEAMS:
        q = t * T
        level(iq, 0, q - 200, q + 200, STRONG)
        level(iq, 1, q - 400, q - 200, STRONG)
        level(iq, 1, q + 200, q + 400, STRONG)
        level(iq, 2, q - 300, q - 200, STRONG)
        level(iq, 2, q - 200, q + T + 100, MEDIUM)
        keep.append((2, t, t))
        level(iq, 3, q - 300, q - 200, STRONG)
        level(iq, 3, q - 200, q - lag(W, lo, hi, M_QUIET), MEDIUM)
        owed.append((3, q, 0))
        level(iq, 4, q - 300, q - lag(W, lo, hi, M_STRONG), MEDIUM)
        level(iq, 4, q - lag(W, lo, hi, M_STRONG), q + 500, STRONG)
        owed.append((4, q, 1))
    level(iq, 5, 62 * T + 100, 62 * T + 200, STRONG)
    level(iq, 5, 62 * T + 200, 129 * T + 300, MEDIUM)
    keep.append((5, 63, 128))
    level(iq, 6, 62 * T + 100, 129 * T + 300, STRONG)
    level(iq, 7, T // 2, T // 2 + 100, STRONG)
    level(iq, 7, T // 2 + 300, 129 * T, MEDIUM)
    level(iq, 7, 129 * T + 200, 129 * T + 300, STRONG)
    keep.append((7, 1, 128))
    return iq, owed, keep


def tiles_many_case(W, how):
    T = tile()
    iq, owed, keep = tiles_many_streams(W)
    calls = [iq] if how == "one" else split(iq, [64 * T, 64 * T + 4])
    return Case("tiles_many_%d_%s" % (W, how), cfg(*SETTINGS[W]), 8, calls, {"owed": owed, "keep": keep, "seams": True})


# ---- 8. boxes that are no power of two --------------------------------------------------------------------------------------------------

BOXES = (2, 3, 7, 9, 31, 33, 63)


def boxes_case(W, equal):
    """Three streams of traffic over T + 1000 samples at the box W; `equal`: lo == hi, in the middle of the scaled pair, and a
    pulse_cap of 3 that every stream overflows; else the scaled pair and a pulse_cap of 100."""
    n = tile() + 1000
    iq = np.concatenate([traffic(n, 200 + 10 * W + k) for k in range(3)])
    _, lo, hi = scaled(W)
    g = cfg(W, 2 * lo, 2 * lo, 3) if equal else cfg(W, lo, hi, 100)
    return Case("boxes_%d_%s" % (W, "equal" if equal else "pair"), g, 3, [iq], {"traffic": True})


# ---- 9. the thresholds at the ends of their domain -------------------------------------------------------------------------------------

def limits_case(kind):
    """top: W 64, lo = hi = 64 * 65025 -- only 64 saturated samples set.  Streams: a block of 100 samples of bytes 255 (one pulse, whose
    fall is the second call's first sample); a block of exactly 64 of bytes 0 across the first tile's end (a pulse one sample wide); a
    block of 63 (nothing); saturated throughout (set at sample 63, never cleared).
    one, two: W 1 with lo = hi = 1 and W 2 with lo = hi = 2 -- a box is never below W, so one rise and never a fall.  Streams: quiet,
    noise, saturated.
    wide: W 63, lo = 1, hi = 63 * 65025 -- set by a block of 63 saturated samples and never cleared; a block of 62 sets nothing."""
    T = tile()
    n = T + 1000
    if kind == "top":
        iq = quiet(4, n)
        iq[0, 2 * 500:2 * 600] = 255
        iq[1, 2 * (T - 32):2 * (T + 32)] = 0
        iq[2, 2 * 700:2 * 763] = 255
        iq[3] = 255
        return Case("limits_top", cfg(64, E_MAX, E_MAX, 3), 4, split(iq, [600]), {"top": True})
    if kind in ("one", "two"):
        W = 1 if kind == "one" else 2
        iq = np.concatenate([quiet(1, n), noise(1, n, 61), np.full((1, 2 * n), 255, np.uint8)])
        return Case("limits_" + kind, cfg(W, W, W, 3), 3, split(iq, [8, 2000]), {"never_clear": W})
    assert kind == "wide", kind
    iq = quiet(2, n)
    iq[0, 2 * 500:2 * 563] = 255
    iq[1, 2 * 500:2 * 562] = 0
    return Case("limits_wide", cfg(63, 1, 63 * 65025, 100), 2, split(iq, [T]), {"wide": True})


CASE_NAMES = (["tiles_many_%d_%s" % (W, how) for W in (1, 64) for how in ("one", "three")] +
              ["boxes_%d_%s" % (W, e) for W in BOXES for e in ("pair", "equal")] + ["limits_top", "limits_one", "limits_two", "limits_wide"])


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.rpartition("_")
    if kind.startswith("tiles_many"):
        return tiles_many_case(int(kind.rpartition("_")[2]), arg)
    if kind.startswith("boxes"):
        return boxes_case(int(kind.rpartition("_")[2]), arg == "equal")
    assert kind == "limits", name
    return limits_case(arg)


def all_cases():
    return [case(n) for n in CASE_NAMES]


@functools.lru_cache(maxsize=None)
def expected(name):
    """The definition's result for the case: (per call (counts, kept records per stream), info per stream).  Computed once."""
    c = case(name)
    return pulses_ref.run_bank(c.cfg, c.calls, c.n_streams)


@functools.lru_cache(maxsize=None)
def uncapped(name):
    """Every record of every stream of the case, whatever pulse_cap is, with "p", the fall's absolute position."""
    c = case(name)
    per_call, _ = pulses_ref.run_bank(dict(c.cfg, pulse_cap=1 << 30), c.calls, c.n_streams)
    return [absolute(per_call, c.calls, s) for s in range(c.n_streams)]


def check_case(name):
    """The definition's result for the case shows what the case is there for."""
    c = case(name)
    per_call, info = expected(name)
    every, want, T, cap = uncapped(name), c.want, tile(), c.cfg["pulse_cap"]
    total = [sum(cnt[s] for cnt, _ in per_call) for s in range(c.n_streams)]
    n = sum(iq.shape[1] for iq in c.calls) // 2
    assert [len(e) for e in every] == total == [i["pulses"] for i in info] and all(i["samples"] == n for i in info), name
    rise = lambda r: r["p"] - r["width"]
    if want.get("seams"):
        assert n == 130 * T and every == uncapped(name.replace("three", "one"))
        if name.endswith("three"):
            assert [iq.shape[1] // 2 for iq in c.calls] == [64 * T, 4, 66 * T - 4]
        assert [(rise(r) // T, r["p"] // T) for r in every[0]] == [(63, 64), (127, 128)]
        gaps = [(r["p"] - r["width"] - r["gap"]) // T for r in every[1]]             # the tile of the fall in front of each gap
        assert [(g, rise(r) // T) for g, r in zip(gaps, every[1])][1::2] == [(63, 64), (127, 128)], (name, every[1])
        for s, at, polarity in want["owed"]:
            definite, value, state = trace(c, s)
            first = at + int(np.argmax(definite[at:at + T]))
            assert at % T == 0 and first == at and bool(value[at]) == bool(polarity) and bool(state[at - 1]) != bool(polarity), (name, s, at)
            assert not definite[at - 100:at].any()           # "keep" up to it
            assert at in ([rise(r) for r in every[s]] if polarity else [r["p"] for r in every[s]]), (name, s, at, every[s])
        for s, a, b in want["keep"]:
            definite, _, state = trace(c, s)
            assert not definite[a * T:(b + 1) * T].any() and (state[a * T:(b + 1) * T] == (s != 7)).all(), (name, s)
        assert [(rise(r) // T, r["p"] // T) for r in every[5]] == [(62, 129)] and [(rise(r) // T, r["p"] // T) for r in every[6]] == [(62, 129)]
        assert every[5][0]["width"] > 66 * T and every[7][1]["gap"] > 128 * T and total[2] == 2
        assert total[3] == 2 and total[4] == 3 and every[4][1]["gap"] > 62 * T
    if want.get("traffic"):
        assert c.cfg["W"] in BOXES and all(t >= 5 for t in total), (name, total)
        if c.cfg["lo"] == c.cfg["hi"]:
            assert min(total) > cap == 3
        else:
            assert max(total) < cap == 100 and c.cfg["lo"] < c.cfg["hi"]
            assert every != uncapped(name.replace("pair", "equal"))       # the hysteresis matters
    if want.get("top"):
        assert [[(r["p"], r["width"], r["level"]) for r in e] for e in every] == [[(600, 37, E_MAX)], [(T + 32, 1, E_MAX)], [], []]
        assert per_call[1][1][0][0]["k_rel"] == 0            # the fall is the second call's first sample
        assert info[3] == {"samples": n, "pulses": 0, "rises": 1, "state": 1, "run": n - 63} and info[2]["rises"] == 0
    if "never_clear" in want:
        W = want["never_clear"]
        assert all(i["pulses"] == 0 and i["rises"] == 1 and i["state"] == 1 for i in info), (name, info)
        assert [n - i["run"] for i in info] == ([0, 0, 0] if W == 1 else [1, n - info[1]["run"], 0]) and n - info[1]["run"] in (0, 1)
        assert c.calls[0].shape[1] // 2 == 8
    if want.get("wide"):
        assert info[0] == {"samples": n, "pulses": 0, "rises": 1, "state": 1, "run": n - 562}
        assert info[1] == {"samples": n, "pulses": 0, "rises": 0, "state": 0, "run": n}
    return every, info


# ---- 10. beyond 2^32 samples -----------------------------------------------------------------------------------------------------------

STRETCH = 1 << 30                                            # samples of one call over the constant buffer
SAT_CFG = cfg(*SETTINGS[8], pulse_cap=4)


def advance(st, n):
    """pulses_ref.Stream `st` over n more samples that equal its 64 carried ones, without materialising them: the box stays what it
    is, so no edge falls, and only pos, run_len and the totals move.  Returns what Stream.run returns."""
    assert len(set(st.tail.tolist())) == 1, "the carried samples differ"
    e = st.W * int(st.tail[0])
    assert (e >= st.hi and st.state == 1) or (e < st.lo and st.state == 0) or st.lo <= e < st.hi, "the stretch would make an edge"
    st.pos += n
    st.run_len += n
    st.info["samples"] += n
    st.info["run"] = st.run_len
    return 0, []


def small(*runs):
    """A small call: (level, samples) runs as u8 IQ [1, 2 n]."""
    n = sum(k for _, k in runs)
    iq, p = quiet(1, n), 0
    for v, k in runs:
        level(iq, 0, p, p + k, v)
        p += k
    return iq


def saturation_script():
    """The calls: ("bytes", uint8 [1, 2 n]) or ("stretch", level), the constant buffer of STRETCH samples at that level."""
    return ([("bytes", small((QUIET, 100), (STRONG, 50), (QUIET, 102)))] + [("stretch", QUIET)] * 5 +
            [("bytes", small((QUIET, 40), (STRONG, 60), (QUIET, 100), (STRONG, 100)))] + [("stretch", STRONG)] * 5 +
            [("bytes", small((STRONG, 20), (QUIET, 80)))])


@functools.lru_cache(maxsize=None)
def saturation_expected():
    """Per call of the script (count, records, info) of the definition, the stretches by `advance`."""
    st = pulses_ref.Stream(SAT_CFG["W"], SAT_CFG["lo"], SAT_CFG["hi"])
    out = []
    for kind, x in saturation_script():
        count, recs = st.run(x[0]) if kind == "bytes" else advance(st, STRETCH)
        out.append((count, recs, dict(st.info)))
    return out


def check_saturation():
    out = saturation_expected()
    recs = [r for _, rr, _ in out for r in rr]
    assert [c for c, _, _ in out] == [1] + [0] * 5 + [1] + [0] * 5 + [1]
    assert recs[1]["gap"] == pulses_ref.SAT and recs[1]["width"] < 100 and recs[2]["width"] == pulses_ref.SAT and recs[2]["gap"] < 200
    assert out[5][2]["run"] == 5 * STRETCH + 252 - recs[0]["k_rel"] > 1 << 32 and out[5][2]["state"] == 0
    assert out[11][2]["run"] > 1 << 32 and out[11][2]["state"] == 1 and out[12][2]["state"] == 0
    assert out[12][2]["samples"] == 10 * STRETCH + 252 + 300 + 100
    return out
