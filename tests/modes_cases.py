"""The Mode S bank's cases: the inputs of tests/test_gpu_modes.py, built from seeds and the four published messages, with what
tests/modes_ref.py (the definition) makes of them.  Every case says what it is there to exercise, and `check_case` holds the
definition's result to that -- a case that stopped exercising its edge fails on the CPU (tests/test_modes.py), not silently on the
GPU.  T is the tile length the library reports (positions per workgroup of the first pass)."""
import functools
from collections import namedtuple

import numpy as np

import modes_ref

VECTORS = ["8D4840D6202CC371C32CE0576098", "8D40621D58C382D690C8AC2863A7", "8D40621D58C386435CC412692AD6",
           "8D485020994409940838175B284F"]
LONG = [bytes.fromhex(h) for h in VECTORS]
AMP = 60
M_PULSE = ((2 * (128 + AMP) - 255) ** 2 + 1) >> 1            # m of a pulse sample of modes_encode(amplitude=AMP)

Case = namedtuple("Case", "name cfg n_streams calls want")   # calls: uint8 [n_streams, nbytes] each; want: what check_case asserts


def cfg(min_power=0, fix_errors=0, df11=0, msg_cap=32):
    return {"min_power": min_power, "fix_errors": fix_errors, "df11": df11, "msg_cap": msg_cap}


def tile():
    import rtl_sdr_rs_amd as fmd
    return fmd.modes_tile()


def short_msg(k=0):
    import rtl_sdr_rs_amd as fmd
    return fmd.modes_df11(0x4840D6 + k, iid=(5 * k) % 128)


def flip(msg, *bits):
    b = bytearray(msg)
    for t in bits:
        b[t >> 3] ^= 0x80 >> (t & 7)
    return bytes(b)


def noise(n_streams, n, seed, sigma=12.0):
    """Seeded Gaussian noise of `sigma` LSB around 127.5 as u8 IQ [n_streams, 2 n]."""
    g = np.random.default_rng(seed).normal(127.5, sigma, (n_streams, 2 * n))
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def quiet(n_streams, n):
    return np.full((n_streams, 2 * n), 128, np.uint8)


def place(iq, s, p, msg, amplitude=AMP):
    """The message's samples over stream s of iq [n_streams, nbytes] from sample p on."""
    import rtl_sdr_rs_amd as fmd
    e = fmd.modes_encode(msg, amplitude)
    assert p >= 0 and 2 * p + e.size <= iq.shape[1], "message outside the stream"
    iq[s, 2 * p:2 * p + e.size] = e


def split(iq, cuts):
    """iq [n_streams, nbytes] as calls that end at the samples `cuts` (increasing; multiples of 4) and at the end."""
    edges = [0] + [2 * c for c in cuts] + [iq.shape[1]]
    assert all(e % 8 == 0 for e in edges) and edges == sorted(edges)
    return [iq[:, a:b] for a, b in zip(edges[:-1], edges[1:])]


def tile_edge_case(kind):
    """One stream per offset: a message whose preamble begins at each of T - 260 ... T + 20, in one call of 2 (T + 512) samples over
    noise, so that its 240 samples lie on every side of the first tile's end."""
    T = tile()
    offs = list(range(T - 260, T + 21))
    iq = noise(len(offs), 2 * (T + 512), 11 if kind == "long" else 12)
    for s, d in enumerate(offs):
        place(iq, s, d, LONG[s % 4] if kind == "long" else short_msg(s))
    want = {"at": [(s, d, LONG[s % 4] if kind == "long" else short_msg(s)) for s, d in enumerate(offs)], "candidates_everywhere": True}
    return Case("tile_edges_" + kind, cfg(df11=1), len(offs), [iq], want)


def cuts_stream():
    """One stream of 4 T samples over noise with long, short and single-bit-damaged messages, and the samples at which the `random`
    cutting ends its calls: the first calls are too short to decide anything, and a message straddles a cut by 1 ... 239 samples."""
    T = tile()
    iq = noise(1, 4 * T, 21)
    cuts, at = [4, 104, 204], []
    msgs = [LONG[0], short_msg(1), flip(LONG[1], 40), LONG[2], short_msg(2), flip(LONG[3], 111), LONG[3], flip(LONG[0], 5), LONG[1]]
    straddle = [1, 2, 3, 60, 119, 120, 237, 238, 239]        # samples of the message's 240 that lie behind the cut
    p = 600
    for msg, k in zip(msgs, straddle):
        cut = (p + 240 - k + 3) // 4 * 4                     # a multiple of 4 at or behind p + 240 - k ...
        p = cut - (240 - k)                                  # ... and the message moved so that exactly k samples lie behind it
        place(iq, 0, p, msg)
        at.append((0, p, msg))
        cuts.append(cut)
        p += 700
    assert p < 4 * T
    rng = np.random.default_rng(22)
    more = sorted(set((rng.integers(1, T, 12) * 4).tolist()) - set(cuts))
    return iq, sorted(cuts + more), at


def cuts_case(how):
    iq, cuts, at = cuts_stream()
    n = iq.shape[1] // 2
    calls = {"one": [iq], "random": split(iq, cuts), "four": split(iq, list(range(4, n, 4)))}[how]
    return Case("cuts_" + how, cfg(fix_errors=1, df11=1, msg_cap=32), 1, calls, {"at": at, "fixed": 3})


def streams_case(n_streams):
    """Seeded noise over every stream, messages in every other one: two tiles and a tail."""
    T = tile()
    iq = noise(n_streams, T + 1000, 30 + n_streams)
    at = []
    for s in range(0, n_streams, 2):
        for i, p in enumerate((17 + 3 * s, T - 100 - s, T + 500)):
            msg = LONG[(s + i) % 4] if i != 1 else short_msg(s)
            place(iq, s, p, msg)
            at.append((s, p, msg))
    return Case("streams_%d" % n_streams, cfg(df11=1), n_streams, [iq], {"at": at, "candidates_everywhere": True})


def overflow_case(msg_cap):
    """More acceptances than msg_cap: stream 0 has six messages packed into its first tile, stream 1 six spread over four tiles,
    stream 2 three in its second tile and two in its fourth, stream 3 none."""
    T = tile()
    iq = quiet(4, 4 * T)
    at = []
    for i in range(6):
        at.append((0, 300 + 260 * i, LONG[i % 4]))
        at.append((1, 50 + i * (4 * T - 400) // 6, LONG[(i + 1) % 4]))
    for i in range(3):
        at.append((2, T + 10 + 300 * i, LONG[i]))
    at += [(2, 3 * T + 7, LONG[3]), (2, 3 * T + 400, LONG[0])]
    for s, p, msg in at:
        place(iq, s, p, msg)
    return Case("overflow_%d" % msg_cap, cfg(msg_cap=msg_cap), 4, [iq], {"at": at, "counts": [6, 6, 5, 0], "tiles_of_1": 4})


def fix_case(fix_errors):
    """The same input with and without the fix: a clean message, single flips at the bits 5, 40 and 111, a flip inside the DF field
    and a double flip."""
    iq = quiet(1, 4000)
    msgs = [LONG[0], flip(LONG[1], 5), flip(LONG[2], 40), flip(LONG[3], 111), flip(LONG[0], 2), flip(LONG[1], 20, 77)]
    at = [(0, 100 + 400 * i, m) for i, m in enumerate(msgs)]
    for s, p, m in at:
        place(iq, s, p, m)
    kept = [(0, p, LONG[i]) for i, (_, p, _) in enumerate(at[:4 if fix_errors else 1])]       # as they come out: restored
    return Case("fix_%d" % fix_errors, cfg(fix_errors=fix_errors), 1, [iq], {"exactly": kept, "fixed": 3 if fix_errors else 0})


def power_case(above):
    """min_power on either side of a message's S = 4 m(pulse)."""
    iq = quiet(1, 1000)
    place(iq, 0, 300, LONG[2])
    S = 4 * M_PULSE
    return Case("min_power_" + ("above" if above else "at"), cfg(min_power=S + 1 if above else S), 1, [iq],
                {"exactly": [] if above else [(0, 300, LONG[2])], "fixed": 0})


def all_cases():
    out = [tile_edge_case("long"), tile_edge_case("short")]
    out += [cuts_case(h) for h in ("one", "random", "four")]
    out += [streams_case(n) for n in (1, 3, 64, 65)]
    out += [overflow_case(1), overflow_case(4), fix_case(0), fix_case(1), power_case(False), power_case(True)]
    return out


CASE_NAMES = ["tile_edges_long", "tile_edges_short", "cuts_one", "cuts_random", "cuts_four", "streams_1", "streams_3", "streams_64",
              "streams_65", "overflow_1", "overflow_4", "fix_0", "fix_1", "min_power_at", "min_power_above"]


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.rpartition("_")
    if kind == "tile_edges":
        return tile_edge_case(arg)
    if kind == "cuts":
        return cuts_case(arg)
    if kind == "streams":
        return streams_case(int(arg))
    if kind == "overflow":
        return overflow_case(int(arg))
    if kind == "fix":
        return fix_case(int(arg))
    assert kind == "min_power", name
    return power_case(arg == "above")


@functools.lru_cache(maxsize=None)
def expected(name):
    """The definition's result for the case: (per call (counts, kept records per stream), info per stream).  Computed once."""
    c = case(name)
    return modes_ref.run_bank(c.cfg, c.calls, c.n_streams)


def absolute(per_call, calls, s):
    """Stream s's kept records of every call with "p", the absolute position, in place of k_rel."""
    out, pos = [], 0
    for (counts, recs), iq in zip(per_call, calls):
        if iq.shape[1]:
            out += [dict({k: v for k, v in r.items() if k != "k_rel"}, p=pos + r["k_rel"]) for r in recs[s]]
        pos += iq.shape[1] // 2
    return out


def check_case(name):
    """The definition's result for the case shows what the case is there for."""
    c = case(name)
    per_call, info = expected(name)
    recs = [absolute(per_call, c.calls, s) for s in range(c.n_streams)]
    total = [sum(cnt[s] for (cnt, _), iq in zip(per_call, c.calls) if iq.shape[1]) for s in range(c.n_streams)]
    want = c.want
    undamaged = lambda m: modes_ref.syndrome_bits(np.unpackbits(np.frombuffer(m, np.uint8)).tolist()) & (0xFFFF80 if len(m) == 7 else -1) == 0
    for s, p, msg in want.get("at", []):
        hit = [r for r in recs[s] if r["p"] == p]
        if c.cfg["msg_cap"] >= 6:                            # (an overflow case keeps only the first)
            assert len(hit) == 1, (name, s, p)
            if undamaged(msg):
                assert hit[0]["bytes"][:len(msg)] == msg and hit[0]["n_bytes"] == len(msg) and hit[0]["fixed_bit"] == 0xFF
            else:
                assert hit[0]["fixed_bit"] != 0xFF and hit[0]["bytes"] != msg
    if "exactly" in want:
        assert [(r["p"], r["bytes"][:r["n_bytes"]]) for r in recs[0]] == [(p, m) for _, p, m in want["exactly"]], name
        assert total[0] == len(want["exactly"])
    if "fixed" in want:
        assert info[0]["fixed"] == want["fixed"], (name, info[0])
    if want.get("candidates_everywhere"):
        assert all(i["candidates"] > i["messages"] for i in info), name      # the queue is used where no message lies
    if "counts" in want:
        assert total == want["counts"] and any(t > c.cfg["msg_cap"] for t in total), (name, total)
        T = tile()
        assert len({p // T for s, p, _ in want["at"] if s == 1}) == want["tiles_of_1"]
        for s in range(c.n_streams):
            assert [r["p"] for r in recs[s]] == sorted(p for t, p, _ in want["at"] if t == s)[:c.cfg["msg_cap"]], (name, s)
    if name.startswith("cuts_"):
        assert all(cnt[0] <= c.cfg["msg_cap"] for cnt, _ in per_call), name
        if name != "cuts_one":
            assert per_call[0][0] == [0] and per_call[1][0] == [0]           # calls that decide nothing
    return recs, info
