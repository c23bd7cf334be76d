"""The Mode S bank's domain cases: the inputs of tests/test_gpu_modes_domain.py, built from seeds by a sender of their own, with what
tests/modes_ref.py (the definition) makes of them.  They enter what the cases of tests/modes_cases.py leave out: a candidate queue
longer than a wave, the single-bit fix at every bit, every downlink format on either side of the selection, more acceptances than
msg_cap inside every tile and summed over many tiles, more than 64 tiles, full-scale samples and a message at absolute position 0.
`check_case` holds the definition's result to what each case is there for, so a case that stopped reaching its path fails on the
CPU (tests/test_modes_domain.py).  T is the tile length the library reports.

The sender: a frame is a list of bits -- DF, seeded data, and the parity of modes_ref.remainder XOR an overlay -- and `put` writes
its pulses at any sample level.  A frame is "clean" when, alone on a quiet stream, its own preamble is the only candidate."""
import functools
import itertools
from collections import namedtuple

import numpy as np

import modes_ref
from modes_cases import absolute, cfg, noise, split, tile

Case = namedtuple("Case", "name cfg n_streams calls want")   # calls: uint8 [n_streams, nbytes] each; want: what check_case asserts

ON = (188, 128)                                              # a pulse of modes_encode(amplitude=60)
M_FULL = 65025                                               # m of a sample whose bytes are 0 or 255 in both I and Q
TEETH = (0, 2, 7, 9)


def quiet(n_streams, n, floor=(128, 128)):
    iq = np.empty((n_streams, 2 * n), np.uint8)
    iq[:, 0::2], iq[:, 1::2] = floor
    return iq


def frame_bits(df, seed, overlay=0):
    """The bits of a frame of downlink format df (112 bits where df >= 16, else 56): seeded data and parity XOR overlay."""
    n = 112 if df >= 16 else 56
    data = [(df >> (4 - i)) & 1 for i in range(5)] + np.random.default_rng([df, seed]).integers(0, 2, n - 29).tolist()
    parity = modes_ref.remainder(data) ^ overlay
    return data + [(parity >> (23 - i)) & 1 for i in range(24)]


def flipped(bits, *at):
    out = list(bits)
    for t in at:
        out[t] ^= 1
    return out


def as_bytes(bits):
    return bytes(np.packbits(np.array(bits, np.uint8)).tolist())


def put(iq, s, p, bits, on=ON):
    """The frame's pulses over stream s of iq from sample p on: the preamble, then pulse-gap for a 1 and gap-pulse for a 0."""
    at = [p + j for j in TEETH] + [p + 16 + 2 * t + (1 - b) for t, b in enumerate(bits)]
    assert p >= 0 and 2 * (p + 16 + 2 * len(bits)) <= iq.shape[1], "frame outside the stream"
    for j in at:
        iq[s, 2 * j], iq[s, 2 * j + 1] = on


def comb(iq, s, p, n, on=ON):
    """n bare preambles, 16 samples apart, from sample p on."""
    for i in range(n):
        for j in TEETH:
            iq[s, 2 * (p + 16 * i + j)], iq[s, 2 * (p + 16 * i + j) + 1] = on


def candidates(b, min_power=0):
    """The absolute positions that pass pre(p) in one stream's bytes taken as one call from creation."""
    v = np.concatenate([np.zeros(modes_ref.SPAN - 1, np.int64), modes_ref.magnitude(b)])
    ok, _ = modes_ref.preamble(v, min_power)
    ok[:modes_ref.SPAN - 1] = False
    return np.nonzero(ok)[0] - (modes_ref.SPAN - 1)


def is_clean(bits, follow=False):
    """The frame's own preamble is its only candidate, on quiet or (follow) with the next frame's preamble right behind it."""
    iq = quiet(1, 20 + 16 + 2 * len(bits) + 300)
    put(iq, 0, 20, bits)
    if follow:
        comb(iq, 0, 20 + 16 + 2 * len(bits), 1)
    return candidates(iq[0]).tolist() == [20] + ([20 + 16 + 2 * len(bits)] if follow else [])


@functools.lru_cache(maxsize=None)
def clean_frame(df, seed, flips=(), follow=False):
    """The first frame of the seeds seed, seed + 1000, ... that is clean (with `flips` applied): (bits as sent, bits undamaged)."""
    for k in itertools.count():
        good = frame_bits(df, seed + 1000 * k)
        sent = flipped(good, *flips)
        if is_clean(sent, follow):
            return tuple(sent), tuple(good)


# ---- 1. a candidate queue longer than a wave -----------------------------------------------------------------------------------------

QUEUE_AT = (0, 63, 64, 65, 127, 128, 160)                    # the acceptances' indices among the second tile's candidates
QUEUE_DAMAGED = 128                                          # the acceptance that is single-bit damaged (bit 70)


def queue_long_case(msg_cap):
    """A quiet stream of 3 T samples.  Its second tile holds combs of bare preambles -- each a candidate that decodes as DF 24 -- with
    clean DF 17 frames between and behind them, so that the acceptances stand at QUEUE_AT in the tile's queue; one more frame lies in
    the first tile and one in the third."""
    T = tile()
    iq = quiet(1, 3 * T)
    at, p, index = [], T - 239 + 8, 0                        # p: the next free sample; index: the tile's candidates so far
    first = clean_frame(17, 1)
    put(iq, 0, 500, first[0])
    at.append((0, 500, first[1], None))
    for k, want in enumerate(QUEUE_AT):
        comb(iq, 0, p, want - index)
        p += 16 * (want - index)
        sent, good = clean_frame(17, 10 + k, (70,) if want == QUEUE_DAMAGED else ())
        put(iq, 0, p, sent)
        at.append((0, p, good, 70 if want == QUEUE_DAMAGED else None))
        p, index = p + 256, want + 1
    assert p - 256 < 2 * T - 239, "the last acceptance left the second tile"
    last = clean_frame(17, 30)
    put(iq, 0, 2 * T + 300, last[0])
    at.append((0, 2 * T + 300, last[1], None))
    return Case("queue_long_%d" % msg_cap, cfg(fix_errors=1, msg_cap=msg_cap), 1, [iq], {"at": at, "queue": (1, list(QUEUE_AT)), "fixed": 1})


# ---- 2. the single-bit fix at every bit ------------------------------------------------------------------------------------------------

DOUBLES = ((63, 64), (47, 48), (5, 111))


def fix_every_bit_case(fix_errors):
    """112 streams: stream t carries one DF 17 frame with its bit t flipped, on quiet."""
    good = frame_bits(17, 3)
    iq = quiet(112, 600)
    for t in range(112):
        put(iq, t, 40 + t, flipped(good, t))
    return Case("fix_every_bit_%d" % fix_errors, cfg(fix_errors=fix_errors), 112, [iq], {"every_bit": as_bytes(good), "on": fix_errors})


def fix_doubles_case():
    """Double flips on either side of the seam between the two ballots of the fix: nothing is accepted."""
    good = frame_bits(18, 4)
    iq = quiet(len(DOUBLES), 600)
    for s, pair in enumerate(DOUBLES):
        put(iq, s, 60 + s, flipped(good, *pair))
    return Case("fix_doubles", cfg(fix_errors=1), len(DOUBLES), [iq], {"nothing": True, "doubles": True})


# ---- 3. the selection of downlink formats ----------------------------------------------------------------------------------------------

LONG_DFS, SHORT_DFS = (16, 17, 18, 19, 20, 21, 24, 31), (0, 4, 5, 11)
OVERLAYS = (1, 0x7F, 0x80, 0x800000)                         # of further DF 11 frames


def df_selection_frames():
    """[(df, overlay, bits)], one per stream."""
    out = [(df, 0, frame_bits(df, 5)) for df in LONG_DFS + SHORT_DFS]
    return out + [(11, o, frame_bits(11, 6 + i, o)) for i, o in enumerate(OVERLAYS)]


def df_selection_case(df11):
    frames = df_selection_frames()
    iq = quiet(len(frames), 600)
    for s, (_, _, bits) in enumerate(frames):
        put(iq, s, 30 + 7 * s, bits)
    accepted = [s for s, (df, o, _) in enumerate(frames) if df in (17, 18) or (df == 11 and df11 and o < 0x80)]
    return Case("df_selection_%d" % df11, cfg(df11=df11), len(frames), [iq], {"accepted": accepted, "frames": frames})


# ---- 4. more acceptances than msg_cap, inside a tile and over many ---------------------------------------------------------------------

DENSE_FIRST, DENSE_EVERY = 100, 128


def dense_short_case(msg_cap):
    """DF 11 frames back to back, one every 128 samples from sample 100 on, over 10 T + 500 samples: as many as lie whole inside the
    stream.  The call decides every one but the last, whose 240 samples end behind it."""
    T = tile()
    n = 10 * T + 500
    iq = quiet(1, n)
    frames = [clean_frame(11, 40 + k, (), True)[0] for k in range(8)]
    at = []
    for i, p in enumerate(range(DENSE_FIRST, n - 127, DENSE_EVERY)):
        put(iq, 0, p, frames[i % 8])
        at.append(p)
    return Case("dense_short_%d" % msg_cap, cfg(df11=1, msg_cap=msg_cap), 1, [iq], {"dense": at})


def dense_per_tile(T, n, at):
    """How many of the frames at `at` each tile of a call of n samples decides: position p is the tile's (p + 239) // T."""
    tiles = [(p + 239) // T for p in at if p + 239 < n]
    return np.bincount(tiles, minlength=(n + T - 1) // T).tolist()


# ---- 5. more than 64 tiles --------------------------------------------------------------------------------------------------------------

MANY_TILES = (0, 62, 63, 64, 65, 127, 128, 129)


def tiles_many_case(how):
    """130 T samples on 2 streams.  Stream 0: quiet with a frame decided in each of the tiles MANY_TILES and one more whose samples
    straddle the end of tile 63.  Stream 1: noise only.  As one call, or as two cut inside tile 64."""
    T = tile()
    iq = np.concatenate([quiet(1, 130 * T), noise(1, 130 * T, 51)])
    at = []
    for k, t in enumerate(MANY_TILES):
        p = t * T + 300 + 17 * k                             # decided at u = p + 239: inside tile t
        sent, good = clean_frame(17 + k % 2, 60 + k)
        put(iq, 0, p, sent)
        at.append((0, p, good, None))
    sent, good = clean_frame(17, 70)
    put(iq, 0, 64 * T - 100 - 239, sent)                     # decided at u = 64 T - 100, its last samples come with tile 64
    at.append((0, 64 * T - 100 - 239, good, None))
    calls = [iq] if how == "one" else split(iq, [64 * T + 2000])
    return Case("tiles_many_" + how, cfg(), 2, calls, {"at": at, "tiles": sorted(MANY_TILES + (63,)), "noise": 1})


# ---- 6. full-scale samples, and a message at absolute position 0 ---------------------------------------------------------------------

FLOOR = (128, 127)


def full_scale_case(kind):
    """Over a floor of (128, 127).  Stream 0: a frame of pulses at (255, 255); stream 1: at (0, 0); stream 2: a frame at absolute
    position 0; stream 3: at position 1.  `at`: min_power is the frames' S; `above`: one more; `cut`: as `at`, in two calls of which
    the first ends at sample 100, so that position 0 is the second call's first decided one."""
    iq = quiet(4, 800, FLOOR)
    at = []
    for s, (p, on) in enumerate(((300, (255, 255)), (301, (0, 0)), (0, (255, 255)), (1, (0, 0)))):
        sent, good = clean_frame(17 + s % 2, 80 + s)
        put(iq, s, p, sent, on)
        at.append((s, p, good, None))
    calls = split(iq, [100]) if kind == "cut" else [iq]
    want = {"at": [] if kind == "above" else at, "power": 4 * M_FULL, "nothing": kind == "above"}
    return Case("full_scale_" + kind, cfg(min_power=4 * M_FULL + (1 if kind == "above" else 0)), 4, calls, want)


CASE_NAMES = ["queue_long_2", "queue_long_32", "fix_every_bit_1", "fix_every_bit_0", "fix_doubles", "df_selection_0", "df_selection_1",
              "dense_short_8", "dense_short_40", "dense_short_256", "tiles_many_one", "tiles_many_two", "full_scale_at",
              "full_scale_above", "full_scale_cut"]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "fix_doubles":
        return fix_doubles_case()
    kind, _, arg = name.rpartition("_")
    if kind == "queue_long":
        return queue_long_case(int(arg))
    if kind == "fix_every_bit":
        return fix_every_bit_case(int(arg))
    if kind == "df_selection":
        return df_selection_case(int(arg))
    if kind == "dense_short":
        return dense_short_case(int(arg))
    if kind == "tiles_many":
        return tiles_many_case(arg)
    assert kind == "full_scale", name
    return full_scale_case(arg)


def all_cases():
    return [case(n) for n in CASE_NAMES]


@functools.lru_cache(maxsize=None)
def expected(name):
    """The definition's result for the case: (per call (counts, kept records per stream), info per stream).  Computed once."""
    c = case(name)
    return modes_ref.run_bank(c.cfg, c.calls, c.n_streams)


@functools.lru_cache(maxsize=None)
def uncapped(name):
    """Every acceptance of every stream of the case, whatever msg_cap is, with "p", the absolute position."""
    c = case(name)
    per_call, _ = modes_ref.run_bank(dict(c.cfg, msg_cap=1 << 30), c.calls, c.n_streams)
    return [absolute(per_call, c.calls, s) for s in range(c.n_streams)]


def queue_indices(c, s, t):
    """(the acceptances' indices among the candidates of tile t of stream s of a one-call case, the tile's candidate count)"""
    T = tile()
    cand = [p for p in candidates(c.calls[0][s], c.cfg["min_power"]).tolist() if (p + 239) // T == t]
    return [cand.index(r["p"]) for r in uncapped(c.name)[s] if (r["p"] + 239) // T == t], len(cand)


def check_case(name):
    """The definition's result for the case shows what the case is there for."""
    c = case(name)
    per_call, info = expected(name)
    every, want, T, cap = uncapped(name), c.want, tile(), c.cfg["msg_cap"]
    kept = [absolute(per_call, c.calls, s) for s in range(c.n_streams)]
    total = [sum(cnt[s] for cnt, _ in per_call) for s in range(c.n_streams)]
    assert [len(e) for e in every] == total == [i["messages"] for i in info], name
    if "at" in want:                                         # exactly the frames that were put, restored where they were damaged
        for s in range(c.n_streams):
            if s == want.get("noise"):
                continue
            mine = sorted((p, good, bit) for t, p, good, bit in want["at"] if t == s)
            assert [(r["p"], r["bytes"], r["fixed_bit"]) for r in every[s]] == [(p, as_bytes(g), 0xFF if b is None else b) for p, g, b in mine], (name, s)
            assert all(r["n_bytes"] == 14 and r["df"] in (17, 18) for r in every[s])
    if want.get("nothing"):
        assert total == [0] * c.n_streams, (name, total)
    if "queue" in want:
        t, at = want["queue"]
        got, n_cand = queue_indices(c, 0, t)
        assert got == at and n_cand > 128 and n_cand < T, (name, got, n_cand)
        assert info[0]["fixed"] == want["fixed"] and every[0][1 + at.index(QUEUE_DAMAGED)]["fixed_bit"] == 70
        assert len(kept[0]) == min(cap, len(at) + 2) and kept[0] == every[0][:cap]
        assert queue_indices(c, 0, 0)[0] == [0] and queue_indices(c, 0, 2)[0] == [0]
    if "every_bit" in want:
        for t in range(112):
            if want["on"] and t >= 5:
                assert [(r["p"], r["fixed_bit"], r["bytes"], r["df"]) for r in every[t]] == [(40 + t, t, want["every_bit"], 17)], (name, t)
            else:
                assert every[t] == [], (name, t)             # "no record": a flip inside DF, or no fix
        assert sum(i["fixed"] for i in info) == (107 if want["on"] else 0)
    if want.get("doubles"):
        fixable = set(modes_ref.T112[5:])
        assert all(modes_ref.T112[a] ^ modes_ref.T112[b] not in fixable for a, b in DOUBLES)
        assert all(i["candidates"] == 1 for i in info)       # (they are refused by the decode, not by the preamble)
    if "accepted" in want:
        assert [s for s in range(c.n_streams) if total[s]] == want["accepted"] and max(total) == 1, (name, total)
        for s, (df, overlay, bits) in enumerate(want["frames"]):
            assert modes_ref.syndrome_bits(bits) == overlay and info[s]["candidates"] >= 1
            if total[s]:
                assert (every[s][0]["df"], every[s][0]["n_bytes"], every[s][0]["bytes"]) == (df, len(bits) // 8, as_bytes(bits) + bytes(14 - len(bits) // 8))
        assert {df for df, _, _ in want["frames"]} == set(LONG_DFS + SHORT_DFS)
    if "dense" in want:
        n = c.calls[0].shape[1] // 2
        decided = [p for p in want["dense"] if p + 239 < n]
        assert len(want["dense"]) == 323 and len(decided) == 322
        assert [r["p"] for r in every[0]] == decided and info[0]["candidates"] == len(decided)       # and no other candidate
        per_tile = dense_per_tile(T, n, [r["p"] for r in every[0]])
        assert per_tile == [30] + [32] * 9 + [4], (name, per_tile)
        assert [r["p"] for r in kept[0]] == decided[:cap]
        assert all(r["n_bytes"] == 7 and r["df"] == 11 for r in every[0])
        # 8: the overflow is inside every tile; 40: the first tile gives 30 and the second the rest; 256: the cut is in the ninth
        cum = np.cumsum(per_tile)
        assert {8: min(per_tile[:10]) > 8, 40: per_tile[0] < 40 < cum[1], 256: cum[7] < 256 < cum[8]}[cap]
    if "tiles" in want:
        one = uncapped("tiles_many_one")
        assert every == one and sorted((r["p"] + 239) // T for r in every[0]) == want["tiles"], name
        s = want["noise"]
        assert total[s] == 0 and info[s]["candidates"] > 1000
        assert info[0]["candidates"] == len(want["at"]) and info[0]["samples"] == 130 * T
        if name == "tiles_many_one":
            per = np.bincount((candidates(c.calls[0][s]) + 239) // T, minlength=130)
            assert per[:64].sum() > 0 and per[64:128].sum() > 0 and per[128:].sum() > 0      # all three batches of summaries count
        else:
            assert [iq.shape[1] // 2 for iq in c.calls] == [64 * T + 2000, 66 * T - 2000]
    if "power" in want:
        assert all(r["power"] == want["power"] == 260100 for e in every for r in e)
        if name == "full_scale_cut":
            assert every == uncapped("full_scale_at") and per_call[0][0] == [0] * 4 and per_call[1][1][2][0]["k_rel"] == -100
        elif name == "full_scale_at":
            assert [e[0]["p"] for e in every] == [300, 301, 0, 1]
    return every, info
