"""Case table of tests/test_gpu_demod_domain.py: the demodulation kernels (fmd_demod_*) over every instantiation that
fmd_launch_tile can pick and every prologue, in plain numpy.  Each case names, call by call, the kernel it must run -- the exact
string DemodBank.last_kernel() reports.  The claim is derived here from the plan arithmetic alone (fmd_index.h: fmd_make_plan,
fmd_make_tiling, fmd_tile_fast; fmd_tile_launch.hip: fmd_fast_geometry; fmd_api.cpp: enqueue and the streaming kernel's tile
planner), never from a GPU run.  tests/test_demod_cases.py checks the table against the references without a GPU.

A fast prologue needs one phase class, >= 8 channels, a call length that is a multiple of 16 bytes and tiles within the LDS
sizing; the table (FAST == 2) at most 32 tiles, the closed form (FAST == 1) tiles that repeat exactly (kt * fr % sr == 0).
Everything else runs the general prologue (FAST == 0).  Calls stay small through explicit small tiles (set_tiling): a few audio
samples per tile put 32 or 33 tiles into a few KiB per channel."""
import math
from types import SimpleNamespace as NS

import numpy as np

from domain_cases import fuzz

FAST_ROWS = 32                                                     # FMD_FAST_ROWS
LDS_EVEN = tuple(range(2, 33, 2)) + (64, 128)                      # fmd_launch_tile's FMD_CASE list: DH = D / 2 ...
LDS_ODD = tuple(range(1, 32, 2))                                   # ... and DH = -D
CATCH_ALL = (33, 34, 63, 65, 66, 96, 127)                          # samples of instantiation 0: both sides of 64, both ends
STREAM = (2, 4)
LDS_FACTORS = tuple(sorted(LDS_EVEN + LDS_ODD))
ALL_FACTORS = LDS_FACTORS + CATCH_ALL
FAST_CHANNELS = (8, 9, 15, 16, 17, 64)                             # grid (8, tiles, ceil(C / 8)): 9, 15, 17 leave blocks with channel >= C
BLOCK_FACTORS = (2, 5, 6, 10, 16, 31, 64, 96)
BLOCK_COUNTS = (1, 2, 5, 33)
KINDS = ("random", "square", "axis", "diag", "silence", "dcflip")
# (fr, sr) of the deterministic table, times BASE: 5 : 2 and its kin have kt * fr % sr == 0 exactly when sr divides kt
RATE_PAIRS = ((5, 2), (7, 3), (16, 3), (85, 16), (3, 2), (9, 4))
RATE_PAIRS_WIDE = ((3, 2), (5, 3))                                 # beyond downsample 32: a low ratio keeps 33 tiles within 64 KiB
BASE = 2000


# ---- the plan arithmetic (fmd_index.h) -------------------------------------------------------------------------------------------

def rates(D, fast, slow, kt):
    g = math.gcd(fast, slow)
    return NS(D=D, fast=fast, slow=slow, g=g, fr=fast // g, sr=slow // g, R=fast // slow, kt=kt)


def lp_cap(r):
    return (r.kt * r.fr + r.sr - 1) // r.sr + (r.fr + r.sr - 1) // r.sr + 3


def raw_cap(r):
    return ((lp_cap(r) + 1) * 2 * r.D + 32 + 15) & ~15


def make_plan(r, p0, i0r, ns):
    M = (p0 + ns) // r.D
    K = (i0r + M * r.sr) // r.fr
    a0 = r.fr - i0r - 1
    return NS(p0=p0, i0r=i0r, M=M, K=K, nt=max(1, (K + r.kt - 1) // r.kt), eq0=a0 // r.sr, er0=a0 % r.sr)


def make_tiling(r):
    a, b = r.kt * r.fr, (r.kt - 1) * r.fr
    return NS(Qt=a // r.sr, Rt=a % r.sr, fq=r.fr // r.sr, frr=r.fr % r.sr, Bq=b // r.sr, Br=b % r.sr)


def tile_fast(r, P, g, ns, t):
    last = t + 1 == P.nt
    k0 = t * r.kt
    k1 = max(k0, min(k0 + r.kt, P.K))
    x = P.er0 + t * g.Rt
    eq, er = t * g.Qt + P.eq0 + x // r.sr, x % r.sr
    jA = 0 if t == 0 else eq - g.fq + (1 if er >= g.frr else 0)
    jB = P.M - 1 if last else eq + g.Bq + (1 if er + g.Br >= r.sr else 0)
    nLo = max(0, r.D * (jA - 1) - P.p0) if jA >= 1 else 0
    nHi = ns if last else r.D * (jB + 1) - P.p0
    return NS(k0=k0, k1=k1, eq=eq, er=er, jA=jA, jB=jB, nLo=nLo, nHi=max(nHi, nLo), last=last)


def next_phase(r, P, ns):
    return (P.p0 + ns) % r.D, P.i0r + P.M * r.sr - P.K * r.fr


def supported(r):
    """fmd_tile_kernel_supports + the LDS bound of choose_tiling: the tile kernels take these rates with this tile."""
    return (r.D <= 128 and r.sr * (r.kt + 2) < 1 << 24 and ((r.fr + r.sr - 1) // r.sr + 2) * 32768 < 1 << 24 and r.R < 1 << 24
            and raw_cap(r) <= 60 * 1024 and raw_cap(r) + 6 * lp_cap(r) + 32 <= 64 * 1024)


def ranges_fit32(r, ns):
    return ns <= 1 << 30 and 2 * r.fr + ((r.D - 1 + ns) // r.D) * r.sr < 1 << 32 and (r.kt + 2) * r.fr < 1 << 32


def fast_mode(r, P, nch, nbytes, stream, tiles_limit=FAST_ROWS, out_cap=None):
    """fmd_fast_geometry for a bank in ONE phase class on the XCD-aware grid: 2 the table, 1 the closed form, 0 neither.  `out_cap`
    is the caller's output pitch in samples: the table addresses the output with 32-bit products and is refused from
    nch * out_cap * 2 == 2^32 bytes on (the closed form then takes the call where it applies); None is an output far below that."""
    if nch < 8 or nbytes % 16 or P.nt == 0 or nbytes >= 1 << 31:
        return 0
    ns, g = nbytes // 2, make_tiling(r)
    lc, rc = lp_cap(r), raw_cap(r)
    tiles = [tile_fast(r, P, g, ns, t) for t in range(P.nt)]
    fits = all(T.jB - T.jA + 2 <= lc and (stream or 2 * (T.nHi - T.nLo) + 30 <= rc) for T in tiles)
    if P.nt <= tiles_limit and (out_cap is None or nch * out_cap * 2 < 1 << 32):
        return 2 if fits else 0
    if g.Rt:
        return 0
    jA_off = P.eq0 - g.fq + (1 if P.er0 >= g.frr else 0)
    jB_off = P.eq0 + g.Bq + (1 if P.er0 + g.Br >= r.sr else 0)
    lo_off2, hi_off2 = 2 * (r.D * (jA_off - 1) - P.p0), 2 * (r.D * (jB_off + 1) - P.p0)
    step2 = 2 * r.D * g.Qt
    if jA_off > 0 or step2 * P.nt + max(hi_off2, 0) >= 1 << 31:
        return 0
    for t, T in enumerate(tiles):
        jA = max(t * g.Qt + jA_off, 0)
        jB = P.M - 1 if T.last else t * g.Qt + jB_off
        nLo2 = max(t * step2 + lo_off2, 0)
        nHi2 = nbytes if T.last else t * step2 + hi_off2
        if (jA, jB, nLo2, nHi2) != (T.jA, T.jB, 2 * T.nLo, 2 * T.nHi):
            return 0
    return 1 if fits else 0


def stream_tile(D, fast, slow):
    """The streaming kernel's audio samples per tile (fmd_demod_new): least wave-instructions per audio sample among tiles of
    64, 96, ... whose decimated samples fit 4 waves x 127 x the straight-line rounds.  None where no such tile exists."""
    if D not in STREAM:
        return None
    r = rates(D, fast, slow, 0)
    nw = 4
    cap_cnt = nw * 127 * (16 if D == 2 else 8) - 8
    kts, best = 0, 0.0
    for k in range(64, 4097, 32):
        r.kt = k
        if lp_cap(r) > cap_cnt or r.sr * (k + 2) >= 1 << 24:
            break
        cnt = (k * r.fr + r.sr - 1) // r.sr + 1
        rounds = (cnt + 126) // 127
        per_wave, passes = (rounds + nw - 1) // nw, (k + 64 * nw - 1) // (64 * nw)
        work = float(per_wave) * nw * 100.0 + float(passes) * nw * (70.0 + 6.0 * float(r.fr // r.sr)) + nw * (250.0 if D == 2 else 150.0)
        if kts == 0 or work / float(k) < best:
            best, kts = work / float(k), k
    if kts == 0:
        return None                                                # (the library would take the LDS tile: not derivable here)
    r.kt = kts
    ok = 2 * (lp_cap(r) + r.fr // r.sr + 3) + 48 <= 60 * 1024 and D <= 128 and ((r.fr + r.sr - 1) // r.sr + 2) * 32768 < 1 << 24 and r.R < 1 << 24
    return kts if ok else None


def default_tile_bound(r):
    """choose_tiling plans within 20480 bytes of LDS, of which the staged bytes alone are more than 2 D kt fr / sr: the planner's
    tile is below this bound (its exemption for a tile of 1 changes nothing: 1 is below it too, or the bound is <= 1)."""
    return max(2, -(-20480 * r.sr // (2 * r.D * r.fr)))


def name(D, mode, stream=False):
    if stream:
        return "fmd_tk::fmd_demod_stream_kernel<%d, %d>" % (D // 2, mode)
    dh = (D // 2 if D % 2 == 0 else -D) if D in LDS_FACTORS else 0
    return "fmd_tk::fmd_demod_tile_kernel<%d, %d>" % (dh, mode)


class Illegal(ValueError):
    """A call the library refuses (length, block length, fewer than two decimated samples, ranges)."""


class PlannerTile(ValueError):
    """The prologue of a call depends on the tile choose_tiling picks, which this module does not restate."""


class Model:
    """Host bookkeeping of one DemodBank: the phase classes and what enqueue() would launch for a call."""

    def __init__(self, D, fast, slow, nch, kt=None, block=0, out_cap=None):
        self.D, self.fast, self.slow, self.nch, self.kt, self.block, self.out_cap = D, fast, slow, nch, kt, block, out_cap
        self.r = rates(D, fast, slow, kt or 1)
        self.kts = None if kt else stream_tile(D, fast, slow)
        self.classes = [(0, 0)]                                    # (p0, i0r) per class

    def legal(self, nbytes):
        if nbytes % 8 or (self.block and (nbytes % self.block or self.block // 2 < 2 * self.D)):
            return False
        return ranges_fit32(self.r, nbytes // 2) and all((p0 + nbytes // 2) // self.D >= 2 for p0, _ in self.classes)

    def call(self, nbytes):
        """-> NS(kernel, mode, nt, stream; K, M, p0, i0r per class); advances the classes."""
        ns, D, r = nbytes // 2, self.D, self.r
        one = len(self.classes) == 1
        p0s = [p for p, _ in self.classes]
        res = None
        if self.kts and self.nch >= 8 and not self.block and one and p0s[0] % 2 == 0 and nbytes >= 64 * D:
            rs = rates(D, self.fast, self.slow, self.kts)
            P = make_plan(rs, *self.classes[0], ns)
            mode = fast_mode(rs, P, self.nch, nbytes, True, out_cap=self.out_cap)
            if mode:
                res = NS(kernel=name(D, mode, True), mode=mode, nt=P.nt, stream=True)
        plans = [make_plan(r, p0, i0r, ns) for p0, i0r in self.classes]
        if res is None and self.kt:
            mode = fast_mode(r, plans[0], self.nch, nbytes, False, out_cap=self.out_cap) if one else 0
            res = NS(kernel=name(D, mode), mode=mode, nt=max(P.nt for P in plans), stream=False)
        elif res is None:
            # the planner's own LDS tile: only what holds for every tile it can choose is claimed
            K, bound = max(P.K for P in plans), default_tile_bound(r)
            if self.nch < 8 or nbytes % 16 or not one:
                mode = 0
            elif self.out_cap is not None and self.nch * self.out_cap * 2 >= 1 << 32:
                raise PlannerTile("without the table, the prologue of this call depends on the planner's tile")
            elif K <= FAST_ROWS:
                mode = 2                                           # at most 32 tiles whatever the tile
            elif r.sr > 1 and bound <= r.sr and K > FAST_ROWS * bound:
                mode = 0                                           # more than 32 tiles, and kt < sr cannot repeat exactly
            else:
                raise PlannerTile("the prologue of this call depends on the planner's tile")
            res = NS(kernel=name(D, mode), mode=mode, nt=None, stream=False)
        res.K, res.M, res.p0, res.i0r = [P.K for P in plans], [P.M for P in plans], p0s, [i for _, i in self.classes]
        self.classes = [next_phase(r, P, ns) for P in plans]
        return res

    def set_p0(self, p0):
        assert len(self.classes) == 1
        self.classes = [(p0, self.classes[0][1])]

    def split(self, pre):
        """The odd channels consume `pre` bytes first (checkpointed from a Demod that is further along): two classes."""
        assert len(self.classes) == 1 and self.classes[0] == (0, 0)
        P = make_plan(self.r, 0, 0, pre // 2)
        assert P.M >= 2
        nxt = next_phase(self.r, P, pre // 2)
        if nxt == self.classes[0]:
            return False
        self.classes.append(nxt)
        return True


# ---- data ------------------------------------------------------------------------------------------------------------------------

def data(case, ci):
    """[C, nbytes] bytes of call ci: every channel its own stream, so that a channel-index slip cannot pass."""
    from test_gpu_parity import axis_pattern
    call = case.calls[ci]
    rng = np.random.default_rng([case.seed, ci])
    C, n, D = case.nch, call.nbytes, case.D
    kind = call.kind
    if kind == "random":
        return rng.integers(0, 256, (C, n), dtype=np.uint8)
    if kind == "square":
        return np.where(rng.integers(0, 2, (C, n)) > 0, 255, 0).astype(np.uint8)
    if kind == "silence":
        b = rng.integers(126, 131, (C, n)).astype(np.uint8)
        b[::2, ::2] = 128                                          # even channels: I constant, Q moving
        # channel 0: the real part of EVERY rotated and centred sample is zero (bytes 0, 3, 4, 7 of each 8 at 127, 128, 128, 127), so
        # every decimated sample is (0, s) and every product (s s', 0): y == 0 with either sign of x, at any downsample
        # (its imaginary parts, bytes 1, 2 less 127 and 128 less bytes 5, 6, are drawn from -2 ... 2: sums of either sign)
        b[0] = rng.integers(126, 131, n)
        for k, v in ((0, 127), (3, 128), (4, 128), (7, 127)):
            b[0, k::8] = v
        for k in (1, 2):
            b[0, k::8] -= 1
        return b
    seg = 8 * D                                                    # bytes: four whole windows, a multiple of the rotation period
    nseg = -(-n // seg)
    out = np.empty((C, nseg * seg), np.uint8)
    if kind in ("axis", "diag"):
        axes = [(128, 0), (-127, 0), (0, 128), (0, -127), (0, 0)]
        vals = axes if kind == "axis" else [(128, 128), (-127, -127), (128, -127), (-127, 128)] + axes
        for c in range(C):
            picks = rng.integers(0, 4 if kind == "diag" and c % 4 == 1 else len(vals), nseg)
            if kind == "diag" and c % 4 == 2:
                picks[:] = 0                                       # the saturated constant: every product is the wrap point
            out[c] = np.concatenate([np.tile(axis_pattern(*vals[k]), seg // 8) for k in picks])
        return np.ascontiguousarray(out[:, :n])
    assert kind == "dcflip"
    pos = axis_pattern(128, 128)
    # channel 0: full-scale DC of alternating sign in stretches of 4 D + 4 samples -- at least three whole windows of one sign, and a
    # flip that moves through the window by 4 samples from one flip to the next
    alt = np.concatenate([np.tile(pos if k % 2 == 0 else 255 - pos, D + 1) for k in range(-(-n // (8 * D + 8)))])
    out[0, :n] = alt[:n]
    for c in range(1, C):
        parts, left = [], n
        while left > 0:
            m = min(left, 8 * int(rng.integers(1, 3 * D)))
            k = int(rng.integers(0, 3))
            parts.append(np.tile(pos if k == 0 else 255 - pos, m // 8) if k < 2 else rng.integers(0, 256, m, dtype=np.uint8))
            left -= m
        out[c, :n] = np.concatenate(parts)
    return np.ascontiguousarray(out[:, :n])


def prefeed(case):
    """The bytes the odd channels of a two-class case consume before the first call."""
    return np.random.default_rng([case.seed, 999]).integers(0, 256, case.pre, dtype=np.uint8)


def lp_for(p0, c):
    """The partial boxcar sum that goes with a boxcar phase set by hand: |.| <= 128 p0 (what p0 samples can add up to), per channel."""
    return (min(128 * p0, 37 * c) * (1 if c % 2 else -1), -(p0 * ((7 * c) % 129)))


def reference(case, oracle):
    """Runs the case through the C oracle (tests/oracle_lib.py), block by block where the case sets a block length.  Yields per
    call (ci, install, iq, audio, states): `install` maps channels to the state (Oracle.state_of) the handle under test must be
    given before the call -- the checkpoint of a Demod that is further along, or a boxcar phase no call length reaches."""
    nch = case.nch
    obank = oracle.new_bank(oracle.config(case.D, case.fast, case.slow), nch)
    install = {}
    if case.pre:
        for c in range(1, nch, 2):
            oracle.demodulate(obank[c], prefeed(case))
            install[c] = oracle.state_of(obank[c])
    for ci, call in enumerate(case.calls):
        if call.set_p0 is not None:
            for c in range(nch):
                obank[c].prev_index = call.set_p0
                obank[c].lp_now.re, obank[c].lp_now.im = lp_for(call.set_p0, c)
                install[c] = oracle.state_of(obank[c])
        iq = data(case, ci)
        if case.block:
            audio = [np.concatenate([oracle.demodulate(obank[c], iq[c, o:o + case.block]) for o in range(0, call.nbytes, case.block)])
                     for c in range(nch)]
        else:
            out, lens = oracle.demodulate_batch(obank, iq)
            audio = [out[c, :lens[c]] for c in range(nch)]
        yield ci, install, iq, audio, [oracle.state_of(obank[c]) for c in range(nch)]
        install = {}


def describe(case):
    return "case %d %s: D=%d %d->%d channels=%d tile=%s block=%s pre=%s calls=%s" % (
        case.i, case.cause, case.D, case.fast, case.slow, case.nch, case.kt, case.block, case.pre,
        [(c.nbytes, c.kind, c.set_p0, c.kernel) for c in case.calls])


# ---- the deterministic table -----------------------------------------------------------------------------------------------------

def _len_for(m, want_nt, align16=True, frac=0.0, min_bytes=0, exact=True):
    """The call length (bytes) from the model's present state at which the call has want_nt tiles: the shortest such length
    plus `frac` of the way to the shortest with one more tile.  align16 False: lengths that are 8 mod 16.  exact False (the random
    leg, whose wanted count may be one that no length gives): the nearest count from above will do."""
    r = m.r if not (m.kts and not m.kt) else rates(m.D, m.fast, m.slow, m.kts)
    off = 0 if align16 else 8

    def nt(nbytes):
        return max(make_plan(r, p0, i0r, nbytes // 2).nt for p0, i0r in m.classes)

    def first(want):
        lo, hi = 0, 1
        while nt(16 * hi + off) < want:
            hi *= 2
        while lo < hi:                                             # smallest q with nt(16 q + off) >= want
            mid = (lo + hi) // 2
            lo, hi = (mid + 1, hi) if nt(16 * mid + off) < want else (lo, mid)
        return lo
    a, b = first(want_nt), first(want_nt + 1)
    q = a + int(frac * (b - 1 - a))
    nbytes = 16 * q + off
    while (not m.legal(nbytes) or nbytes < min_bytes) and nbytes < 1 << 26:
        nbytes += 16
    assert nt(nbytes) == want_nt or not exact, (m.D, m.kt, want_nt, nbytes, nt(nbytes))
    return nbytes


def _pair(D):
    pairs = RATE_PAIRS if D <= 32 else RATE_PAIRS_WIDE
    fr, sr = pairs[D % len(pairs)]
    if sr * D > 160:
        fr, sr = pairs[0]                                          # (85 : 16 only where 33 tiles of 16 stay small)
    return fr * BASE, sr * BASE, sr


def _extreme(D, j):
    kinds = ["square", "axis", "diag", "silence"] + (["dcflip"] if D >= 64 else [])
    return kinds[(D + j) % len(kinds)]


def _case(cases, cause, D, fast, slow, nch, kt, steps, block=0, pre=0, exact=True, out_cap=None):
    """steps: (want_nt or ('bytes', n), options) per call.  Every case gets random data in one call and an extreme kind in
    another (the first two), then alternates.  `out_cap`: the output pitch the case's calls will be given (fast_mode)."""
    m = Model(D, fast, slow, nch, kt, block, out_cap)
    while pre and not m.split(pre):
        pre += 8                                                   # (the same phases again: a little more)
    case = NS(i=len(cases), cause=cause, D=D, fast=fast, slow=slow, nch=nch, kt=kt, block=block, pre=pre, calls=[],
              seed=1000 * len(cases) + D)
    for j, (want, opt) in enumerate(steps):
        if "set_p0" in opt:
            m.set_p0(opt["set_p0"])
        if isinstance(want, tuple):
            nbytes = want[1]
        else:
            nbytes = _len_for(m, want, opt.get("align16", True), opt.get("frac", 0.0), opt.get("min_bytes", 0), exact)
        if not m.legal(nbytes):
            raise Illegal("%s D=%d: a call of %d bytes is refused" % (cause, D, nbytes))
        res = m.call(nbytes)
        kind = opt.get("kind") or ("random" if j % 2 == 0 else _extreme(D, len(cases) + j))
        case.calls.append(NS(nbytes=nbytes, kind=kind, set_p0=opt.get("set_p0"), kernel=res.kernel, mode=res.mode, nt=res.nt,
                             stream=res.stream, K=res.K, M=res.M, p0=res.p0, i0r=res.i0r))
    assert len(case.calls) >= 3 and supported(m.r), (cause, D)
    cases.append(case)
    return case


def _roundup(n, a):
    return -(-n // a) * a


def deterministic():
    cases = []
    for idx, D in enumerate(ALL_FACTORS):
        fast, slow, sr = _pair(D)
        rep, odd = sr, sr + 1                                      # tiles that repeat exactly / that do not
        few = FAST_CHANNELS[idx % 5]                               # 8, 9, 15, 16, 17 in turn
        # the table prologue at 1, 2 and 32 tiles; the first call is the smallest legal one (often no audio at all)
        nch = 64 if D in (3, 10, 33) else few
        # (the extreme data kinds sit on the long calls of this case and the next: every kind at every factor on >= 96 decimated samples)
        _case(cases, "table", D, fast, slow, nch, odd,
              [(("bytes", _roundup(4 * D, 16)), {"kind": "random"}), (2, {"frac": 0.5, "kind": "square"}), (32, {"frac": 1.0, "kind": "diag"}),
               (1, {"frac": 0.3, "kind": "random"}), (32, {"kind": "axis"})])
        # its boundary: 33 tiles leave the table -- the closed form where the tiles repeat ...
        _case(cases, "closed", D, fast, slow, FAST_CHANNELS[(idx + 2) % 5], rep,
              [(33, {"kind": "silence"}), (32, {"frac": 1.0, "kind": "square"}),
               (33 + idx % 7, {"frac": 0.6, "kind": "dcflip" if D >= 64 else "random"}), (2, {"frac": 0.5, "kind": "random"})])
        # ... and the general prologue where they do not
        _case(cases, "general-tiles", D, fast, slow, FAST_CHANNELS[(idx + 1) % 5], odd,
              [(33, {}), (32, {"frac": 1.0}), (34 + idx % 5, {"frac": 0.4})])
        for nch in (1, 7):
            _case(cases, "general-channels", D, fast, slow, nch, odd, [(3, {"frac": 0.5}), (1, {}), (33, {}), (2, {"frac": 0.9})])
        # 8 mod 16: the odd channels start 8 bytes off a 16-byte boundary (stage_slow); one aligned call in between
        _case(cases, "general-length", D, fast, slow, FAST_CHANNELS[(idx + 3) % 5], odd,
              [(4, {"align16": False, "frac": 0.5}), (5, {"frac": 0.2}), (1, {"align16": False}), (7, {"align16": False, "frac": 0.8})])
        _case(cases, "general-classes", D, fast, slow, FAST_CHANNELS[(idx + 4) % 5], odd,
              [(3, {"frac": 0.5}), (2, {}), (6, {"frac": 0.7})], pre=8 * (2 * D + 13 + idx))
        if D % 2 == 0 and D <= 16:
            # boxcar phases that no call length reaches (lengths are multiples of 4 samples): set like a restored checkpoint
            _case(cases, "phases", D, fast, slow, few, odd, [(2 + p % 3, {"set_p0": p, "frac": 0.5}) for p in range(D)] + [(3, {})])
    # lengths that walk the phase through every reachable value; small odd factors reach them all
    for D in (1, 3, 5, 7, 6, 12):
        fast, slow, sr = _pair(D)
        _case(cases, "phases", D, fast, slow, 8, sr + 1, [(("bytes", 16 * (2 * D + 1 + j)), {}) for j in range(max(3, 2 * D))])
    # rate_out == rate_resample with tiles of one audio sample: tile t starts AT decimated sample t, so tile 1 has jfirst = 0
    for D in (6, 7, 10, 33, 64):
        _case(cases, "ratio-one", D, 8 * BASE, 8 * BASE, 8 + D % 3, 1, [(5, {}), (32, {}), (33, {}), (2, {})])
    # the streaming kernel (no explicit tile): the table at 1, 2 and 32 tiles; 33 tiles leave it for the LDS kernel
    for D in STREAM:
        _case(cases, "stream-table", D, 1000000, 44100, 8 + D, None,
              [(1, {"frac": 0.5, "min_bytes": 64 * D}), (2, {}), (32, {"frac": 1.0}), (33, {}), (1, {"frac": 0.9, "min_bytes": 64 * D})])
        fast, slow = (500000, 32000) if D == 2 else (256000, 48000)
        _case(cases, "stream-table", D, fast, slow, 16 if D == 2 else 9, None, [(1, {"min_bytes": 64 * D}), (3, {"frac": 0.5}), (2, {})])
        # an odd phase takes the LDS kernel (a call of at most 32 audio samples: the table whatever the planner's tile), back to even
        small = {"kind": "random"}
        _case(cases, "stream-phase", D, fast, slow, 8, None,
              [(1, {"min_bytes": 64 * D}), (("bytes", 16 * 12 * D), dict(small, set_p0=1)), (("bytes", 16 * 9 * D), {"set_p0": D - 1}),
               (2, {"set_p0": 0}), (("bytes", 16 * 2 * D), {}), (("bytes", 16 * 10 * D), {"set_p0": 1}), (1, {"set_p0": D - 2, "frac": 0.5})])
    # several reference calls per launch (set_block_len), rates 4 : 1 (a tile of kt audio samples is 8 kt D bytes) ...
    for D in BLOCK_FACTORS:
        for cause, kt, block in (("blocks-sub-tile", 4, 16 * D), ("blocks-one-tile", 2, 16 * D), ("blocks-tiles", 1, 32 * D if D < 64 else 16 * D),
                                 ("blocks-phase", 1, 16 * D + 16)):
            if cause == "blocks-phase" and (8 * D + 8) % D == 0:
                continue                                           # downsample 2: every legal block is a whole number of windows
            _case(cases, cause, D, 128000, 32000, FAST_CHANNELS[(D + kt) % 5], kt,
                  [(("bytes", B * block), {}) for B in BLOCK_COUNTS], block=block)
        # ... and 85 : 16, where tiles of 3 or 1 do not repeat: the table, then (33 blocks of 1.5 tiles each) the general prologue
        _case(cases, "blocks-table", D, 170000, 32000, 8, 3, [(("bytes", B * 16 * D), {}) for B in BLOCK_COUNTS], block=16 * D)
        _case(cases, "blocks-general", D, 170000, 32000, 9, 1, [(("bytes", B * 16 * D), {}) for B in (33, 2, 5)], block=16 * D)
    return cases


def device_cases(cases):
    """One case per prologue for the device entry point."""
    return [next(c for c in cases if c.cause == cause and c.D == D) for cause, D in (("table", 6), ("closed", 10), ("general-tiles", 7))]


# ---- the seeded random leg -------------------------------------------------------------------------------------------------------

FUZZ_SLOW = (8000, 11025, 16000, 32000, 44100, 48000)


def draw(rng, i):
    """One random case: any instantiation, 8 ... 40 channels, lengths that are multiples of 16, tile and block length at random.
    None where the model already knows the library refuses it (the caller draws again)."""
    D = int(rng.choice(ALL_FACTORS))
    slow = int(rng.choice(FUZZ_SLOW))
    fast = slow * int(rng.integers(1, 7)) if rng.random() < 0.4 else int(slow * rng.uniform(1.0, 8.0))
    nch = int(rng.integers(8, 41))
    kt = None if D in STREAM and rng.random() < 0.5 else int(rng.integers(1, 13)) * (rates(D, fast, slow, 1).sr if rng.random() < 0.4 else 1)
    block = 16 * int(rng.integers(max(1, -(-D // 4)), D + 24)) if kt and rng.random() < 0.4 else 0
    steps = []
    for _ in range(int(rng.integers(3, 6))):
        if block:
            steps.append((("bytes", block * int(rng.integers(1, 40))), {}))
        elif kt is None:
            steps.append((int(rng.integers(1, 4)), {"frac": float(rng.random()), "min_bytes": 64 * D}))
        else:
            steps.append((int(rng.integers(1, 70)), {"frac": float(rng.random())}))
    kinds = [str(rng.choice(KINDS[:5] if D < 64 else KINDS)) for _ in steps]
    kinds[int(rng.integers(0, len(kinds)))] = "random"
    steps = [(w, dict(o, kind=k)) for (w, o), k in zip(steps, kinds)]
    r = rates(D, fast, slow, kt or 1)
    if not supported(r) or r.fr > 1 << 20 or (kt is None and stream_tile(D, fast, slow) is None):
        return None
    if max(lp_cap(r) * 2 * D * 70, 0) > 1 << 22 and kt:           # keeps a call of up to 70 tiles small
        return None
    out = []
    try:
        c = _case(out, "fuzz", D, fast, slow, nch, kt, steps, block=block, exact=False)
    except (Illegal, PlannerTile):
        return None
    if max(x.nbytes for x in c.calls) * nch > 16 << 20:
        return None
    c.i, c.seed = 100000 + i, 7000000 + 1000 * i + D
    return c


def fuzz_source():
    """-> (number of cases wanted, generator of legal-by-the-model cases without end)."""
    n, rng = fuzz(40, 77)

    def gen():
        i = 0
        while True:
            c = draw(rng, i)
            i += 1
            if c is not None:
                yield c
    return n, gen()
