"""Case table of tests/test_gpu_fir_domain.py: the tapped FIR (csrc/fmd_fir.hip) and the FIR fused with the discriminator and the
resampler (csrc/fmd_firdemod.hip) over every template instantiation the shipped library can launch, in plain numpy.  Each case
names the exact string kernel_name() must return after each of its calls, plus tap_digits() and, for the fused kernel, the tile.
The claims come from the planner's arithmetic alone, restated here -- fmd_fir_common.h: fmd_fir_build_mfma; fmd_fir.hip: fmd_fir_new,
fir_enqueue; fmd_firdemod.hip: fmd_firdemod_new, fd_sizes, fd_enqueue, launch<> -- never from a GPU run.
tests/test_fir_cases.py checks the table against the sources, the shipped code object and two references without a GPU.

Only the shipped library is in scope: the forms behind experiment knobs (dense reg1, NG 10 / 12, RS 2, SWZ) keep their knob tests.

A CLASS is what selects one template instantiation apart from the table flag: (family, NKU, several K passes) for the FIR,
(family, NKU, NG or RS) for the fused kernel.  `sweep_fir` / `sweep_fused` walk the whole domain (1 ... 1024 taps, even decimation
2 ... 64, 8- and 12-bit taps, f32 / integer discriminator, the rate ratios that give every column parameter) and define which classes
are reachable; the deterministic table holds a case at the smallest (taps, decimation) of every class, and the edges of the issue at the
lowest and the highest NKU of every family."""
import math
from types import SimpleNamespace as NS

import numpy as np

from domain_cases import fuzz

PRE = "(anonymous namespace)::"
NKU = tuple(range(1, 9))                                          # the `case N: launch...<N>` lists of both files
FIR_GROUPS_PER_WAVE = 4                                            # kFirGroupsPerWave
FD_ROWS = 160                                                      # kFdRows: calls of more tiles run the table-less instantiation
FD_BUDGET = (0, 0, 0, 0, 20480, 20480, 26880, 32000, 32000, 32000, 40960, 40960, 53760)   # budget[]: LDS per tile by NG
FD_LDS = 20480                                                     # fmd_firdemod::lds_budget without the register form
FD_MAX_OUTPUTS = 64 * 4 * 4                                        # kMaxOutputs
FD_NG = {"reg": (4, 5, 6, 7, 8), "regs": (4, 6, 8), "reg1s": (4, 6, 8)}   # launch<> outside FMD_EXPERIMENT
FD_RS = (0, 1)
FIR_FAMILIES = ("valu", "mfma1", "mfma2", "mfma3")                 # vector pipe; matrix cores with digit form 1 / 2 / 3 (sparse split)
FD_FAMILIES = ("lds0", "lds1", "regs", "reg1s", "reg")             # LDS-array kernel RS 0 / 1; register forms (those run before come first)
CHANNELS = (1, 7, 8, 9, 17)                                        # grid (8, tiles, ceil(C / 8)): the surplus blocks exit
KINDS = ("random", "zeros", "ones", "square", "axis", "diag")      # all 0, all 255, the 0 / 255 square, axis and diagonal full scale
TAPS8 = ("pm127", "pos8", "neg8", "runs8")                         # every |tap| <= 127: one digit
TAPS12 = ("p128", "m128", "pm2047", "split", "pos12", "neg12", "runs12")
SPLIT_EDGES = (192, 191, -65, -64, 64, 63)                         # h = 128 hi + lo, |lo| <= 64: both sides of every digit boundary


class Unsupported(ValueError):
    """A shape or a call outside the documented domain (the library refuses it)."""


# ---- the planner (fmd_fir_common.h, fmd_fir.hip, fmd_firdemod.hip) -----------------------------------------------------------------

def mfma_plan(T, M, opc):
    """fmd_fir_build_mfma: K chunks of 64 bytes for `opc` outputs per column (4: two dense digits; 8: one digit, or the split)."""
    nk = (2 * ((opc - 1) * M + T) + 63) // 64
    if M > 64 or nk > 64:
        return None
    n_pass = (nk + 7) // 8
    return NS(nk=nk, n_pass=n_pass, nku=(nk + n_pass - 1) // n_pass, opc=opc)


def tap_pairs(T):
    return ((T + 1) // 2 + 3) & ~3                                 # NP: tap pairs, zero-padded to a multiple of 4


def hist_words(T):
    return (T - 1 + ((T - 1) & 1)) // 2                            # Hw: history dwords per channel


def fir_select(T, M, small):
    """fmd_fir_new: the kernel a filter of T taps (small: every |tap| <= 127) at decimation M runs."""
    form, plan = (1 if small else 2), None
    if not small and M >= 8:
        sp = mfma_plan(T, M, 8)
        if sp and sp.n_pass == 1:
            form, plan = 3, sp                                     # two digits on the 4:2 sparse instruction, re / im split
    if plan is None:
        plan = mfma_plan(T, M, 8 if form == 1 else 4)
    s = NS(T=T, M=M, small=small, NP=tap_pairs(T), Hw=hist_words(T))
    if plan is None:                                               # decimation beyond 64: the vector-pipe kernel
        s.family, s.nku, s.n_pass, s.form, s.digits, s.groups = "valu", 0, 0, 0, 0, 0
        s.out_tile = min(1024, max(1, (4500 - s.NP) // (M // 2) + 1))
        s.kernel = PRE + "fmd_fir_kernel"
        s.cls = ("valu", 0, False)
        return s
    groups = min(16, max(1, 16384 // ((256 if form != 2 else 128) * M)))
    if form == 3:
        groups = min(groups, 8)                                    # (never binds: M >= 8 gives at most 8)
    assert groups <= 4 * FIR_GROUPS_PER_WAVE
    s.family, s.nku, s.n_pass, s.form, s.digits, s.groups = "mfma%d" % form, min(plan.nku, 8), plan.n_pass, form, min(form, 2), groups
    s.out_tile = 16 * (8 if form != 2 else 4) * groups
    s.kernel = PRE + "fmd_fir_mfma_kernel<%d, false, %d>" % (s.nku, form)
    s.cls = (s.family, s.nku, plan.n_pass > 1)
    return s


def counts(pos, T, M, ns):
    m0 = (pos - T) // M + 1 if pos >= T else 0
    m1 = (pos + ns - T) // M + 1 if pos + ns >= T else 0
    return m0, m1


class FirModel:
    """Host bookkeeping of one FirBank."""

    def __init__(self, sel):
        self.s, self.pos = sel, 0

    def call(self, nbytes):
        s, ns = self.s, nbytes // 2
        assert nbytes % 8 == 0 and nbytes > 0
        m0, m1 = counts(self.pos, s.T, s.M, ns)
        res = NS(nbytes=nbytes, m0=m0, n_out=m1 - m0, par_first=(s.M * m0 // 2) & 1, par_step=(s.M // 2) & 1,
                 tiles=-(-(m1 - m0) // s.out_tile), short=nbytes // 4 < s.Hw, kernel=s.kernel)
        self.pos += ns
        return res

    def len_for(self, want):
        """The shortest call with at least `want` outputs (exactly `want` wherever 4 samples hold at most one window)."""
        s = self.s
        m0, _ = counts(self.pos, s.T, s.M, 0)
        need = s.M * (m0 + want - 1) + s.T - self.pos if want else 4
        return 8 * max(1, -(-need // 4))


def lp_bound(taps, shift):
    return (128 * int(np.abs(np.asarray(taps, np.int64)).sum()) + (1 << shift) - 1) >> shift


def auto_shift(taps, limit):
    g, s = 128 * int(np.abs(np.asarray(taps, np.int64)).sum()), 0
    while (g >> s) > limit:
        s += 1
    return s


def fused_select(T, M, small, f32, fast, slow):
    """fmd_firdemod_new: kernel family, column parameter and tile of a fused bank; f32: lp_bound <= 2048.  None: refused."""
    dense = mfma_plan(T, M, 4)
    if dense is None or slow == 0 or fast < slow:
        return None
    g = math.gcd(fast, slow)
    fr, sr, R = fast // g, slow // g, fast // slow
    fa = fr // sr
    if fr > 1 << 24 or (fa + 2) * 32768 >= 1 << 24 or R >= 1 << 24:
        return None
    plan, digits, ng, sparse, budget = dense, 2, 0, False, FD_LDS
    if M == 8 and dense.n_pass == 1 and f32:
        want = min(fa // 4, 8)
        if want >= 4 and fa >= 4 * want and sr * 64 * (4 * want - 2) < 1 << 24:
            ng = want                                              # the longest columns the audio groups admit
            budget = FD_BUDGET[ng]
        one = mfma_plan(T, M, 8) if small else None
        one_fits = one is not None and one.n_pass == 1
        if one_fits and ng in (5, 7):
            ng -= 1                                                # an 8-bit filter takes the even parameter below an odd one
            budget = FD_BUDGET[ng]
        even = ng in (4, 6, 8)
        if one_fits and even:
            plan, digits = one, 1
        sparse = even
        if sparse and digits == 2:
            sp = mfma_plan(T, M, 8)
            if sp and sp.n_pass == 1:
                plan = sp                                          # two digits, re / im split
            else:
                sparse = False                                     # 201 ... 232 taps: the dense kernel with the even parameter
    s = NS(T=T, M=M, small=small, f32=f32, fast=fast, slow=slow, fr=fr, sr=sr, fa=fa, R=R, g=g, NP=tap_pairs(T), Hw=hist_words(T),
           nku=min(plan.nku, 8), n_pass=plan.n_pass, digits=digits, ng=ng, sparse=sparse, budget=budget,
           reuse=1 if M == 8 and plan.n_pass == 1 else 0)
    s.family = ("reg1s" if digits == 1 else "regs" if sparse else "reg") if ng else "lds%d" % s.reuse
    s.cls = (s.family, s.nku, ng if ng else s.reuse)
    best = 0
    for kt in range(1, 1025):
        if sr * (kt + 2) >= 1 << 24:
            break
        z = fd_sizes(s, kt)
        if z is None or (z.lds > budget and best):
            break
        best = kt
    if not best:
        return None
    s.kt = best
    z = fd_sizes(s, best)
    s.lp_cap, s.raw_bytes, s.lds = z.cap, z.raw, z.lds
    return s


def fd_sizes(s, kt):
    """LDS of one tile of kt audio samples; None where it does not fit."""
    half = s.M // 2
    if s.ng:
        cap = (kt * s.fr + s.sr - 1) // s.sr + 3
        staged = ((((cap - 1) * half + s.NP + 3) // 4 + 3) & ~3) * 16
        pc = 4 * s.ng - 2
        if cap > 64 * pc - 3:
            return None
        touched = 16 * (63 * pc - 3) + 64 * (s.nku + s.ng)
        raw = (max(staged, touched) + 15) & ~15
        total = raw + 12 * (kt + 2) + 8 + 16
    else:
        cap = (kt * s.fr + s.sr - 1) // s.sr + (s.fr + s.sr - 1) // s.sr + 3      # fmd_tile_lp_cap
        if cap > FD_MAX_OUTPUTS:
            return None
        staged = ((((cap - 1) * half + s.NP + 3) // 4 + 3) & ~3) * 16
        touched = 16 * ((cap + 63) // 64) * (8 * s.M) + 64 * s.n_pass * s.nku
        raw = (max(staged, touched) + 15) & ~15
        total = raw + 4 * (cap + 1) + 12 * (kt + 2) + 16
    return None if total > 60 * 1024 else NS(cap=cap, raw=raw, lds=total)


def fused_name(s, rows=True):
    if s.ng:
        return PRE + "fmd_firdemod_reg%s%s_kernel<%d, %d, %s>" % ("1" if s.digits == 1 else "", "s" if s.sparse else "", s.nku, s.ng,
                                                                  "true" if rows else "false")
    return PRE + "fmd_firdemod_kernel<%d, %d>" % (s.nku, s.reuse)


class FusedModel:
    """Host bookkeeping of one FirDemodBank: position, resampler phase, and what fd_enqueue launches for a call."""

    def __init__(self, sel):
        self.s, self.pos, self.i0r = sel, 0, 0

    def call(self, nbytes):
        s, ns = self.s, nbytes // 2
        assert nbytes % 8 == 0 and nbytes > 0
        m0, m1 = counts(self.pos, s.T, s.M, ns)
        md = m1 - m0
        if md < 2:
            raise Unsupported("fewer than 2 filter outputs")
        K = (self.i0r + md * s.sr) // s.fr
        nt = K // s.kt + 1 if s.ng else max(1, -(-K // s.kt))
        assert nt <= 65535 and 2 * s.fr + md * s.sr < 1 << 32
        res = NS(nbytes=nbytes, m0=m0, M=md, K=K, nt=nt, rows=nt <= FD_ROWS, i0r=self.i0r, par_first=(s.M * m0 // 2) & 1,
                 par_step=(s.M // 2) & 1, short=nbytes // 4 < s.Hw)
        res.kernel = fused_name(s, res.rows)
        self.i0r += md * s.sr - K * s.fr
        self.pos += ns
        return res

    def len_for_outputs(self, md):
        s = self.s
        m0, _ = counts(self.pos, s.T, s.M, 0)
        need = s.M * (m0 + md - 1) + s.T - self.pos
        return 8 * max(1, -(-need // 4))

    def len_for(self, want_k):
        """The shortest legal call with at least want_k audio samples (exactly that many from decimation 4 on)."""
        s = self.s
        md = max(2, -(-(want_k * s.fr - self.i0r) // s.sr))
        return self.len_for_outputs(md)


# ---- the domain sweep ---------------------------------------------------------------------------------------------------------------

SWEEP_T = range(1, 1025)
SWEEP_M = range(2, 65, 2)
VALU_M = (66, 128)                                                 # beyond the matrix-core form: the vector-pipe kernel's samples
# rate pairs of the fused sweep: fa = fr / sr from 1 up, every NG at fa == 4 NG and 4 NG + 3, power-of-two and other sr, and an sr
# too large for the register form's range condition (sr * 64 * (4 NG - 2) < 2^24)
RATES = ([(8000, 8000), (24000, 8000), (250000, 32000), (120000, 8000)] + [(8000 * fa, 8000) for fa in range(16, 36)] +
         [(2500000, 48000), (2050000, 32000), (1600001, 48000), (1000000, 44100)])
_sweeps = {}


def sweep_fir():
    """{class: [(T, M, small), ...]} over the whole domain, smallest first."""
    if "fir" not in _sweeps:
        out = {}
        for M in tuple(SWEEP_M) + VALU_M:
            for T in SWEEP_T:
                for small in (True, False):
                    out.setdefault(fir_select(T, M, small).cls, []).append((T, M, small))
        for v in out.values():
            v.sort()
        _sweeps["fir"] = out
    return _sweeps["fir"]


def fused_class(T, M, small, f32, fast, slow):
    """fused_select without the tile search (the class does not depend on it)."""
    dense = mfma_plan(T, M, 4)
    if dense is None:
        return None
    g = math.gcd(fast, slow)
    fr, sr = fast // g, slow // g
    fa, ng, plan, digits = fr // sr, 0, dense, 2
    if M == 8 and dense.n_pass == 1 and f32:
        want = min(fa // 4, 8)
        if want >= 4 and sr * 64 * (4 * want - 2) < 1 << 24:
            ng = want
        one = mfma_plan(T, M, 8) if small else None
        one_fits = one is not None and one.n_pass == 1
        if one_fits and ng in (5, 7):
            ng -= 1
        if ng in (4, 6, 8):
            if one_fits:
                return ("reg1s", min(one.nku, 8), ng)
            sp = mfma_plan(T, M, 8)
            if sp.n_pass == 1:
                return ("regs", min(sp.nku, 8), ng)
        if ng:
            return ("reg", min(dense.nku, 8), ng)
    rs = 1 if M == 8 and dense.n_pass == 1 else 0
    return ("lds%d" % rs, min(plan.nku, 8), rs)


def sweep_fused():
    """{class: [(T, M, small, f32, fast, slow), ...]}, smallest first.  The rates only matter at decimation 8."""
    if "fused" not in _sweeps:
        out = {}
        for M in SWEEP_M:
            for T in SWEEP_T:
                for small in (True, False):
                    for f32 in (True, False):
                        for fast, slow in (RATES if M == 8 else RATES[2:3]):
                            out.setdefault(fused_class(T, M, small, f32, fast, slow), []).append((T, M, small, f32, fast, slow))
        for v in out.values():
            v.sort(key=lambda x: (x[0], x[1], not x[2], not x[3], x[4] // x[5], x[4]))
        _sweeps["fused"] = out
    return _sweeps["fused"]


def members(sweep, family, nku):
    return [x for c in sorted(sweep) if c[0] == family and c[1] == nku for x in sweep[c]]


def family_nkus(sweep, family):
    return sorted({c[1] for c in sweep if c[0] == family})


# ---- taps and data ------------------------------------------------------------------------------------------------------------------

def make_taps(kind, T, rng):
    lim = 127 if kind in TAPS8 or kind == "ones" else 2047
    t = rng.integers(-lim, lim + 1, T).astype(np.int64)
    if kind == "ones":
        t[:] = 1
    elif kind in ("pm127", "pm2047"):
        t[0] = lim
        t[-1 if T > 1 else 0] = -lim if T > 1 else lim
    elif kind in ("pos8", "pos12", "neg8", "neg12"):
        t = np.abs(t) + (t == 0)
        t[T // 2] = lim
        t = -t if kind.startswith("neg") else t
    elif kind in ("runs8", "runs12"):                              # zero runs longer than a K chunk (64 bytes = 32 taps)
        keep = np.zeros(T, bool)
        keep[[0, T - 1]] = True
        keep[::47] = True
        t = np.where(keep, np.where(t == 0, lim, t), 0)
        t[0] = lim
    elif kind in ("p128", "m128"):                                 # one tap one step beyond the one-digit range
        t = rng.integers(-127, 128, T).astype(np.int64)
        t[T // 2] = 128 if kind == "p128" else -128
    elif kind == "split":
        t[0] = SPLIT_EDGES[0]
        if T >= 6:
            t[rng.permutation(T)[:6]] = SPLIT_EDGES
    else:
        raise ValueError(kind)
    return t.astype(np.int16)


def axis_pattern(re, im):
    """8 raw bytes whose rotated and centred samples are all (re, im), for re, im in {-127, 0, 128}."""
    p, n = (lambda v: v + 127), (lambda v: 128 - v)
    return np.array([p(re), p(im), p(im), n(re), n(re), n(im), n(im), p(re)], np.uint8)


def data(case, ci):
    """[C, nbytes] bytes of call ci: every channel its own stream, so that a channel-index slip cannot pass."""
    call = case.calls[ci]
    rng = np.random.default_rng([case.seed, ci])
    C, n, kind = case.nch, call.nbytes, call.kind
    if kind == "random":
        return rng.integers(0, 256, (C, n), dtype=np.uint8)
    if kind in ("zeros", "ones"):
        out = np.full((C, n), 0 if kind == "zeros" else 255, np.uint8)
        out[1::2] = rng.integers(0, 256, (len(out[1::2]), n), dtype=np.uint8)   # (the odd channels stay random: rows must differ)
        return out
    if kind == "square":
        return np.where(rng.integers(0, 2, (C, n)) > 0, 255, 0).astype(np.uint8)
    axes = [(128, 0), (-127, 0), (0, 128), (0, -127)]
    vals = axes if kind == "axis" else [(128, 128), (-127, -127), (128, -127), (-127, 128)]
    seg = 8 * max(2, case.M // 2)                                  # stretches of one value: a few per window
    nseg = -(-n // seg)
    out = np.empty((C, nseg * seg), np.uint8)
    for c in range(C):
        picks = rng.integers(0, 4, nseg) if c else np.zeros(nseg, np.int64)     # channel 0: one full-scale constant throughout
        out[c] = np.concatenate([np.tile(axis_pattern(*vals[k]), seg // 8) for k in picks])
    return np.ascontiguousarray(out[:, :n])


# ---- references in numpy --------------------------------------------------------------------------------------------------------------

def rotated(stream):
    """rotate_90 + centre of a whole stream of bytes (a multiple of 8) -> (re, im) int64."""
    b = np.asarray(stream, np.uint8).reshape(-1, 8).astype(np.int64)
    rot = np.stack([b[:, 0], b[:, 1], 255 - b[:, 3], b[:, 2], 255 - b[:, 4], 255 - b[:, 5], b[:, 7], 255 - b[:, 6]], 1).reshape(-1) - 127
    return rot[0::2], rot[1::2]


def fir_np(taps, M, re, im, m0, m1):
    """Outputs m0 ... m1 - 1 of the int64 convolution y[m] = sum_t h[t] x[M m + t] -> [m1 - m0, 2]."""
    if m1 <= m0:
        return np.empty((0, 2), np.int64)
    T, h = len(taps), np.asarray(taps, np.int64)
    win = np.lib.stride_tricks.sliding_window_view
    lo, hi = M * m0, M * (m1 - 1) + T
    return np.stack([win(x[lo:hi], T)[::M] @ h for x in (re, im)], 1)


class FirNp:
    """The streaming FIR as an int64 numpy convolution of the rotated, centred stream: keeps the last taps - 1 samples (rounded up to whole
    groups of 4, so that the rotation phase of the kept bytes is the stream's) between calls."""

    def __init__(self, taps, M):
        self.taps, self.M, self.pos, self.tail = np.asarray(taps, np.int64), M, 0, np.empty(0, np.uint8)

    def feed(self, iq):
        T, M = len(self.taps), self.M
        buf = np.concatenate([self.tail, np.asarray(iq, np.uint8)])
        skip = self.pos - self.tail.size // 2                      # stream samples in front of `buf`: a multiple of 4
        m0, m1 = counts(self.pos, T, M, iq.size // 2)
        re, im = rotated(buf)
        off = M * m0 - skip if m1 > m0 else 0
        assert skip % 4 == 0 and off >= 0
        y = fir_np(self.taps, M, re[off:], im[off:], 0, m1 - m0)
        self.pos += iq.size // 2
        self.tail = buf[buf.size - min(buf.size, 8 * -(-T // 4)):]
        return y


def wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def wrap16(v):
    return ((v + (1 << 15)) & 0xFFFF) - (1 << 15)


def fast_atan2_np(y, x):
    """Demod::fast_atan2 on int64 arrays with explicit 32-bit wrapping (vector form of pyref.fast_atan2)."""
    yabs = np.where(y < 0, wrap32(-y), y)
    pos = x >= 0
    num = wrap32(4096 * wrap32(np.where(pos, x - yabs, x + yabs)))
    den = wrap32(np.where(pos, x + yabs, yabs - x))
    zero = (x == 0) & (y == 0)
    den = np.where(zero, 1, den)
    assert not np.any(den == 0)
    q = np.abs(num) // np.abs(den)
    q = np.where((num < 0) == (den < 0), q, -q)                    # truncation toward zero
    angle = wrap32(np.where(pos, 4096, 3 * 4096) - q)
    return np.where(zero, 0, np.where(y < 0, wrap32(-angle), angle))


class ChainNp:
    """fm_demod + low_pass_real of the reference chain on arrays, call by call: the vector form of pyref.Demod for the calls that
    are too long for a per-sample Python loop.  tests/test_fir_cases.py holds it to pyref on every case pyref can run."""

    def __init__(self, fast, slow):
        import pyref
        self.pyref, self.fast, self.slow = pyref, fast, slow
        self.demod_pre, self.now_lpr, self.prev_lpr_index = (0, 0), 0, 0

    def state(self):
        return (self.now_lpr, self.prev_lpr_index, list(self.demod_pre))

    def feed(self, lp):
        re, im = lp[:, 0].astype(np.int64), lp[:, 1].astype(np.int64)
        assert len(re) > 1
        pr = np.concatenate([[self.demod_pre[0]], re[:-1]])
        pi = np.concatenate([[self.demod_pre[1]], im[:-1]])
        cr, ci = wrap32(re * pr + im * pi), wrap32(im * pr - re * pi)
        d = wrap16(fast_atan2_np(ci, cr))
        d[0] = self.pyref.wrap16(self.pyref.polar_discriminant((int(re[0]), int(im[0])), self.demod_pre))   # the f64 sample
        self.demod_pre = (int(re[-1]), int(im[-1]))
        # low_pass_real: sample j closes an audio sample when floor((i0 + (j + 1) slow) / fast) steps
        e = (self.prev_lpr_index + (np.arange(len(d), dtype=np.int64) + 1) * self.slow) // self.fast
        ends = np.nonzero(np.diff(np.concatenate([[0], e])))[0]
        cs = np.concatenate([[0], np.cumsum(d)])
        starts = np.concatenate([[0], ends[:-1] + 1]) if len(ends) else ends
        sums = cs[ends + 1] - cs[starts]
        if len(sums):
            sums[0] += self.now_lpr
        tail = int(cs[-1] - (cs[ends[-1] + 1] if len(ends) else 0)) + (0 if len(ends) else self.now_lpr)
        assert np.all(np.abs(sums) < 1 << 31) and abs(tail) < 1 << 31
        R = self.fast // self.slow
        out = wrap16(np.where(sums < 0, -(-sums // R), sums // R))
        self.now_lpr = tail
        self.prev_lpr_index = int(self.prev_lpr_index + len(d) * self.slow - len(ends) * self.fast)
        return out.astype(np.int16)


# ---- cases --------------------------------------------------------------------------------------------------------------------------

def describe(case):
    extra = "" if case.op == "fir" else " shift=%d %d->%d tile=%d lp_bound=%d" % (case.shift, case.fast, case.slow, case.sel.kt, case.lp_bound)
    return "%s case %d [%s] %s: taps=%d (%s) decim=%d channels=%d%s calls=%s" % (
        case.op, case.i, ",".join(sorted(case.tags)), case.sel.cls, case.T, case.tapkind, case.M, case.nch, extra,
        [(c.nbytes, c.kind, c.kernel.split("::")[-1]) for c in case.calls])


def _kinds(i, n, tapkind=""):
    if tapkind.startswith(("pos", "neg")):
        i = 4                                                      # same-sign taps: all 0 and all 255 on the two longest calls (4th and 5th)
    ks = [KINDS[(i + j) % len(KINDS)] for j in range(n)]
    if "random" not in ks:
        ks[0] = "random"
    return ks


def _align_for_short(model, legal_min, short_bytes, min_out, count):
    """Length of a call after which a call of short_bytes still yields min_out outputs (the windows end just inside it)."""
    for a in range(legal_min, legal_min + 8 * (2 * model.s.M + 8), 8):
        m0, m1 = counts(model.pos + a // 2, model.s.T, model.s.M, short_bytes // 2)
        if m1 - m0 >= min_out and count(model.pos, a // 2) >= (min_out if min_out > 1 else 0):
            return a
    raise AssertionError("no alignment for the short call")


def fir_case(cases, taps, M, nch, tags, tapkind, big=False):
    """The call walk of the stand-alone FIR: a call that emits nothing, one output, out_tile - 1 / out_tile / out_tile + 1 outputs, three
    tiles with a partial last one, and an 8-byte call that emits while being shorter than the carried history -- each streaming on."""
    T = len(taps)
    sel = fir_select(T, M, int(np.abs(taps.astype(np.int64)).max()) <= 127)
    m = FirModel(sel)
    case = NS(op="fir", i=len(cases), T=T, M=M, taps=taps, nch=nch, tags=set(tags), tapkind=tapkind, sel=sel, calls=[], seed=5000 + 7 * len(cases) + M,
              device=False, ckpt=None)
    ot = sel.out_tile
    for label, nbytes in (("nothing", 8), ("one", None)):          # (up to 4 taps even the first 8 bytes emit)
        case.calls.append(m.call(nbytes or m.len_for(1)))
        case.calls[-1].label = label
    for label, want in (("tile-1", ot - 1), ("tile", ot), ("tile+1", ot + 1), ("three-tiles", 2 * ot + max(1, ot // 3))):
        case.calls.append(m.call(m.len_for(want)))
        case.calls[-1].label = label
    a = _align_for_short(m, 8, 8, 1, lambda pos, ns: 0)
    case.calls.append(m.call(a))
    case.calls[-1].label = "align"
    case.calls.append(m.call(8))
    case.calls[-1].label = "short"
    case.calls.append(m.call(m.len_for(3)))
    case.calls[-1].label = "after-short"
    for call, kind in zip(case.calls, _kinds(case.i, len(case.calls), tapkind)):
        call.kind = kind
    cases.append(case)
    return case


def fused_case(cases, taps, M, shift, fast, slow, nch, tags, tapkind, tiles=None):
    """The call walk of the fused kernel: the shortest legal call, then kt - 1 / kt / kt + 1 audio samples (one tile, and the step to two),
    three tiles with a partial last one, and the shortest legal call again where it is shorter than the carried history (8 bytes at
    decimation 2; from 4 on the kernel refuses a call of fewer than 2 filter outputs).  tiles: the table-less walk instead -- calls
    of exactly 160 and 161 tiles."""
    T = len(taps)
    small = int(np.abs(taps.astype(np.int64)).max()) <= 127
    lpb = lp_bound(taps, shift)
    if ((128 * int(np.abs(taps.astype(np.int64)).sum())) >> shift) > 16384:
        raise Unsupported("gain")
    sel = fused_select(T, M, small, lpb <= 2048, fast, slow)
    if sel is None:
        raise Unsupported("shape or rates")
    m = FusedModel(sel)
    case = NS(op="fused", i=len(cases), T=T, M=M, taps=taps, shift=shift, fast=fast, slow=slow, nch=nch, tags=set(tags), tapkind=tapkind,
              sel=sel, lp_bound=lpb, calls=[], seed=9000 + 7 * len(cases) + M, device=False, ckpt=None)
    kt = sel.kt

    def add(label, nbytes):
        case.calls.append(m.call(nbytes))
        case.calls[-1].label = label

    add("min", m.len_for_outputs(2))
    if tiles:
        for nt in tiles:
            want = (nt - 1) * kt + (0 if sel.ng else 1)           # register form: nt = K / kt + 1; LDS-array kernel: ceil(K / kt)
            add("tiles%d" % nt, m.len_for(want))
        add("after", m.len_for(2))
    else:
        for label, want in (("tile-1", kt - 1), ("tile", kt), ("tile+1", kt + 1), ("three-tiles", 2 * kt + max(1, kt // 3))):
            add(label, m.len_for(max(want, 0)))
        ns_short = 4 * -(-(M + 1) // 4)                            # the fewest samples that can hold two window ends
        lo = m.len_for_outputs(2)
        a = _align_for_short(m, lo, 2 * ns_short, 2, lambda pos, ns: counts(pos, T, M, ns)[1] - counts(pos, T, M, ns)[0])
        add("align", a)
        add("short", 2 * ns_short)
        add("after-short", m.len_for(2))
    for call, kind in zip(case.calls, _kinds(case.i, len(case.calls), tapkind)):
        call.kind = "random" if call.label.startswith("tiles") else kind
    cases.append(case)
    return case


def _rng(*key):
    return np.random.default_rng([20261, *key])


def fir_pick(family, nku, half_odd, tmin=6):
    """The smallest decimation of the wanted half-parity, then the fewest taps >= tmin, in (family, nku) -> (T, M)."""
    sweep = sweep_fir()
    best = None
    for cls, members in sweep.items():
        if cls[0] != family or cls[1] != nku:
            continue
        for T, M, small in members:
            if M == 2 and T % 4 not in (0, 3):
                continue                                           # (decimation 2: calls end on multiples of 4 samples, one window must end in the last 2)
            if T >= tmin and (M // 2) % 2 == int(half_odd) and (best is None or (M, T) < best):
                best = (M, T)
    return (best[1], best[0]) if best else None


def fused_pick(family, nku, ng_rs=None, half_odd=None, tmin=6, f32=None):
    best = None
    for cls, members in sweep_fused().items():
        if cls[0] != family or cls[1] != nku or (ng_rs is not None and cls[2] != ng_rs):
            continue
        for mem in members:
            T, M = mem[0], mem[1]
            if T >= tmin and (half_odd is None or (M // 2) % 2 == int(half_odd)) and (f32 is None or mem[3] == f32):
                if best is None or (M, T) < (best[1], best[0]):
                    best = mem
    return best


def realise(T, small, f32, rng, kind=None):
    """Taps and shift of a fused bank with the wanted width and discriminator form."""
    kind = kind or ("pm127" if small else "pm2047")
    taps = make_taps(kind, T, rng)
    if not small and int(np.abs(taps.astype(np.int64)).max()) <= 127:
        taps[0] = 2047
    shift = auto_shift(taps, 2048 if f32 else 16384)
    if f32 and lp_bound(taps, shift) > 2048:                       # (the library rounds the bound up: 2049 is the integer form)
        shift += 1
    if not f32 and lp_bound(taps, shift) <= 2048:                  # a gain this small cannot leave the f32 range
        return None
    return taps, shift


def rates_for(ng, plus=0):
    return 8000 * (4 * ng + plus), 8000


def bound_pair(T, small, rng):
    """The same filter with lp_bound exactly 2048 (f32 discriminator) and, one tap a step larger, 2049 (integer): sum|h| = 2048 at shift 7."""
    if (small and T * 127 < 2049) or T < 2:
        return None
    head = 0 if small else 200                                     # (12-bit: one tap beyond the one-digit range)
    n = T - (0 if small else 1)
    mag = np.full(n, (2048 - head) // n, np.int64)
    mag[:2048 - head - mag.sum()] += 1
    if not small:
        mag = np.concatenate([[head], mag])
    assert mag.sum() == 2048 and mag.min() < (127 if small else 2047)
    sign = np.where(rng.integers(0, 2, T) > 0, 1, -1)
    a = (mag * sign).astype(np.int16)
    b = a.copy()
    k = int(np.argmin(mag))
    b[k] += 1 if b[k] >= 0 else -1
    assert lp_bound(a, 7) == 2048 and lp_bound(b, 7) == 2049
    return a, b


def deterministic():
    """-> (fir cases, fused cases)."""
    if "table" in _sweeps:
        return _sweeps["table"]
    fir, fus = [], []
    sf, sd = sweep_fir(), sweep_fused()
    # -- FIR: one case at the smallest shape of every class ------------------------------------------------------------------------------
    for n, cls in enumerate(sorted(sf)):
        T, M, small = sf[cls][0]
        kinds = TAPS8 if small else TAPS12
        kind = kinds[n % len(kinds)]
        fir_case(fir, make_taps(kind, T, _rng(1, n)), M, CHANNELS[n % 5], {"class"}, kind)
    # -- FIR: the edges at the lowest and the highest NKU of every family -----------------------------------------------------------------
    for fam in FIR_FAMILIES:
        nkus = family_nkus(sf, fam)
        for nku in sorted({nkus[0], nkus[-1]}):
            kinds = TAPS8 if fam in ("mfma1",) else TAPS12 if fam != "valu" else TAPS8 + TAPS12
            picks = [fir_pick(fam, nku, True), fir_pick(fam, nku, False)]
            variants = max(len(kinds), len(CHANNELS))
            for v in range(variants):
                T, M = picks[v % 2] or picks[(v + 1) % 2]
                kind = kinds[v % len(kinds)]
                if kind in ("runs8", "runs12") and T < 48:         # a zero run longer than a K chunk needs the taps for it
                    T = max(t for t, mm, s in members(sf, fam, nku) if mm == M and (M > 2 or t % 4 in (0, 3)))
                fir_case(fir, make_taps(kind, T, _rng(2, len(fir))), M, CHANNELS[v % 5], {"edge", "nku%d" % nku}, kind)
    # the boxcar, which the reference's own KATs anchor: all ones, taps == decimation
    for M in (2, 8, 10, 64, 66):
        fir_case(fir, np.ones(M, np.int16), M, CHANNELS[M % 5], {"boxcar"}, "ones")
    # one case per family through filter_device
    for fam in FIR_FAMILIES:
        next(c for c in fir if c.sel.family == fam and "edge" in c.tags and c.nch >= 8).device = True

    # -- fused: one case at the smallest shape of every class ----------------------------------------------------------------------------
    for n, cls in enumerate(sorted(sd)):
        done = False
        for T, M, small, f32, fast, slow in sd[cls]:
            kinds = TAPS8 if small else TAPS12
            got = realise(T, small, f32, _rng(3, n), kinds[n % len(kinds)])
            if got is None:
                continue
            c = fused_case(fus, got[0], M, got[1], fast, slow, CHANNELS[n % 5], {"class"}, kinds[n % len(kinds)])
            assert c.sel.cls == cls, (cls, describe(c))
            done = True
            break
        assert done, cls
    # -- fused: the edges at the lowest and the highest NKU of every family --------------------------------------------------------------
    for fam in FD_FAMILIES:
        nkus = family_nkus(sd, fam)
        for nku in sorted({nkus[0], nkus[-1]}):
            small_fam = fam == "reg1s"
            kinds = TAPS8 if small_fam else TAPS12 if fam in ("regs", "reg") else TAPS12 + TAPS8
            mems = [fused_pick(fam, nku, half_odd=True), fused_pick(fam, nku, half_odd=False)]
            for v in range(max(len(kinds), len(CHANNELS))):
                kind = kinds[v % len(kinds)]
                small = kind in TAPS8
                mem = mems[v % 2] or mems[(v + 1) % 2]
                cand = [x for x in members(sd, fam, nku) if x[2] == small and x[1] == mem[1] and x[0] >= 6 and (x[1] > 2 or x[0] % 4 in (0, 3))]      # (decimation 2: both window parities need such a tap count)
                if not cand:
                    continue                                       # (the family does not take this tap width at this NKU)
                # enough taps for the shortest legal call to be shorter than the history, where the class has them (not at 1 - 2 K chunks of decimation 8)
                cand = [x for x in cand if hist_words(x[0]) > 2 * -(-(x[1] + 1) // 4)] or cand
                mem = cand[0] if kind not in ("runs8", "runs12") or cand[0][0] >= 48 else cand[-1]
                T, M, _, f32, fast, slow = mem
                got = realise(T, small, f32, _rng(4, len(fus)), kind)
                if got is None:
                    continue
                c = fused_case(fus, got[0], M, got[1], fast, slow, CHANNELS[v % 5], {"edge", "nku%d" % nku}, kind)
                assert c.sel.family == fam and c.sel.nku == nku, describe(c)
            # lp_bound exactly 2048 and 2049 for the same filter: the register families lose the 2049 twin to the LDS-array kernel
            for small in ((True,) if small_fam else (False,) if fam in ("regs", "reg") else (False, True)):
                cand = [x for x in members(sd, fam, nku) if x[2] == small and x[3]]
                pair = None
                for x in cand:
                    pair = bound_pair(x[0], small, _rng(5, len(fus)))
                    if pair:
                        break
                if not pair:
                    continue                                       # (8-bit taps: sum|h| = 2048 needs 17 taps, beyond this NKU)
                T, M, _, _, fast, slow = x
                a = fused_case(fus, pair[0], M, 7, fast, slow, 8, {"bound2048", "nku%d" % nku}, "bound")
                b = fused_case(fus, pair[1], M, 7, fast, slow, 9, {"bound2049", "nku%d" % nku}, "bound")
                assert a.sel.family == fam and a.sel.nku == nku and a.lp_bound == 2048 and b.lp_bound == 2049, (describe(a), describe(b))
                a.twin = b.i
    # every NG at fa == 4 NG exactly and at 4 NG + 3, 8- and 12-bit taps (8-bit: 5 -> 4, 7 -> 6)
    for ng in range(4, 9):
        for plus in (0, 3):
            for small in (False, True):
                fast, slow = rates_for(ng, plus)
                taps, shift = realise(33, small, True, _rng(6, ng, plus, small))
                c = fused_case(fus, taps, 8, shift, fast, slow, CHANNELS[(ng + plus) % 5], {"ng-edge"}, "pm127" if small else "pm2047")
                assert c.sel.ng == (ng - (ng % 2 if small else 0)) and c.sel.fa == 4 * ng + plus, describe(c)
    # power-of-two and other reduced resample rates in the register forms and in the LDS-array kernel; an sr beyond the register form's range
    for fast, slow, tag in ((2050000, 32000, "sr-pow2"), (2500000, 48000, "sr-other"), (250000, 32000, "sr-pow2"), (1000000, 44100, "sr-other"),
                            (100000, 44100, "sr-other"),                            (1600001, 48000, "sr-range")):
        for small in (False, True):
            taps, shift = realise(63, small, True, _rng(7, fast, small))
            fused_case(fus, taps, 8, shift, fast, slow, 8, {tag}, "pm127" if small else "pm2047")
    # rate_out == rate_resample, where the kernel admits it: the LDS-array kernel, both mappings
    for T, M in ((5, 2), (31, 8), (300, 8), (129, 64)):
        taps, shift = realise(T, False, True, _rng(8, T))
        fused_case(fus, taps, M, shift, 48000, 48000, 7, {"ratio-one"}, "pm2047")
    # the tap counts at which the plans change, decimation 8, register-form rates: 8-bit 200 / 201 (one digit fits, then does not);
    # 12-bit 200 / 201 / 232 / 233 (split, dense even NG, outside the register form)
    for small, Ts in ((True, (200, 201, 232, 233)), (False, (200, 201, 232, 233))):
        for T in Ts:
            for ng in (8, 7):
                fast, slow = rates_for(ng)
                taps, shift = realise(T, small, True, _rng(9, T, small, ng))
                fused_case(fus, taps, 8, shift, fast, slow, 8, {"tap-boundary"}, "pm127" if small else "pm2047")
    # the boxcar: all ones, taps == decimation, shift 0 -- the reference chain itself
    for M, fast, slow in ((2, 48000, 48000), (8, 250000, 8000), (8, 170000, 32000), (10, 240000, 32000), (64, 37500, 8000)):
        fused_case(fus, np.ones(M, np.int16), M, 0, fast, slow, CHANNELS[M % 5], {"boxcar"}, "ones")
    # table-less launches: calls of exactly 160 and 161 tiles on one channel, at the lowest rate ratio the form admits
    for fam, ngs in (("lds0", (0,)), ("lds1", (1,)), ("regs", (4, 8)), ("reg1s", (4, 8)), ("reg", (5, 7)), ("reg-even", (4, 8))):
        for ng in ngs:
            small = fam == "reg1s"
            T = 201 if fam == "reg-even" else 9
            M = 2 if fam == "lds0" else 8
            fast, slow = (8000, 8000) if fam.startswith("lds") else rates_for(ng)
            taps, shift = realise(T, small, True, _rng(10, len(fus)))
            c = fused_case(fus, taps, M, shift, fast, slow, 1, {"tableless"}, "pm127" if small else "pm2047", tiles=(FD_ROWS, FD_ROWS + 1))
            assert c.sel.family == fam.split("-")[0] and (not c.sel.ng or c.sel.ng == ng), describe(c)
    # one case per family through demodulate_device + check, one with a checkpoint / resume in the middle
    for fam in FD_FAMILIES:
        mine = [c for c in fus if c.sel.family == fam and "edge" in c.tags]
        next(c for c in mine if c.nch >= 8).device = True
        next(c for c in mine if c.nch >= 8 and not c.device).ckpt = 3
    _sweeps["table"] = (fir, fus)
    return fir, fus


def groups_of(cases):
    """[(family, nku)] in run order: the families that ran before this table first, the table-less launches last."""
    fams = FIR_FAMILIES if cases and cases[0].op == "fir" else FD_FAMILIES
    keys = sorted({(c.sel.family, c.sel.nku) for c in cases if "tableless" not in c.tags}, key=lambda k: (fams.index(k[0]), k[1]))
    return keys


# ---- references -----------------------------------------------------------------------------------------------------------------------

def reference_fir(case, oracle):
    """Per call (ci, iq, [per-channel int32 [n, 2]]) from the C oracle."""
    hs = [oracle.fir_new(case.taps, case.M) for _ in range(case.nch)]
    try:
        for ci in range(len(case.calls)):
            iq = data(case, ci)
            yield ci, iq, [oracle.fir_filter(hs[c], iq[c]) for c in range(case.nch)]
    finally:
        for h in hs:
            oracle.lib.fmo_fir_free(h)


def state_tuple(s):
    return (s["now_lpr"], s["prev_lpr_index"], list(s["demod_pre"]))


def reference_fused(case, oracle):
    """Per call (ci, iq, [per-channel int16], [per-channel state tuple]) from the C oracle's composition."""
    hs = [oracle.firdemod_new(case.taps, case.M, case.shift, case.fast, case.slow) for _ in range(case.nch)]
    try:
        for ci in range(len(case.calls)):
            iq = data(case, ci)
            audio = [oracle.firdemod(hs[c], iq[c]) for c in range(case.nch)]
            yield ci, iq, audio, [state_tuple(oracle.firdemod_state(hs[c])) for c in range(case.nch)]
    finally:
        for h in hs:
            oracle.lib.fmo_firdemod_free(h)


# ---- what the hand-picked shapes of tests/test_fir.py and tests/test_firdemod.py reached ---------------------------------------------

LEGACY_FIR = [(127, 8), (6, 6), (10, 10), (5, 2), (16, 16), (33, 4), (1, 2), (64, 6), (255, 32), (300, 8), (1024, 2), (129, 64), (77, 66),
              (31, 128), (63, 8), (200, 8), (64, 16), (31, 12), (100, 10), (9, 26)]
LEGACY_FUSED = ([(127, 8, 2500000, 48000), (33, 4, 250000, 48000), (5, 2, 96000, 48000), (64, 6, 170000, 32000), (255, 32, 625000, 8000),
                 (300, 8, 100000, 44100), (16, 16, 48000, 48000), (129, 64, 37500, 8000), (1, 2, 500000, 32000), (127, 16, 1250000, 48000),
                 (200, 16, 625000, 44100), (255, 16, 625000, 48000)],                      # both discriminator forms possible (drawn)
                [(127, 8, 2500000, 48000), (127, 8, 1000000, 44100), (8, 8, 250000, 8000), (200, 8, 480000, 8000), (33, 8, 960000, 48000),
                 (1, 8, 640000, 32000)],                                                   # REG_SHAPES: 12-bit, f32
                [(127, 8, 2500000, 48000), (200, 8, 480000, 8000), (64, 8, 768000, 48000), (100, 8, 1200000, 48000), (8, 8, 256000, 8000),
                 (1, 8, 1280000, 32000), (127, 8, 1000000, 44100), (33, 8, 960000, 32000)])  # REG1_SHAPES: 8-bit, f32


def legacy_reach():
    """The classes the named shapes can reach at best (the drawn discriminator form counted both ways) -> (fir set, fused set)."""
    fir = {fir_select(T, M, small).cls for T, M in LEGACY_FIR for small in (True, False) if not (T == M and not small)}
    fus = set()
    for T, M, fast, slow in LEGACY_FUSED[0]:
        fus |= {fused_class(T, M, False, f32, fast, slow) for f32 in (True, False)}
    fus |= {fused_class(T, M, False, True, fast, slow) for T, M, fast, slow in LEGACY_FUSED[1]}
    fus |= {fused_class(T, M, True, True, fast, slow) for T, M, fast, slow in LEGACY_FUSED[2]}
    return {c for c in fir if c[0] != "valu"}, fus


# ---- the seeded random leg ------------------------------------------------------------------------------------------------------------

def draw_fir(rng, i):
    sf = sweep_fir()
    cls = sorted(sf)[int(rng.integers(0, len(sf)))]
    T, M, small = sf[cls][int(rng.integers(0, len(sf[cls])))]
    kinds = TAPS8 if small else TAPS12
    kind = kinds[int(rng.integers(0, len(kinds)))]
    taps = make_taps(kind, T, rng)
    sel = fir_select(T, M, int(np.abs(taps.astype(np.int64)).max()) <= 127)
    m = FirModel(sel)
    case = NS(op="fir", i=100000 + i, T=T, M=M, taps=taps, nch=int(rng.integers(1, 19)), tags={"fuzz"}, tapkind=kind, sel=sel, calls=[],
              seed=7100000 + i, device=False, ckpt=None)
    for _ in range(int(rng.integers(3, 7))):
        r = rng.random()
        nbytes = 8 * int(rng.integers(1, 6)) if r < 0.25 else m.len_for(int(rng.integers(1, 3 * sel.out_tile))) + 8 * int(rng.integers(0, 4))
        case.calls.append(m.call(nbytes))
        case.calls[-1].label, case.calls[-1].kind = "fuzz", KINDS[int(rng.integers(0, len(KINDS)))]
    return case


def draw_fused(rng, i):
    """One random case inside the documented domain (gain <= 16384 behind the shift, rate range, >= 2 filter outputs per call);
    None where the draw cannot be realised (the caller draws again)."""
    sd = sweep_fused()
    cls = sorted(sd)[int(rng.integers(0, len(sd)))]
    T, M, small, f32, fast, slow = sd[cls][int(rng.integers(0, len(sd[cls])))]
    if M != 8 and rng.random() < 0.7:                              # away from decimation 8 the rates do not decide the class
        slow = int(rng.choice([8000, 32000, 44100, 48000]))
        fast = slow * int(rng.integers(1, 12)) + int(rng.integers(0, slow)) * int(rng.integers(0, 2))
    kinds = TAPS8 if small else TAPS12
    kind = kinds[int(rng.integers(0, len(kinds)))]
    got = realise(T, small, f32, rng, kind)
    if got is None:
        return None
    taps, shift = got
    if f32 and rng.random() < 0.5:
        shift = min(24, shift + int(rng.integers(0, 3)))
    cases = []
    try:
        c = fused_case(cases, taps, M, shift, fast, slow, int(rng.integers(1, 19)), {"fuzz"}, kind)
    except Unsupported:
        return None
    if c.sel.cls != cls or max(k.nbytes for k in c.calls) * c.nch > 8 << 20:
        return None
    # a random walk in place of the fixed one
    m = FusedModel(c.sel)
    c.calls = []
    for _ in range(int(rng.integers(3, 7))):
        r = rng.random()
        nbytes = m.len_for_outputs(int(rng.integers(2, 6))) if r < 0.25 else m.len_for(int(rng.integers(0, 3 * c.sel.kt))) + 8 * int(rng.integers(0, 4))
        c.calls.append(m.call(nbytes))
        c.calls[-1].label, c.calls[-1].kind = "fuzz", KINDS[int(rng.integers(0, len(KINDS)))]
    c.i, c.seed = 200000 + i, 7200000 + i
    return c


def fuzz_source(op):
    """-> (number of cases wanted, generator of cases without end)."""
    n, rng = fuzz(40, 91 if op == "fir" else 92)

    def gen():
        i = 0
        while True:
            c = draw_fir(rng, i) if op == "fir" else draw_fused(rng, i)
            i += 1
            if c is not None:
                yield c
    return n, gen()
