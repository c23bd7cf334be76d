"""Integer definition of the code squelch (include/fmd.h, "code squelch"), restated for the tests.

Per row, with P = block, B = box, T = len(lp), i the sample index since creation or reset, everything at a negative index 0:
    m[i]    = x[i][0]  (width 1)   or   (x[i][0] + x[i][1]) >> 1  (width 2)
    b[k]    = (sum_{r<B} m[k B + r]) >> log2 B
    soft[k] = sat16((sum_{t<T} lp[t] b[k - (T-1) + t]) >> lshift)
    bit j of w[k] = 23 soft[k - tap[j]] > sum_j' soft[k - tap[j']]
    d_f = popcount(w[k] ^ u_f);  f(k) = the smallest f with d_f minimal;  k is a hit on f(k) if that d_f <= tol
    block j = samples [jP, (j+1)P), its k are jP/B <= k < (j+1)P/B:  hits_f;  f* = the smallest f with hits_f maximal
    hit_j = f* if hits_f* >= min_hits, else NONE
    state (t, cand, cnt, h) from (NONE, NONE, 0, 0), once per completed block (the tone squelch's rule):
        hit != NONE: cnt = min(cnt + 1, 65535) if hit == cand else (cand, cnt) = (hit, 1);   hit == NONE: cand = NONE, cnt = 0
        then cnt >= confirm: t = cand, h = hang;  else h > 0: h -= 1;  else t = NONE
    s_j = 256 if t != NONE and bit t of accept is set, else 0;  s_{-1} = s_{-2} = 0
    g[i] = s_{j-2} + (((s_{j-1} - s_{j-2}) (min(r, Q - 1) + 1)) >> log2 Q),  Q = ramp, r = i mod P;   out[i][c] = (x[i][c] g[i]) >> 8

`dcs_row` is the definition in plain Python integers, sample by sample.  `CodeSquelch` is the handle's call semantics over many
rows, vectorised in int64 (every sum stays below 2^31); tests/test_dcs.py holds it against `dcs_row`."""
from collections import namedtuple

import numpy as np

Cfg = namedtuple("Cfg", "block box lp lshift tap tol min_hits confirm hang ramp accept")
NONE = -1
_POP16 = np.array([bin(v).count("1") for v in range(1 << 16)], np.uint8)


def popcount(v):
    """of a uint32 array"""
    v = np.asarray(v, dtype=np.uint32)
    return _POP16[v & 0xFFFF].astype(np.int64) + _POP16[v >> 16]


def mono(x):
    """x int [..., width] -> m int64 [...]"""
    x = np.asarray(x, dtype=np.int64)
    return x[..., 0] if x.shape[-1] == 1 else (x[..., 0] + x[..., 1]) >> 1


def step(state, hit, cfg):
    """(t, cand, cnt, h) after a block whose decision is `hit`, and the block's s."""
    t, cand, cnt, h = state
    if hit != NONE:
        if hit == cand:
            cnt = min(cnt + 1, 65535)
        else:
            cand, cnt = hit, 1
    else:
        cand, cnt = NONE, 0
    if cnt >= cfg.confirm:
        t, h = cand, cfg.hang
    elif h > 0:
        h -= 1
    else:
        t = NONE
    s = 256 if t != NONE and (cfg.accept >> t) & 1 else 0
    return (t, cand, cnt, h), s


def decide(hits, cfg):
    """hits: the F counters of one block (ints) -> (hit, f*, hits_f*)."""
    fs = max(range(len(hits)), key=lambda f: (hits[f], -f))
    return (fs if hits[fs] >= cfg.min_hits else NONE), fs, hits[fs]


def _cfg(cfg):
    cfg = Cfg(*cfg)
    return cfg._replace(lp=[int(v) for v in cfg.lp], tap=[int(v) for v in cfg.tap], accept=int(cfg.accept))


def dcs_row(x, words, cfg):
    """The definition in plain Python integers: x int [N, width] of one row, words the F table words ->
    (out: list of N lists of width ints, reports: per completed block (hit, t, hits_f*, s_j), soft: every soft[k], w: every w[k])."""
    cfg = _cfg(cfg)
    P, B, T, F = cfg.block, cfg.box, len(cfg.lp), len(words)
    lgB, Q = B.bit_length() - 1, cfg.ramp
    lgQ = Q.bit_length() - 1
    assert 1 << lgB == B and 1 << lgQ == Q <= P and P % 64 == 0 and len(cfg.tap) == 23
    words = [int(u) for u in words]
    xs = [[int(v) for v in s] for s in x]
    state, sp, sc = (NONE, NONE, 0, 0), 0, 0
    b, soft, ws = [], [], []
    box = 0
    hits = [0] * F
    out, reports = [], []
    for i, smp in enumerate(xs):
        r = i % P
        m = smp[0] if len(smp) == 1 else (smp[0] + smp[1]) >> 1
        g = sp + (((sc - sp) * (min(r, Q - 1) + 1)) >> lgQ)
        out.append([(v * g) >> 8 for v in smp])
        box += m
        if i % B == B - 1:
            k = len(b)
            b.append(box >> lgB)
            box = 0
            acc = 0
            for t in range(T):
                kk = k - (T - 1) + t
                if kk >= 0:
                    acc += cfg.lp[t] * b[kk]
            soft.append(max(-32768, min(32767, acc >> cfg.lshift)))
            v = [soft[k - d] if k - d >= 0 else 0 for d in cfg.tap]
            total = sum(v)
            w = 0
            for j in range(23):
                if 23 * v[j] > total:
                    w |= 1 << j
            ws.append(w)
            best, bf = 99, 0
            for f in range(F):
                d = bin(w ^ words[f]).count("1")
                if d < best:
                    best, bf = d, f
            if best <= cfg.tol:
                hits[bf] += 1
        if r == P - 1:
            hit, _, n = decide(hits, cfg)
            state, s = step(state, hit, cfg)
            sp, sc = sc, s
            reports.append((hit, state[0], n, s))
            hits = [0] * F
    return out, reports, soft, ws


class CodeSquelch:
    """The handle's call semantics over many rows: push(x) returns the gated samples of the call; the open box's samples, the last
    T - 1 b, the last tap[22] soft, the hit counters, the state and (s_{j-2}, s_{j-1}) per row are carried.  `hits` collects (block,
    row, hit, f*, hits_f*) of every completed block."""

    def __init__(self, words, cfg):
        self.cfg = _cfg(cfg)
        c = self.cfg
        self.words = np.asarray(words, dtype=np.uint32).reshape(-1)
        self.F, self.P, self.B, self.T = len(self.words), c.block, c.box, len(c.lp)
        self.lgB = self.B.bit_length() - 1
        assert 1 << self.lgB == self.B and self.P % 64 == 0 and len(c.tap) == 23 and c.tap[0] == 0
        assert max(abs(v) for v in c.lp) <= 1023 and int(self.words.max()) < 1 << 23
        self.lp = np.array(c.lp, np.int64)
        self.tap = np.array(c.tap, np.int64)
        self.reset()

    def reset(self):
        self.N = 0
        self.open = None

    def _start(self, rows):
        if self.open is None:
            self.open = np.zeros((rows, 0), np.int64)                       # m of the open box
            self.bh = np.zeros((rows, self.T - 1), np.int64)
            self.sh = np.zeros((rows, int(self.tap[22])), np.int64)
            self.cnt = np.zeros((rows, self.F), np.int64)
            self.state = [(NONE, NONE, 0, 0)] * rows
            self.sp, self.sc = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
            self.last = [0] * rows
            self.hits = []

    def status(self):
        """(code [rows], hits [rows], open [rows]) after the last completed block."""
        return ([s[0] for s in self.state], list(self.last), [bool(v) for v in self.sc])

    def _search(self, m):
        """The samples m [rows, n] that follow the open box, all inside one block: boxes, soft, words, hits."""
        rows = m.shape[0]
        m = np.concatenate([self.open, m], axis=1)
        nb = m.shape[1] // self.B
        self.open = m[:, nb * self.B:]
        if nb == 0:
            return
        b = m[:, :nb * self.B].reshape(rows, nb, self.B).sum(axis=2) >> self.lgB
        bb = np.concatenate([self.bh, b], axis=1)
        acc = np.zeros((rows, nb), np.int64)
        for t in range(self.T):
            acc += self.lp[t] * bb[:, t:t + nb]
        assert np.abs(acc).max() < 1 << 31
        soft = np.clip(acc >> self.cfg.lshift, -32768, 32767)
        self.bh = bb[:, bb.shape[1] - (self.T - 1):]
        ss = np.concatenate([self.sh, soft], axis=1)
        t22 = int(self.tap[22])
        self.sh = ss[:, ss.shape[1] - t22:]
        for lo in range(0, nb, 512):                                        # (in pieces: [rows, k, F] stays small)
            hi = min(nb, lo + 512)
            idx = t22 + np.arange(lo, hi)[:, None] - self.tap[None, :]      # [k, 23]
            v = ss[:, idx]                                                  # [rows, k, 23]
            bits = 23 * v > v.sum(axis=2, keepdims=True)
            w = (bits.astype(np.uint32) << np.arange(23, dtype=np.uint32)).sum(axis=2).astype(np.uint32)
            d = popcount(w[:, :, None] ^ self.words[None, None, :])
            f = d.argmin(axis=2)                                            # the first smallest
            ok = np.take_along_axis(d, f[:, :, None], axis=2)[:, :, 0] <= self.cfg.tol
            rr = np.broadcast_to(np.arange(rows)[:, None], f.shape)
            np.add.at(self.cnt, (rr[ok], f[ok]), 1)

    def push(self, x):
        x = np.asarray(x, dtype=np.int16)
        assert x.ndim == 3
        rows, n, _ = x.shape
        self._start(rows)
        c = self.cfg
        lgQ = c.ramp.bit_length() - 1
        assert 1 << lgQ == c.ramp <= self.P
        xi = x.astype(np.int64)
        m = mono(xi)
        out = np.empty_like(xi)
        lo = 0
        while lo < n:
            r0 = self.N % self.P
            hi = min(n, lo + self.P - r0)
            r = np.arange(r0, r0 + hi - lo, dtype=np.int64)
            g = self.sp[:, None] + (((self.sc - self.sp)[:, None] * (np.minimum(r, c.ramp - 1) + 1)[None, :]) >> lgQ)
            out[:, lo:hi] = (xi[:, lo:hi] * g[:, :, None]) >> 8
            self._search(m[:, lo:hi])
            self.N += hi - lo
            lo = hi
            if self.N % self.P == 0:
                assert self.open.shape[1] == 0
                for row in range(rows):
                    hit, fs, cnt = decide([int(v) for v in self.cnt[row]], c)
                    self.state[row], s = step(self.state[row], hit, c)
                    self.sp[row], self.sc[row] = self.sc[row], s
                    self.last[row] = cnt
                    self.hits.append((self.N // self.P - 1, row, hit, fs, cnt))
                self.cnt[:] = 0
        return out.astype(np.int16)


def dcs_all(x, words, cfg):
    """x int16 [rows, N, width] -> the gated int16 [rows, N, width] in one piece."""
    return CodeSquelch(words, cfg).push(x)
