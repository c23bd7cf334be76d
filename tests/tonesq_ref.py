"""Integer definition of the tone squelch (include/fmd.h, "tone squelch"), restated for the tests.

Per row, with P = block, i the sample index since creation or reset, r = i mod P, j = i // P:
    m[i]   = x[i][0]  (width 1)   or   (x[i][0] + x[i][1]) >> 1  (width 2)
    Re_f(j) = sum_r c_f[r] m[jP + r],  Im_f(j) = sum_r s_f[r] m[jP + r]              tab[f][r] = (c_f[r], s_f[r]), |entry| <= 1023
    A_f = Re_f >> 14,  B_f = Im_f >> 14,  W_f = A_f^2 + B_f^2
    f*   = the smallest f with W_f maximal;  rest = max W_f over |f - f*| > guard (0 if none)
    hit_j = f* if W_f* >= min_power and (W_f* >> dom_shift) >= rest, else NONE
    state (t, cand, cnt, h) from (NONE, NONE, 0, 0), once per completed block:
        hit != NONE: cnt = min(cnt + 1, 65535) if hit == cand else (cand, cnt) = (hit, 1);   hit == NONE: cand = NONE, cnt = 0
        then cnt >= confirm: t = cand, h = hang;  else h > 0: h -= 1;  else t = NONE
    s_j = 256 if t != NONE and bit t of accept is set, else 0;  s_{-1} = s_{-2} = 0
    g[i] = s_{j-2} + (((s_{j-1} - s_{j-2}) (min(r, Q - 1) + 1)) >> log2 Q),  Q = ramp;   out[i][c] = (x[i][c] g[i]) >> 8

`tonesq_row` is the definition in plain Python integers, sample by sample.  `ToneSquelch` is the handle's call semantics over many
rows; its block sums are a float64 matrix product, which is exact: every product is an integer below 2^25 and every partial sum an
integer below 2^39, far inside the 2^53 that float64 holds exactly, in whatever order they are added (tests/test_tonesq.py holds it
against `tonesq_row`).  Everything after the sums is Python integers."""
from collections import namedtuple

import numpy as np

Cfg = namedtuple("Cfg", "block guard dom_shift confirm hang ramp min_power accept")
NONE = -1


def mono(x):
    """x int [..., width] -> m int64 [...]"""
    x = np.asarray(x, dtype=np.int64)
    return x[..., 0] if x.shape[-1] == 1 else (x[..., 0] + x[..., 1]) >> 1


def decide(W, cfg):
    """W: the F powers of one block (Python ints) -> (hit, f*, W_f*)."""
    fs = max(range(len(W)), key=lambda f: (W[f], -f))
    rest = max([W[f] for f in range(len(W)) if abs(f - fs) > cfg.guard], default=0)
    hit = fs if W[fs] >= cfg.min_power and (W[fs] >> cfg.dom_shift) >= rest else NONE
    return hit, fs, W[fs]


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


def gains(sp, sc, r, cfg):
    """g at the positions r (int array or int) of a block whose two decisions before it were sp = s_{j-2}, sc = s_{j-1}."""
    Q = cfg.ramp
    lg = Q.bit_length() - 1
    assert 1 << lg == Q
    return sp + (((sc - sp) * (np.minimum(r, Q - 1) + 1)) >> lg)


def tonesq_row(x, tab, cfg):
    """The definition in plain Python integers: x int [N, width] of one row, tab int [F][P][2] ->
    (out: list of N lists of width ints, reports: per completed block (hit, t, W_f*, s_j))."""
    cfg = Cfg(*cfg)
    P, F = cfg.block, len(tab)
    Q = cfg.ramp
    lg = Q.bit_length() - 1
    assert 1 << lg == Q <= P
    xs = [[int(v) for v in s] for s in x]
    tb = [[(int(c), int(s)) for c, s in row] for row in tab]
    state, sp, sc = (NONE, NONE, 0, 0), 0, 0
    re, im = [0] * F, [0] * F
    out, reports = [], []
    for i, smp in enumerate(xs):
        r = i % P
        m = smp[0] if len(smp) == 1 else (smp[0] + smp[1]) >> 1
        g = sp + (((sc - sp) * (min(r, Q - 1) + 1)) >> lg)
        out.append([(v * g) >> 8 for v in smp])
        for f in range(F):
            re[f] += tb[f][r][0] * m
            im[f] += tb[f][r][1] * m
        if r == P - 1:
            W = [(re[f] >> 14) ** 2 + (im[f] >> 14) ** 2 for f in range(F)]
            hit, _, w = decide(W, cfg)
            state, s = step(state, hit, cfg)
            sp, sc = sc, s
            reports.append((hit, state[0], w, s))
            re, im = [0] * F, [0] * F
    return out, reports


class ToneSquelch:
    """The handle's call semantics over many rows: push(x) returns the gated samples of the call; the 2 F partial sums, the state
    and (s_{j-2}, s_{j-1}) per row are carried.  `hits` collects (block, row, hit) of every completed block."""

    def __init__(self, tab, cfg):
        self.cfg = Cfg(*cfg)
        self.tab = np.asarray(tab, dtype=np.int64)           # [F, P, 2]
        self.F, self.P = self.tab.shape[0], self.tab.shape[1]
        assert self.P == self.cfg.block and self.tab.shape[2] == 2 and np.abs(self.tab).max() <= 1023
        # [P, 2 F] as float64 for the exact matrix product
        self.mat = np.ascontiguousarray(self.tab.transpose(1, 0, 2).reshape(self.P, 2 * self.F).astype(np.float64))
        self.reset()

    def reset(self):
        self.N = 0
        self.sums = None                                     # int64 [rows, 2 F]
        self.state = None                                    # per row (t, cand, cnt, h)
        self.sp = self.sc = None                             # int64 [rows]
        self.power = None
        self.hits = []

    def _start(self, rows):
        if self.sums is None:
            self.sums = np.zeros((rows, 2 * self.F), np.int64)
            self.state = [(NONE, NONE, 0, 0)] * rows
            self.sp, self.sc = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
            self.power = [0] * rows

    def status(self):
        """(tone [rows], power [rows], open [rows]) after the last completed block."""
        return ([s[0] for s in self.state], list(self.power), [bool(v) for v in self.sc])

    def push(self, x):
        x = np.asarray(x, dtype=np.int16)
        assert x.ndim == 3
        rows, n, _ = x.shape
        self._start(rows)
        xi = x.astype(np.int64)
        m = mono(xi).astype(np.float64)
        out = np.empty_like(xi)
        lo = 0
        while lo < n:
            r0 = self.N % self.P
            hi = min(n, lo + self.P - r0)
            r = np.arange(r0, r0 + hi - lo, dtype=np.int64)
            g = self.sp[:, None] + gains(0, (self.sc - self.sp)[:, None], r[None, :], self.cfg)
            out[:, lo:hi] = (xi[:, lo:hi] * g[:, :, None]) >> 8
            part = m[:, lo:hi] @ self.mat[r0:r0 + hi - lo]
            assert np.abs(part).max(initial=0) < 2.0 ** 52
            self.sums += part.astype(np.int64)
            self.N += hi - lo
            lo = hi
            if self.N % self.P == 0:
                for row in range(rows):
                    ab = [int(v) >> 14 for v in self.sums[row]]
                    W = [ab[2 * f] ** 2 + ab[2 * f + 1] ** 2 for f in range(self.F)]
                    hit, _, w = decide(W, self.cfg)
                    self.state[row], s = step(self.state[row], hit, self.cfg)
                    self.sp[row], self.sc[row] = self.sc[row], s
                    self.power[row] = w
                    self.hits.append((self.N // self.P - 1, row, hit))
                self.sums[:] = 0
        return out.astype(np.int16)


def tonesq_all(x, tab, cfg):
    """x int16 [rows, N, width] -> the gated int16 [rows, N, width] in one piece."""
    return ToneSquelch(tab, cfg).push(x)
