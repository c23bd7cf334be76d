"""Integer definition of the FSK front end of the pager decoder (include/fmd.h, "pager decoder", fmd_fsk_*), restated for the tests.

Per row, i the sample index since creation or reset, everything at a negative index 0:
    b[k]    = sum_{r<D} x[k D + r]
    soft[k] = (sum_{t<W} b[k - t]) >> shift = out[k]                 (D W <= 2^shift: an int16 by construction)
    thr[k]  = sum_{j<32} soft[k - tap[j]];   bit j of w[k] = 32 soft[k - tap[j]] > thr[k]
    d[k]    = popcount(w[k] ^ sync);   C[k] = sum_j (bit j of sync ? +1 : -1) soft[k - tap[j]]
    normal hit: d <= tol and C >= min_corr;   inverted hit: d >= 32 - tol and -C >= min_corr
    record (k_rel, d | inverted << 31, C, thr), k_rel the index of out[k] in the call that brings x[k D + D - 1]

`fsk_row` is the definition in plain Python integers, sample by sample.  `FskDemod` is the handle's call semantics over many rows,
vectorised in int64 (every sum stays below 2^31); tests/test_fsk.py holds it against `fsk_row`."""
from collections import namedtuple

import numpy as np

Cfg = namedtuple("Cfg", "D W shift tap sync tol min_corr hit_cap")
HIT_DTYPE = np.dtype([("k_rel", np.uint32), ("d", np.uint32), ("corr", np.int32), ("thr", np.int32)])
_POP16 = np.array([bin(v).count("1") for v in range(1 << 16)], np.uint8)


def popcount(v):
    """of a uint32 array"""
    v = np.asarray(v, dtype=np.uint32)
    return _POP16[v & 0xFFFF].astype(np.int64) + _POP16[v >> 16]


def fsk_row(x, cfg):
    """One row, whole: (soft list, hits list of (k, d | inverted << 31, C, thr)) in plain integers."""
    x = [int(v) for v in x]
    nk = len(x) // cfg.D
    b = [sum(x[k * cfg.D:(k + 1) * cfg.D]) for k in range(nk)]
    soft = [sum(b[k - t] for t in range(cfg.W) if k - t >= 0) >> cfg.shift for k in range(nk)]
    hits = []
    for k in range(nk):
        v = [soft[k - int(t)] if k - int(t) >= 0 else 0 for t in cfg.tap]
        thr = sum(v)
        w = sum((1 if 32 * v[j] > thr else 0) << j for j in range(32))
        d = bin(w ^ cfg.sync).count("1")
        c = sum(v[j] if (cfg.sync >> j) & 1 else -v[j] for j in range(32))
        if d <= cfg.tol and c >= cfg.min_corr:
            hits.append((k, d, c, thr))
        elif d >= 32 - cfg.tol and -c >= cfg.min_corr:
            hits.append((k, d | 1 << 31, c, thr))
    return soft, hits


class FskDemod:
    """The handle: run(x [rows, n_in]) -> (out int16 [rows, n_out], counts uint32 [rows], records [rows, hit_cap] zero-filled)."""

    def __init__(self, cfg, rows):
        self.cfg, self.rows = cfg, rows
        self.tap = np.asarray(cfg.tap, np.int64)
        self.reset()

    def reset(self):
        self.pos = 0
        self.part = np.zeros((self.rows, 0), np.int64)       # the open box's samples
        self.b = np.zeros((self.rows, self.cfg.W - 1), np.int64)
        self.soft = np.zeros((self.rows, int(self.tap[31])), np.int64)

    def outputs(self):
        return self.pos // self.cfg.D

    def run(self, x):
        c = self.cfg
        x = np.asarray(x, np.int64)
        assert x.ndim == 2 and x.shape[0] == self.rows
        n_in = x.shape[1]
        n_out = (self.pos % c.D + n_in) // c.D
        self.pos += n_in
        buf = np.concatenate([self.part, x], axis=1)
        self.part = buf[:, n_out * c.D:]
        counts, rec = np.zeros(self.rows, np.uint32), np.zeros((self.rows, c.hit_cap), HIT_DTYPE)
        if n_out == 0:
            return np.zeros((self.rows, 0), np.int16), counts, rec
        b = np.concatenate([self.b, buf[:, :n_out * c.D].reshape(self.rows, n_out, c.D).sum(axis=2)], axis=1)
        cs = np.concatenate([np.zeros((self.rows, 1), np.int64), np.cumsum(b, axis=1)], axis=1)
        new = (cs[:, c.W:] - cs[:, :-c.W]) >> c.shift
        assert new.shape[1] == n_out and new.min() >= -32768 and new.max() <= 32767
        self.b = b[:, b.shape[1] - (c.W - 1):]
        soft = np.concatenate([self.soft, new], axis=1)
        h = self.soft.shape[1]
        k = h + np.arange(n_out)
        v = soft[:, k[None, :] - self.tap[:, None]]          # [rows, 32, n_out]
        thr = v.sum(axis=1)
        bits = (32 * v > thr[:, None, :]).astype(np.uint32)
        w = (bits << np.arange(32, dtype=np.uint32)[None, :, None]).sum(axis=1).astype(np.uint32)
        d = popcount(w ^ np.uint32(c.sync))
        sign = np.array([1 if (c.sync >> j) & 1 else -1 for j in range(32)], np.int64)
        corr = (v * sign[None, :, None]).sum(axis=1)
        normal = (d <= c.tol) & (corr >= c.min_corr)
        inverted = (d >= 32 - c.tol) & (-corr >= c.min_corr)
        for r in range(self.rows):
            ks = np.nonzero(normal[r] | inverted[r])[0]
            counts[r] = len(ks)
            for s, q in enumerate(ks[:c.hit_cap]):
                rec[r, s] = (q, int(d[r, q]) | (int(inverted[r, q]) << 31), corr[r, q], thr[r, q])
        self.soft = soft[:, soft.shape[1] - h:]
        return new.astype(np.int16), counts, rec


def random_cfg(rng, D, W, last, tol=3, min_corr=0, hit_cap=64):
    """A configuration with random non-decreasing taps up to `last`, repeated taps included, at the smallest shift, and a word that
    such taps can see: bits that read the same soft sample are equal."""
    shift = 0
    while (1 << shift) < D * W:
        shift += 1
    tap = np.sort(rng.integers(0, last // W + 1, 32)) * W    # (W apart, so that the box filter does not smear two bits into one)
    tap[0], tap[31] = 0, last
    bits = rng.integers(0, 2, 32)
    for j in range(1, 32):
        if tap[j] == tap[j - 1]:
            bits[j] = bits[j - 1]
    bits[1 + int(np.argmax(tap[1:] != tap[:-1]))] ^= bits.min() == bits.max()         # not all equal
    sync = int(sum(int(b) << j for j, b in enumerate(bits)))
    return Cfg(D, W, shift, tap.astype(np.uint32), sync, tol, min_corr, hit_cap)


def laid_signal(rng, cfg, rows, n, amp=2000):
    """int16 [rows, n]: noise with cfg.sync laid into it at the taps' spacing every tap[31] + 40 soft samples, at another phase and
    on another DC in every row, every third word inverted: something to hit, whatever D, W and the taps are."""
    nk = n // cfg.D + 2
    soft = rng.integers(-amp // 4, amp // 4, (rows, nk))
    for r in range(rows):
        for at in range(int(cfg.tap[31]) + cfg.W + 3 + 17 * r, nk - 2, int(cfg.tap[31]) + 40):
            sign = -1 if (at + r) % 3 == 0 else 1
            for j in range(31, -1, -1):                      # W box sums at the bit's level end at its tap
                hi = at - int(cfg.tap[j]) + 1
                soft[r, hi - cfg.W:hi] = sign * (amp if (cfg.sync >> j) & 1 else -amp) + 300 * r
    x = np.repeat(soft, cfg.D, axis=1)[:, :n] * (1 << cfg.shift) // (cfg.D * cfg.W)
    return np.clip(x, -32768, 32767).astype(np.int16)
