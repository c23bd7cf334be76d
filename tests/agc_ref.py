"""Integer definition of the automatic gain control (include/fmd.h, "automatic gain control"), restated in numpy for the tests.

Per row, with P = block:
    m[i] = max_c |x[i][c]|;  p_j = max of m over block j;  e_j = max(p_j, p_{j+1})
    d_j  = min(gain_max, (1024 target) // e_j)                                      for e_j > 0
    (G, h) from (gain_max, 0), per block j: e_j == 0 holds; d_j <= G: G = d_j, h = hang; h > 0: h -= 1;
                                           otherwise G = min(d_j, G + max(1, ((d_j - G) decay) >> 8))
    G_j = G after block j, G_{-1} := G_0
    g[i] = G_{j-1} + (((G_j - G_{j-1}) (r + 1)) >> log2 P),  out[i][c] = (x[i][c] g[i]) >> 10
Block j exists once block j + 1 is complete: after N samples, P max(0, N // P - 1) outputs."""
from collections import namedtuple

import numpy as np

Cfg = namedtuple("Cfg", "block target gain_max hang decay")


def outputs(N, P):
    """Outputs that exist after N inputs."""
    return P * max(0, N // P - 1)


def step(G, h, e, cfg):
    """One block of the recursion on Python ints: (G, h) after a block whose e_j is e."""
    if e == 0:
        return G, h
    d = min(cfg.gain_max, (cfg.target * 1024) // e)
    if d <= G:
        return d, cfg.hang
    if h > 0:
        return G, h - 1
    return min(d, G + max(1, ((d - G) * cfg.decay) >> 8)), h


def agc_row(x, cfg):
    """x int [N, width] of one row -> (out int16 [outputs(N), width], [(G_j, h_j) for every emitted block j])."""
    cfg = Cfg(*cfg)
    P = cfg.block
    lg = P.bit_length() - 1
    assert 1 << lg == P
    x = np.asarray(x, dtype=np.int64)
    nb = max(0, x.shape[0] // P - 1)
    p = [int(np.abs(x[j * P:(j + 1) * P]).max()) for j in range(nb + 1)] if nb else []
    G, h, states = cfg.gain_max, 0, []
    for j in range(nb):
        G, h = step(G, h, max(p[j], p[j + 1]), cfg)
        states.append((G, h))
    out = np.zeros((nb * P, x.shape[1]), dtype=np.int64)
    r1 = np.arange(1, P + 1, dtype=np.int64)
    for j in range(nb):
        Gp = states[j - 1][0] if j else states[0][0]
        g = Gp + (((states[j][0] - Gp) * r1) >> lg)
        prod = x[j * P:(j + 1) * P] * g[:, None]
        assert np.abs(prod).max(initial=0) <= 1024 * cfg.target
        out[j * P:(j + 1) * P] = prod >> 10
    assert np.abs(out).max(initial=0) <= cfg.target
    return out.astype(np.int16), states


def agc_all(x, cfg):
    """x int16 [rows, N, width] -> int16 [rows, outputs(N), width]: everything that exists after N samples, in one piece."""
    x = np.asarray(x)
    assert x.ndim == 3
    return np.stack([agc_row(row, cfg)[0] for row in x])


def from_peaks(rng, amps, P, width, tail=0):
    """Test input int16 [len(amps) P + tail, width]: block j is random within +-amps[j] and reaches it (32768 as -32768); the `tail`
    samples of a last, partial block are within +-40."""
    x = np.zeros((len(amps) * P + tail, width), np.int64)
    for j, a in enumerate(amps):
        if a:
            seg = x[j * P:(j + 1) * P]
            seg[:] = rng.integers(-min(a, 32767), min(a, 32767) + 1, seg.shape)
            seg[int(rng.integers(0, P)), int(rng.integers(0, width))] = -a if a == 32768 or rng.random() < 0.5 else a
    if tail:
        x[len(amps) * P:] = rng.integers(-40, 41, (tail, width))
    return x.astype(np.int16)


def envelope(rng, rows, blocks, P, width, levels=(0, 3, 40, 900, 32767, 32768)):
    """Test input int16 [rows, blocks P + a part of a block, width]: every block draws its peak from `levels`, a zero starts a run of
    1 ... 3 silent blocks."""
    tail = int(rng.integers(0, P))
    out = []
    for _ in range(rows):
        amps = []
        while len(amps) < blocks:
            a = int(rng.choice(levels))
            amps += [a] * (int(rng.integers(1, 4)) if a == 0 else 1)
        out.append(from_peaks(rng, amps[:blocks], P, width, tail))
    return np.stack(out)


class Agc:
    """The handle's call semantics, vectorised over the rows: push(x) returns the blocks the call completes (an empty array when it
    completes none) and carries the samples not yet emitted and (G, h) per row."""

    def __init__(self, cfg):
        self.cfg = Cfg(*cfg)
        self.P = self.cfg.block
        self.lg = self.P.bit_length() - 1
        assert 1 << self.lg == self.P
        self.reset()

    def reset(self):
        self.N = 0                                           # inputs taken
        self.hist = None                                     # [rows, N - outputs, width]
        self.G = self.h = None                               # int64 [rows]: after the last emitted block
        self.peak = 0                                        # the largest |out| so far

    def history(self):
        return self.N - outputs(self.N, self.P)

    def gain(self, row=0):
        """(G, h) after the last emitted block; gain_max, 0 before any."""
        return (self.cfg.gain_max, 0) if self.G is None else (int(self.G[row]), int(self.h[row]))

    def push(self, x):
        x = np.asarray(x, dtype=np.int16)
        assert x.ndim == 3
        c, P = self.cfg, self.P
        virt = x if self.hist is None else np.concatenate([self.hist, x], axis=1)
        B0, self.N = outputs(self.N, P) // P, self.N + x.shape[1]
        nb = outputs(self.N, P) // P - B0
        assert virt.shape[1] == self.N - B0 * P
        if self.G is None:
            self.G, self.h = np.full(x.shape[0], c.gain_max, np.int64), np.zeros(x.shape[0], np.int64)
        v = virt.astype(np.int64)
        p = np.abs(v[:, :(nb + 1) * P]).reshape(x.shape[0], nb + 1, P * x.shape[2]).max(axis=2) if nb else None
        Gs = np.empty((x.shape[0], nb + 1), np.int64)        # G_{j-1}, then G_j of the call's blocks
        Gs[:, 0] = self.G
        for k in range(nb):
            G, h = self.G, self.h
            e = np.maximum(p[:, k], p[:, k + 1])
            d = np.minimum(c.gain_max, (c.target * 1024) // np.maximum(e, 1))
            live = e > 0
            attack = live & (d <= G)
            hang = live & ~attack & (h > 0)
            release = live & ~attack & ~hang
            up = np.minimum(d, G + np.maximum(1, ((d - G) * c.decay) >> 8))
            self.G = np.where(attack, d, np.where(release, up, G))
            self.h = np.where(attack, c.hang, np.where(hang, h - 1, h))
            Gs[:, k + 1] = self.G
        if nb and B0 == 0:
            Gs[:, 0] = Gs[:, 1]                              # G_{-1} := G_0
        r1 = np.arange(1, P + 1, dtype=np.int64)
        g = Gs[:, :-1, None] + (((Gs[:, 1:] - Gs[:, :-1])[:, :, None] * r1) >> self.lg)       # [rows, nb, P]
        prod = v[:, :nb * P] * g.reshape(x.shape[0], nb * P)[:, :, None]
        assert np.abs(prod).max(initial=0) < 2 ** 31
        self.peak = max(self.peak, int(np.abs(prod >> 10).max(initial=0)))     # before the cast to int16
        self.hist = virt[:, nb * P:].copy()
        assert self.hist.shape[1] == self.history() <= 2 * P - 1
        return (prod >> 10).astype(np.int16)
