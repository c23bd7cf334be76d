"""Integer definition of the rational resampler (include/fmd.h, "rational resampler"), restated in numpy for the tests.

Per row and component c < width:
    q_n = n M,  i_n = q_n // L,  p_n = q_n % L
    v[n][c]   = sum_{t < T} g[p_n][t] x[i_n + t][c]
    out[n][c] = sat16(v[n][c] >> shift)
Output n comes with the call in which x[i_n + T - 1] arrives.  A call that completes no output is refused and changes nothing."""
import numpy as np


def outputs(N, L, M, T):
    """Outputs that exist after N inputs: N >= T ? ceil((N - T + 1) L / M) : 0."""
    return -((-(N - T + 1) * L) // M) if N >= T else 0


def resample_all(x, g, L, M, shift):
    """x int16 [..., N, width] -> int16 [..., outputs(N), width]: every output of the N samples, in one piece."""
    x = np.asarray(x, dtype=np.int64)
    g = np.asarray(g, dtype=np.int64).reshape(L, -1)
    T = g.shape[1]
    n = np.arange(outputs(x.shape[-2], L, M, T), dtype=np.int64)
    i, p = (n * M) // L, (n * M) % L
    idx = i[:, None] + np.arange(T)[None, :]                 # [n_out, T]
    win = x[..., idx, :]                                     # [..., n_out, T, width]
    v = (win * g[p][:, :, None]).sum(axis=-2)
    assert np.abs(v).max(initial=0) < 2 ** 31
    return np.clip(v >> shift, -32768, 32767).astype(np.int16)


class TooShort(Exception):
    pass


class Resampler:
    """The handle's call semantics: push(x) returns the outputs the call completes; history as the definition carries it."""

    def __init__(self, g, L, M, shift):
        self.g = np.asarray(g, dtype=np.int64).reshape(L, -1)
        self.L, self.M, self.T, self.shift = int(L), int(M), self.g.shape[1], int(shift)
        self.reset()

    def reset(self):
        self.N = 0                                           # inputs taken
        self.hist = None                                     # [..., h, width]: the samples x[N - h ... N)

    def history(self):
        """max(0, N - i_next) with i_next = floor(outputs(N) M / L): what the next call's first output still reads."""
        i_next = outputs(self.N, self.L, self.M, self.T) * self.M // self.L
        return max(0, self.N - i_next)

    def push(self, x):
        x = np.asarray(x, dtype=np.int16)
        n_in = x.shape[-2]
        o0, o1 = outputs(self.N, self.L, self.M, self.T), outputs(self.N + n_in, self.L, self.M, self.T)
        if o1 == o0:
            raise TooShort()
        h = self.history()
        assert h <= self.T - 1
        virt = x if self.hist is None else np.concatenate([self.hist, x], axis=-2)   # virtual sample 0 is x[base]
        base = self.N - (0 if self.hist is None else self.hist.shape[-2])
        n = np.arange(o0, o1, dtype=np.int64)
        i, p = (n * self.M) // self.L - base, (n * self.M) % self.L
        assert i.min() >= 0
        idx = i[:, None] + np.arange(self.T)[None, :]
        v = (virt.astype(np.int64)[..., idx, :] * self.g[p][:, :, None]).sum(axis=-2)
        self.N += n_in
        hn = self.history()
        assert hn <= self.T - 1 and hn <= virt.shape[-2]
        self.hist = virt[..., virt.shape[-2] - hn:, :].copy()
        return np.clip(v >> self.shift, -32768, 32767).astype(np.int16)
