"""The tone-pair demodulator's definition (include/fmd.h, fmd_afsk_*) restated in numpy and in plain Python integers, for the tests
and the bench tool.  Integers only, exact.  Per row, with x[i] the int16 input counted from creation or reset, tab[4][T] the int16
table (mark-cos, mark-sin, space-cos, space-sin, every |entry| <= 1023) and i_n = n D:

    S_q[n] = sum_{t < T} tab[q][t] x[i_n + t]            (exact in i32: 64 * 32768 * 1023 < 2^31)
    A_q    = S_q >> pre_shift                            (arithmetic)
    E_m    = A_0^2 + A_1^2,  E_s = A_2^2 + A_3^2         (i64)
    out[n] = sat16((E_m - E_s) >> out_shift)             (arithmetic; positive: mark)

Output n exists once x[i_n + T - 1] has arrived: after N inputs, N >= T ? ceil((N - T + 1) / D) : 0 outputs."""
import numpy as np


def outputs(T, D, n):
    """Outputs per row that exist once n samples have arrived."""
    return (n - T + D) // D if n >= T else 0


def out_cap(D, n_in):
    return (n_in + D - 1) // D + 1


def afsk_row(x, tab, D, pre_shift, out_shift):
    """The definition on one whole row in Python integers: the list of every output the samples x complete."""
    T = len(tab[0])
    x = [int(v) for v in x]
    out = []
    for n in range(outputs(T, D, len(x))):
        A = [sum(int(tab[q][t]) * x[n * D + t] for t in range(T)) >> pre_shift for q in range(4)]
        v = (A[0] * A[0] + A[1] * A[1] - A[2] * A[2] - A[3] * A[3]) >> out_shift
        out.append(max(-32768, min(32767, v)))
    return out


def demod(x, tab, D, pre_shift, out_shift, first=0):
    """int16 [rows, cnt]: the outputs first, first + 1, ... that the samples x (int16 [rows, N], the stream from sample 0) complete."""
    tab = np.asarray(tab, np.int64)
    T = tab.shape[1]
    x = np.asarray(x, np.int64)
    cnt = outputs(T, D, x.shape[1]) - first
    if cnt <= 0:
        return np.zeros((x.shape[0], 0), np.int16)
    win = np.lib.stride_tricks.sliding_window_view(x, T, axis=1)[:, first * D::D][:, :cnt]     # [rows, cnt, T]
    A = (win @ tab.T) >> pre_shift                                                             # [rows, cnt, 4], exact in i64
    # |A| < 2^31, so each square is below 2^62 and E_m - E_s fits i64
    v = (A[..., 0] * A[..., 0] + A[..., 1] * A[..., 1] - A[..., 2] * A[..., 2] - A[..., 3] * A[..., 3]) >> out_shift
    return np.clip(v, -32768, 32767).astype(np.int16)


class AfskDemod:
    """The stream form: push(x int16 [rows, n]) returns the outputs the call completes (None where it completes none: the call is
    refused and nothing is taken), whatever the cuts."""

    def __init__(self, tab, D, pre_shift, out_shift, rows=1):
        self.tab, self.D, self.pre_shift, self.out_shift = np.asarray(tab, np.int16), int(D), int(pre_shift), int(out_shift)
        self.T = self.tab.shape[1]
        self.rows = rows
        self.reset()

    def reset(self):
        self.pos = 0
        self.tail = np.zeros((self.rows, 0), np.int16)      # the samples from x[first output still to come * D] on
        self.tail0 = 0                                      # the stream index of tail[:, 0]

    def push(self, x):
        x = np.asarray(x, np.int16)
        o0, o1 = outputs(self.T, self.D, self.pos), outputs(self.T, self.D, self.pos + x.shape[1])
        if o1 == o0:
            return None
        buf = np.concatenate([self.tail, x], axis=1)        # buf[:, 0] is x[o0 D]: tail0 == o0 D
        y = demod(buf, self.tab, self.D, self.pre_shift, self.out_shift)[:, :o1 - o0]
        self.pos += x.shape[1]
        keep = o1 * self.D                                  # the next output's first sample; <= pos because D <= T
        self.tail, self.tail0 = buf[:, keep - self.tail0:], keep
        assert self.tail.shape[1] <= self.T - 1
        return y
