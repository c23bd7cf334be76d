"""Test-side definition of the narrow-band bank (include/fmd.h, "narrow-band bank"), in numpy int64 and Python integers: the
channelizer's y (tests/channelizer_ref.py), the complex decimating FIR, the shift, the exact integer magnitude, the block sums,
the four detectors, the gain and the squelch.  Independent of the library.  `direct` is the same definition one sample at a time
in Python integers.  Also synthesizers of AM, NFM and SSB channels as u8 IQ bytes."""
import math

import numpy as np

import channelizer_ref as cr
import stereo_ref as st
from stations_ref import TooShort  # noqa: F401  (re-exported: a call that completes no audio sample)

IQ, FM, AM, SSB = 0, 1, 2, 3


def isqrt_vec(x):
    """floor(sqrt(x)) of an int64 array, exact."""
    x = np.asarray(x, dtype=np.int64)
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > x, r - 1, r)
    return np.where((r + 1) * (r + 1) <= x, r + 1, r)


def width(mode):
    return 2 if mode == IQ else 1


class NarrowRef:
    """One input stream, K stations; feed() mirrors one fmd_narrow call of that stream and returns int64 [K, n] ([K, n, 2] in IQ
    mode).  Keeps every y and u since reset (test sizes only)."""

    def __init__(self, taps, decim, incs, shift, gr, gi, mode, chan_decim, chan_shift, block, squelch, gain, z=None):
        self.ch = cr.ChannelizerRef(taps, decim, incs, shift, z=z)
        self.K = len(self.ch.incs)
        self.gr = np.asarray(gr, dtype=np.int64)
        self.gi = np.zeros_like(self.gr) if gi is None else np.asarray(gi, dtype=np.int64)
        self.Ta, self.R, self.P = self.gr.size, int(chan_decim), int(block)
        self.mode, self.chan_shift, self.squelch, self.gain = int(mode), int(chan_shift), int(squelch), int(gain)
        self.lg = self.P.bit_length() - 1
        assert 1 << self.lg == self.P
        self.reset()

    def reset(self):
        self.ch.reset()
        self.y = [np.zeros((0, 2), np.int64) for _ in range(self.K)]
        self.u = [np.zeros((0, 2), np.int64) for _ in range(self.K)]
        self.a = [np.zeros(0, np.int64) for _ in range(self.K)]
        self.n_next = 0
        self.v_max = 0
        self.a_max = 0

    def audio_after(self, m):
        return (m - self.Ta) // self.R + 1 if m >= self.Ta else 0

    def completes(self, nbytes):
        """Audio samples a call of nbytes completes (0: refused)."""
        return self.audio_after(self.ch.outputs_after(nbytes // 2)) - self.n_next

    def block(self, k, j):
        """(E_j, A_j) of a complete block."""
        u, a = self.u[k][j * self.P:(j + 1) * self.P], self.a[k][j * self.P:(j + 1) * self.P]
        return int((u * u).sum()), int(a.sum())

    def estimate(self, k, j):
        """(open_j, dc_j); block -1: (squelch == 0, 0)."""
        if j < 0:
            return self.squelch == 0, 0
        E, A = self.block(k, j)
        return self.squelch == 0 or E >= self.squelch * self.squelch * self.P, A >> self.lg

    def feed(self, buf):
        b = np.asarray(buf, dtype=np.uint8)
        if self.completes(b.size) < 1:
            raise TooShort()
        y = self.ch.feed(b)                                   # [K, M, 2]
        out = []
        n0 = self.n_next
        for k in range(self.K):
            self.y[k] = np.concatenate([self.y[k], y[k]])
            n1 = self.audio_after(self.y[k].shape[0])
            lo, hi = self.R * n0, self.R * (n1 - 1) + self.Ta
            yr, yi = self.y[k][lo:hi, 0], self.y[k][lo:hi, 1]
            vr = (np.correlate(yr, self.gr, "valid") - np.correlate(yi, self.gi, "valid"))[::self.R]
            vi = (np.correlate(yi, self.gr, "valid") + np.correlate(yr, self.gi, "valid"))[::self.R]
            self.v_max = max(self.v_max, int(np.abs(vr).max()), int(np.abs(vi).max()))
            u = np.stack([vr >> self.chan_shift, vi >> self.chan_shift], axis=1)
            a = isqrt_vec((u * u).sum(axis=1))
            self.a_max = max(self.a_max, int(a.max()))
            uprev = self.u[k][-1] if n0 else np.zeros(2, np.int64)
            self.u[k] = np.concatenate([self.u[k], u])
            self.a[k] = np.concatenate([self.a[k], a])
            n = np.arange(n0, n1, dtype=np.int64)
            jprev = n // self.P - 1
            opn, dc = np.zeros(n.size, bool), np.zeros(n.size, np.int64)
            for jp in np.unique(jprev):
                opn[jprev == jp], dc[jprev == jp] = self.estimate(k, int(jp))
            if self.mode == IQ:
                out.append(np.where(opn[:, None], u, 0))
                continue
            if self.mode == FM:
                uu = np.concatenate([uprev[None, :], u])
                w = st.wrap16(st.disc_fast(uu[1:, 0], uu[1:, 1], uu[:-1, 0], uu[:-1, 1]))
            elif self.mode == AM:
                w = a - dc
            else:
                w = u[:, 0]
            out.append(np.where(opn, st.sat16((w * self.gain) >> 8), 0))
        self.n_next = self.audio_after(self.y[0].shape[0])
        return np.stack(out)

    def level(self, k):
        """(open, rms) of the last completed block; (False, 0) before one."""
        jn = self.n_next // self.P
        if jn == 0:
            return False, 0
        E, _ = self.block(k, jn - 1)
        return self.squelch == 0 or E >= self.squelch * self.squelch * self.P, math.isqrt(E >> self.lg)


def direct(y, gr, gi, mode, R, chan_shift, P, squelch, gain):
    """The definition one sample at a time in Python integers, over one station's whole y [M, 2]: a list of ints (pairs in IQ
    mode)."""
    import pyref
    gi = [0] * len(gr) if gi is None else gi
    Ta, lg = len(gr), P.bit_length() - 1
    M = len(y)
    N = (M - Ta) // R + 1 if M >= Ta else 0
    out, E, A = [], 0, 0
    opn, dc = squelch == 0, 0
    prev = (0, 0)
    for n in range(N):
        if n % P == 0 and n > 0:
            opn, dc = squelch == 0 or E >= squelch * squelch * P, A >> lg
            E, A = 0, 0
        vr = sum(int(gr[t]) * int(y[R * n + t][0]) - int(gi[t]) * int(y[R * n + t][1]) for t in range(Ta))
        vi = sum(int(gr[t]) * int(y[R * n + t][1]) + int(gi[t]) * int(y[R * n + t][0]) for t in range(Ta))
        ur, ui = vr >> chan_shift, vi >> chan_shift
        a = math.isqrt(ur * ur + ui * ui)
        E += ur * ur + ui * ui
        A += a
        if mode == IQ:
            out.append((ur, ui) if opn else (0, 0))
        else:
            w = pyref.wrap16(pyref.polar_discriminant_fast((ur, ui), prev)) if mode == FM else (a - dc if mode == AM else ur)
            out.append(max(-32768, min(32767, (w * gain) >> 8)) if opn else 0)
        prev = (ur, ui)
    return out


# ---- synthesizers ---------------------------------------------------------------------------------------------------------------

def to_u8(z, noise=0.0, seed=0):
    z = np.asarray(z, np.complex128)
    if noise:
        rng = np.random.default_rng(seed)
        z = z + rng.normal(0, noise, z.size) + 1j * rng.normal(0, noise, z.size)
    iq = np.empty(2 * z.size, np.uint8)
    iq[0::2] = np.clip(np.round(z.real + 127.5), 0, 255)
    iq[1::2] = np.clip(np.round(z.imag + 127.5), 0, 255)
    return iq


def carrier(n, fs, off, amp=1.0):
    return amp * np.exp(2j * np.pi * off * np.arange(n) / fs)


def am(n, fs, off, amp, tone_hz, depth=0.5):
    t = np.arange(n) / fs
    return amp * (1 + depth * np.sin(2 * np.pi * tone_hz * t)) * np.exp(2j * np.pi * off * t)


def nfm(n, fs, off, amp, tone_hz, dev_hz=2500.0):
    t = np.arange(n) / fs
    ph = -dev_hz / tone_hz * np.cos(2 * np.pi * tone_hz * t)          # integral of dev sin
    return amp * np.exp(1j * (2 * np.pi * off * t + ph))


def ssb_tone(n, fs, off, amp, tone_hz):
    """A single tone `tone_hz` above (negative: below) a suppressed carrier at `off`."""
    return carrier(n, fs, off + tone_hz, amp)
