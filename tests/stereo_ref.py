"""Test-side definition of the stereo station bank (include/fmd.h, "stereo station bank"), in numpy int64 and Python integers:
the channelizer's y (tests/channelizer_ref.py), the reference's integer discriminator at the MPX rate, the block-wise pilot
estimate, the subcarrier, and the FIR of the sum and the difference signal.  Independent of the library.  Also a synthesizer of
standard stereo FM stations as u8 IQ bytes, for the separation tests."""
import numpy as np

import channelizer_ref as cr
import stations_ref as sr
from stations_ref import TooShort  # noqa: F401  (re-exported: a call that completes no audio sample)


def wrap32(v):
    v = np.asarray(v, dtype=np.int64) & 0xFFFFFFFF
    return np.where(v & 0x80000000, v - (1 << 32), v)


def wrap16(v):
    v = np.asarray(v, dtype=np.int64) & 0xFFFF
    return np.where(v & 0x8000, v - (1 << 16), v)


def _tdiv(a, b):
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) == (b < 0), q, -q)


def disc_fast(ar, ai, br, bi):
    """pyref.polar_discriminant_fast((ar, ai), (br, bi)) over arrays (simple_fm.rs:377-405, i32 wrapping), int64."""
    ar, ai, br, bi = (np.asarray(v, dtype=np.int64) for v in (ar, ai, br, bi))
    x = wrap32(ar * br + ai * bi)
    y = wrap32(ai * br - ar * bi)
    yabs = np.where(y < 0, wrap32(-y), y)
    pos = x >= 0
    num = np.where(pos, wrap32(4096 * wrap32(x - yabs)), wrap32(4096 * wrap32(x + yabs)))
    den = np.where(pos, wrap32(x + yabs), wrap32(yabs - x))
    zero = (x == 0) & (y == 0)
    q = _tdiv(num, np.where(zero, 1, den))
    angle = np.where(pos, wrap32(4096 - q), wrap32(3 * 4096 - q))
    res = np.where(y < 0, wrap32(-angle), angle)
    return np.where(zero, 0, res)


def pilot_inc(capture_rate, decim):
    return ((19000 * decim * (1 << 32) + capture_rate // 2) // capture_rate) % (1 << 32)


def tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def estimate(I, Q, pilot_min, P):
    """(present, c2, s2) of a block with correlations I, Q (Python ints)."""
    present = pilot_min > 0 and I * I + Q * Q >= (pilot_min * P * 8192) ** 2
    if not present:
        return False, 0, 0
    return (True,) + angle_terms(I, Q)


def angle_terms(I, Q):
    """(c2, s2): cos 2 alpha and sin 2 alpha in Q14 of correlations I, Q (not both 0)."""
    e = max(0, max(abs(I), abs(Q)).bit_length() - 23)
    a, b = I >> e, Q >> e
    E = a * a + b * b
    return tdiv((b * b - a * a) << 14, E), tdiv((2 * a * b) << 14, E)


def isqrt(v):
    import math
    return math.isqrt(v)


def sat16(v):
    return np.clip(v, -32768, 32767)


def default_pilot_min(capture_rate, decim):
    """A quarter of a 6.75 kHz pilot in discriminator units at the MPX rate: 32768 * 6750 / f_m / 4."""
    return (32768 * 6750 * decim) // (4 * capture_rate)


class StereoRef:
    """One input stream, K stations; feed() mirrors one fmd_stereo call of that stream and returns int64 [K, n, 2] (L, R).  Keeps
    every x and s since reset (test sizes only)."""

    def __init__(self, taps, decim, incs, shift, capture_rate, audio_taps, audio_decim, block, pilot_min, audio_shift, z=None):
        self.ch = cr.ChannelizerRef(taps, decim, incs, shift, z=z)
        self.K = len(self.ch.incs)
        self.g = np.asarray(audio_taps, dtype=np.int64)
        self.Ta, self.R, self.P = self.g.size, int(audio_decim), int(block)
        self.pilot_min, self.audio_shift = int(pilot_min), int(audio_shift)
        self.inc_p = pilot_inc(int(capture_rate), int(decim))
        self.reset()

    def reset(self):
        self.ch.reset()
        self.yprev = np.zeros((self.K, 2), dtype=np.int64)
        self.x = [np.zeros(0, np.int64) for _ in range(self.K)]
        self.s = [np.zeros(0, np.int64) for _ in range(self.K)]
        self.kc_max = 0                                      # max |kc|, |s|, |M| + |S| and correlation since reset
        self.s_max = 0
        self.ms_max = 0
        self.corr_max = 0
        self.n_next = 0

    def audio_after(self, m):
        return (m - self.Ta) // self.R + 1 if m >= self.Ta else 0

    def completes(self, nbytes):
        """Audio samples a call of nbytes completes (0: refused)."""
        return self.audio_after(self.ch.outputs_after(nbytes // 2)) - self.n_next

    def theta(self, m):
        return (np.asarray(m, dtype=np.uint64) * np.uint64(self.inc_p)) & 0xFFFFFFFF

    def block_iq(self, k, j):
        m = np.arange(j * self.P, (j + 1) * self.P, dtype=np.int64)
        x = self.x[k][j * self.P:(j + 1) * self.P]
        th = self.theta(m)
        return int((x * sr.cosq(th)).sum()), int((x * sr.sinq(th)).sum())

    def feed(self, buf):
        b = np.asarray(buf, dtype=np.uint8)
        if self.completes(b.size) < 1:
            raise TooShort()
        y = self.ch.feed(b)                                   # [K, M, 2]
        M = y.shape[1]
        out = []
        for k in range(self.K):
            yy = np.concatenate([self.yprev[k][None, :], y[k]], axis=0)
            x = wrap16(disc_fast(yy[1:, 0], yy[1:, 1], yy[:-1, 0], yy[:-1, 1]))
            self.yprev[k] = y[k, -1]
            m0 = self.x[k].size
            self.x[k] = np.concatenate([self.x[k], x])
            m = np.arange(m0, m0 + M, dtype=np.int64)
            jprev = m // self.P - 1
            kc = np.zeros(M, np.int64)
            for jp in np.unique(jprev):
                if jp < 0:
                    continue
                I, Q = self.block_iq(k, int(jp))
                present, c2, s2 = estimate(I, Q, self.pilot_min, self.P)
                if present:
                    self.corr_max = max(self.corr_max, abs(I), abs(Q))
                    sel = jprev == jp
                    th2 = (self.theta(m[sel]) * np.uint64(2)) & 0xFFFFFFFF
                    kc[sel] = (sr.sinq(th2) * c2 + sr.cosq(th2) * s2) >> 13
            self.kc_max = max(self.kc_max, int(np.abs(kc).max()))
            self.s[k] = np.concatenate([self.s[k], (x * kc) >> 14])
            self.s_max = max(self.s_max, int(np.abs((x * kc) >> 14).max()))
            n1 = self.audio_after(self.x[k].size)
            lo, hi = self.R * self.n_next, self.R * (n1 - 1) + self.Ta
            Mf = np.correlate(self.x[k][lo:hi], self.g, "valid")[::self.R]
            Sf = np.correlate(self.s[k][lo:hi], self.g, "valid")[::self.R]
            sh = self.audio_shift + 1
            out.append(np.stack([sat16((Mf + Sf) >> sh), sat16((Mf - Sf) >> sh)], axis=1))
            self.last_MS = (Mf, Sf)
            self.ms_max = max(self.ms_max, int((np.abs(Mf) + np.abs(Sf)).max()))
        self.n_next = self.audio_after(self.x[0].size)
        return np.stack(out)

    def pilot(self, k):
        """(present, level) of the last completed block."""
        jn = self.x[k].size // self.P
        if jn == 0:
            return False, 0
        I, Q = self.block_iq(k, jn - 1)
        present = self.pilot_min > 0 and I * I + Q * Q >= (self.pilot_min * self.P * 8192) ** 2
        return present, isqrt(I * I + Q * Q) // (self.P * 8192)


# ---- synthesizer ---------------------------------------------------------------------------------------------------------------

def mpx(t, left, right, phi0, pilot=True):
    """Standard stereo multiplex: 0.45 (L + R) + 0.45 (L - R) sin(2 w t + 2 phi0) + 0.1 sin(w t + phi0), w = 2 pi 19 kHz."""
    w = 2 * np.pi * 19000.0
    m = 0.45 * (left + right) + 0.45 * (left - right) * np.sin(2 * w * t + 2 * phi0)
    if pilot:
        m = m + 0.1 * np.sin(w * t + phi0)
    return m


def synth_iq(n, fs, stations, amp=40.0, noise=1.0, seed=0):
    """u8 IQ bytes (2 n of them) at fs: every station (offset_hz, left(t), right(t), phi0, pilot) FM-modulated at 75 kHz deviation
    at its offset from the centre, summed, plus white noise."""
    t = np.arange(n) / fs
    z = np.zeros(n, np.complex128)
    for off, lf, rf, phi0, pilot in stations:
        m = mpx(t, lf(t), rf(t), phi0, pilot)
        ph = 2 * np.pi * 75000.0 * np.cumsum(m) / fs
        z += amp * np.exp(1j * (2 * np.pi * off * t + ph))
    rng = np.random.default_rng(seed)
    z += rng.normal(0, noise, n) + 1j * rng.normal(0, noise, n)
    iq = np.empty(2 * n, np.uint8)
    iq[0::2] = np.clip(np.round(z.real + 127.5), 0, 255)
    iq[1::2] = np.clip(np.round(z.imag + 127.5), 0, 255)
    return iq


def lowpass(T, cutoff):
    """Hamming-windowed sinc, cutoff in cycles per sample, peak 2047 (the front end's prototype)."""
    nn = np.arange(T) - (T - 1) / 2
    h = np.sinc(2 * cutoff * nn) * np.hamming(T)
    return np.round(h / np.abs(h).max() * 2047).astype(np.int16)


def tone_db(a, f, fs, skip):
    """Amplitude of the tone f in a[skip:] (projection), in dB."""
    v = np.asarray(a[skip:], dtype=np.float64)
    n = np.arange(v.size)
    c = np.abs(np.sum(v * np.exp(-2j * np.pi * f * n / fs))) * 2 / v.size
    return 20 * np.log10(c + 1e-9)
