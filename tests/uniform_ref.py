"""Test-side definition of the uniform channelizer (include/fmd.h, "uniform channelizer"): the channelizer's definition
(tests/channelizer_ref.py) with decim = hop and the fixed grid of phase steps inc_k, plus the prototype filter the host layers
offer.  Independent of the library."""
import numpy as np

import channelizer_ref as cr
import stations_ref as sr
from stations_ref import TooShort  # noqa: F401  (re-exported: a call that completes no output)


def channel_inc(k, n):
    """inc_k = floor((k 2^33 / n + 1) / 2) mod 2^32 in exact integers."""
    return ((((k << 33) // n) + 1) >> 1) % (1 << 32)


def channel_incs(n, channels=None):
    return [channel_inc(int(k), n) for k in (range(n) if channels is None else channels)]


def taps(n_channels, taps_per_channel, amplitude=2047):
    """h[t] = floor(amplitude s[t] / max|s| + 1/2), s[t] = sinc((t - (T - 1) / 2) / N) hamming(T), T = N taps_per_channel."""
    T = n_channels * taps_per_channel
    t = np.arange(T, dtype=np.float64)
    s = np.sinc((t - (T - 1) / 2.0) / n_channels) * np.hamming(T)
    return np.floor(amplitude * s / np.abs(s).max() + 0.5).astype(np.int64)


def min_shift(h, incs, limit=16384):
    """The smallest shift with ceil(256 G / 2^shift) <= limit, G = max over the channels of sum_t |Wr| + |Wi|."""
    g, s = 256 * sr.max_gain(h, incs), 0
    while -(-g >> s) > limit:
        s += 1
    return s


def digits(h, incs):
    """1 when every |W| of these channels <= 127, else 2."""
    for inc in incs:
        wr, wi = sr.complex_taps(h, int(inc))
        if max(np.abs(wr).max(), np.abs(wi).max()) > 127:
            return 2
    return 1


class UniformRef(cr.ChannelizerRef):
    """One input stream; feed() mirrors one fmd_uniform call of that stream (whole hops) and returns int64 [n_selected, n, 2]."""

    def __init__(self, h, n_channels, hop, shift, channels=None, z=sr.z_corr):
        self.N, self.hop = int(n_channels), int(hop)
        super().__init__(h, hop, channel_incs(self.N, channels), shift, z=z)

    def feed(self, buf):
        assert np.asarray(buf).size % (2 * self.hop) == 0
        return super().feed(buf)
