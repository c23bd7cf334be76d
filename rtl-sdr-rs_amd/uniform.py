"""Host-side wrapper of the uniform channelizer (include/fmd.h, fmd_uniform_*): one prototype filter applied to all N equally
spaced channels of every wideband IQ stream (or a selection of them) in one pass, each channel's complex baseband as int16
(yr, yi) pairs.  `channelizer.as_complex` serves the output."""
import ctypes as C

import numpy as np

from ._ffi import DeviceConfig, DownConverter, check, lib
from .stations import stations_auto_shift


def uniform_channel_inc(k, n):
    """inc_k = floor((k 2^33 / n + 1) / 2) mod 2^32: the phase step of channel k of n (include/fmd.h)."""
    inc = C.c_uint32(0)
    check(lib().fmd_uniform_channel_inc(int(k), int(n), C.byref(inc)))
    return inc.value


def uniform_channel_offsets(rate, n_channels):
    """Centre of every channel in Hz from the capture's centre, natural order: (k < N/2 ? k : k - N) rate / N."""
    k = np.arange(int(n_channels))
    return np.where(2 * k < n_channels, k, k - n_channels) * (float(rate) / n_channels)


def uniform_taps(n_channels, taps_per_channel, amplitude=2047):
    """The prototype h[t] = floor(amplitude s[t] / max|s| + 1/2), s[t] = sinc((t - (T - 1) / 2) / N) hamming(T), T = N
    taps_per_channel: a windowed-sinc low-pass whose first nulls lie one channel spacing from the centre."""
    N, T = int(n_channels), int(n_channels) * int(taps_per_channel)
    if T < 1 or not 1 <= int(amplitude) <= 2047:
        raise ValueError("need n_channels * taps_per_channel >= 1 and 1 <= amplitude <= 2047")
    t = np.arange(T, dtype=np.float64)
    s = np.sinc((t - (T - 1) / 2.0) / N) * np.hamming(T)
    return np.floor(int(amplitude) * s / np.abs(s).max() + 0.5).astype(np.int16)


def uniform_auto_shift(taps, n_channels, channels=None):
    """Smallest normalisation shift with ceil(256 G / 2^shift) <= 16384, G over the selected channels (None: all)."""
    ks = range(int(n_channels)) if channels is None else channels
    incs = np.asarray([uniform_channel_inc(k, n_channels) for k in ks], dtype=np.uint32)
    return stations_auto_shift(taps, incs, limit=16384)


class UniformChannelizer(DownConverter):
    """All `n_channels` channels (or the strictly increasing selection `channels`) of every stream, one output per `hop` input
    samples.  `shift=None` takes the smallest normalisation shift with |y| <= 16384."""
    _prefix = "uniform"
    _rows = "n_selected"                                     # run_batch: [n_streams, n_selected, n_out, 2] of (yr, yi)

    def __init__(self, taps, n_channels, hop, channels=None, n_streams=1, shift=None, device_id=-1):
        self.taps = np.ascontiguousarray(taps, dtype=np.int16)
        self.n_channels, self.hop, self.n_streams = int(n_channels), int(hop), int(n_streams)
        self.channels = (np.arange(self.n_channels, dtype=np.uint32) if channels is None
                         else np.ascontiguousarray(channels, dtype=np.uint32).ravel())
        self.n_selected = int(self.channels.size)
        self.shift = uniform_auto_shift(self.taps, self.n_channels, self.channels) if shift is None else int(shift)
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_streams, device_id, 0)
        sel = None if channels is None else self.channels.ctypes.data_as(C.POINTER(C.c_uint32))
        check(lib().fmd_uniform_new(self.taps.ctypes.data_as(C.POINTER(C.c_int16)), self.taps.size, self.n_channels, self.hop,
                                    self.shift, sel, self.n_selected, C.byref(dev), C.byref(self._h)))

    def out_cap(self, nbytes):
        return int(lib().fmd_uniform_out_cap(self.hop, nbytes))

    def tap_digits(self):
        """1 or 2: the i8 digits per tap on the matrix cores."""
        return int(lib().fmd_uniform_tap_digits(self._h))
