"""Host-side wrapper of the station bank (include/fmd.h, fmd_stations_*): K FM stations demodulated out of each wideband IQ
stream -- mix by the station's offset, filter with one real prototype, decimate -- each followed by the reference's own
fm_demod (simple_fm.rs:355-367) and low_pass_real (:408-426)."""
import ctypes as C

import numpy as np

from ._ffi import DemodState, BankHandle, DeviceConfig, check, lib, stream_phase_incs


def phase_inc(offset_hz, rate):
    """Q32 phase increment per input sample of a station `offset_hz` from the capture's centre (|offset_hz| <= rate / 2)."""
    inc = C.c_uint32(0)
    check(lib().fmd_stations_phase_inc(int(offset_hz), int(rate), C.byref(inc)))
    return inc.value


def _nco_table():
    return np.round(16384.0 * np.cos(2.0 * np.pi * np.arange(1024) / 1024.0)).astype(np.int64)


def _max_gain(taps, phase_incs):
    """max over stations of sum_t |Wr| + |Wi| (the complex taps of include/fmd.h)."""
    h = np.asarray(taps, dtype=np.int64)
    tab = _nco_table()
    t = np.arange(h.size, dtype=np.uint64)
    g = 0
    for inc in np.unique(np.asarray(phase_incs, dtype=np.uint64).ravel()):
        ix = ((t * inc) & 0xFFFFFFFF) >> 22
        wr = (h * tab[ix] + 8192) >> 14
        wi = (-h * tab[(ix - 256) & 1023] + 8192) >> 14
        g = max(g, int(np.abs(wr).sum() + np.abs(wi).sum()))
    return g


def stations_auto_shift(taps, phase_incs, limit=2048):
    """Smallest normalisation shift with ceil(256 * max_gain / 2^shift) <= limit.  2048 (the default) selects the kernel's f32
    discriminator; 16384 is the most the bank admits."""
    g = 256 * _max_gain(taps, phase_incs)
    s = 0
    while -(-g >> s) > limit:
        s += 1
    return s


class StationBank(BankHandle):
    """`phase_incs` is [n_streams][n_stations] (a flat list of n_stations is taken for every stream)."""
    _prefix = "stations"

    def __init__(self, taps, decim, phase_incs, rate_out, rate_resample, n_streams=1, shift=None, device_id=-1):
        self.taps = np.ascontiguousarray(taps, dtype=np.int16)
        self.decim, self.n_streams = int(decim), int(n_streams)
        self.phase_incs = stream_phase_incs(phase_incs, self.n_streams)
        self.n_stations = self.phase_incs.shape[1]
        self.rate_out, self.rate_resample = int(rate_out), int(rate_resample)
        self.shift = stations_auto_shift(self.taps, self.phase_incs) if shift is None else int(shift)
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_streams, device_id, 0)
        check(lib().fmd_stations_new(self.taps.ctypes.data_as(C.POINTER(C.c_int16)), self.taps.size, self.decim, self.shift,
                                     self.phase_incs.ctypes.data_as(C.POINTER(C.c_uint32)), self.n_stations, self.rate_out,
                                     self.rate_resample, C.byref(dev), C.byref(self._h)))

    def out_cap(self, nbytes):
        return int(lib().fmd_stations_out_cap(self.decim, self.rate_out, self.rate_resample, nbytes))

    def demodulate_batch(self, iq):
        """iq uint8 [n_streams, nbytes] -> int16 array [n_streams, n_stations, n_audio]."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim != 2 or iq.shape[0] != self.n_streams:
            raise ValueError("iq must be [n_streams, nbytes]")
        cap = max(1, self.out_cap(iq.shape[1]))
        out = np.empty((self.n_streams, self.n_stations, cap), dtype=np.int16)
        lens = (C.c_size_t * (self.n_streams * self.n_stations))()
        check(lib().fmd_stations_demodulate_batch(self._h, iq.ctypes.data, iq.shape[1], out.ctypes.data, cap, lens))
        return out[:, :, :lens[0]].copy()

    def demodulate_device(self, d_iq, nbytes, d_out, out_cap, stream=None):
        """Enqueue on device pointers (d_out [n_streams][n_stations][out_cap] int16).  `stream` must stay alive until the handle's
        next `demodulate_device` call or `check` has returned (stream lifetime rule of include/fmd.h)."""
        n = C.c_size_t(0)
        check(lib().fmd_stations_demodulate_device(self._h, d_iq, nbytes, d_out, out_cap, C.byref(n), stream))
        return n.value

    def get_state(self, stream=0, station=0):
        s = DemodState()
        check(lib().fmd_stations_get_state(self._h, stream, station, C.byref(s)))
        return s

    def f64_stats(self):
        g, p = C.c_uint64(), C.c_uint64()
        check(lib().fmd_stations_f64_stats(self._h, C.byref(g), C.byref(p)))
        return g.value, p.value
