"""Host-side wrapper of the channelizer (include/fmd.h, fmd_channelizer_*): K digital down-converters per wideband IQ stream -- mix
by the station's offset, filter with one real prototype, decimate -- each returning the station's complex baseband as int16
(yr, yi) pairs.  The station bank (stations.py) is this followed by fm_demod and low_pass_real."""
import ctypes as C

import numpy as np

from ._ffi import DeviceConfig, DownConverter, check, lib, stream_phase_incs
from .stations import stations_auto_shift


def as_complex(x):
    """int16 [..., 2] (yr, yi) pairs -> complex64 [...]."""
    x = np.asarray(x)
    if x.shape[-1:] != (2,):
        raise ValueError("expected a trailing axis of 2 (yr, yi)")
    return (x[..., 0].astype(np.float32) + 1j * x[..., 1].astype(np.float32)).astype(np.complex64)


class Channelizer(DownConverter):
    """`phase_incs` is [n_streams][n_stations] (a flat list of n_stations is taken for every stream).  `shift=None` takes the
    smallest normalisation shift with |y| <= 16384.  run_batch returns [n_streams, n_stations, n_out, 2] of (yr, yi)."""
    _prefix = "channelizer"

    def __init__(self, taps, decim, phase_incs, n_streams=1, shift=None, device_id=-1):
        self.taps = np.ascontiguousarray(taps, dtype=np.int16)
        self.decim, self.n_streams = int(decim), int(n_streams)
        self.phase_incs = stream_phase_incs(phase_incs, self.n_streams)
        self.n_stations = self.phase_incs.shape[1]
        self.shift = stations_auto_shift(self.taps, self.phase_incs, limit=16384) if shift is None else int(shift)
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_streams, device_id, 0)
        check(lib().fmd_channelizer_new(self.taps.ctypes.data_as(C.POINTER(C.c_int16)), self.taps.size, self.decim, self.shift,
                                        self.phase_incs.ctypes.data_as(C.POINTER(C.c_uint32)), self.n_stations, C.byref(dev),
                                        C.byref(self._h)))

    def out_cap(self, nbytes):
        return int(lib().fmd_channelizer_out_cap(self.decim, nbytes))
