"""Host-side wrapper of the band-plan bank (include/fmd.h, fmd_bandplan_*): every channel of a band plan (or a selection of them)
of every wideband IQ stream -- the uniform channelizer's baseband, a second, complex decimating FIR, one of four detectors (IQ,
NFM, AM, SSB) and a block-wise squelch -- as int16 at capture_rate / (hop R), and the plan's activity map."""
import ctypes as C

import numpy as np

from ._ffi import DeviceConfig, DownConverter, check, lib
from .narrow import NARROW_FM, NARROW_IQ, Y_LIMIT, ChanStage, narrow_auto_shift
from .stereo import FRONT_END_LIMIT
from .uniform import uniform_auto_shift, uniform_channel_inc


def bandplan_auto_shifts(taps, n_channels, channels, gr, gi=None, mode=NARROW_IQ, shift=None):
    """(shift, chan_shift): the smallest legal ones -- uniform_auto_shift for stage one and narrow_auto_shift applied to the uniform
    channelizer's B_y for stage two (|u| <= 256 in FM mode, 16384 otherwise)."""
    ks = range(int(n_channels)) if channels is None else channels
    incs = np.asarray([uniform_channel_inc(k, n_channels) for k in ks], dtype=np.uint32)
    s = uniform_auto_shift(taps, n_channels, channels) if shift is None else int(shift)
    limit = FRONT_END_LIMIT if int(mode) == NARROW_FM else Y_LIMIT
    return s, narrow_auto_shift(taps, incs, s, gr, gi, mode, limit=limit)


class BandPlanBank(ChanStage, DownConverter):
    """All `n_channels` channels (or the strictly increasing selection `channels`) of every stream through one second stage:
    `chan_taps` is gr or the pair (gr, gi) (narrow_taps at capture_rate / hop), `chan_decim` R in 1 ... 8, at most 64 taps.
    `shift=None` and `chan_shift=None` take the smallest legal shifts (bandplan_auto_shifts).  `gain` is Q8."""
    _prefix = "bandplan"
    _rows = "n_selected"                                     # run_batch: [n_streams, n_selected, n] ([..., 2] in IQ mode)
    _passes = 2                                              # 0: the uniform channelizer; 1: channel FIR, detector, squelch

    def __init__(self, taps, n_channels, hop, chan_taps, chan_decim, mode=NARROW_FM, channels=None, n_streams=1, block=256,
                 squelch=0, gain=256, chan_shift=None, shift=None, device_id=-1):
        self.taps = np.ascontiguousarray(taps, dtype=np.int16)
        self._chan_setup(chan_taps, mode, chan_decim, block, squelch, gain)
        self.n_channels, self.hop, self.n_streams = int(n_channels), int(hop), int(n_streams)
        self.channels = (np.arange(self.n_channels, dtype=np.uint32) if channels is None
                         else np.ascontiguousarray(channels, dtype=np.uint32).ravel())
        self.n_selected = int(self.channels.size)
        auto = bandplan_auto_shifts(self.taps, self.n_channels, self.channels, self.gr, self.gi, self.mode, shift)
        self.shift = auto[0]
        self.chan_shift = auto[1] if chan_shift is None else int(chan_shift)
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_streams, device_id, 0)
        sel = None if channels is None else self.channels.ctypes.data_as(C.POINTER(C.c_uint32))
        check(lib().fmd_bandplan_new(self.taps.ctypes.data_as(C.POINTER(C.c_int16)), self.taps.size, self.n_channels, self.hop, self.shift,
                                     sel, self.n_selected, *self._chan_args(), C.byref(dev), C.byref(self._h)))

    def out_cap(self, nbytes):
        return int(lib().fmd_bandplan_out_cap(self.hop, self.chan_decim, nbytes))

    def levels(self):
        """The activity map of the last completed block: (open bool [n_streams, n_selected], rms uint32 [n_streams, n_selected]),
        the squelch state and each channel's RMS amplitude in units of u; all zero before the first block completes."""
        o = np.zeros((self.n_streams, self.n_selected), dtype=np.uint8)
        r = np.zeros((self.n_streams, self.n_selected), dtype=np.uint32)
        check(lib().fmd_bandplan_levels(self._h, o.ctypes.data_as(C.POINTER(C.c_uint8)), r.ctypes.data_as(C.POINTER(C.c_uint32))))
        return o.astype(bool), r
