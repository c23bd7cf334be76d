"""Host-side wrapper of the narrow-band bank (include/fmd.h, fmd_narrow_*): K narrow channels per wideband IQ stream -- the
channelizer's baseband, a second, complex decimating FIR, one of four detectors (IQ, NFM, AM, SSB) and a block-wise squelch -- as
int16 at capture_rate / (decim R)."""
import ctypes as C

import numpy as np

from ._ffi import DeviceConfig, DownConverter, check, lib, stream_phase_incs
from .stations import _max_gain, stations_auto_shift
from .stereo import FRONT_END_LIMIT

NARROW_IQ, NARROW_FM, NARROW_AM, NARROW_SSB = 0, 1, 2, 3
MODES = {"iq": NARROW_IQ, "raw": NARROW_IQ, "fm": NARROW_FM, "am": NARROW_AM, "usb": NARROW_SSB, "lsb": NARROW_SSB, "ssb": NARROW_SSB}

# The bound on every |y| component the front end is scaled to: the channelizer's own.  (The channel filter's output is what the
# discriminator sees, so FRONT_END_LIMIT applies to |u| in FM mode: narrow_auto_shift.)
Y_LIMIT = 16384


class NarrowConfig(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("chan_decim", C.c_uint32), ("chan_shift", C.c_uint32), ("block", C.c_uint32),
                ("squelch", C.c_uint32), ("gain", C.c_uint32)]


def narrow_taps(rate, n_taps, lo_hz, hi_hz):
    """Channel taps (gr, gi) for a NarrowBank at the channelizer's output rate `rate`: a Hamming-windowed complex band-pass from
    lo_hz to hi_hz (a low-pass of half that width shifted to the band's centre), scaled so that sum |gr| + |gi| <= 65535 with every
    tap within 16383, int16.  Real (gi is None) when lo_hz == -hi_hz.  USB is e.g. (300, 3000), LSB (-3000, -300)."""
    n = int(n_taps)
    if n < 1 or n > 256 or not hi_hz > lo_hz:
        raise ValueError("need 1 <= n_taps <= 256 and lo_hz < hi_hz")
    fs = float(rate)
    t = np.arange(n) - (n - 1) / 2
    bw, fc = (hi_hz - lo_hz) / fs, (hi_hz + lo_hz) / (2 * fs)
    lp = bw * np.sinc(bw * t) * (np.hamming(n) if n > 1 else np.ones(1))
    real = lo_hz == -hi_hz
    # the filter is the correlation sum_t g[t] y[R n + t]: its response to exp(j w m) is sum_t g[t] exp(j w t), so the low-pass is
    # shifted by exp(-j 2 pi fc t) to pass +fc
    g = lp.astype(np.complex128) if real else lp * np.exp(-2j * np.pi * fc * t)
    total = np.abs(g.real).sum() + np.abs(g.imag).sum()
    scale = min((65535 - 2 * n) / total, 16383 / max(np.abs(g.real).max(), np.abs(g.imag).max()))   # rounding adds at most n
    gr = np.floor(g.real * scale + 0.5).astype(np.int16)
    gi = None if real else np.floor(g.imag * scale + 0.5).astype(np.int16)
    return gr, gi


def narrow_gain_sum(gr, gi=None):
    g = np.abs(np.asarray(gr, dtype=np.int64)).sum()
    return int(g + (np.abs(np.asarray(gi, dtype=np.int64)).sum() if gi is not None else 0))


def narrow_y_bound(taps, phase_incs, shift):
    """B_y of the definition: ceil(256 max_k sum_t (|Wr| + |Wi|) / 2^shift)."""
    g = _max_gain(taps, phase_incs)
    return -(-256 * g >> int(shift))


def narrow_auto_shift(taps, phase_incs, shift, gr, gi=None, mode=NARROW_IQ, limit=None):
    """The smallest chan_shift that keeps every |u| component <= limit: 256 in FM mode (the wrap reason at stereo.FRONT_END_LIMIT),
    16384 otherwise."""
    if limit is None:
        limit = FRONT_END_LIMIT if int(mode) == NARROW_FM else Y_LIMIT
    peak = narrow_y_bound(taps, phase_incs, shift) * narrow_gain_sum(gr, gi)
    s = 0
    while s < 30 and -(-peak >> s) > limit:
        s += 1
    return s


class ChanStage:
    """The second stage's side of a wrapper -- the channel taps, the mode, the config -- for the two handles that have it:
    NarrowBank and bandplan.BandPlanBank.  A mixin in front of DownConverter."""

    def _chan_setup(self, chan_taps, mode, chan_decim, block, squelch, gain):
        gr, gi = chan_taps if isinstance(chan_taps, tuple) else (chan_taps, None)
        self.gr = np.ascontiguousarray(gr, dtype=np.int16)
        self.gi = None if gi is None else np.ascontiguousarray(gi, dtype=np.int16)
        if self.gi is not None and self.gi.size != self.gr.size:
            raise ValueError("gr and gi differ in length")
        self.mode = MODES[mode] if isinstance(mode, str) else int(mode)
        self.chan_decim, self.block, self.squelch, self.gain = int(chan_decim), int(block), int(squelch), int(gain)
        self.width = 2 if self.mode == NARROW_IQ else 1

    def _chan_args(self):
        """chan_taps_re, chan_taps_im, n_chan_taps, cfg of a *_new (once self.chan_shift is set)"""
        p16 = C.POINTER(C.c_int16)
        cfg = NarrowConfig(self.mode, self.chan_decim, self.chan_shift, self.block, self.squelch, self.gain)
        return (self.gr.ctypes.data_as(p16), None if self.gi is None else self.gi.ctypes.data_as(p16), self.gr.size, C.byref(cfg))

    def run_batch(self, iq):
        """iq uint8 [n_streams, nbytes] -> int16 [n_streams, rows, n] ([..., 2] of (re, im) in IQ mode)."""
        out = super().run_batch(iq)
        return out if self.mode == NARROW_IQ else out[..., 0].copy()


class NarrowBank(ChanStage, DownConverter):
    """`phase_incs` is [n_streams][n_stations] (a flat list of n_stations is taken for every stream).  `chan_taps` is gr or the
    pair (gr, gi) (narrow_taps).  `shift=None` takes the smallest front-end shift with every |y| component <= 16384;
    `chan_shift=None` narrow_auto_shift.  `gain` is Q8."""
    _prefix = "narrow"
    _passes = 2                                              # 0: front end; 1: channel FIR, detector, squelch

    def __init__(self, taps, decim, phase_incs, chan_taps, chan_decim, mode=NARROW_FM, n_streams=1, block=256, squelch=0, gain=256,
                 chan_shift=None, shift=None, device_id=-1):
        self.taps = np.ascontiguousarray(taps, dtype=np.int16)
        self._chan_setup(chan_taps, mode, chan_decim, block, squelch, gain)
        self.decim, self.n_streams = int(decim), int(n_streams)
        self.phase_incs = stream_phase_incs(phase_incs, self.n_streams)
        self.n_stations = self.phase_incs.shape[1]
        self.shift = stations_auto_shift(self.taps, self.phase_incs, limit=Y_LIMIT) if shift is None else int(shift)
        self.chan_shift = (narrow_auto_shift(self.taps, self.phase_incs, self.shift, self.gr, self.gi, self.mode)
                           if chan_shift is None else int(chan_shift))
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_streams, device_id, 0)
        check(lib().fmd_narrow_new(self.taps.ctypes.data_as(C.POINTER(C.c_int16)), self.taps.size, self.decim, self.shift,
                                   self.phase_incs.ctypes.data_as(C.POINTER(C.c_uint32)), self.n_stations, *self._chan_args(),
                                   C.byref(dev), C.byref(self._h)))

    def out_cap(self, nbytes):
        return int(lib().fmd_narrow_out_cap(self.decim, self.chan_decim, nbytes))

    def level(self, stream=0, station=0):
        """(open, rms) of the last completed block: the squelch state and the channel's RMS amplitude in units of u."""
        o, r = C.c_int(0), C.c_uint32(0)
        check(lib().fmd_narrow_level(self._h, int(stream), int(station), C.byref(o), C.byref(r)))
        return bool(o.value), r.value
