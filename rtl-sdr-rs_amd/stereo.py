"""Host-side wrapper of the stereo station bank (include/fmd.h, fmd_stereo_*): K FM stations per wideband IQ stream, each returned as
pilot-locked stereo -- the channelizer's baseband, the reference's integer discriminator at the multiplex rate, a block-wise pilot
estimate, and one FIR over the sum and the difference signal -- as interleaved (L, R) int16 at capture_rate / (decim R)."""
import ctypes as C

import numpy as np

from ._ffi import DeviceConfig, DownConverter, check, lib, stream_phase_incs
from .stations import stations_auto_shift


# The default front-end bound on every |y| component.  The reference's discriminator truncates 4096 (x - |y|) to i32, with
# x + j y = a conj(b): it wraps once |a| |b| nears 2^19 / sqrt 2.  With components <= 256, |a| |b| <= 2^17 and it never does; the
# channelizer's own bound (16384) is valid input too, but strong stations then come out as wrapped noise.
FRONT_END_LIMIT = 256


class StereoConfig(C.Structure):
    _fields_ = [("capture_rate", C.c_uint32), ("block", C.c_uint32), ("audio_decim", C.c_uint32), ("audio_shift", C.c_uint32),
                ("pilot_min", C.c_uint32)]


def stereo_taps(mpx_rate, audio_decim, n_taps, cutoff_hz=15000, tau_us=75):
    """Audio taps g for a StereoBank: a Hamming-windowed sinc low-pass at `cutoff_hz` convolved with the sampled de-emphasis response
    (first order, tau 50 or 75 us; None or 0: none), scaled so that sum |g| <= 16383, int16.  `audio_decim` is the stride the taps
    are used with; it does not change them (the low-pass already removes what the decimation would fold)."""
    n = int(n_taps)
    if n < 1 or n > 256 or int(audio_decim) < 1:
        raise ValueError("need 1 <= n_taps <= 256 and audio_decim >= 1")
    fs = float(mpx_rate)
    if tau_us:
        nd = max(1, n // 2)                                  # de-emphasis response: (1 - a) a^i, i < nd
        a = np.exp(-1.0 / (tau_us * 1e-6 * fs))
        d = (1 - a) * a ** np.arange(nd)
    else:
        nd, d = 1, np.ones(1)
    nl = n - nd + 1
    t = np.arange(nl) - (nl - 1) / 2
    lp = 2 * cutoff_hz / fs * np.sinc(2 * cutoff_hz / fs * t) * (np.hamming(nl) if nl > 1 else np.ones(1))
    g = np.convolve(lp, d)
    g = g / np.abs(g).sum() * (16383 - n)                    # rounding adds at most n / 2 to sum |g|
    return np.floor(g + 0.5).astype(np.int16)


def default_pilot_min(capture_rate, decim):
    """A quarter of a nominal 6.75 kHz pilot at f_m = capture_rate / decim, in discriminator units (32768 f / f_m)."""
    return (32768 * 6750 * int(decim)) // (4 * int(capture_rate))


def default_audio_shift(audio_taps, capture_rate, decim):
    """Smallest shift (<= 16) at which mono at full deviation (75 kHz) stays inside int16: sum(g) 32768 75 kHz / f_m >> (shift + 1)."""
    peak = abs(int(np.asarray(audio_taps, dtype=np.int64).sum())) * 32768 * 75000 * int(decim) // int(capture_rate)
    s = 0
    while s < 16 and peak >> (s + 1) > 32767:
        s += 1
    return s


def pilot_inc(capture_rate, decim):
    inc = C.c_uint32(0)
    check(lib().fmd_stereo_pilot_inc(int(capture_rate), int(decim), C.byref(inc)))
    return inc.value


class MpxStage:
    """The common side of the two wrappers whose handle runs a second stage over the multiplex -- the front end's arguments, the
    rates, the pilot -- for StereoBank and rds.RdsBank.  A mixin in front of DownConverter."""

    def _mpx_setup(self, taps, decim, phase_incs, capture_rate, n_streams, block, pilot_min, shift):
        self.taps = np.ascontiguousarray(taps, dtype=np.int16)
        self.decim, self.n_streams, self.capture_rate, self.block = int(decim), int(n_streams), int(capture_rate), int(block)
        self.phase_incs = stream_phase_incs(phase_incs, self.n_streams)
        self.n_stations = self.phase_incs.shape[1]
        self.shift = stations_auto_shift(self.taps, self.phase_incs, limit=FRONT_END_LIMIT) if shift is None else int(shift)
        self.pilot_min = default_pilot_min(self.capture_rate, self.decim) if pilot_min is None else int(pilot_min)

    def _mpx_new(self, g, cfg, device_id):
        """fmd_<_prefix>_new with the second stage's taps `g` and the bank's config"""
        p16 = C.POINTER(C.c_int16)
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_streams, device_id, 0)
        check(self._fn("new")(self.taps.ctypes.data_as(p16), self.taps.size, self.decim, self.shift,
                              self.phase_incs.ctypes.data_as(C.POINTER(C.c_uint32)), self.n_stations, g.ctypes.data_as(p16), g.size,
                              C.byref(cfg), C.byref(dev), C.byref(self._h)))

    def pilot(self, stream=0, station=0):
        """(present, level) of the last completed block: the stereo indicator and the pilot amplitude in discriminator units."""
        p, lv = C.c_int(0), C.c_uint32(0)
        check(self._fn("pilot")(self._h, int(stream), int(station), C.byref(p), C.byref(lv)))
        return bool(p.value), lv.value


class StereoBank(MpxStage, DownConverter):
    """`phase_incs` is [n_streams][n_stations] (a flat list of n_stations is taken for every stream).  `shift=None` takes the smallest
    front-end shift with every |y| component <= 256 (FRONT_END_LIMIT); `pilot_min=None` a quarter of a nominal pilot;
    `audio_shift=None` default_audio_shift.  run_batch returns [n_streams, n_stations, n_audio, 2] of (L, R)."""
    _prefix = "stereo"
    _passes = 2                                              # 0: front end, discriminator, pilot sums; 1: carrier, FIRs, matrix

    def __init__(self, taps, decim, phase_incs, capture_rate, audio_taps, audio_decim, n_streams=1, block=4096, pilot_min=None,
                 audio_shift=None, shift=None, device_id=-1):
        self._mpx_setup(taps, decim, phase_incs, capture_rate, n_streams, block, pilot_min, shift)
        self.audio_taps = np.ascontiguousarray(audio_taps, dtype=np.int16)
        self.audio_decim = int(audio_decim)
        self.audio_shift = (default_audio_shift(self.audio_taps, self.capture_rate, self.decim) if audio_shift is None
                            else int(audio_shift))
        self.audio_rate = self.capture_rate / (self.decim * self.audio_decim)
        self._mpx_new(self.audio_taps, StereoConfig(self.capture_rate, self.block, self.audio_decim, self.audio_shift, self.pilot_min),
                      device_id)

    def out_cap(self, nbytes):
        return int(lib().fmd_stereo_out_cap(self.decim, self.audio_decim, nbytes))
