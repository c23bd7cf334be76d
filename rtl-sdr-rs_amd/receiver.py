"""Host-side wrapper of the FM receiver bank (include/fmd.h, fmd_receiver_*): K FM stations per wideband IQ stream, each returned as
pilot-locked stereo audio AND as the RDS baseband, out of one multiplex pass -- what a StereoBank and an RdsBank over the same bytes
return, bit for bit, without running the front end, the discriminator and the pilot sums twice."""
import ctypes as C

import numpy as np

from ._ffi import BankHandle, DeviceConfig, check, lib
from .rds import RdsDecoder, rds_shift_for
from .stereo import MpxStage, default_audio_shift


class ReceiverConfig(C.Structure):
    _fields_ = [("capture_rate", C.c_uint32), ("block", C.c_uint32), ("pilot_min", C.c_uint32), ("audio_decim", C.c_uint32),
                ("audio_shift", C.c_uint32), ("rds_decim", C.c_uint32), ("rds_shift", C.c_uint32)]


class ReceiverBank(MpxStage, BankHandle):
    """`phase_incs`, `shift`, `pilot_min` as StereoBank; `audio_shift=None` stereo.default_audio_shift, `rds_shift=None` the smallest
    exact one.  run_batch returns (audio [n_streams, n_stations, na, 2] of (L, R), rds [n_streams, n_stations, nr, 2] of (ur, ui)).  A
    call must complete an output of each (FmdError FMD_ERR_TOO_SHORT otherwise; nothing changes)."""
    _prefix = "receiver"

    def __init__(self, taps, decim, phase_incs, capture_rate, audio_taps, audio_decim, rds_taps, rds_decim, n_streams=1, block=4096,
                 pilot_min=None, audio_shift=None, rds_shift=None, shift=None, device_id=-1):
        self._mpx_setup(taps, decim, phase_incs, capture_rate, n_streams, block, pilot_min, shift)
        self.audio_taps = np.ascontiguousarray(audio_taps, dtype=np.int16)
        self.rds_taps = np.ascontiguousarray(rds_taps, dtype=np.int16)
        self.audio_decim, self.rds_decim = int(audio_decim), int(rds_decim)
        self.audio_shift = (default_audio_shift(self.audio_taps, self.capture_rate, self.decim) if audio_shift is None
                            else int(audio_shift))
        self.rds_shift = rds_shift_for(self.rds_taps) if rds_shift is None else int(rds_shift)
        self.audio_rate = self.capture_rate / (self.decim * self.audio_decim)
        self.rate_num, self.rate_den = self.capture_rate, self.decim * self.rds_decim       # the baseband's rate, for RdsDecoder
        cfg = ReceiverConfig(self.capture_rate, self.block, self.pilot_min, self.audio_decim, self.audio_shift, self.rds_decim,
                             self.rds_shift)
        p16 = C.POINTER(C.c_int16)
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_streams, device_id, 0)
        check(lib().fmd_receiver_new(self.taps.ctypes.data_as(p16), self.taps.size, self.decim, self.shift,
                                     self.phase_incs.ctypes.data_as(C.POINTER(C.c_uint32)), self.n_stations,
                                     self.audio_taps.ctypes.data_as(p16), self.audio_taps.size,
                                     self.rds_taps.ctypes.data_as(p16), self.rds_taps.size, C.byref(cfg), C.byref(dev), C.byref(self._h)))

    def out_caps(self, nbytes):
        """(audio, rds) capacities per (stream, station) that bound a call of nbytes: the two banks' own."""
        return (int(lib().fmd_stereo_out_cap(self.decim, self.audio_decim, nbytes)),
                int(lib().fmd_rds_out_cap(self.decim, self.rds_decim, nbytes)))

    def kernel_name(self, which=0):
        """The kernel of pass `which` (0: multiplex, 1: both second stages), as rocprofv3 --kernel-trace prints it."""
        buf = C.create_string_buffer(128)
        check(lib().fmd_receiver_kernel_name(self._h, int(which), buf, len(buf)))
        return buf.value.decode()

    def outputs(self):
        """(audio samples, RDS baseband samples) per row produced since creation or reset."""
        a, r = C.c_uint64(0), C.c_uint64(0)
        check(lib().fmd_receiver_outputs(self._h, C.byref(a), C.byref(r)))
        return a.value, r.value

    def run_batch(self, iq):
        """iq uint8 [n_streams, nbytes] -> (audio, rds), int16 [n_streams, n_stations, n, 2] each."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim != 2 or iq.shape[0] != self.n_streams:
            raise ValueError("iq must be [n_streams, nbytes]")
        ca, cr = (max(1, c) for c in self.out_caps(iq.shape[1]))
        audio = np.empty((self.n_streams, self.n_stations, ca, 2), dtype=np.int16)
        rds = np.empty((self.n_streams, self.n_stations, cr, 2), dtype=np.int16)
        na, nr = C.c_size_t(0), C.c_size_t(0)
        check(lib().fmd_receiver_run_batch(self._h, iq.ctypes.data, iq.shape[1], audio.ctypes.data, ca, C.byref(na), rds.ctypes.data, cr,
                                           C.byref(nr)))
        return audio[:, :, :na.value].copy(), rds[:, :, :nr.value].copy()

    def run_device(self, d_iq, nbytes, d_audio, audio_cap, d_rds, rds_cap, stream=None):
        """Enqueue on device pointers (d_audio [n_streams][n_stations][audio_cap][2], d_rds likewise, int16); returns (na, nr).
        `stream` must stay alive until the handle's next `run_device` call or `check` has returned (include/fmd.h)."""
        na, nr = C.c_size_t(0), C.c_size_t(0)
        check(lib().fmd_receiver_run_device(self._h, d_iq, nbytes, d_audio, audio_cap, C.byref(na), d_rds, rds_cap, C.byref(nr), stream))
        return na.value, nr.value


def receive_stations(bank, iq_calls):
    """Every call of `iq_calls` (uint8 [n_streams, nbytes] each) through `bank`, every (stream, station)'s baseband through a decoder
    of its own: (audio int16 [n_streams, n_stations, n, 2] of all calls, a list [n_streams][n_stations] of RdsDecoder.info() dicts
    with the delivered groups under "groups")."""
    decs = [[RdsDecoder(bank.rate_num, bank.rate_den) for _ in range(bank.n_stations)] for _ in range(bank.n_streams)]
    groups = [[[] for _ in range(bank.n_stations)] for _ in range(bank.n_streams)]
    audio = []
    for iq in iq_calls:
        a, u = bank.run_batch(iq)
        audio.append(a)
        for s in range(bank.n_streams):
            for k in range(bank.n_stations):
                groups[s][k] += decs[s][k].push(u[s, k])
    infos = [[dict(decs[s][k].info(), groups=groups[s][k]) for k in range(bank.n_stations)] for s in range(bank.n_streams)]
    return np.concatenate(audio, axis=2), infos
