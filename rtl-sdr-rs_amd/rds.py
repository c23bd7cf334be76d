"""Host-side wrapper of the RDS bank (include/fmd.h, fmd_rds_*) and the RDS decoder (fmd_rds_decoder_*): K FM stations per wideband
IQ stream, each station's 57 kHz subcarrier returned as a complex baseband of a few kHz (int16 (ur, ui) pairs at capture_rate /
(decim R)), and the host decoder that turns one station's baseband into groups, PI, PS and RadioText."""
import ctypes as C

import numpy as np

from ._ffi import DownConverter, check, lib
from .channelizer import as_complex
from .stereo import MpxStage


class RdsConfig(C.Structure):
    _fields_ = [("capture_rate", C.c_uint32), ("block", C.c_uint32), ("out_decim", C.c_uint32), ("rds_shift", C.c_uint32),
                ("pilot_min", C.c_uint32)]


class RdsGroup(C.Structure):
    _fields_ = [("block", C.c_uint16 * 4), ("ok_mask", C.c_uint8), ("first_sample", C.c_uint64)]


class RdsInfo(C.Structure):
    _fields_ = [("pi", C.c_uint16), ("ps", C.c_char * 9), ("rt", C.c_char * 65), ("groups_ok", C.c_uint64), ("blocks_bad", C.c_uint64),
                ("synced", C.c_int)]


def rds_taps(mpx_rate, out_decim, n_taps, cutoff_hz=2400):
    """(g, rds_shift) for an RdsBank: a Hamming-windowed sinc low-pass at +-`cutoff_hz` around the subcarrier, scaled so that
    sum |g| <= 16383, int16, and the smallest rds_shift at which the int16 store is exact (ceil(32768 sum|g| / 2^shift) <= 32767).
    `out_decim` is the stride the taps are used with; it does not change them."""
    n = int(n_taps)
    if n < 1 or n > 256 or int(out_decim) < 1:
        raise ValueError("need 1 <= n_taps <= 256 and out_decim >= 1")
    fc = float(cutoff_hz) / float(mpx_rate)
    t = np.arange(n) - (n - 1) / 2
    g = 2 * fc * np.sinc(2 * fc * t) * (np.hamming(n) if n > 1 else np.ones(1))
    g = g / np.abs(g).sum() * (16383 - n)                    # rounding adds at most n / 2 to sum |g|
    g = np.floor(g + 0.5).astype(np.int16)
    return g, rds_shift_for(g)


def rds_shift_for(g):
    total = 32768 * int(np.abs(np.asarray(g, dtype=np.int64)).sum())
    s = 0
    while -(-total >> s) > 32767:
        s += 1
    return s


class RdsBank(MpxStage, DownConverter):
    """`phase_incs` is [n_streams][n_stations] (a flat list of n_stations is taken for every stream).  `shift=None` takes the smallest
    front-end shift with every |y| component <= 256 (stereo.FRONT_END_LIMIT); `pilot_min=None` a quarter of a nominal pilot;
    `rds_shift=None` the smallest exact one.  run_batch returns [n_streams, n_stations, n, 2] of (ur, ui)."""
    _prefix = "rds"
    _passes = 2                                              # 0: the stereo bank's multiplex pass; 1: carrier, FIRs, shift

    def __init__(self, taps, decim, phase_incs, capture_rate, rds_taps, out_decim, n_streams=1, block=4096, pilot_min=None,
                 rds_shift=None, shift=None, device_id=-1):
        self._mpx_setup(taps, decim, phase_incs, capture_rate, n_streams, block, pilot_min, shift)
        self.rds_taps = np.ascontiguousarray(rds_taps, dtype=np.int16)
        self.out_decim = int(out_decim)
        self.rds_shift = rds_shift_for(self.rds_taps) if rds_shift is None else int(rds_shift)
        self.rate_num, self.rate_den = self.capture_rate, self.decim * self.out_decim
        self.out_rate = self.rate_num / self.rate_den
        self._mpx_new(self.rds_taps, RdsConfig(self.capture_rate, self.block, self.out_decim, self.rds_shift, self.pilot_min), device_id)

    def out_cap(self, nbytes):
        return int(lib().fmd_rds_out_cap(self.decim, self.out_decim, nbytes))

    def run_complex(self, iq):
        """run_batch as complex64 [n_streams, n_stations, n]."""
        return as_complex(self.run_batch(iq))

class RdsDecoder:
    """The host decoder of one (stream, station): push() takes int16 [n, 2] (ur, ui) at rate_num / rate_den Hz and returns the
    groups completed since, as dicts {"blocks": (A, B, C, D), "ok_mask", "first_sample"}; info() the station's PI, PS and text."""

    def __init__(self, rate_num, rate_den=1):
        self._h = C.c_void_p()
        check(lib().fmd_rds_decoder_new(int(rate_num), int(rate_den), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().fmd_rds_decoder_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(lib().fmd_rds_decoder_reset(self._h))

    def push(self, u):
        u = np.ascontiguousarray(u, dtype=np.int16)
        if u.ndim != 2 or u.shape[1] != 2:
            raise ValueError("u must be [n, 2] (ur, ui)")
        buf = (RdsGroup * 64)()
        n = C.c_size_t(0)
        groups = []
        check(lib().fmd_rds_decoder_push(self._h, u.ctypes.data, u.shape[0], buf, 64, C.byref(n)))
        while True:
            groups += [{"blocks": tuple(buf[i].block), "ok_mask": buf[i].ok_mask, "first_sample": buf[i].first_sample} for i in range(n.value)]
            if n.value < 64:
                return groups
            check(lib().fmd_rds_decoder_push(self._h, None, 0, buf, 64, C.byref(n)))

    def info(self):
        i = RdsInfo()
        check(lib().fmd_rds_decoder_info(self._h, C.byref(i)))
        return {"pi": i.pi, "ps": i.ps.decode("latin-1"), "rt": i.rt.decode("latin-1"), "groups_ok": i.groups_ok,
                "blocks_bad": i.blocks_bad, "synced": bool(i.synced)}


def decode_stations(bank, iq_calls):
    """Every call of `iq_calls` (uint8 [n_streams, nbytes] each) through `bank`, every (stream, station) through a decoder of its own:
    a list [n_streams][n_stations] of RdsDecoder.info() dicts with the delivered groups under "groups"."""
    decs = [[RdsDecoder(bank.rate_num, bank.rate_den) for _ in range(bank.n_stations)] for _ in range(bank.n_streams)]
    groups = [[[] for _ in range(bank.n_stations)] for _ in range(bank.n_streams)]
    for iq in iq_calls:
        u = bank.run_batch(iq)
        for s in range(bank.n_streams):
            for k in range(bank.n_stations):
                groups[s][k] += decs[s][k].push(u[s, k])
    return [[dict(decs[s][k].info(), groups=groups[s][k]) for k in range(bank.n_stations)] for s in range(bank.n_streams)]
