"""Host-side wrapper of the rational resampler (include/fmd.h, fmd_resample_*): a polyphase L / M filter over the int16 rows a bank
leaves on the device -- mono audio at width 1, interleaved (L, R) or (I, Q) at width 2 -- so that any bank's output reaches a rate a
sound device, a codec or the RDS decoder takes.  Exact in integers; the output does not depend on how the stream is cut."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

from ._ffi import DeviceConfig, RowProcessor, bank_rows, check, lib


def _fraction(rate):
    """A rate as a Fraction: an int, a Fraction or a (num, den) pair."""
    if isinstance(rate, (tuple, list)):
        return Fraction(int(rate[0]), int(rate[1]))
    return Fraction(rate)


def resample_ratio(rate_in, rate_out):
    """(L, M) with L / M = rate_out / rate_in in lowest terms; `rate_in` is an int, a fractions.Fraction or a (num, den) pair (the
    banks' rates are rational: capture_rate / (decim R)).  FmdError (FMD_ERR_UNSUPPORTED) outside the resampler's domain."""
    r = _fraction(rate_in)
    L, M = C.c_uint32(0), C.c_uint32(0)
    check(lib().fmd_resample_ratio(r.numerator, r.denominator, int(rate_out), C.byref(L), C.byref(M)))
    return L.value, M.value


def resample_prototype(L, M, T, cutoff=0.45):
    """The float64 prototype of resample_taps: a Hamming-windowed sinc of L T points at cutoff / max(L, M) cycles per upsampled
    sample, unnormalised.  Scalar libm arithmetic in a fixed order, as fm::resample_taps (csrc/demod.hpp) does it."""
    n = int(L) * int(T)
    fc = cutoff / max(int(L), int(M))
    h = [0.0] * n
    for i in range(n):
        x = 2 * math.pi * fc * (i - (n - 1) / 2.0)
        s = 1.0 if x == 0 else math.sin(x) / x
        w = 0.54 - 0.46 * math.cos(2 * math.pi * i / (n - 1)) if n > 1 else 1.0
        h[i] = s * w
    return h


def resample_taps(L, M, T, cutoff=0.45):
    """(g int16 [L, T], shift): g[p][t] takes prototype point L (T - 1 - t) + p; every phase is scaled to the sum 2^shift, rounded
    to nearest, and the rounding's remainder goes to its largest tap, so that sum_t g[p][t] == 2^shift exactly (DC in is DC out);
    shift is the largest value <= 14 at which every phase has sum |g| <= 32767."""
    L, M, T = int(L), int(M), int(T)
    if L < 1 or M < 1 or T < 1:
        raise ValueError("need L, M, T >= 1")
    h = resample_prototype(L, M, T, cutoff)
    for shift in range(14, -1, -1):
        g = np.zeros((L, T), dtype=np.int64)
        ok = True
        for p in range(L):
            a = [h[L * (T - 1 - t) + p] for t in range(T)]
            s = 0.0
            for v in a:
                s += v
            if not s > 0:
                raise ValueError("phase %d of the prototype has no positive sum: more taps per phase or a lower cutoff" % p)
            scale = math.ldexp(1.0, shift) / s
            row = [int(math.floor(v * scale + 0.5)) for v in a]
            big = max(range(T), key=lambda t: (row[t], -t))          # the first of the largest taps
            row[big] += (1 << shift) - sum(row)
            g[p] = row
            if sum(abs(v) for v in row) > 32767:
                ok = False
                break
        if ok:
            return g.astype(np.int16), shift
    raise ValueError("no shift keeps every phase's sum |g| <= 32767")


class Resampler(RowProcessor):
    """`taps` is int16 [L, T] (phase-major), `n_rows` the rows of the bank whose output it takes (n_streams x stations or channels),
    `width` 1 or 2 int16 per sample.  run_batch takes [n_rows, n_in, width] (or [n_rows, n_in] at width 1) on the host;
    run_device takes a bank's d_out as it stands, with the bank's out_cap as in_cap."""
    _prefix = "resample"

    def __init__(self, taps, L, M, shift, n_rows=1, width=1, device_id=-1):
        self.L, self.M, self.shift, self.n_rows, self.width = int(L), int(M), int(shift), int(n_rows), int(width)
        self.taps = np.ascontiguousarray(taps, dtype=np.int16)
        if self.L < 1 or self.taps.size % self.L:
            raise ValueError("taps must be [L, T]")
        self.T = self.taps.size // self.L
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_rows, device_id, 0)
        check(lib().fmd_resample_new(self.taps.ctypes.data_as(C.POINTER(C.c_int16)), self.L, self.M, self.T, self.shift, self.width,
                                     C.byref(dev), C.byref(self._h)))

    def out_cap(self, n_in):
        return int(lib().fmd_resample_out_cap(self.L, self.M, n_in))


def bank_rate(bank, capture_rate=None):
    """The output rate of a bank as a Fraction: capture_rate over the product of its decimations.  A bank that was not given its
    capture rate (the channelizers) needs `capture_rate`."""
    cap = getattr(bank, "capture_rate", None) if capture_rate is None else capture_rate
    if cap is None:
        raise ValueError("this bank does not know its capture rate: pass capture_rate")
    d = bank.decim if hasattr(bank, "decim") else bank.hop
    for name in ("audio_decim", "chan_decim", "out_decim"):
        if hasattr(bank, name):
            d *= getattr(bank, name)
            break
    return Fraction(int(cap), int(d))


def fixed_rate(bank, rate_out, taps_per_phase=32, capture_rate=None, device_id=-1):
    """A Resampler matched to `bank`: its rows (n_streams x stations or selected channels), its width and its output rate, to
    `rate_out` Hz with resample_taps(L, M, taps_per_phase)."""
    L, M = resample_ratio(bank_rate(bank, capture_rate), rate_out)
    g, shift = resample_taps(L, M, taps_per_phase)
    rows, width = bank_rows(bank)
    return Resampler(g, L, M, shift, n_rows=rows, width=width, device_id=device_id)
