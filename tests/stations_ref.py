"""Test-side definition of the station bank (include/fmd.h, "station bank"): steps 1 - 5 in numpy int64, then the oracle's own
fm_demod + low_pass_real (oracle/fm_oracle.c, simple_fm.rs:355-367, 408-426) per station.  Independent of the library."""
import ctypes as C

import numpy as np


class TooShort(Exception):
    pass


def nco_table():
    return np.round(16384.0 * np.cos(2.0 * np.pi * np.arange(1024) / 1024.0)).astype(np.int64)


TAB = nco_table()


def cosq(phi):
    return TAB[(np.asarray(phi, dtype=np.uint64) & 0xFFFFFFFF) >> 22]


def sinq(phi):
    return TAB[(((np.asarray(phi, dtype=np.uint64) & 0xFFFFFFFF) >> 22).astype(np.int64) - 256) & 1023]


def complex_taps(h, inc):
    h = np.asarray(h, dtype=np.int64)
    phi = (np.arange(h.size, dtype=np.uint64) * np.uint64(inc)) & 0xFFFFFFFF
    return (h * cosq(phi) + 8192) >> 14, (-h * sinq(phi) + 8192) >> 14


def max_gain(h, incs):
    g = 0
    for inc in np.asarray(incs).ravel():
        wr, wi = complex_taps(h, int(inc))
        g = max(g, int(np.abs(wr).sum() + np.abs(wi).sum()))
    return g


def phase_inc(offset, rate):
    """floor((offset * 2^32 + floor(rate / 2)) / rate) mod 2^32 in exact integers."""
    return ((offset * (1 << 32) + rate // 2) // rate) % (1 << 32)


def rot90(b):
    """rotate_90 (simple_fm.rs:276-299) on a byte buffer, numpy."""
    b = np.array(b, dtype=np.uint8).reshape(-1, 8).copy()
    out = b.copy()
    out[:, 2], out[:, 3] = 255 - b[:, 3], b[:, 2]
    out[:, 4], out[:, 5] = 255 - b[:, 4], 255 - b[:, 5]
    out[:, 6], out[:, 7] = b[:, 7], 255 - b[:, 6]
    return out.ravel()


class StationsRef:
    """One input stream, K stations; feed() mirrors one fmd_stations call of that stream."""

    def __init__(self, oracle, taps, decim, incs, rate_out, rate_resample, shift):
        self.o = oracle
        self.h = np.asarray(taps, dtype=np.int64)
        self.T, self.D, self.shift = self.h.size, int(decim), int(shift)
        self.incs = [int(i) for i in incs]
        w = [complex_taps(self.h, i) for i in self.incs]
        self.wr = np.stack([a for a, _ in w])                # [K, T]
        self.wi = np.stack([b for _, b in w])
        self.cfg = oracle.config(self.D, rate_out, rate_resample)
        self.demods = [oracle.new(self.cfg) for _ in self.incs]
        self.cr = np.zeros(0, dtype=np.int64)
        self.ci = np.zeros(0, dtype=np.int64)
        self.base = 0                                        # global index of cr[0]
        self.pos = 0                                         # samples fed so far
        self.m_next = 0

    def feed(self, buf):
        b = np.asarray(buf, dtype=np.uint8)
        assert b.size % 8 == 0
        cr = np.concatenate([self.cr, b[0::2].astype(np.int64) - 127])
        ci = np.concatenate([self.ci, b[1::2].astype(np.int64) - 127])
        end = self.pos + b.size // 2
        m1 = (end - self.T) // self.D + 1 if end >= self.T else 0
        ms = np.arange(self.m_next, max(m1, self.m_next), dtype=np.int64)
        if ms.size < 2:
            raise TooShort()
        idx = (self.D * ms - self.base)[:, None] + np.arange(self.T)[None, :]
        xr, xi = cr[idx], ci[idx]                            # [M, T]
        zr = xr @ self.wr.T - xi @ self.wi.T                 # [M, K], exact in int64
        zi = xr @ self.wi.T + xi @ self.wr.T
        outs = []
        for k, inc in enumerate(self.incs):
            psi = (ms.astype(np.uint64) * np.uint64((self.D * inc) & 0xFFFFFFFF)) & 0xFFFFFFFF
            Cq, Sq = cosq(psi), sinq(psi)
            sh = 14 + self.shift
            yr = (zr[:, k] * Cq + zi[:, k] * Sq) >> sh
            yi = (zi[:, k] * Cq - zr[:, k] * Sq) >> sh
            y = np.ascontiguousarray(np.stack([yr, yi], axis=1).astype(np.int32))
            lp = y.ctypes.data_as(C.POINTER(self.o_cplx()))
            d = self.demods[k]
            dem = np.empty(ms.size, dtype=np.int16)
            self.o.lib.fmo_fm_demod(C.byref(d), lp, ms.size, dem.ctypes.data_as(C.POINTER(C.c_int16)))
            res = np.empty(ms.size, dtype=np.int16)
            n = self.o.lib.fmo_low_pass_real(C.byref(d), dem.ctypes.data_as(C.POINTER(C.c_int16)), ms.size,
                                             res.ctypes.data_as(C.POINTER(C.c_int16)))
            assert n >= 0
            outs.append(res[:n].copy())
        self.m_next = int(ms[-1]) + 1
        keep = self.D * self.m_next - self.base               # samples before the next window are never read again
        self.cr, self.ci = cr[keep:], ci[keep:]
        self.base += keep
        self.pos = end
        return outs

    def state(self, k):
        return self.o.state_of(self.demods[k])

    @staticmethod
    def o_cplx():
        import oracle_lib
        return oracle_lib.Cplx
