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


def z_direct(cr, ci, wr, wi, D, first, M):
    """z[i][k] = sum_t W[k][t] c[first + D i + t] for i < M: [M, T] gather matrices times the tap matrix, int64.  Memory grows as
    M T: the small shapes only."""
    idx = (first + D * np.arange(M, dtype=np.int64))[:, None] + np.arange(wr.shape[1])[None, :]
    xr, xi = cr[idx], ci[idx]                                # [M, T]
    return xr @ wr.T - xi @ wi.T, xr @ wi.T + xi @ wr.T       # [M, K], exact in int64


def z_corr(cr, ci, wr, wi, D, first, M):
    """z_direct by exact integer correlation, one polyphase branch at a time: taps t = D a + p meet samples D (i + a) + p, so
    branch p is np.correlate of the samples c[first + p :: D] with the taps W[p :: D] -- only the M outputs are formed, memory
    grows as the input."""
    T = wr.shape[1]
    cr = np.asarray(cr[first:first + D * (M - 1) + T], dtype=np.int64)
    ci = np.asarray(ci[first:first + D * (M - 1) + T], dtype=np.int64)
    zr = np.zeros((M, wr.shape[0]), dtype=np.int64)
    zi = np.zeros((M, wr.shape[0]), dtype=np.int64)
    for p in range(min(D, T)):
        xr, xi = cr[p::D], ci[p::D]
        for k in range(wr.shape[0]):
            a, b = wr[k, p::D], wi[k, p::D]
            n = M + a.size - 1
            zr[:, k] += np.correlate(xr[:n], a, "valid") - np.correlate(xi[:n], b, "valid")
            zi[:, k] += np.correlate(xr[:n], b, "valid") + np.correlate(xi[:n], a, "valid")
    return zr, zi


class StationsRef:
    """One input stream, K stations; feed() mirrors one fmd_stations call of that stream.  `z` selects how the filter outputs
    are formed: z_direct (gather matrices) or z_corr (correlation, for production-size calls); both are exact."""

    def __init__(self, oracle, taps, decim, incs, rate_out, rate_resample, shift, z=None):
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
        self.z = z or z_direct

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
        zr, zi = self.z(cr, ci, self.wr, self.wi, self.D, self.D * int(ms[0]) - self.base, ms.size)
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
        keep = min(self.D * self.m_next - self.base, cr.size)  # samples before the next window are never read again (with
                                                               # n_taps < decim that window can start past the call's end)
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
