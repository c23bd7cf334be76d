"""Test-side definition of the channelizer (include/fmd.h, "channelizer"): the station bank's steps 1 - 5 in numpy int64
(tests/stations_ref.py), returning y per call with the filter history and the output counter m carried.  Independent of the
library; `oracle_chain` runs the oracle's fm_demod + low_pass_real over it, which is the station bank."""
import ctypes as C

import numpy as np

import stations_ref as sr
from stations_ref import TooShort  # noqa: F401  (re-exported: a call that completes no output)


class ChannelizerRef:
    """One input stream, K stations; feed() mirrors one fmd_channelizer call of that stream and returns int64 [K, n, 2] (yr, yi).
    `z` selects how the filter outputs are formed: sr.z_direct (gather matrices) or sr.z_corr (production-size calls)."""

    def __init__(self, taps, decim, incs, shift, z=None):
        self.h = np.asarray(taps, dtype=np.int64)
        self.T, self.D, self.shift = self.h.size, int(decim), int(shift)
        self.incs = [int(i) for i in incs]
        w = [sr.complex_taps(self.h, i) for i in self.incs]
        self.wr = np.stack([a for a, _ in w])                # [K, T]
        self.wi = np.stack([b for _, b in w])
        self.z = z or sr.z_direct
        self.reset()

    def reset(self):
        self.cr = np.zeros(0, dtype=np.int64)
        self.ci = np.zeros(0, dtype=np.int64)
        self.base = 0                                        # global index of cr[0]
        self.pos = 0                                         # samples fed so far
        self.m_next = 0                                      # outputs produced so far

    def outputs_after(self, nsamples):
        end = self.pos + nsamples
        return (end - self.T) // self.D + 1 if end >= self.T else 0

    def feed(self, buf):
        b = np.asarray(buf, dtype=np.uint8)
        assert b.size % 8 == 0
        m1 = self.outputs_after(b.size // 2)
        ms = np.arange(self.m_next, max(m1, self.m_next), dtype=np.int64)
        if ms.size < 1:
            raise TooShort()                                 # nothing changes
        cr = np.concatenate([self.cr, b[0::2].astype(np.int64) - 127])
        ci = np.concatenate([self.ci, b[1::2].astype(np.int64) - 127])
        zr, zi = self.z(cr, ci, self.wr, self.wi, self.D, self.D * int(ms[0]) - self.base, ms.size)
        y = np.empty((len(self.incs), ms.size, 2), dtype=np.int64)
        sh = 14 + self.shift
        for k, inc in enumerate(self.incs):
            psi = (ms.astype(np.uint64) * np.uint64((self.D * inc) & 0xFFFFFFFF)) & 0xFFFFFFFF
            Cq, Sq = sr.cosq(psi), sr.sinq(psi)
            y[k, :, 0] = (zr[:, k] * Cq + zi[:, k] * Sq) >> sh
            y[k, :, 1] = (zi[:, k] * Cq - zr[:, k] * Sq) >> sh
        self.m_next = int(ms[-1]) + 1
        keep = min(self.D * self.m_next - self.base, cr.size)  # samples before the next window are never read again
        self.cr, self.ci = cr[keep:], ci[keep:]
        self.base += keep
        self.pos += b.size // 2
        return y


def oracle_chain(oracle, demods, y):
    """The oracle's fm_demod (simple_fm.rs:355-367) + low_pass_real (:408-426) over one call's y [K, n, 2], one Demod per
    station (state carried in `demods`): the station bank's audio of that call."""
    import oracle_lib
    outs = []
    for k, d in enumerate(demods):
        yk = np.ascontiguousarray(y[k].astype(np.int32))
        n = yk.shape[0]
        dem = np.empty(n, dtype=np.int16)
        oracle.lib.fmo_fm_demod(C.byref(d), yk.ctypes.data_as(C.POINTER(oracle_lib.Cplx)), n, dem.ctypes.data_as(C.POINTER(C.c_int16)))
        res = np.empty(n, dtype=np.int16)
        m = oracle.lib.fmo_low_pass_real(C.byref(d), dem.ctypes.data_as(C.POINTER(C.c_int16)), n, res.ctypes.data_as(C.POINTER(C.c_int16)))
        assert m >= 0
        outs.append(res[:m].copy())
    return outs


def oracle_low_pass_complex(oracle, d, buf):
    """The oracle's center + buf_to_complex + low_pass_complex (simple_fm.rs:258-261, 337-352) of one call, rotate_90 NOT applied:
    int64 [n, 2]."""
    import oracle_lib
    b = np.ascontiguousarray(buf, dtype=np.uint8)
    c = (b.astype(np.int32) - 127).reshape(-1, 2)
    cp = np.ascontiguousarray(c)
    out = (oracle_lib.Cplx * (c.shape[0] + 1))()
    n = oracle.lib.fmo_low_pass_complex(C.byref(d), cp.ctypes.data_as(C.POINTER(oracle_lib.Cplx)), c.shape[0], out)
    return np.array([[out[i].re, out[i].im] for i in range(n)], dtype=np.int64).reshape(-1, 2)
