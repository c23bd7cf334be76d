"""Host-side wrapper of the tone squelch (include/fmd.h, fmd_tonesq_*): every int16 row a bank leaves on the device is correlated,
block by block, against a table of windowed reference tones (CTCSS), and gated by the tone the blocks before decided on -- mono
audio at width 1, interleaved (L, R) whose mean is correlated at width 2.  Exact in integers; the output and every report do not
depend on how the stream is cut."""
import ctypes as C
import math

import numpy as np

from ._ffi import DeviceConfig, RowProcessor, bank_rows, check, lib

# the 38 standard CTCSS tones, Hz
CTCSS_TONES = (67.0, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3,
               131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 162.2, 167.9, 173.8, 179.9, 186.2, 192.8, 203.5, 210.7, 218.1, 225.7, 233.6,
               241.8, 250.3)


class ToneSquelchConfig(C.Structure):
    """struct fmd_tonesq_config"""
    _fields_ = [("block", C.c_uint32), ("guard", C.c_uint32), ("dom_shift", C.c_uint32), ("confirm", C.c_uint32), ("hang", C.c_uint32),
                ("ramp", C.c_uint32), ("min_power", C.c_uint64), ("accept", C.c_uint64)]


def tone_table(rate, freqs, block):
    """int16 [len(freqs), block, 2]: (c_f[r], s_f[r]) = rint(1023 w[r] cos(2 pi f r / rate)), rint(-1023 w[r] sin(2 pi f r / rate))
    under the Hann window w[r] = 0.5 - 0.5 cos(2 pi (r + 0.5) / block).  Scalar libm arithmetic in one fixed order, as fm::tone_table
    (csrc/demod.hpp) does it; every |entry| <= 1023."""
    rate, P = float(rate), int(block)
    if not rate > 0 or P < 1:
        raise ValueError("need rate > 0 and block >= 1")
    tab = np.zeros((len(freqs), P, 2), dtype=np.int16)
    for k, f in enumerate(freqs):
        f = float(f)
        for r in range(P):
            w = 0.5 - 0.5 * math.cos(2 * math.pi * (r + 0.5) / P)
            a = 2 * math.pi * f * r / rate
            tab[k, r, 0] = round(1023 * w * math.cos(a))     # (round(): to nearest, ties to even, as rint)
            tab[k, r, 1] = round(-1023 * w * math.sin(a))
    return tab


def accept_mask(tones, accept):
    """The u64 `accept` of the tones of `tones` whose frequency is listed in `accept` (Hz, as in `tones`); None: all of them."""
    if accept is None:
        return (1 << len(tones)) - 1
    mask = 0
    for hz in accept:
        if hz not in tones:
            raise ValueError("%r is not one of the table's tones" % (hz,))
        mask |= 1 << list(tones).index(hz)
    return mask


class ToneSquelch(RowProcessor):
    """`table` is int16 [n_tones, block, 2] (tone_table), `n_rows` the rows of the bank whose output it takes, `width` 1 or 2 int16
    per sample.  A block's tone f* is a hit when its power W reaches `min_power` and W >> `dom_shift` is at least the power of every
    tone more than `guard` tones away; `confirm` equal hits in a row select the tone, which is held `hang` blocks; the gate is open
    while the selected tone's bit of `accept` is set and moves over the first `ramp` samples of a block.  n_out = n_in: run_batch
    takes [n_rows, n_in, width] (or [n_rows, n_in] at width 1) on the host; run_device takes a bank's d_out as it stands, with the
    bank's out_cap as in_cap, and may write in place (d_out == d_in with out_cap == in_cap)."""
    _prefix = "tonesq"

    def __init__(self, table, n_rows=1, width=1, accept=(1 << 64) - 1, guard=1, dom_shift=3, min_power=20_000_000, confirm=2, hang=2,
                 ramp=64, device_id=-1):
        self.table = np.ascontiguousarray(table, dtype=np.int16)
        if self.table.ndim != 3 or self.table.shape[2] != 2:
            raise ValueError("table must be [n_tones, block, 2]")
        self.n_tones, self.block = int(self.table.shape[0]), int(self.table.shape[1])
        self.n_rows, self.width = int(n_rows), int(width)
        self.guard, self.dom_shift, self.confirm, self.hang, self.ramp = int(guard), int(dom_shift), int(confirm), int(hang), int(ramp)
        self.min_power, self.accept = int(min_power), int(accept)
        for name in ("guard", "dom_shift", "confirm", "hang", "ramp", "n_rows", "width"):
            if not 0 <= getattr(self, name) < 1 << 32:
                raise ValueError("%s out of range" % name)
        for name in ("min_power", "accept"):
            if not 0 <= getattr(self, name) < 1 << 64:
                raise ValueError("%s out of range" % name)
        self._h = C.c_void_p()
        cfg = ToneSquelchConfig(self.block, self.guard, self.dom_shift, self.confirm, self.hang, self.ramp, self.min_power, self.accept)
        dev = DeviceConfig(self.n_rows, device_id, 0)
        check(lib().fmd_tonesq_new(C.byref(cfg), self.table.ctypes.data_as(C.POINTER(C.c_int16)), self.n_tones, self.width, C.byref(dev),
                                   C.byref(self._h)))

    def out_cap(self, n_in):
        return int(lib().fmd_tonesq_out_cap(n_in))

    def status(self):
        """(tone int32 [n_rows], power uint64 [n_rows], open bool [n_rows]) after the last completed block: the selected tone's index
        (-1: none), W of the block's strongest tone, and whether the gate opens; -1 / 0 / False before the first block.
        Synchronises."""
        tone, power = np.zeros(self.n_rows, np.int32), np.zeros(self.n_rows, np.uint64)
        gate = np.zeros(self.n_rows, np.uint8)
        check(self._fn("status")(self._h, tone.ctypes.data_as(C.POINTER(C.c_int32)), power.ctypes.data_as(C.POINTER(C.c_uint64)),
                                 gate.ctypes.data_as(C.POINTER(C.c_uint8))))
        return tone, power, gate.astype(bool)


def tone_squelched(bank, rate, accept=None, tones=CTCSS_TONES, block=4096, guard=1, dom_shift=3, min_power=20_000_000, confirm=2, hang=2,
                   ramp=64, device_id=-1):
    """A ToneSquelch matched to `bank`: its rows (n_streams x stations or selected channels) and its width, over the tones `tones`
    (Hz) at the bank's output rate `rate`; `accept` lists the tones (Hz) that open the gate, None for every one of them."""
    rows, width = bank_rows(bank)
    return ToneSquelch(tone_table(rate, tones, block), n_rows=rows, width=width, accept=accept_mask(tones, accept), guard=guard,
                       dom_shift=dom_shift, min_power=min_power, confirm=confirm, hang=hang, ramp=ramp, device_id=device_id)
