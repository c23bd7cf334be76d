"""Host-side wrapper of the code squelch (include/fmd.h, fmd_dcs_*): every int16 row a bank leaves on the device is searched for one
of a table of 23-bit words (DCS, the digital-coded squelch: a Golay word at 134.4 bit/s under the voice band) and gated by the code
the blocks before decided on -- mono audio at width 1, interleaved (L, R) whose mean is searched at width 2.  Exact in integers; the
output and every report do not depend on how the stream is cut."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

from ._ffi import DeviceConfig, RowProcessor, bank_rows, check, lib

# the 104 standard DCS codes (written in octal)
DCS_CODES = (
    0o023, 0o025, 0o026, 0o031, 0o032, 0o036, 0o043, 0o047, 0o051, 0o053, 0o054, 0o065, 0o071, 0o072, 0o073, 0o074,
    0o114, 0o115, 0o116, 0o122, 0o125, 0o131, 0o132, 0o134, 0o143, 0o145, 0o152, 0o155, 0o156, 0o162, 0o165, 0o172, 0o174,
    0o205, 0o212, 0o223, 0o225, 0o226, 0o243, 0o244, 0o245, 0o246, 0o251, 0o252, 0o255, 0o261, 0o263, 0o265, 0o266, 0o271, 0o274,
    0o306, 0o311, 0o315, 0o325, 0o331, 0o332, 0o343, 0o346, 0o351, 0o356, 0o364, 0o365, 0o371,
    0o411, 0o412, 0o413, 0o423, 0o431, 0o432, 0o445, 0o446, 0o452, 0o454, 0o455, 0o462, 0o464, 0o465, 0o466,
    0o503, 0o506, 0o516, 0o523, 0o526, 0o532, 0o546, 0o565,
    0o606, 0o612, 0o624, 0o627, 0o631, 0o632, 0o654, 0o662, 0o664,
    0o703, 0o712, 0o723, 0o731, 0o732, 0o734, 0o743, 0o754)

DCS_BAUD = 134.4
DCS_POLY = 0xC75                                             # x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1, bit i = coefficient of x^i


class CodeSquelchConfig(C.Structure):
    """struct fmd_dcs_config"""
    _fields_ = [("block", C.c_uint32), ("box", C.c_uint32), ("n_taps", C.c_uint32), ("lp", C.c_int16 * 64), ("lshift", C.c_uint32),
                ("tap", C.c_uint32 * 23), ("tol", C.c_uint32), ("min_hits", C.c_uint32), ("confirm", C.c_uint32), ("hang", C.c_uint32),
                ("ramp", C.c_uint32), ("accept", C.c_uint64 * 2)]


def dcs_remainder(c):
    """c(x) mod the DCS polynomial, c below 2^23."""
    for i in range(22, 10, -1):
        if (c >> i) & 1:
            c ^= DCS_POLY << (i - 11)
    return c


def dcs_codeword(code):
    """The 23-bit word c = (p << 12) | 0x800 | code of a 9-bit code, bit 0 sent first: the 11 parity bits p make c(x) divisible by
    the DCS polynomial.  dcs_codeword(0o023) = 0x763813."""
    code = int(code)
    if not 0 <= code < 512:
        raise ValueError("need a code below 0o1000")
    d = 0x800 | code
    for p in range(2048):
        if dcs_remainder((p << 12) | d) == 0:
            return (p << 12) | d
    raise AssertionError("no parity")                        # (x^12 is invertible modulo the polynomial: there is exactly one)


def dcs_word(code, inverted=False):
    """The table word of a code for CodeSquelch: the codeword, complemented if `inverted`, in the order of arrival -- bit 0 of the
    codeword is sent first, and table bit j is the bit tap[j] back from the newest, so table bit j = bit 22 - j of the codeword.
    dcs_word(0o023) = 0x640E37."""
    c = dcs_codeword(code)
    if inverted:
        c ^= 0x7FFFFF
    w = 0
    for j in range(23):
        w |= ((c >> (22 - j)) & 1) << j
    return w


Design = namedtuple("Design", "block box lp lshift tap tol min_hits confirm hang ramp")


def dcs_design(rate):
    """The parameters of a CodeSquelch for DCS at the sample rate `rate`: `box` the power of two that puts rate / box nearest 1500 Hz;
    `lp` a Hamming-windowed sinc of 32 taps at 200 Hz, scaled to peak 1023; lshift = ceil(log2(sum |lp|)); tap[j] = floor(j rate /
    (134.4 box) + 0.5); block = two whole word periods, up to a multiple of 64; tol 1, min_hits 8, confirm 1, hang 1, ramp 64.
    Scalar libm arithmetic in one fixed order, as fm::dcs_design (csrc/demod.hpp) does it."""
    rate = float(rate)
    if not rate > 0:
        raise ValueError("need rate > 0")
    box, best = 1, abs(rate - 1500.0)
    for lg in range(1, 7):
        d = abs(rate / float(1 << lg) - 1500.0)
        if d < best:
            box, best = 1 << lg, d
    T = 32
    fc = 200.0 * float(box) / rate
    h = []
    for t in range(T):
        x = 2 * math.pi * fc * (float(t) - float(T - 1) / 2.0)
        s = 1.0 if x == 0 else math.sin(x) / x
        h.append(s * (0.54 - 0.46 * math.cos(2 * math.pi * float(t) / float(T - 1))))
    peak = max(h)
    lp = [int(round(1023.0 * v / peak)) for v in h]          # (round(): to nearest, ties to even, as rint)
    mag = sum(abs(v) for v in lp)
    lshift = 0
    while (1 << lshift) < mag:
        lshift += 1
    tap = [int(math.floor(float(j) * rate / (DCS_BAUD * float(box)) + 0.5)) for j in range(23)]
    block = 64 * int(math.ceil(46.0 * rate / (DCS_BAUD * 64.0)))
    if tap[22] > 511 or block > 32768:
        raise ValueError("rate out of range")
    return Design(block, box, np.array(lp, np.int16), lshift, np.array(tap, np.uint32), 1, 8, 1, 1, 64)


def accept_mask(codes, accept):
    """The 128-bit `accept` (a Python int) of the codes of `codes` listed in `accept`; None: all of them."""
    if accept is None:
        return (1 << len(codes)) - 1
    mask = 0
    for code in accept:
        if code not in codes:
            raise ValueError("%r is not one of the table's codes" % (code,))
        mask |= 1 << list(codes).index(code)
    return mask


class CodeSquelch(RowProcessor):
    """`words` is the table of 23-bit words (dcs_word), `n_rows` the rows of the bank whose output it takes, `width` 1 or 2 int16
    per sample.  Every `box` samples give one decimated sample, low-passed by `lp` (>> `lshift`); every decimated sample forms a word
    from the 23 samples `tap[j]` back, sliced at their mean, and is a hit on the nearest table word if at most `tol` bits differ.  A
    block of `block` samples is a hit on its most-hit word if that has `min_hits`; `confirm` equal hits in a row select the code,
    which is held `hang` blocks; the gate is open while the selected code's bit of `accept` (an int of up to 128 bits) is set and
    moves over the first `ramp` samples of a block.  n_out = n_in: run_batch takes [n_rows, n_in, width] (or [n_rows, n_in] at width
    1) on the host; run_device takes a bank's d_out as it stands, with the bank's out_cap as in_cap, and may write in place."""
    _prefix = "dcs"

    def __init__(self, words, block, box, lp, lshift, tap, n_rows=1, width=1, accept=(1 << 128) - 1, tol=1, min_hits=8, confirm=1,
                 hang=1, ramp=64, device_id=-1):
        self.words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        self.lp = np.ascontiguousarray(lp, dtype=np.int16).reshape(-1)
        self.tap = np.ascontiguousarray(tap, dtype=np.uint32).reshape(-1)
        if self.tap.size != 23:
            raise ValueError("tap must have 23 entries")
        if self.lp.size > 64:
            raise ValueError("lp must have at most 64 entries")
        self.n_words, self.n_taps = int(self.words.size), int(self.lp.size)
        self.block, self.box, self.lshift = int(block), int(box), int(lshift)
        self.n_rows, self.width = int(n_rows), int(width)
        self.tol, self.min_hits, self.confirm, self.hang, self.ramp = int(tol), int(min_hits), int(confirm), int(hang), int(ramp)
        self.accept = int(accept)
        for name in ("block", "box", "lshift", "tol", "min_hits", "confirm", "hang", "ramp", "n_rows", "width"):
            if not 0 <= getattr(self, name) < 1 << 32:
                raise ValueError("%s out of range" % name)
        if not 0 <= self.accept < 1 << 128:
            raise ValueError("accept out of range")
        self._h = C.c_void_p()
        cfg = CodeSquelchConfig()
        cfg.block, cfg.box, cfg.n_taps, cfg.lshift = self.block, self.box, self.n_taps, self.lshift
        cfg.lp[:self.n_taps] = self.lp.tolist()
        cfg.tap[:] = self.tap.tolist()
        cfg.tol, cfg.min_hits, cfg.confirm, cfg.hang, cfg.ramp = self.tol, self.min_hits, self.confirm, self.hang, self.ramp
        cfg.accept[0], cfg.accept[1] = self.accept & ((1 << 64) - 1), self.accept >> 64
        dev = DeviceConfig(self.n_rows, device_id, 0)
        check(lib().fmd_dcs_new(C.byref(cfg), self.words.ctypes.data_as(C.POINTER(C.c_uint32)), self.n_words, self.width, C.byref(dev),
                                C.byref(self._h)))

    def out_cap(self, n_in):
        return int(lib().fmd_dcs_out_cap(n_in))

    def status(self):
        """(code int32 [n_rows], hits uint32 [n_rows], open bool [n_rows]) after the last completed block: the selected word's index
        (-1: none), the hits of the block's most-hit word, and whether the gate opens; -1 / 0 / False before the first block.
        Synchronises."""
        code, hits = np.zeros(self.n_rows, np.int32), np.zeros(self.n_rows, np.uint32)
        gate = np.zeros(self.n_rows, np.uint8)
        check(self._fn("status")(self._h, code.ctypes.data_as(C.POINTER(C.c_int32)), hits.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 gate.ctypes.data_as(C.POINTER(C.c_uint8))))
        return code, hits, gate.astype(bool)


def code_squelched(bank, rate, accept=None, codes=DCS_CODES, device_id=-1, **overrides):
    """A CodeSquelch matched to `bank`: its rows (n_streams x stations or selected channels) and its width, over the words of
    `codes` with dcs_design(rate) at the bank's output rate `rate`; `accept` lists the codes that open the gate, None for every one
    of them.  `overrides`: fields of the design (tol, min_hits, confirm, hang, ramp, block) to replace.  A station whose
    discriminator has the other sign is reported under its code's inverse partner (023 as 047)."""
    rows, width = bank_rows(bank)
    d = dcs_design(rate)._replace(**overrides)
    return CodeSquelch([dcs_word(c) for c in codes], d.block, d.box, d.lp, d.lshift, d.tap, n_rows=rows, width=width,
                       accept=accept_mask(codes, accept), tol=d.tol, min_hits=d.min_hits, confirm=d.confirm, hang=d.hang, ramp=d.ramp,
                       device_id=device_id)
