"""Host-side wrapper of the packet demodulator (include/fmd.h): the tone-pair demodulator fmd_afsk_* -- every mono int16 row a bank
leaves on the device correlated against a mark and a space tone, one signed soft decision per `stride` samples -- and the host's
AX.25 frame decoder fmd_ax25_decoder_* (clock recovery, NRZI, HDLC, FCS), one per row: 1200 baud AFSK packet (APRS) out of any bank's
NFM rows.  Both are exact in integers and independent of how the stream is cut."""
import ctypes as C
import math

import numpy as np

from ._ffi import DeviceConfig, RowProcessor, bank_rows, check, lib


class Ax25Frame(C.Structure):
    """struct fmd_ax25_frame"""
    _fields_ = [("data", C.c_uint8 * 512), ("len", C.c_uint32), ("end_sample", C.c_uint64)]


class Ax25Info(C.Structure):
    """struct fmd_ax25_info"""
    _fields_ = [("frames_ok", C.c_uint64), ("bad_fcs", C.c_uint64), ("aborts", C.c_uint64), ("in_frame", C.c_int)]


def afsk_stride(taps):
    """The default stride of a window of `taps` samples: a fifth of a bit, at least 1 and at most 32."""
    return max(1, min(32, int(taps), (2 * int(taps) + 5) // 10))


def afsk_table(rate, baud=1200, mark=1200, space=2200, taps=None):
    """(table int16 [4, T], pre_shift, out_shift) of an AfskDemod: rectangular windows one bit long, T = taps or round(rate / baud),
    rows mark-cos, mark-sin, space-cos, space-sin = rint(1023 cos(2 pi f t / rate)), rint(-1023 sin(2 pi f t / rate)).  pre_shift is
    8; out_shift is the smallest at which a full window of either tone at amplitude 1024, x[t] = rint(1024 cos(2 pi f t / rate)),
    stays inside int16.  Scalar libm arithmetic in one fixed order, as fm::afsk_table (csrc/demod.hpp) does it."""
    rate, baud = float(rate), float(baud)
    if not rate > 0 or not baud > 0:
        raise ValueError("need rate > 0 and baud > 0")
    T = int(taps) if taps is not None else int(round(rate / baud))
    if not 2 <= T <= 64:
        raise ValueError("need 2 <= taps <= 64")
    tab = np.zeros((4, T), dtype=np.int16)
    for k, f in enumerate((float(mark), float(space))):
        for t in range(T):
            a = 2 * math.pi * f * t / rate
            tab[2 * k, t] = round(1023 * math.cos(a))        # (round(): to nearest, ties to even, as rint)
            tab[2 * k + 1, t] = round(-1023 * math.sin(a))
    pre_shift, peak = 8, 0
    for f in (float(mark), float(space)):
        x = [round(1024 * math.cos(2 * math.pi * f * t / rate)) for t in range(T)]
        A = [sum(int(tab[q, t]) * x[t] for t in range(T)) >> pre_shift for q in range(4)]
        peak = max(peak, abs(A[0] * A[0] + A[1] * A[1] - A[2] * A[2] - A[3] * A[3]))
    out_shift = 0
    while (peak >> out_shift) > 32767:
        out_shift += 1
    return tab, pre_shift, out_shift


class AfskDemod(RowProcessor):
    """`table` is int16 [4, T] (afsk_table), `stride` the samples between two soft decisions (1 <= stride <= min(T, 32)), `n_rows`
    the rows of the bank whose output it takes; width is 1.  Output n = sat16((E_mark - E_space) >> out_shift) of the window that
    starts at sample n * stride, positive for mark; it exists once the window's last sample has arrived, and a call that completes
    none is refused (FMD_ERR_TOO_SHORT) and takes nothing.  run_batch takes [n_rows, n_in] on the host; run_device takes a bank's
    d_out as it stands, with the bank's out_cap as in_cap.  `rate` and `baud` (optional) are what decode_rows builds its decoders
    from."""
    _prefix = "afsk"

    def __init__(self, table, stride, pre_shift=8, out_shift=12, n_rows=1, width=1, device_id=-1, rate=None, baud=1200):
        self.table = np.ascontiguousarray(table, dtype=np.int16)
        if self.table.ndim != 2 or self.table.shape[0] != 4:
            raise ValueError("table must be [4, T]")
        self.taps, self.stride = int(self.table.shape[1]), int(stride)
        self.pre_shift, self.out_shift, self.n_rows, self.width = int(pre_shift), int(out_shift), int(n_rows), int(width)
        self.rate, self.baud = rate, baud
        for name in ("stride", "pre_shift", "out_shift", "n_rows", "width"):
            if not 0 <= getattr(self, name) < 1 << 32:
                raise ValueError("%s out of range" % name)
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_rows, device_id, 0)
        check(lib().fmd_afsk_new(self.table.ctypes.data_as(C.POINTER(C.c_int16)), self.taps, self.stride, self.pre_shift, self.out_shift,
                                 self.width, C.byref(dev), C.byref(self._h)))

    def out_cap(self, n_in):
        return int(lib().fmd_afsk_out_cap(self.stride, n_in))


class Ax25Decoder:
    """The host decoder of one row: push() takes the int16 soft decisions of an AfskDemod at rate_num / rate_den per second (the
    audio rate over the stride) and returns the frames completed since, as dicts {"data": bytes without the FCS, "end_sample"};
    info() the counters."""

    def __init__(self, rate_num, rate_den=1, baud=1200):
        self._h = C.c_void_p()
        check(lib().fmd_ax25_decoder_new(int(rate_num), int(rate_den), int(baud), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().fmd_ax25_decoder_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(lib().fmd_ax25_decoder_reset(self._h))

    def push(self, soft):
        soft = np.ascontiguousarray(soft, dtype=np.int16)
        if soft.ndim != 1:
            raise ValueError("soft must be [n]")
        buf = (Ax25Frame * 16)()
        n = C.c_size_t(0)
        frames = []
        check(lib().fmd_ax25_decoder_push(self._h, soft.ctypes.data, soft.shape[0], buf, 16, C.byref(n)))
        while True:
            frames += [{"data": bytes(buf[i].data[:buf[i].len]), "end_sample": buf[i].end_sample} for i in range(n.value)]
            if n.value < 16:
                return frames
            check(lib().fmd_ax25_decoder_push(self._h, None, 0, buf, 16, C.byref(n)))

    def info(self):
        i = Ax25Info()
        check(lib().fmd_ax25_decoder_info(self._h, C.byref(i)))
        return {"frames_ok": i.frames_ok, "bad_fcs": i.bad_fcs, "aborts": i.aborts, "in_frame": int(i.in_frame)}


def _call(a):
    """"CALL" or "CALL-SSID" of a 7-byte address, None where it is malformed (a character that is not shifted ASCII upper case or
    digit, or one behind a padding space)."""
    if any(b & 1 for b in a[:6]):
        return None
    name = bytes(b >> 1 for b in a[:6]).decode("latin-1").rstrip(" ")
    if not name or " " in name or not all(c.isdigit() or "A" <= c <= "Z" for c in name):
        return None
    ssid = (a[6] >> 1) & 15
    return name + ("-%d" % ssid if ssid else "")


def ax25_text(frame):
    """A frame (bytes, or a dict of Ax25Decoder.push) in TNC2 form `SRC>DST,DIGI*:info`: `*` behind a digipeater whose has-been-
    repeated bit is set, non-printable bytes of the information field as `.`; what follows the address field (control, PID,
    information) is shown from the third byte on when control is 0x03 and PID 0xF0 (UI), whole otherwise.  A frame whose address
    field is malformed is shown as hex."""
    data = bytes(frame["data"] if isinstance(frame, dict) else frame)
    addrs, pos = [], 0
    while True:
        if pos + 7 > len(data) or len(addrs) == 10:
            return data.hex()
        a = data[pos:pos + 7]
        name = _call(a)
        if name is None:
            return data.hex()
        addrs.append((name, bool(a[6] & 0x80)))
        pos += 7
        if a[6] & 1:
            break
    if len(addrs) < 2:
        return data.hex()
    rest = data[pos:]
    if rest[:2] == b"\x03\xf0":
        rest = rest[2:]
    path = "".join("," + n + ("*" if rep else "") for n, rep in addrs[2:])
    return "%s>%s%s:%s" % (addrs[1][0], addrs[0][0], path, "".join(chr(b) if 32 <= b < 127 else "." for b in rest))


def packets(bank, rate, baud=1200, mark=1200, space=2200, taps=None, stride=None, device_id=-1):
    """An AfskDemod matched to `bank` (a narrow-band or band-plan bank in NFM mode: mono rows at `rate` Hz): its rows, the designed
    table, a stride of a fifth of a bit unless given."""
    rows, width = bank_rows(bank)
    tab, pre_shift, out_shift = afsk_table(rate, baud, mark, space, taps)
    return AfskDemod(tab, afsk_stride(tab.shape[1]) if stride is None else stride, pre_shift, out_shift, n_rows=rows, width=width,
                     device_id=device_id, rate=rate, baud=baud)


def decode_rows(demod, calls):
    """Every call of `calls` (int16 [n_rows, n_in] each) through `demod` (an AfskDemod that knows its `rate`), every row through a
    decoder of its own: a list [n_rows] of Ax25Decoder.info() dicts with the delivered frames under "frames"."""
    if demod.rate is None:
        raise ValueError("the demodulator does not know its rate")
    decs = [Ax25Decoder(int(demod.rate), demod.stride, demod.baud) for _ in range(demod.n_rows)]
    frames = [[] for _ in range(demod.n_rows)]
    for x in calls:
        soft = demod.run_batch(x)
        for r in range(demod.n_rows):
            frames[r] += decs[r].push(soft[r])
    return [dict(decs[r].info(), frames=frames[r]) for r in range(demod.n_rows)]
