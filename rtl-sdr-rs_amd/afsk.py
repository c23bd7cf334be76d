"""Host-side wrapper of the packet demodulator (include/fmd.h): the tone-pair demodulator fmd_afsk_* -- every mono int16 row a bank
leaves on the device correlated against a mark and a space tone, one signed soft decision per `stride` samples -- and the host's
AX.25 frame decoder fmd_ax25_decoder_* (clock recovery, NRZI, HDLC, FCS), one per row: 1200 baud AFSK packet (APRS) out of any bank's
NFM rows; and the frame bank fmd_hdlc_*, the same decoder for every row on the device, which returns only the frames.  All are exact
in integers and independent of how the stream is cut."""
import ctypes as C
import math

import numpy as np

from ._ffi import DeviceConfig, RecordBank, RowProcessor, bank_rows, check, lib


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


def _frame_dict(f):
    return {"data": bytes(f.data[:f.len]), "end_sample": f.end_sample}


def ax25_max_frames(rate_num, rate_den, baud, n):
    """The frames one row can complete in a call of n soft decisions at most (include/fmd.h, fmd_hdlc_*): a sample takes at most one
    bit, the clock's phase gains at most step + (mod // 2 + 3) // 4 per sample, and the shortest frame is 144 line bits."""
    mod, step, n = int(rate_num), int(baud) * int(rate_den), int(n)
    bits = min(n, (mod - 1 + n * (step + (mod // 2 + 3) // 4)) // mod)
    return (bits + 143) // 144


class Ax25Framer(RecordBank):
    """The frame bank (fmd_hdlc_*): an Ax25Decoder(rate_num, rate_den, baud) per row, on the device.  run_batch takes int16 [n_rows,
    n_in] on the host, run_device an AfskDemod's d_out as it stands with its out_cap as in_cap; both return nothing.  Behind a call:
    counts() uint32 [n_rows], the frames that passed in it; frames(rows) the first min(count, frame_cap) of each listed row as dicts
    {"data", "end_sample"}, in the order they closed; info() the rows' cumulative counters as Ax25Decoder.info() gives them."""
    _prefix, _cap, _reader, _record, _info, _as_dict = "hdlc", "frame_cap", "frames", Ax25Frame, Ax25Info, staticmethod(_frame_dict)
    frame_records, frames = RecordBank.records, RecordBank.delivered

    def __init__(self, rate_num, rate_den=1, baud=1200, frame_cap=4, n_rows=1, device_id=-1):
        self._new(device_id, rate_num=rate_num, rate_den=rate_den, baud=baud, frame_cap=frame_cap, n_rows=n_rows)

    def max_frames(self, n_in):
        return ax25_max_frames(self.rate_num, self.rate_den, self.baud, n_in)
    max_records = max_frames

    def run_batch(self, soft):
        soft = np.ascontiguousarray(soft, dtype=np.int16)
        if soft.ndim != 2 or soft.shape[0] != self.n_rows:
            raise ValueError("soft must be [n_rows, n_in]")
        check(lib().fmd_hdlc_run_batch(self._h, soft.ctypes.data, soft.shape[1], soft.shape[1]))

    def run_device(self, d_in, n_in, in_cap, stream=None):
        """Enqueue on a device pointer (d_in [n_rows][in_cap], the first n_in samples of each row valid).  `stream` must stay alive
        until the handle's next `run_device` call or `check` has returned (include/fmd.h)."""
        check(lib().fmd_hdlc_run_device(self._h, d_in, n_in, in_cap, stream))


def framed(demod, frame_cap=4, device_id=-1):
    """An Ax25Framer matched to `demod` (an AfskDemod that knows its `rate`): its rows, rate / stride soft decisions per second, its
    baud."""
    if demod.rate is None:
        raise ValueError("the demodulator does not know its rate")
    return Ax25Framer(int(demod.rate), demod.stride, demod.baud, frame_cap, n_rows=demod.n_rows, device_id=device_id)


def decode_rows_gpu(demod, calls):
    """What decode_rows(demod, calls) returns, with the decoders on the device: the soft rows go from the demodulator to a framer
    (framed(demod, 16)) without leaving the device; after each call only the counts come back, and the frames of only the rows whose
    count is not zero.  A call's soft decisions are handed over in pieces short enough that no row can complete more than 16 frames
    in one."""
    import torch
    framer = framed(demod, 16)
    piece = framer.piece()                                   # (>= 2161: a sample takes at most one bit)
    frames = [[] for _ in range(demod.n_rows)]
    for x in calls:
        x = np.ascontiguousarray(x, dtype=np.int16)
        if x.ndim != 2 or x.shape[0] != demod.n_rows:
            raise ValueError("a call must be [n_rows, n_in]")
        n_in = x.shape[1]
        d_in = torch.from_numpy(np.ascontiguousarray(x) if n_in else np.zeros((demod.n_rows, 1), np.int16)).cuda()
        cap = max(1, demod.out_cap(n_in))
        d_soft = torch.empty((demod.n_rows, cap), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        n = demod.run_device(d_in.data_ptr(), n_in, max(1, n_in), d_soft.data_ptr(), cap)
        for lo in range(0, n, piece):
            framer.run_device(d_soft.data_ptr() + 2 * lo, min(piece, n - lo), cap)
            framer.harvest(frames)
    info = framer.info()
    framer.close()
    return [dict(info[r], frames=frames[r]) for r in range(demod.n_rows)]
