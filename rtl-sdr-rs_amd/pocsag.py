"""Host-side wrapper of the pager decoder (include/fmd.h): the FSK front end fmd_fsk_* -- every mono int16 row a bank leaves on the
device through a box matched filter one bit long, one soft decision per `D` samples, and a record wherever the 32-bit sync word
ends -- and the host's POCSAG batch decoder fmd_pocsag_decoder_*, one per row, which reads bit timing, slicer level and polarity
from those records: pager messages at 512, 1200 or 2400 bit/s out of any bank's NFM rows; and the page bank fmd_pager_*, the same
decoder for every row on the device, which takes the soft decisions and records where they lie and returns only the messages.  All
are exact in integers and independent of how the stream is cut."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

from ._ffi import DeviceConfig, RecordBank, RowProcessor, bank_rows, check, lib

POCSAG_SYNC = 0x7CD215D8
POCSAG_IDLE = 0x7A89C197
POCSAG_POLY = 0x769                                          # x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1, bit i = coefficient of x^i
NUMERIC = "0123456789*U -)("

HIT_DTYPE = np.dtype([("k_rel", np.uint32), ("d", np.uint32), ("corr", np.int32), ("thr", np.int32)])


class FskConfig(C.Structure):
    """struct fmd_fsk_config"""
    _fields_ = [("D", C.c_uint32), ("W", C.c_uint32), ("shift", C.c_uint32), ("tap", C.c_uint32 * 32), ("sync", C.c_uint32),
                ("tol", C.c_uint32), ("min_corr", C.c_int32), ("hit_cap", C.c_uint32)]


class FskHit(C.Structure):
    """struct fmd_fsk_hit"""
    _fields_ = [("k_rel", C.c_uint32), ("d", C.c_uint32), ("corr", C.c_int32), ("thr", C.c_int32)]


class PocsagMsg(C.Structure):
    """struct fmd_pocsag_msg"""
    _fields_ = [("address", C.c_uint32), ("function", C.c_uint32), ("n_bits", C.c_uint32), ("bits", C.c_uint8 * 320),
                ("corrected", C.c_uint32), ("inverted", C.c_uint32), ("end_sample", C.c_uint64)]


class PocsagInfo(C.Structure):
    """struct fmd_pocsag_info"""
    _fields_ = [("messages", C.c_uint64), ("batches", C.c_uint64), ("bad_codewords", C.c_uint64), ("orphans", C.c_uint64),
                ("locked", C.c_int), ("searching", C.c_int)]


FskDesign = namedtuple("FskDesign", "D W shift tap sync tol min_corr hit_cap")


def fsk_design(rate, baud=1200):
    """The parameters of an FskDemod for POCSAG at `baud` bit/s in audio at `rate` Hz: D = max(1, floor(rate / (5 baud) + 0.5)), a
    fifth of a bit; W = floor(rate / (baud D) + 0.5), so that D W samples are one bit; shift = ceil(log2(D W)); tap[j] = floor(j rate
    / (baud D) + 0.5); the sync word 0x7CD215D8, tol 2, min_corr 1024, hit_cap 16.  Scalar libm arithmetic in one fixed order, as
    fm::fsk_design (csrc/demod.hpp) does it.  A pair whose result leaves the kernel's domain is refused."""
    rate, baud = float(rate), float(baud)
    if not rate > 0 or not baud > 0:
        raise ValueError("need rate > 0 and baud > 0")
    d = math.floor(rate / (5.0 * baud) + 0.5)
    if d > 64:
        raise ValueError("rate / baud out of range")
    D = max(1, int(d))
    w = math.floor(rate / (baud * float(D)) + 0.5)
    if not 1 <= w <= 16:
        raise ValueError("rate / baud out of range")
    W = int(w)
    shift = 0
    while (1 << shift) < D * W:
        shift += 1
    tap = [int(math.floor(float(j) * rate / (baud * float(D)) + 0.5)) for j in range(32)]
    if shift > 10 or tap[31] > 255 or any(tap[j] < tap[j - 1] for j in range(1, 32)):
        raise ValueError("rate / baud out of range")
    return FskDesign(D, W, shift, np.array(tap, np.uint32), POCSAG_SYNC, 2, 1024, 16)


class FskDemod(RowProcessor):
    """`D` samples give one box sum, `W` box sums >> `shift` one soft decision (D W <= 2^shift), `n_rows` the rows of the bank
    whose output it takes; width is 1.  Every soft decision forms a word from the 32 soft samples `tap[j]` back, sliced at their
    mean, and is a hit when at most `tol` bits differ from `sync` (or from its complement: an inverted hit) and the signed sum C has
    |C| >= min_corr.  run_batch takes [n_rows, n_in] on the host; run_device takes a bank's d_out as it stands, with the bank's
    out_cap as in_cap; a call that completes no soft decision is taken.  hits() reads what the last call found.  `rate`, `baud` and
    `max_errors` (optional) are what decode_pages builds its decoders from."""
    _prefix = "fsk"

    def __init__(self, D, W, shift, tap, sync=POCSAG_SYNC, tol=2, min_corr=1024, hit_cap=16, n_rows=1, width=1, device_id=-1,
                 rate=None, baud=1200, max_errors=1):
        self.tap = np.ascontiguousarray(tap, dtype=np.uint32).reshape(-1)
        if self.tap.size != 32:
            raise ValueError("tap must have 32 entries")
        self.D, self.W, self.shift, self.sync, self.tol = int(D), int(W), int(shift), int(sync), int(tol)
        self.min_corr, self.hit_cap, self.n_rows, self.width = int(min_corr), int(hit_cap), int(n_rows), int(width)
        self.rate, self.baud, self.max_errors = rate, baud, max_errors
        for name in ("D", "W", "shift", "sync", "tol", "hit_cap", "n_rows", "width"):
            if not 0 <= getattr(self, name) < 1 << 32:
                raise ValueError("%s out of range" % name)
        if not -(1 << 31) <= self.min_corr < 1 << 31:
            raise ValueError("min_corr out of range")
        self._h = C.c_void_p()
        cfg = FskConfig()
        cfg.D, cfg.W, cfg.shift, cfg.sync, cfg.tol, cfg.min_corr, cfg.hit_cap = (self.D, self.W, self.shift, self.sync, self.tol,
                                                                                 self.min_corr, self.hit_cap)
        cfg.tap[:] = self.tap.tolist()
        dev = DeviceConfig(self.n_rows, device_id, 0)
        check(lib().fmd_fsk_new(C.byref(cfg), self.width, C.byref(dev), C.byref(self._h)))

    def out_cap(self, n_in):
        return int(lib().fmd_fsk_out_cap(self.D, n_in))

    def hit_counts(self):
        """uint32 [n_rows]: the hits of every row in the last call that launched, all of them.  Synchronises."""
        counts = np.zeros(self.n_rows, np.uint32)
        check(self._fn("hits")(self._h, counts.ctypes.data, None))
        return counts

    def hits(self):
        """(counts uint32 [n_rows], records [n_rows, hit_cap] with the fields k_rel, d, corr, thr) of the last call that launched:
        the first min(count, hit_cap) records of a row are its hits in increasing k, zeros behind them.  Synchronises."""
        counts, rec = np.zeros(self.n_rows, np.uint32), np.zeros((self.n_rows, self.hit_cap), HIT_DTYPE)
        check(self._fn("hits")(self._h, counts.ctypes.data, rec.ctypes.data))
        return counts, rec

    def hits_device(self):
        """(d_counts, d_hits): device addresses of what hits() would read, uint32 [n_rows] and records [n_rows][hit_cap].  Does not
        synchronise; valid until the handle's next call that launches, its reset or its close."""
        c, h = C.c_void_p(), C.c_void_p()
        check(lib().fmd_pager_fsk_hits(self._h, C.byref(c), C.byref(h)))
        return c.value, h.value


def pocsag_valid(w):
    """Bits 31 ... 1 of w divisible by the POCSAG polynomial and even parity over all 32."""
    c = (w >> 1) & 0x7FFFFFFF
    for i in range(30, 9, -1):
        if (c >> i) & 1:
            c ^= POCSAG_POLY << (i - 10)
    return c == 0 and bin(w & 0xFFFFFFFF).count("1") % 2 == 0


def pocsag_codeword(data21):
    """The codeword of 21 data bits (bit 20 is the message flag): 10 BCH check bits and an even parity bit behind them."""
    c = (int(data21) & 0x1FFFFF) << 10
    rem = c
    for i in range(30, 9, -1):
        if (rem >> i) & 1:
            rem ^= POCSAG_POLY << (i - 10)
    w = (c | rem) << 1
    return w | (bin(w).count("1") & 1)


def _rev(v, n):
    return int(format(v, "0%db" % n)[::-1], 2)


def pocsag_message_bits(text, mode):
    """The message bits of `text` as a list of 0 / 1, a multiple of 20: numeric 4 bits per character and padded with spaces, alpha 7
    bits per character and padded with zeros, each character's bits reversed."""
    bits = []
    if mode == "numeric":
        for ch in text:
            bits += [int(b) for b in format(_rev(NUMERIC.index(ch), 4), "04b")]
        while len(bits) % 20:
            bits += [0, 0, 1, 1]                             # a space: 12, reversed
    elif mode == "alpha":
        for ch in text:
            bits += [int(b) for b in format(_rev(ord(ch) & 0x7F, 7), "07b")]
        bits += [0] * (-len(bits) % 20)
    elif mode != "tone":
        raise ValueError("mode must be numeric, alpha or tone")
    return bits


def pocsag_encode(pages, preamble=576, words=None):
    """The sender: `pages` is a list of (address, function, text, mode) with mode "numeric", "alpha", "tone" (no text) or "bits"
    (text is a list of 0 / 1 whose length is a multiple of 20) -> the transmission as uint8 bits in the order they are sent:
    `preamble` bits of 1010..., then batches of the sync word and 16 codewords.  An address word goes into the frame its low three
    bits name, idle words fill what is free, and the last batch is filled up.  `words`: instead of pages, the codewords of the
    batches as they are (a multiple of 16)."""
    cws = []
    if words is not None:
        cws = [int(w) for w in words]
        if len(cws) % 16:
            raise ValueError("need whole batches")
    else:
        for address, function, text, mode in pages:
            address, function = int(address), int(function)
            if not 0 <= address < 1 << 21 or not 0 <= function < 4:
                raise ValueError("need address < 2^21 and function < 4")
            bits = [int(b) for b in text] if mode == "bits" else pocsag_message_bits(text, mode)
            if len(bits) % 20:
                raise ValueError("message bits must be a multiple of 20")
            while (len(cws) % 16) >> 1 != address & 7:
                cws.append(POCSAG_IDLE)
            cws.append(pocsag_codeword((address >> 3) << 2 | function))
            for i in range(0, len(bits), 20):
                cws.append(pocsag_codeword(1 << 20 | int("".join(str(b) for b in bits[i:i + 20]), 2)))
        cws.append(POCSAG_IDLE)
        while len(cws) % 16:
            cws.append(POCSAG_IDLE)
    out = [(i + 1) & 1 for i in range(int(preamble))]
    for i, w in enumerate(cws):
        if i % 16 == 0:
            out += [(POCSAG_SYNC >> b) & 1 for b in range(31, -1, -1)]
        out += [(w >> b) & 1 for b in range(31, -1, -1)]
    return np.array(out, np.uint8)


def _msg_bits(msg):
    data, n = bytes(msg["bits"]), min(int(msg["n_bits"]), 2560)
    return [(data[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


def pocsag_numeric(msg):
    """The message's bits as numeric text: 4 bits per character, each nibble bit-reversed, from the table `0123456789*U -)(`."""
    b = _msg_bits(msg)
    return "".join(NUMERIC[b[i] | b[i + 1] << 1 | b[i + 2] << 2 | b[i + 3] << 3] for i in range(0, len(b) - 3, 4))


def pocsag_alpha(msg):
    """The message's bits as text: 7 bits per character, each reversed; trailing NUL, ETX and EOT dropped, other non-printable
    characters as `.`."""
    b = _msg_bits(msg)
    ch = [sum(b[i + j] << j for j in range(7)) for i in range(0, len(b) - 6, 7)]
    while ch and ch[-1] in (0, 3, 4):
        ch.pop()
    return "".join(chr(c) if 32 <= c < 127 else "." for c in ch)


def pocsag_text(msg, baud=1200, mode="auto"):
    """One line per message, `POCSAG<baud>: Address: <7 digits>  Function: <f>  Numeric|Alpha|Tone: <text>`; mode "auto" takes
    function 0 as numeric and the rest as alpha; a message without bits is a tone-only page."""
    if mode not in ("auto", "numeric", "alpha"):
        raise ValueError("mode must be auto, numeric or alpha")
    head = "POCSAG%d: Address: %07d  Function: %d  " % (int(baud), msg["address"], msg["function"])
    if msg["n_bits"] == 0:
        return head + "Tone: "
    if mode == "numeric" or (mode == "auto" and msg["function"] == 0):
        return head + "Numeric: " + pocsag_numeric(msg)
    return head + "Alpha: " + pocsag_alpha(msg)


def pocsag_correct(word, max_errors=1):
    """(codeword, bits flipped) of the valid codeword within `max_errors` bit errors of `word`, None when there is none."""
    cw, n = C.c_uint32(0), C.c_uint32(0)
    rc = lib().fmd_pocsag_correct(int(word), int(max_errors), C.byref(cw), C.byref(n))
    if rc == -7:                                             # FMD_ERR_BAD_STATE: no codeword that near
        return None
    check(rc)
    return cw.value, n.value


class PocsagDecoder:
    """The host decoder of one row: push() takes the int16 soft decisions of an FskDemod at rate_num / rate_den per second (the
    audio rate over D) with the row's records of the same call, and returns the messages closed since, as dicts {"address",
    "function", "n_bits", "bits": bytes, "corrected", "inverted", "end_sample"}; info() the counters."""

    def __init__(self, rate_num, rate_den=1, baud=1200, max_errors=1):
        self._h = C.c_void_p()
        check(lib().fmd_pocsag_decoder_new(int(rate_num), int(rate_den), int(baud), int(max_errors), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().fmd_pocsag_decoder_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(lib().fmd_pocsag_decoder_reset(self._h))

    def push(self, soft, hits=None):
        soft = np.ascontiguousarray(soft, dtype=np.int16)
        if soft.ndim != 1:
            raise ValueError("soft must be [n]")
        hits = np.zeros(0, HIT_DTYPE) if hits is None else np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(-1)
        buf = (PocsagMsg * 16)()
        n = C.c_size_t(0)
        msgs = []
        check(lib().fmd_pocsag_decoder_push(self._h, soft.ctypes.data, soft.shape[0], hits.ctypes.data, hits.shape[0], buf, 16, C.byref(n)))
        while True:
            msgs += [{"address": m.address, "function": m.function, "n_bits": m.n_bits, "bits": bytes(m.bits[:(min(m.n_bits, 2560) + 7) // 8]),
                      "corrected": m.corrected, "inverted": m.inverted, "end_sample": m.end_sample} for m in buf[:n.value]]
            if n.value < 16:
                return msgs
            check(lib().fmd_pocsag_decoder_push(self._h, None, 0, None, 0, buf, 16, C.byref(n)))

    def info(self):
        i = PocsagInfo()
        check(lib().fmd_pocsag_decoder_info(self._h, C.byref(i)))
        return {"messages": i.messages, "batches": i.batches, "bad_codewords": i.bad_codewords, "orphans": i.orphans,
                "locked": int(i.locked), "searching": int(i.searching)}


def pages(bank, rate, baud=1200, max_errors=1, device_id=-1, **overrides):
    """An FskDemod matched to `bank` (a narrow-band or band-plan bank in NFM mode: mono rows at `rate` Hz): its rows and
    fsk_design(rate, baud); `overrides`: fields of the design (tol, min_corr, hit_cap) to replace."""
    rows, width = bank_rows(bank)
    d = fsk_design(rate, baud)._replace(**overrides)
    return FskDemod(d.D, d.W, d.shift, d.tap, d.sync, d.tol, d.min_corr, d.hit_cap, n_rows=rows, width=width, device_id=device_id,
                    rate=rate, baud=baud, max_errors=max_errors)


def decode_pages(demod, calls):
    """Every call of `calls` (int16 [n_rows, n_in] each) through `demod` (an FskDemod that knows its `rate`) on the device, every
    row through a decoder of its own: a list [n_rows] of PocsagDecoder.info() dicts with the delivered messages under "messages_list"
    and the row's calls that reached its decoder under "pushes".  After each call only the hit counts come back; the soft decisions
    of a row are copied, and its decoder pushed, only when the row has a hit or its decoder is locked or searching.  The samples a
    decoder did not see are added to its messages' end_sample, which counts the row's soft decisions."""
    import torch
    if demod.rate is None:
        raise ValueError("the demodulator does not know its rate")
    decs = [PocsagDecoder(int(demod.rate), demod.D, demod.baud, demod.max_errors) for _ in range(demod.n_rows)]
    found = [[] for _ in range(demod.n_rows)]
    busy, skipped, pushes = [False] * demod.n_rows, [0] * demod.n_rows, [0] * demod.n_rows
    for x in calls:
        x = np.ascontiguousarray(x, dtype=np.int16)
        if x.ndim != 2 or x.shape[0] != demod.n_rows:
            raise ValueError("a call must be [n_rows, n_in]")
        n_in = x.shape[1]
        if n_in == 0:
            continue
        d_in = torch.from_numpy(x).cuda()
        cap = max(1, demod.out_cap(n_in))
        d_out = torch.empty((demod.n_rows, cap), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        n = demod.run_device(d_in.data_ptr(), n_in, n_in, d_out.data_ptr(), cap)
        counts = demod.hit_counts()
        rec = demod.hits()[1] if counts.any() else None
        for r in range(demod.n_rows):
            if not counts[r] and not busy[r]:
                skipped[r] += n
                continue
            soft = d_out[r, :n].cpu().numpy()
            got = decs[r].push(soft, rec[r, :min(int(counts[r]), demod.hit_cap)] if counts[r] else None)
            for m in got:
                m["end_sample"] += skipped[r]
            found[r] += got
            pushes[r] += 1
            i = decs[r].info()
            busy[r] = bool(i["locked"] or i["searching"])
    return [dict(decs[r].info(), messages_list=found[r], pushes=pushes[r]) for r in range(demod.n_rows)]


def _msg_dict(m):
    return {"address": m.address, "function": m.function, "n_bits": m.n_bits, "bits": bytes(m.bits[:(min(m.n_bits, 2560) + 7) // 8]),
            "corrected": m.corrected, "inverted": m.inverted, "end_sample": m.end_sample}


def pocsag_max_messages(rate_num, rate_den, baud, n):
    """The messages one row can complete in a call of n soft decisions at most (include/fmd.h, fmd_pager_*): with q = mod // step and
    B = ceil(n / q) bits, (B + 31) // 32 + 1 + B // 512."""
    return int(lib().fmd_pager_max_messages(int(rate_num), int(rate_den), int(baud), int(n)))


class Pager(RecordBank):
    """The page bank (fmd_pager_*): a PocsagDecoder(rate_num, rate_den, baud, max_errors) per row, on the device.  run_batch takes
    int16 [n_rows, n_in] with the counts [n_rows] and records [n_rows, hit_cap] of FskDemod.hits() on the host; run_device an
    FskDemod's d_out as it stands with its out_cap as in_cap, and the addresses of FskDemod.hits_device(); both return nothing.  Behind
    a call: counts() uint32 [n_rows], the messages that closed in it; msgs(rows) the first min(count, msg_cap) of each listed row as
    PocsagDecoder.push returns them, in the order they closed; info() the rows' cumulative counters as PocsagDecoder.info() gives
    them."""
    _prefix, _cap, _reader, _record, _info, _as_dict = "pager", "msg_cap", "msgs", PocsagMsg, PocsagInfo, staticmethod(_msg_dict)
    msg_records, msgs = RecordBank.records, RecordBank.delivered

    def __init__(self, rate_num, rate_den=1, baud=1200, max_errors=1, msg_cap=4, n_rows=1, device_id=-1):
        self._new(device_id, rate_num=rate_num, rate_den=rate_den, baud=baud, max_errors=max_errors, msg_cap=msg_cap, n_rows=n_rows)

    def max_messages(self, n_in):
        return pocsag_max_messages(self.rate_num, self.rate_den, self.baud, n_in)
    max_records = max_messages

    def run_batch(self, soft, counts, hits):
        soft = np.ascontiguousarray(soft, dtype=np.int16)
        if soft.ndim != 2 or soft.shape[0] != self.n_rows:
            raise ValueError("soft must be [n_rows, n_in]")
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        if counts.shape[0] != self.n_rows or hits.ndim != 2 or hits.shape[0] != self.n_rows:
            raise ValueError("counts must be [n_rows] and hits [n_rows, hit_cap]")
        check(lib().fmd_pager_run_batch(self._h, soft.ctypes.data, soft.shape[1], soft.shape[1], counts.ctypes.data, hits.ctypes.data,
                                        hits.shape[1]))

    def run_device(self, d_soft, n_in, in_cap, d_counts, d_hits, hit_cap, stream=None):
        """Enqueue on device pointers (d_soft [n_rows][in_cap], the first n_in samples of each row valid; d_counts [n_rows] uint32;
        d_hits [n_rows][hit_cap] records).  `stream` must stay alive until the handle's next `run_device` call or `check` has
        returned (include/fmd.h)."""
        check(lib().fmd_pager_run_device(self._h, d_soft, n_in, in_cap, d_counts, d_hits, hit_cap, stream))


def paged(demod, msg_cap=4, device_id=-1):
    """A Pager matched to `demod` (an FskDemod that knows its `rate`): its rows, rate / D soft decisions per second, its baud and
    max_errors."""
    if demod.rate is None:
        raise ValueError("the demodulator does not know its rate")
    return Pager(int(demod.rate), demod.D, demod.baud, demod.max_errors, msg_cap, n_rows=demod.n_rows, device_id=device_id)


def decode_pages_gpu(demod, calls):
    """What decode_pages(demod, calls) returns, without the "pushes" key, with the decoders on the device: the soft rows and the
    records go from the demodulator to a page bank (paged(demod, 16)) without leaving the device; after each call only the counts
    come back, and the messages of only the rows whose count is not zero.  Every input call is handed to the demodulator in pieces
    short enough that no row can complete more than 16 messages in one (the front end is exact under cuts).  Equal to decode_pages
    where no row has more than hit_cap hits in a call: there the records kept differ with the cuts."""
    import torch
    pager = paged(demod, 16)
    piece = pager.piece() * demod.D                          # input samples: a piece completes at most ceil(piece / D) soft decisions
    found = [[] for _ in range(demod.n_rows)]
    for x in calls:
        x = np.ascontiguousarray(x, dtype=np.int16)
        if x.ndim != 2 or x.shape[0] != demod.n_rows:
            raise ValueError("a call must be [n_rows, n_in]")
        n_in = x.shape[1]
        if n_in == 0:
            continue
        d_in = torch.from_numpy(x).cuda()
        cap = max(1, demod.out_cap(min(piece, n_in)))
        d_soft = torch.empty((demod.n_rows, cap), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        for lo in range(0, n_in, piece):
            m = min(piece, n_in - lo)
            n = demod.run_device(d_in.data_ptr() + 2 * lo, m, n_in, d_soft.data_ptr(), cap)
            d_counts, d_hits = demod.hits_device()
            pager.run_device(d_soft.data_ptr(), n, cap, d_counts, d_hits, demod.hit_cap)
            if n:
                pager.harvest(found)
    info = pager.info()
    pager.close()
    return [dict(info[r], messages_list=found[r]) for r in range(demod.n_rows)]
