"""Case tables of the *_domain GPU tests of the three digital row processors -- the frame bank (tests/test_gpu_hdlc_domain.py), the
pager front end (tests/test_gpu_fsk_domain.py) and the code squelch (tests/test_gpu_dcs_domain.py) -- in plain Python and numpy.
tests/test_digital_cases.py runs the tables against the test-side definitions alone (tests/hdlc_ref.py over tests/ax25_ref.py,
tests/fsk_ref.py, tests/dcs_ref.py) and asserts what each case reaches; the GPU files feed the same cases to the handles and compare
bit for bit after every call.  The frame bank's lines on the wire (`cases`) and the kernel's per-bit step restated (`Model`) live here
too; tests/test_hdlc.py holds the Model to the definition.  FMD_FUZZ_SEED moves the seeds of the random parts; what a case claims
is built into it and does not hang on the draw."""
from types import SimpleNamespace as NS

import numpy as np

import ax25_ref as xr
import dcs_ref as dr
import fsk_ref as fr
import hdlc_ref as hr
from rows_cases import sampled_rows, seed

U32 = (1 << 32) - 1


# ---- the frame bank: the lines on the wire -----------------------------------------------------------------------------------------
def _soft(bits, num=5, den=1, amp=9000):
    return hr.levels_to_soft(xr.nrzi(bits), num, den, amp)


def _body(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist())


def _find(rng, n, pred):
    """a random frame of n bytes without the FCS whose stuffed bits satisfy `pred(data, stuffed bits)`"""
    for _ in range(20000):
        d = _body(rng, n)
        if pred(d, xr.stuffed_bits(xr.with_fcs(d))):
            return d
    raise AssertionError("no such frame")


def _stuffed_in_fcs(d, bits):
    f = xr.with_fcs(d)
    return len(xr.stuffed_bits(f[-2:])) > 16 and len(bits) - len(xr.stuffed_bits(f[:-2])) > 16


def cases():
    """{name: the bits on the line}, flags and frames; every case ends with a few flags"""
    rng = np.random.default_rng(2025)
    F = xr.FLAG
    out = {}
    for n in (16, 17, 514, 515, 3000):                       # bytes with the FCS: one below and at either limit, and far beyond
        out["bytes-%d" % n] = xr.frame_bits(_body(rng, n - 2), flags=3, closing=2)
    a, b, c = _body(rng, 20), _body(rng, 33), _body(rng, 15)
    out["shared-flag"] = F * 2 + xr.stuffed_bits(xr.with_fcs(a)) + F + xr.stuffed_bits(xr.with_fcs(b)) + F + xr.stuffed_bits(xr.with_fcs(c)) + F * 2
    out["abort"] = F * 2 + xr.stuffed_bits(a)[:77] + [1] * 9 + [0, 1, 0] + xr.frame_bits(b, flags=2, closing=2)
    out["abort-outside"] = F + [1] * 12 + xr.frame_bits(a, flags=2) + [1] * 8 + F
    out["stuffed-in-fcs"] = xr.frame_bits(_find(rng, 25, _stuffed_in_fcs), flags=2, closing=2)
    out["stuffed-before-flag"] = xr.frame_bits(_find(rng, 25, lambda d, s: s[-6:] == [1, 1, 1, 1, 1, 0]), flags=2, closing=2)
    out["ff-514"] = xr.frame_bits(b"\xff" * 512, flags=2, closing=2)
    out["ff-514-raw"] = F * 2 + xr.stuffed_bits(b"\xff" * 514) + F * 2           # 514 bytes of 0xFF with no FCS behind them
    good = xr.stuffed_bits(xr.with_fcs(b))
    for k in (0, 100, len(good) - 1):
        bad = list(good)
        bad[k] ^= 1
        out["flipped-%d" % k] = F * 2 + bad + F * 2
    for extra in (1, 3, 7):
        out["bits-plus-%d" % extra] = F * 2 + good + [0, 1, 0, 0, 1, 0, 1][:extra] + F + xr.stuffed_bits(xr.with_fcs(a)) + F
    out["bits-minus-1"] = F * 2 + good[:-1] + F * 2
    out["flags-back-to-back"] = F * 9 + xr.stuffed_bits(xr.with_fcs(a)) + F * 7
    out["seven-bits"] = F * 2 + [0, 1, 0, 0, 1, 0, 0] + F + [0] + F + xr.stuffed_bits(xr.with_fcs(c)) + F
    return out


CASES = cases()
# (frames_ok, bad_fcs, aborts) of a line that ends with its last flag
WANT = {"bytes-16": (0, 1, 0), "bytes-17": (1, 0, 0), "bytes-514": (1, 0, 0), "bytes-515": (0, 1, 0), "bytes-3000": (0, 1, 0),
        "shared-flag": (3, 0, 0), "abort": (1, 0, 1), "abort-outside": (1, 0, 2), "stuffed-in-fcs": (1, 0, 0),
        "stuffed-before-flag": (1, 0, 0), "ff-514": (1, 0, 0), "ff-514-raw": (0, 1, 0), "flipped-0": (0, 1, 0), "flipped-100": (0, 1, 0),
        "bits-plus-1": (1, 1, 0), "bits-plus-3": (1, 1, 0), "bits-plus-7": (1, 1, 0), "bits-minus-1": (0, 1, 0),
        "flags-back-to-back": (1, 0, 0), "seven-bits": (1, 2, 0)}


# ---- the kernel's per-bit step --------------------------------------------------------------------------------------
class Model:
    """One row of the frame bank as the kernel runs it.  The clock and NRZI are the definition's; per bit, the open frame keeps
    nbits, the last 16 stored bits (`hist`, the newest at bit 15) and a CRC register that takes the bit stored seven bits ago, and
    writes a byte to `mem` per eight stored bits; the flag accepts on the residue 0xF0B8 and copies mem[:len] out."""

    FIELDS = {"ph": "ph", "prev": "prev_inv", "level": "level_inv", "in_frame": "in_frame", "ones": "ones", "sr": "sr", "hist": "hist",
              "nbits": "nbits", "crc": "crc"}                # what a call carries per row besides the counters and the open frame

    def __init__(self, rate_num, rate_den=1, baud=1200):
        self.mod, self.step = int(rate_num), int(baud) * int(rate_den)
        assert self.step >= 1 and 4 * self.step <= self.mod <= 64 * self.step
        self.ph, self.prev_inv, self.level_inv = 0, 0, 0     # all zero: the reset state (prev and level are stored inverted)
        self.sr = self.ones = self.nbits = self.in_frame = self.hist = self.crc = 0
        self.frames_ok = self.bad_fcs = self.aborts = 0
        self.n = 0
        self.mem = bytearray(520)

    def info(self):
        return {"frames_ok": self.frames_ok, "bad_fcs": self.bad_fcs, "aborts": self.aborts, "in_frame": self.in_frame}

    def drop(self, field):
        """A call edge that loses `field`: it comes back as in the reset state.  Whether it held another value."""
        held = getattr(self, self.FIELDS[field]) != 0
        setattr(self, self.FIELDS[field], 0)
        return held

    def _bit(self, bit, frames):
        self.sr = (self.sr >> 1) | (bit << 7)
        if self.sr == 0x7E:
            if self.in_frame and self.nbits > 7:
                nb = self.nbits - 7
                if nb % 8 == 0 and self.nbits <= 514 * 8 + 7 and 17 <= nb // 8 <= 514 and self.crc == 0xF0B8:
                    self.frames_ok += 1
                    frames.append({"data": bytes(self.mem[:nb // 8 - 2]), "end_sample": self.n})
                else:
                    self.bad_fcs += 1
            self.in_frame, self.nbits, self.ones, self.crc = 1, 0, 0, 0xFFFF
            return
        store = self.in_frame == 1
        if bit:
            self.ones += 1
            if self.ones >= 7:
                self.aborts += self.in_frame
                self.in_frame, self.ones, store = 0, 7, False
        else:
            if self.ones == 5:
                store = False
            self.ones = 0
        if store:
            if self.nbits < 514 * 8 + 7:
                if self.nbits >= 7:
                    fb = (self.crc ^ (self.hist >> 9)) & 1
                    self.crc = (self.crc >> 1) ^ (0x8408 if fb else 0)
                self.hist = (self.hist >> 1) | (bit << 15)
                if self.nbits & 7 == 7:
                    self.mem[self.nbits >> 3] = self.hist >> 8
            if self.nbits <= 514 * 8 + 7:
                self.nbits += 1

    def push(self, soft):
        frames = []
        half = self.mod // 2
        for v in np.asarray(soft, np.int16).tolist():
            cur = 1 if v >= 0 else 0
            if cur != self.prev_inv ^ 1:
                self.ph -= (self.ph - half) >> 2
            self.prev_inv = cur ^ 1
            self.ph += self.step
            if self.ph >= self.mod:
                self.ph -= self.mod
                self._bit(1 if cur == self.level_inv ^ 1 else 0, frames)
                self.level_inv = cur ^ 1
            self.n += 1
        assert 0 <= self.ph < self.mod < 1 << 32 and self.hist < 1 << 16 and self.crc < 1 << 16 and self.nbits <= 514 * 8 + 8
        return frames


# ---- the frame bank's cases --------------------------------------------------------------------------------------------------------
HD_CUTS = (1, 7, 1000, 333)
AMP = 9000
# name: (rate_num, rate_den, baud); a level is held mod / step samples, mod = rate_num and step = baud rate_den
HD_CLOCKS = {"6000": (6000, 1, 1200), "11025-2": (11025, 2, 1200), "wide": (U32, 894784, 1200)}


def _hd_case(name, clock, cap, x, runs, **claim):
    num, den, baud = clock
    return NS(name=name, num=num, den=den, baud=baud, mod=num, step=baud * den, cap=cap, rows=x.shape[0], x=np.ascontiguousarray(x, np.int16),
              runs=[list(r) for r in runs], claim=NS(**claim))


def _line(bits, mod, step, nbits=None):
    """The line `bits` as soft decisions; up to `nbits` bits it goes on with flags (flags back to back close nothing and abort nothing)"""
    if nbits is not None:
        bits = (list(bits) + xr.FLAG * ((nbits - len(bits)) // 8 + 2))[:max(nbits, len(bits))]
    return hr.levels_to_soft(xr.nrzi(bits), mod, step, AMP)


def _stack(lines, tail=8):
    """int16 [rows, n]: every line, held at its last level to the common length"""
    n = max(len(s) for s in lines) + tail
    x = np.empty((len(lines), n), np.int16)
    for r, s in enumerate(lines):
        x[r, :len(s)] = s
        x[r, len(s):] = s[-1] if len(s) else AMP
    return x


def _noise_row(rng, kind, n):
    """0: idle on mark, 1: idle on space, 2: full-range noise, 3: bit-like noise of four samples a level (flags, aborts, stuffing)"""
    if kind < 2:
        return np.full(n, AMP if kind == 0 else -AMP, np.int16)
    if kind == 2:
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return (np.repeat(rng.integers(0, 2, n // 4 + 1) * 2 - 1, 4)[:n] * rng.integers(1, 30000, n)).astype(np.int16)


HD_LEAD = 10                                                  # rows of idle and noise in front of the first line


def hd_lines(clock):
    """1a: every line of `cases()` at one clock in one handle of 75 rows: ten idle and noise rows, then per line (sorted by name) the
    line behind one idle bit, the same inverted (NRZI reads it the same once the idle bit has shown the decoder the line's level) and
    an idle or noise row, then two more.  The lines of the last three names lie in
    the second wave.  Every line goes on with flags to the common length, so a row's counters are its line's.  Uncut and under the
    cuts 1 | 7 | 1000 | 333 | rest."""
    num, den, baud = HD_CLOCKS[clock]
    mod, step = num, baud * den
    rng = np.random.default_rng(seed(9000 + num % 1000))
    names = sorted(CASES)
    nbits = max(len(b) for b in CASES.values()) + 17
    n = nbits * mod // step
    rows, where = [_noise_row(rng, k % 4, n) for k in range(HD_LEAD)], {}
    for i, name in enumerate(names):
        s = _line([1] + CASES[name], mod, step, nbits)[:n]
        where[name] = (len(rows), len(rows) + 1)
        rows += [s, -s, _noise_row(rng, i % 4, n)]
    rows += [_noise_row(rng, 2, n), _noise_row(rng, 3, n)]
    return _hd_case("lines-" + clock, HD_CLOCKS[clock], 4, np.stack(rows), [[], HD_CUTS], where=where)


HD_LENGTHS = list(range(15, 513))
HD_LENGTH_GROUPS = [list(g) for g in np.array_split(np.array(HD_LENGTHS), 8)]


def hd_lengths(g):
    """1b: the data lengths of group g of 8 (15 ... 512 in all), one frame per row at 4800 Hz, 4 samples a bit; the last row carries
    a frame of 14 data bytes and, in the last group, one of 513 behind it: one byte outside either limit, counted in bad_fcs.  One
    call and the cut at 1001."""
    lens = HD_LENGTH_GROUPS[g]
    rng = np.random.default_rng(seed(9100 + g))
    bodies = [_body(rng, n) for n in lens]
    outside = [_body(rng, 14)] + ([_body(rng, 513)] if g == len(HD_LENGTH_GROUPS) - 1 else [])
    bits = [xr.frame_bits(d, flags=2 + r % 3, closing=2) for r, d in enumerate(bodies)]
    last = xr.FLAG * 2
    for d in outside:
        last = last + xr.stuffed_bits(xr.with_fcs(d)) + xr.FLAG
    bits.append(last + xr.FLAG)
    nbits = max(len(b) for b in bits) + 8
    x = np.stack([_line(b, 4800, 1200, nbits)[:4 * nbits] for b in bits])
    return _hd_case("lengths-%d" % g, (4800, 1, 1200), 4, x, [[], [1001]], bodies=bodies, outside=outside)


HD_CLOSE_LENS = (15, 64, 65, 511, 512)
HD_CLOSE = [(1, 64), (2, 65), (3, 65), (15, 65)]             # (frame_cap, rows)


def hd_close(cap, rows):
    """1c: every row's last frame closes on the same sample.  Row r's last frame has HD_CLOSE_LENS[r % 5] data bytes, and in front
    of it the row delivers 7 (r // 5) mod (cap + 2) frames of 15 bytes in the same call, one flag between two: the rows with fewer than
    `cap` of them take the last frame's record, the others only count it.  The line idles on mark in front, so that all lines have
    as many bits.  One call."""
    rng = np.random.default_rng(seed(9200 + cap))
    bits, prior, bodies = [], [], []
    for r in range(rows):
        k = ((r // 5) * 7) % (cap + 2)
        b = list(xr.FLAG * 2)
        ds = [_body(rng, 15) for _ in range(k)] + [_body(rng, HD_CLOSE_LENS[r % 5])]
        for d in ds:
            b += xr.stuffed_bits(xr.with_fcs(d)) + xr.FLAG
        bits.append(b)
        prior.append(k)
        bodies.append(ds)
    nbits = max(len(b) for b in bits)
    x = _stack([_line([1] * (nbits - len(b)) + b + xr.FLAG, 6000, 1200) for b in bits])
    return _hd_case("close-cap%d" % cap, (6000, 1, 1200), cap, x, [[]], prior=prior, bodies=bodies, closing_bit=nbits)


# (data bytes, rate): 17 bytes with the FCS and no stuffed bit, 40 data bytes with one.  At 6000 Hz a level is five whole samples and
# the clock sits still, so a lost `prev` -- one pull too many or too few -- never moves a bit there; at 4800 Hz (four samples, the
# edge of the domain, where a take falls next to a transition) it does.
HD_EDGES = ((15, 6000), (40, 6000), (15, 4800))


def hd_edge_line(nbytes, rate=6000):
    """the line of 1d: one flag, the frame (of 15 data bytes without, of 40 with a stuffed bit), two flags"""
    rng = np.random.default_rng(seed(9300 + nbytes))
    want = 0 if nbytes == 15 else 1
    d = _find(rng, nbytes, lambda d, s: (len(s) - 8 * (len(d) + 2) >= 1) == bool(want))
    return d, _line(xr.frame_bits(d, flags=1, closing=2), rate, 1200)


def hd_edges(nbytes, rate=6000):
    """1d: row r carries the line delayed by r samples, as many rows as the line has samples L up to its closing sample; the calls
    are L | 1 | rest, so row r's first call ends r samples before the line's closing sample: some row's call edge lies on every
    sample of the frame, in every phase of the clock and behind every bit."""
    d, s = hd_edge_line(nbytes, rate)
    f = xr.Decoder(rate).push(s)
    assert len(f) == 1 and f[0]["data"] == d
    L = f[0]["end_sample"] + 1
    x = _stack([np.concatenate([np.full(r, AMP, np.int16), s]) for r in range(L)], tail=16)
    return _hd_case("edges-%d-%d" % (nbytes, rate), (rate, 1, 1200), 4, x, [[L, 1]], L=L, data=d)


HD_LONG_DELAYS = tuple(range(0, 180, 15))


def hd_long_edges():
    """1d, the long frame: 512 data bytes, row r delayed by HD_LONG_DELAYS[r] samples, calls c | 1 | rest with c three samples before
    row 0's closing sample: the call edges lie in the closing flag and in the last three bytes, where nbits is beyond 4096."""
    rng = np.random.default_rng(seed(9400))
    d = _body(rng, 512)
    s = _line(xr.frame_bits(d, flags=2, closing=2), 6000, 1200)
    f = xr.Decoder(6000).push(s)
    assert len(f) == 1 and f[0]["data"] == d
    c = f[0]["end_sample"] - 3
    x = _stack([np.concatenate([np.full(r, AMP, np.int16), s]) for r in HD_LONG_DELAYS], tail=16)
    return _hd_case("long-edges", (6000, 1, 1200), 4, x, [[c, 1]], c=c, data=d)


HD_SWITCH = [(m, k) for m in ((1 << 31) - 1, 1 << 31, (1 << 31) + 1) for k in (4, 64)]


def hd_switch(mod, k):
    """1e: rate_num = mod on either side of the clock's switch to 64 bits (mod >= 2^31), with step = mod // 4 (k = 4) or the
    smallest step with mod <= 64 step (k = 64), both at the edge of the host's test.  A framed row, the same inverted, and a row of
    random signs; uncut and cut."""
    step = mod // 4 if k == 4 else -(-mod // 64)
    assert 4 * step <= mod <= 64 * step
    rng = np.random.default_rng(seed(9500 + k + mod % 7))
    bodies = [_body(rng, 15), _body(rng, 31)]
    bits = xr.FLAG * 3
    for d in bodies:
        bits = bits + xr.stuffed_bits(xr.with_fcs(d)) + xr.FLAG
    s = _line(bits + xr.FLAG, mod, step)
    x = np.stack([s, -s, rng.integers(-32768, 32768, len(s)).astype(np.int16)])
    return _hd_case("switch-%d-%d" % (mod, k), (mod, 1, step), 4, x, [[], HD_CUTS], bodies=bodies)


def clock_peak(soft, mod, step):
    """the largest ph + step the definition's clock forms over `soft`, before the compare with mod"""
    ph, prev, half, peak = 0, 1, mod // 2, 0
    for cur in (np.asarray(soft) >= 0).tolist():
        if cur != prev:
            ph -= (ph - half) >> 2
        prev = cur
        ph += step
        peak = max(peak, ph)
        if ph >= mod:
            ph -= mod
    return peak


HD_ROWS = (127, 128, 129)
HD_MANY = 40000


def hd_rows(rows):
    """1f: `rows` rows (the wave's edge at 128, and 40000), row r with one of 64 short frames, delayed by up to 39 samples of its own;
    about 1000 samples per row, cut at 500.  At 40000 rows 16 sampled rows are compared."""
    rng = np.random.default_rng(seed(9600 + rows % 1000))
    bodies = [_body(rng, int(rng.integers(15, 20))) for _ in range(64)]
    lines = _stack([_line(xr.frame_bits(d, flags=2 + i % 3, closing=2), 6000, 1200) for i, d in enumerate(bodies)], tail=48)
    which, delay = (7 * np.arange(rows)) % 64, rng.integers(0, 40, rows)
    n = lines.shape[1]
    x = np.empty((rows, n), np.int16)
    for lo in range(0, rows, 4096):                          # x[r, j] = line[j - delay[r]], on mark in front of it
        hi = min(rows, lo + 4096)
        j = np.maximum(np.arange(n)[None, :] - delay[lo:hi, None], 0)
        x[lo:hi] = np.where(np.arange(n)[None, :] >= delay[lo:hi, None], lines[which[lo:hi, None], j], AMP)
    c = _hd_case("rows-%d" % rows, (6000, 1, 1200), 4, x, [[500]], bodies=[bodies[i] for i in which.tolist()] if rows < 1000 else None)
    c.sample = sampled_rows(np.random.default_rng(c.num + rows), rows) if rows > 1000 else list(range(rows))
    c.which = which
    c.line_bodies = bodies
    return c


# the definition over a case, call by call: computed once per (case, run) and shared
Snap = NS


def pack(every, cap):
    """hdlc_ref.Framer's packaging of a call's frames: (counts, records)"""
    counts, rec = np.zeros(len(every), np.uint32), np.zeros((len(every), cap), hr.FRAME_DTYPE)
    for r, frames in enumerate(every):
        counts[r] = len(frames)
        for k, f in enumerate(frames[:cap]):
            rec[r, k]["data"][:len(f["data"])] = np.frombuffer(f["data"], np.uint8)
            rec[r, k]["len"] = len(f["data"])
            rec[r, k]["end_sample"] = f["end_sample"]
    return counts, rec


_HD_REF = {}


def hd_reference(c, run, rows=None):
    """[Snap(last, info, pos)] after every call of run `run` of the case (its cuts, then the rest), over `rows` (all of them)"""
    key = (c.name, c.x.shape, tuple(c.runs[run]), None if rows is None else tuple(rows))
    if key not in _HD_REF:
        x = c.x if rows is None else c.x[list(rows)]
        ref = hr.Framer(c.num, c.den, c.baud, c.cap, rows=x.shape[0])
        snaps, lo = [], 0
        for m in c.runs[run] + [x.shape[1]]:
            part = x[:, lo:lo + m]
            if part.shape[1] == 0:
                break
            last = ref.run(part)
            snaps.append(Snap(last=last, info=ref.info(), pos=ref.pos))
            lo += part.shape[1]
        _HD_REF[key] = snaps
    return _HD_REF[key]


def merged(snaps, cap):
    """The one call that the calls of `snaps` add up to: the definition is cut invariant (tests/test_hdlc.py), so one call over
    the whole stream completes the frames of all of them, in order."""
    every = [sum((s.last[2][r] for s in snaps), []) for r in range(len(snaps[0].last[2]))]
    counts, rec = pack(every, cap)
    return Snap(last=(counts, rec, every), info=snaps[-1].info, pos=snaps[-1].pos)


class Replay:
    """hdlc_ref.Framer's face over the snapshots of hd_reference: run() steps to the next call's"""

    def __init__(self, snaps):
        self.snaps, self.i = snaps, -1

    def run(self, part):
        if part.shape[1]:
            self.i += 1
        return self.last

    last = property(lambda self: self.snaps[self.i].last)
    pos = property(lambda self: self.snaps[self.i].pos)

    def info(self):
        return self.snaps[self.i].info


# ---- the code squelch's cases ------------------------------------------------------------------------------------------------------
DC_ALL = (1 << 128) - 1
_DC_REF = {}


def dc_run(cuts, mode="call", off_in=0, off_out=0, in_place=False):
    """One run on a fresh handle: the pieces `cuts` and then the rest.  mode "call": rows_gpu.call with an odd in_cap; "at":
    rows_gpu.call_at, every input row off_in samples and every output row off_out samples behind a 16-byte boundary, or in place."""
    return NS(cuts=list(cuts), mode=mode, off_in=off_in, off_out=off_out, in_place=in_place)


def dc_audio(rng, rows, n, width):
    """Rows at different levels, full scale among them, with -32768 and a silent stretch."""
    x = rng.integers(-32768, 32768, (rows, n, width)).astype(np.int64)
    x = (x * rng.choice([1, 64, 4096, 32768], (rows, 1, 1))) >> 15
    x[:, n // 3] = -32768
    x[rows // 2, n // 2:n // 2 + n // 5] = 0
    return x.astype(np.int16)


def dc_taps(rng, last):
    """23 non-decreasing offsets from 0 to `last`, with repeats"""
    if last == 0:
        return [0] * 23
    t = np.sort(rng.integers(0, last + 1, 21)).tolist()
    return [0] + t[:10] + [t[10]] + t[10:20] + [last]


def dc_lp(rng, T):
    lp = rng.integers(-1023, 1024, T).tolist()
    lp[0], lp[-1] = (1023, -1023) if T > 1 else (lp[0], 1023)
    return lp


def dc_loose(rng, P, B, T, last, tol=23):
    """A configuration under which noise opens and closes the gate: at tol 23 every k matches its nearest word and a block is a
    hit when a quarter of its k agree on one; about half of the words open.  lshift leaves soft a few thousand on full-scale noise."""
    lp = dc_lp(rng, T)
    lshift = max(0, int(np.abs(np.array(lp)).sum()).bit_length() - 2 - (B.bit_length() - 1) // 2)
    min_hits = max(1, P // B // 4) if tol == 23 else 1
    accept = int(rng.integers(1, 1 << 62)) | (int(rng.integers(0, 1 << 62)) << 64) | 1
    return dr.Cfg(P, B, lp, lshift, dc_taps(rng, last), tol, min_hits, 1, int(rng.integers(0, 2)), min(64, P), accept)


def dc_words(rng, F):
    w = rng.integers(0, 1 << 23, F).astype(np.uint32)
    if F > 1:
        w[-1] = w[0]                                         # a repeated word: the first of the two is the match
    return w


def _dc_case(name, sd, width, words, cfg, x, runs, **claim):
    return NS(name=name, seed=seed(sd), width=width, words=np.asarray(words, np.uint32), cfg=dr.Cfg(*cfg), rows=x.shape[0], x=x, runs=runs,
              claim=NS(**claim))


_DC_DRAWN = {}


def _dc_drawn(name, sd, build):
    """The case `build(rng)` makes from the first of the draws seed(sd), attempt 0, 1, ... under which the definition has a block
    that hit and an output that is not all zero in every run: what a case claims does not hang on the draw."""
    if name not in _DC_DRAWN:
        for attempt in range(50):
            c = build(np.random.default_rng([seed(sd), attempt]))
            c.name, c.seed = name, (seed(sd), attempt)
            _DC_REF.pop((name, 0), None), _DC_REF.pop((name, 1), None)
            if all(any(h[2] != dr.NONE for h in dc_reference(c, k)[1].hits) and any(e[2].any() for e in dc_reference(c, k)[0])
                   for k in range(len(c.runs))):
                break
        else:
            raise AssertionError("no draw of %s opens" % name)
        _DC_DRAWN[name] = c
    return _DC_DRAWN[name]


def dc_pieces(c, r):
    """(lo, hi) of the run's calls"""
    out, lo = [], 0
    for n in r.cuts + [c.x.shape[1]]:
        hi = min(c.x.shape[1], lo + n)
        if hi > lo:
            out.append((lo, hi))
        lo = hi
    return out


def dc_searches(P, B, pos, n):
    """The kernel's search cadence over one call of n samples that starts at stream sample `pos` (DESIGN.md 9n, and the kernel
    header's prose): the call is walked in chunks of 64 stream samples; behind each chunk the boxes that wait are searched at a
    block's end, at the call's end, or once one more chunk could make them more than 64.  Per chunk (waiting boxes, boxes per chunk,
    block end, call end, whether waiting + NB > 64)."""
    lgB = B.bit_length() - 1
    NB = 64 >> lgB
    pos_r = pos % P
    o_end = pos_r + n
    kdone, out = pos_r >> lgB, []
    for c in range(pos_r >> 6, ((o_end - 1) >> 6) + 1):
        ob = min((c + 1) << 6, o_end)
        eb = ob - (c << 6)
        kcur = c * NB + (eb >> lgB)
        block_end = eb == 64 and ((c << 6) % P) + 64 == P
        full = kcur - kdone + NB > 64
        out.append((kcur - kdone, NB, block_end, ob == o_end, full))
        if block_end or ob == o_end or full:
            assert kcur - kdone <= 64
            kdone = kcur
    return out


DC_BOXES = (2, 4, 16, 32)
DC_BOX_BLOCKS = (64, 192, 4160)


def dc_boxes(B, P, width):
    """3a: 64 calls that start at every offset 0 ... 63 of a chunk in turn (call i has 64 m + 1 samples; m is 1, and 34 for every
    16th call, which then runs 34 chunks: long enough for the boxes that wait to reach 64 at every B where no block end comes
    first, that is at P = 4160), then the rest.  3 rows."""
    cuts = [64 * (34 if i % 16 == 5 else 1) + 1 for i in range(64)]
    n = sum(cuts) + 2 * P + 7

    def build(rng):
        cfg = dc_loose(rng, P, B, int(rng.integers(1, 65)), int(rng.integers(0, 512 // B)))
        return _dc_case("", 0, width, dc_words(rng, 5), cfg, dc_audio(rng, 3, n, width), [dc_run(cuts)])
    return _dc_drawn("box-B%d-P%d-w%d" % (B, P, width), 9700 + 100 * B + P + width, build)


DC_RING_TAPS = (63, 64, 65, 191, 192, 193, 447, 448, 449, 511)


def dc_ring(last, width):
    """3b: tap[22] = `last` on either side of the sizes of the soft ring (128, 256, 512 and 1024 entries hold tap[22] + 64), T = 64,
    B = 1, P = 64: 1190 boxes, so the box index passes 1024 and the carried soft passes 512; calls that begin at box 1023, 1024 and
    1025, and in another run one call."""
    def build(rng):
        cfg = dc_loose(rng, 64, 1, 64, last)
        return _dc_case("", 0, width, dc_words(rng, 3), cfg, dc_audio(rng, 2, 1190, width), [dc_run([1023, 1, 1]), dc_run([])],
                        sring=1 << max(7, (last + 63).bit_length()))
    return _dc_drawn("ring-%d-w%d" % (last, width), 9800 + last + width, build)


def dc_taps_T(T, width):
    """3b: every T at B = 8, P = 192, cut 7 | 333 | rest"""

    def build(rng):
        return _dc_case("", 0, width, dc_words(rng, 4), dc_loose(rng, 192, 8, T, 40), dc_audio(rng, 2, 4 * 192 + 50, width), [dc_run([7, 333])])
    return _dc_drawn("T%d-w%d" % (T, width), 9900 + 2 * T + width, build)


DC_TIES = ((3, 19), (15, 16), (0, 127), (31, 32))            # the same lane of 16, lanes 15 and 0, the ends, lanes 15 and 0 again
DC_UP, DC_DOWN = 0x3FFFFF, 0x400000


def dc_tie(pair, swapped, min_hits, width):
    """3c: F = 128, tap = 0 ... 0, 1: a sample above the one before it slices to 0x3FFFFF and one below it to 0x400000, so 20, 10,
    20, 10, ... gives every whole block (P = 64, B = 1) 32 hits on each of the two words, which stand at the indices `pair` in
    either order; the first index is f*.  min_hits 32 is met exactly, 33 missed by one.  Two blocks and a sample, cut at 64."""
    words = [5] * 128
    words[pair[0]], words[pair[1]] = (DC_DOWN, DC_UP) if swapped else (DC_UP, DC_DOWN)
    cfg = dr.Cfg(64, 1, [1], 0, [0] * 22 + [1], 0, min_hits, 1, 0, 1, DC_ALL)
    x = np.repeat(np.tile(np.array([20, 10], np.int16), 65)[None, :129, None], width, axis=2)
    return _dc_case("tie-%d-%d-%d-%d-w%d" % (pair + (swapped, min_hits, width)), 0, width, words, cfg, x, [dc_run([64])], first=min(pair))


def dc_in_place(off, width):
    """3d: in place with every row `off` samples behind a 16-byte boundary; 35 rows, P = 192, B = 8, calls that begin 37, 137 and
    470 samples into the stream: inside a chunk, a box and a block."""
    def build(rng):
        return _dc_case("", 0, width, dc_words(rng, 65), dc_loose(rng, 192, 8, 33, 22), dc_audio(rng, 35, 4 * 192 + 50, width),
                        [dc_run([37, 100, 333], "at", off, in_place=True)])
    return _dc_drawn("inplace-%d-w%d" % (off, width), 10000 + off + width, build)


DC_CAP_BLOCKS = 65600


def dc_confirm_cap():
    """3e: P = 64, B = 1, confirm = 255, a constant input over 65600 blocks in one call and one row.  Every block's decision is the
    same (a constant soft slices to the word 0, word 1 of the table; the first block has 42 such k, the others 64), so the state
    is dcs_ref.step over 65600 equal decisions: the gate opens with block 254 and stays open while cnt stands at its cap 65535.
    Returns (case, expected output, expected status)."""
    P = 64
    cfg = dr.Cfg(P, 1, [1], 0, list(range(23)), 0, P - 23, 255, 0, 1, 0b10)
    x = np.full((1, DC_CAP_BLOCKS * P, 1), 1234, np.int16)
    state, s = (dr.NONE, dr.NONE, 0, 0), []
    for _ in range(DC_CAP_BLOCKS):
        state, sj = dr.step(state, 1, cfg)
        s.append(sj)
    g = np.repeat(np.array([0] + s[:-1], np.int64), P)       # ramp 1: g[i] = s_{j-1}
    exp = ((x[0, :, 0].astype(np.int64) * g) >> 8).astype(np.int16)[None, :, None]
    c = _dc_case("confirm-cap", 0, 1, [0x2AAAAA, 0], cfg, x, [dc_run([])], opens=s.index(256), state=state)
    return c, exp, ([1], [P], [True])


def dc_reference(c, run):
    """[(lo, hi, the gated samples, N, status)] of every call of run `run` of the case, and the definition behind them"""
    key = (c.name, run)
    if key not in _DC_REF:
        ref, out = dr.CodeSquelch(c.words, c.cfg), []
        for lo, hi in dc_pieces(c, c.runs[run]):
            exp = ref.push(c.x[:, lo:hi])
            out.append((lo, hi, exp, ref.N, ref.status()))
        _DC_REF[key] = (out, ref)
    return _DC_REF[key]


# ---- the pager front end's cases ---------------------------------------------------------------------------------------------------
FK_CHUNK = 64                                                 # boxes per chunk, a lane each, counted from the box the call starts in


def fk_run(cuts, offs=None):
    """One run on a fresh handle: the pieces `cuts`, then the rest.  offs: per call (off_in, off_out) for rows_gpu.call_at (the rows
    start that many samples behind a 16-byte boundary); None: rows_gpu.call with an odd out_cap."""
    return NS(cuts=list(cuts), offs=offs)


def _fk_case(name, sd, cfg, x, runs, **claim):
    return NS(name=name, seed=seed(sd), cfg=cfg, rows=x.shape[0], x=np.ascontiguousarray(x, np.int16), runs=runs, claim=NS(**claim))


def fk_pieces(c, r):
    out, lo = [], 0
    for n in r.cuts + [c.x.shape[1]]:
        hi = min(c.x.shape[1], lo + n)
        if hi > lo:
            out.append((lo, hi))
        lo = hi
    return out


_FK_REF = {}


def fk_reference(c, run, rows=None):
    """[(lo, hi, out, counts, records, (inputs, outputs))] of every call of run `run` of the case over `rows` (all of them)"""
    key = (c.name, run, None if rows is None else tuple(rows))
    if key not in _FK_REF:
        x = c.x if rows is None else c.x[list(rows)]
        ref, out = fr.FskDemod(c.cfg, x.shape[0]), []
        for lo, hi in fk_pieces(c, c.runs[run]):
            want, counts, rec = ref.run(x[:, lo:hi])
            out.append((lo, hi, want, counts, rec, (ref.pos, ref.outputs())))
        _FK_REF[key] = out
    return _FK_REF[key]


def fk_hits(c, run, rows=None):
    """[(row, k, d, C, thr)] of every recorded hit of the run, k counted from the stream's start"""
    out = []
    for lo, hi, want, counts, rec, _ in fk_reference(c, run, rows):
        for r in range(rec.shape[0]):
            for h in rec[r, :min(int(counts[r]), c.cfg.hit_cap)]:
                out.append((r, lo // c.cfg.D + int(h["k_rel"]), int(h["d"]), int(h["corr"]), int(h["thr"])))
    return out


def fk_every_shape(D, W):
    """2a: one (D, W) of all 1024 at tap[31] = 255, three rows of sync words in noise over (255 + 64 + 70) D + r samples, r drawn
    below D, cut 255 D + 3 D + r | rest (the second call carries everything and has a second chunk), and uncut."""
    sd = 11000 + 100 * D + W
    rng = np.random.default_rng(seed(sd))
    cfg = fr.random_cfg(rng, D, W, 255)
    r = int(rng.integers(0, D))
    n = (255 + 64 + 70) * D + r
    return _fk_case("D%d-W%d" % (D, W), sd, cfg, fr.laid_signal(rng, cfg, 3, n), [fk_run([258 * D + r]), fk_run([])], r=r)


FK_CARRY = [(1, 16, 255), (3, 5, 100), (64, 16, 255), (7, 1, 0)]
FK_OUT_OFFS = (0, 3, 5)


def fk_carries(D, W, last):
    """2b: 24 calls of 33 boxes (34 for every e-th call) and, where D > 1, one sample, so that the calls' first boxes take every
    residue mod 16 and the samples of the open box that earlier calls brought every count below min(D, 8); e is the smallest that
    does it.  Call i runs at the input offset i mod 8 and the output offset (0, 3, 5)[i mod 3]; then the rest at (0, 0).  3 rows."""
    sd = 11900 + D + W
    rng = np.random.default_rng(seed(sd))
    cfg = fr.random_cfg(rng, D, W, last, tol=6 if last == 0 else 3)
    for e in range(1, 8):
        cuts = [(33 + (i % e == e - 1)) * D + (D > 1) for i in range(24)]
        starts = np.concatenate([[0], np.cumsum(cuts)[:-1]])
        if {int(p) // D % 16 for p in starts} == set(range(16)) and {int(p) % D for p in starts} >= set(range(min(D, 8))):
            break
    else:
        raise AssertionError("no call pattern")
    n = sum(cuts) + 70 * D
    x = fr.laid_signal(rng, cfg, 3, n) if last else rng.integers(-20000, 20000, (3, n)).astype(np.int16)
    offs = [(i % 8, FK_OUT_OFFS[i % 3]) for i in range(24)] + [(0, 0)]
    return _fk_case("carry-D%d-W%d" % (D, W), sd, cfg, x, [fk_run(cuts, offs)])


FK_LINE = 1 << 16


def lay(soft, cfg, at, sign, amp=2000):
    """the sync word into soft [nk] so that it ends at soft sample `at`: W box sums at the bit's level end at its tap"""
    for j in range(31, -1, -1):
        hi = at - int(cfg.tap[j]) + 1
        soft[hi - cfg.W:hi] = sign * (amp if (cfg.sync >> j) & 1 else -amp)


def fk_line(D):
    """2c: a stream across box 65536, where the host's 16-bit count of the call's first box wraps.  One call ends 100 boxes
    before the line, one of 200 boxes straddles it, one comes after it; then the stream in one call.  Words end 60 boxes before the
    line, 50 behind it (its taps straddle the line: tap[31] = 155) and 250 behind it; row 1 has them inverted."""
    sd = 12000 + D
    rng = np.random.default_rng(seed(sd))
    cfg = fr.random_cfg(rng, D, 2, 155, min_corr=20000, hit_cap=16)       # (min_corr: noise does not hit)
    nk = FK_LINE + 330
    soft = rng.integers(-500, 500, (2, nk))
    ats = (FK_LINE - 60, FK_LINE + 50, FK_LINE + 250)
    for r in range(2):
        for at in ats:
            lay(soft[r], cfg, at, 1 - 2 * r)
    x = np.repeat(soft, D, axis=1) * (1 << cfg.shift) // (D * cfg.W)
    return _fk_case("line-D%d" % D, sd, cfg, x, [fk_run([(FK_LINE - 100) * D, 200 * D]), fk_run([])], ats=ats)


# 2d: the rule's equalities at D = W = 1, shift 0 (x is soft), tap = 0 ... 31, one row of 32 samples: the verdict on k = 31
FK_SYNC = 0x7CD215D8


def _word(w, a, b=None):
    return [a if (w >> (31 - i)) & 1 else (-a if b is None else b) for i in range(32)]


def fk_rule(x, cfg, variant=None):
    """The definition's hits over one row (fsk_ref.fsk_row) with one comparison of the rule exchanged: "bit" 32 v >= thr, "tol"
    d < tol, "inv" d > 32 - tol, "corr" C > min_corr and -C > min_corr."""
    x = [int(v) for v in x]
    nk = len(x) // cfg.D
    b = [sum(x[k * cfg.D:(k + 1) * cfg.D]) for k in range(nk)]
    soft = [sum(b[k - t] for t in range(cfg.W) if k - t >= 0) >> cfg.shift for k in range(nk)]
    hits = []
    for k in range(nk):
        v = [soft[k - int(t)] if k - int(t) >= 0 else 0 for t in cfg.tap]
        thr = sum(v)
        w = sum((1 if (32 * v[j] >= thr if variant == "bit" else 32 * v[j] > thr) else 0) << j for j in range(32))
        d = bin(w ^ cfg.sync).count("1")
        c = sum(v[j] if (cfg.sync >> j) & 1 else -v[j] for j in range(32))
        ok = (lambda a: a > cfg.min_corr) if variant == "corr" else (lambda a: a >= cfg.min_corr)
        if (d < cfg.tol if variant == "tol" else d <= cfg.tol) and ok(c):
            hits.append((k, d, c, thr))
        elif (d > 32 - cfg.tol if variant == "inv" else d >= 32 - cfg.tol) and ok(-c):
            hits.append((k, d | 1 << 31, c, thr))
    return hits


def _flip(w, n):
    """w with n of its bits exchanged, spread over the word"""
    for i in range(n):
        w ^= 1 << ((2 * i + 1) % 32)
    return w


def fk_equalities():
    """[(case, the exchanged comparison that the case tells, whether k = 31 hits)]"""
    tap = np.arange(32, dtype=np.uint32)
    out = []

    def add(name, cfg, soft, variant, hits):
        x = np.asarray(soft, np.int16)[None]
        out.append((_fk_case("rule-" + name, 0, cfg, x, [fk_run([])]), variant, hits))
    cfg = fr.Cfg(1, 1, 0, tap, FK_SYNC, 2, 1024, 64)
    add("corr-at", cfg, _word(FK_SYNC, 32), "corr", True)                        # C = 32 * 32 = min_corr
    add("corr-below", cfg._replace(min_corr=1025), _word(FK_SYNC, 32), None, False)
    for tol in (0, 3, 15):
        c = cfg._replace(tol=tol, min_corr=0)
        add("d-tol-%d" % tol, c, _word(_flip(FK_SYNC, tol), 1000), "tol" if tol else None, True)
        add("d-tol-%d-plus-1" % tol, c, _word(_flip(FK_SYNC, tol + 1), 1000), None, False)
        add("inv-tol-%d" % tol, c, _word(_flip(FK_SYNC, tol) ^ 0xFFFFFFFF, 1000), "inv" if tol else None, True)
        add("inv-tol-%d-plus-1" % tol, c, _word(_flip(FK_SYNC, tol + 1) ^ 0xFFFFFFFF, 1000), None, False)
    w16 = 0xFFFF0000
    soft = _word(w16, 248)
    soft[16] = 8                                             # a sample whose 32-fold is the sum: 16 * 248 - 15 * 248 + 8 = 256 = 32 * 8
    add("bit-at", fr.Cfg(1, 1, 0, tap, w16, 0, 0, 64), soft, "bit", True)
    soft = list(soft)
    soft[16] = 9                                             # above the mean: bit 1, one bit off
    add("bit-above", fr.Cfg(1, 1, 0, tap, w16, 0, 0, 64), soft, None, False)
    add("constant", fr.Cfg(1, 1, 0, tap, 0, 0, 0, 64), [-5] * 32, "bit", True)    # all 32 v == thr: the word is 0
    return out


def fk_top(sync):
    """2d: the top of min_corr: every sample -32768 at D = W = 4, shift 4, so soft is -32768 and C is +-2^20 = min_corr at every
    settled k (k >= 34 of 80): normal hits on sync 0, inverted ones on sync 0xFFFFFFFF, at tol 0."""
    cfg = fr.Cfg(4, 4, 4, np.arange(32, dtype=np.uint32), sync, 0, 1 << 20, 64)
    return _fk_case("top-%08x" % sync, 0, cfg, np.full((1, 320), -32768, np.int16), [fk_run([]), fk_run([131])])


FK_SHIFTS = [(1 << min(s, 6), 1 << (s - min(s, 6)), s) for s in range(11)] + [(3, 5, 4), (1, 1, 10), (64, 15, 10)]


def fk_shift(D, W, shift):
    """2e: one shift: two rows of stretches on either rail, of noise and of -1 (the arithmetic shift), cut inside a stretch"""
    sd = 12100 + 100 * shift + D + W
    rng = np.random.default_rng(seed(sd))
    cfg = fr.random_cfg(rng, D, W, 40 * W if 40 * W <= 255 else 255, tol=15)._replace(shift=shift)
    nk = 400
    kinds = rng.integers(0, 4, (2, nk // 20 + 1))
    kinds[0, :4] = [0, 1, 3, 2]
    lv = np.repeat(kinds, 20 * D, axis=1)[:, :nk * D]
    x = np.where(lv == 0, -32768, np.where(lv == 1, 32767, np.where(lv == 3, -1, rng.integers(-32768, 32768, lv.shape))))
    return _fk_case("shift%d-D%d-W%d" % (shift, D, W), sd, cfg, x, [fk_run([130 * D + D // 2])])


FK_CAPS = (1, 2, 63, 64)


def fk_records(hit_cap):
    """2f: D = 3, W = 1, sync 0 at tol 0: a constant negative stretch of 32 boxes and more slices to the word 0, a hit at every k
    behind its first 31; noise never does.  Row 0 is constant throughout (every lane of a whole chunk hits, and the count passes
    hit_cap inside a chunk), row 1 is constant over the boxes 32 ... 64 (hits at k = 63 and 64: lane 63 of chunk 0 and lane 0 of
    chunk 1 of the one call), row 2 is noise.  One call, and the calls 122 | rest: the second starts inside box 40, and its k_rel
    count from there."""
    rng = np.random.default_rng(seed(12300))
    cfg = fr.Cfg(3, 1, 2, np.arange(32, dtype=np.uint32), 0, 0, 0, hit_cap)
    n = 3 * 200 + 1
    x = rng.integers(-20000, 20000, (3, n)).astype(np.int16)
    x[0] = -1000
    x[1, 3 * 32:3 * 65] = -1000
    return _fk_case("records-cap%d" % hit_cap, 12300, cfg, x, [fk_run([]), fk_run([122])])


FK_ROWS = (4, 5, 8, 9)
FK_MANY = 40000


def fk_rows(rows):
    """2g: the tile of 4 rows at 4, 5, 8 and 9 rows, and 40000 rows (16 sampled ones compared): D = 2, W = 4, row r carries one of
    16 laid signals, cut 333 | rest."""
    sd = 12400 + rows % 1000
    rng = np.random.default_rng(seed(sd))
    cfg = fr.random_cfg(rng, 2, 4, 60, hit_cap=8)
    base = fr.laid_signal(rng, cfg, 16, 2 * 400 + 1)
    which = (5 * np.arange(rows) + np.arange(rows) // 16) % 16
    c = _fk_case("rows-%d" % rows, sd, cfg, base[which], [fk_run([333])])
    c.sample = sampled_rows(np.random.default_rng(sd), rows) if rows > 1000 else list(range(rows))
    return c
