"""The AX.25 frame decoder's definition (include/fmd.h, fmd_ax25_decoder_*) restated in plain Python integers, and the sending side the
tests need: the CRC, a frame's bits (FCS, bit stuffing, flags), NRZI and continuous-phase AFSK audio.  Integers only in the decoder:
C++ and Python agree frame for frame and counter for counter.

Per soft sample v (int16, positive: mark), with mod = rate_num and step = baud * rate_den:
    cur = (v >= 0)
    if cur != the previous sample's cur:  ph -= (ph - mod // 2) >> 2      (arithmetic shift of the signed difference)
    ph += step
    if ph >= mod:  ph -= mod, and a bit is taken:  bit = (cur == the level at the previous take)           (NRZI)
Per bit, in this order:
    sr = (sr >> 1) | (bit << 7); if sr == 0x7E: a flag: close the frame that is open (below), open the next, ones = 0
    else if bit: ones += 1; seven 1s in a row abort the open frame (counted) and close the receiver until the next flag
    else: a 0 after exactly five 1s is dropped (a stuffed bit); any 0 clears ones
    every bit that is not dropped goes to the open frame's buffer, LSB first; behind 514 bytes and 7 bits nothing more is stored
Closing with n = (stored bits) - 7 (the flag's first seven bits went in): n <= 0 is nothing (flags back to back); a frame needs
n % 8 == 0, 17 <= n / 8 <= 514 and the CRC-16/X.25 of all but the last two bytes equal to those two, low byte first; what fails
is counted in bad_fcs and not delivered."""
import numpy as np

MAX_BYTES = 514
MAX_BITS = MAX_BYTES * 8 + 7
MIN_BYTES = 17


def crc16_x25(data):
    crc = 0xFFFF
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    return crc ^ 0xFFFF


class Decoder:
    def __init__(self, rate_num, rate_den=1, baud=1200):
        self.mod, self.step = int(rate_num), int(baud) * int(rate_den)
        if not (self.step >= 1 and 4 * self.step <= self.mod <= 64 * self.step):
            raise ValueError("need 4 <= rate / baud <= 64")
        self.reset()

    def reset(self):
        self.ph, self.prev, self.level = 0, 1, 1
        self.sr, self.ones, self.in_frame, self.nbits = 0, 0, False, 0
        self.buf = bytearray(MAX_BYTES + 1)
        self.n = 0
        self.frames_ok = self.bad_fcs = self.aborts = 0

    def info(self):
        return {"frames_ok": self.frames_ok, "bad_fcs": self.bad_fcs, "aborts": self.aborts, "in_frame": int(self.in_frame)}

    def _close(self, frames):
        n = self.nbits - 7
        if n <= 0:
            return
        nb = n // 8
        if n % 8 == 0 and self.nbits <= MAX_BITS and MIN_BYTES <= nb <= MAX_BYTES:
            body = bytes(self.buf[:nb])
            if crc16_x25(body[:-2]) == body[-2] | body[-1] << 8:
                self.frames_ok += 1
                frames.append({"data": body[:-2], "end_sample": self.n})
                return
        self.bad_fcs += 1

    def _bit(self, bit, frames):
        self.sr = (self.sr >> 1) | (bit << 7)
        if self.sr == 0x7E:
            if self.in_frame:
                self._close(frames)
            self.in_frame, self.nbits, self.ones = True, 0, 0
            return
        if bit:
            self.ones += 1
            if self.ones >= 7:
                if self.in_frame:
                    self.aborts += 1
                self.in_frame = False
                self.ones = 7
                return
        else:
            stuffed = self.ones == 5
            self.ones = 0
            if stuffed:
                return
        if self.in_frame:
            if self.nbits < MAX_BITS:
                if self.nbits & 7 == 0:
                    self.buf[self.nbits >> 3] = 0
                self.buf[self.nbits >> 3] |= bit << (self.nbits & 7)
            self.nbits += 1 if self.nbits <= MAX_BITS else 0

    def push(self, soft):
        """soft: int16 [n]; the frames completed, {"data": bytes without the FCS, "end_sample": the index of the sample that took the
        closing flag's last bit}."""
        frames = []
        mod, step, half = self.mod, self.step, self.mod // 2
        for v in np.asarray(soft, np.int16).tolist():
            cur = 1 if v >= 0 else 0
            if cur != self.prev:
                self.ph -= (self.ph - half) >> 2
            self.prev = cur
            self.ph += step
            if self.ph >= mod:
                self.ph -= mod
                self._bit(1 if cur == self.level else 0, frames)
                self.level = cur
            self.n += 1
        return frames


# ---- the sending side ---------------------------------------------------------------------------------------------------------------
def address(call, ssid=0, last=False, repeated=False):
    return bytes((ord(c) << 1) for c in call.ljust(6)) + bytes([0x60 | (0x80 if repeated else 0) | (ssid << 1) | (1 if last else 0)])


def ui_frame(dst, src, info, digis=()):
    """An APRS-style UI frame without the FCS: dst, src, digis are (call, ssid) or (call, ssid, repeated)."""
    parts = [address(dst[0], dst[1]), address(src[0], src[1], last=not digis)]
    for i, d in enumerate(digis):
        parts.append(address(d[0], d[1], last=i == len(digis) - 1, repeated=len(d) > 2 and d[2]))
    return b"".join(parts) + b"\x03\xf0" + bytes(info)


def with_fcs(data):
    c = crc16_x25(data)
    return bytes(data) + bytes([c & 0xFF, c >> 8])


FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def stuffed_bits(body):
    """The bits of `body` (bytes, FCS included), LSB first, with a 0 behind every five 1s."""
    bits, ones = [], 0
    for b in body:
        for k in range(8):
            bit = (b >> k) & 1
            bits.append(bit)
            ones = ones + 1 if bit else 0
            if ones == 5:
                bits.append(0)
                ones = 0
    return bits


def frame_bits(data, flags=8, closing=1):
    """`flags` flags, the frame `data` with its FCS, `closing` flags."""
    return FLAG * flags + stuffed_bits(with_fcs(data)) + FLAG * closing


def nrzi(bits, level=1):
    """The line levels (1: mark): a 0 toggles, a 1 keeps."""
    out = []
    for b in bits:
        if not b:
            level ^= 1
        out.append(level)
    return out


def afsk_audio(levels, rate, baud=1200, mark=1200, space=2200, amp=8000.0, twist=1.0, phase=0.0):
    """Continuous-phase AFSK of the line levels: float64 [n] and the end phase; the space tone's amplitude is twist * amp."""
    n = (len(levels) * rate) // baud
    lv = np.asarray(levels, np.int64)[(np.arange(n, dtype=np.int64) * baud) // rate]
    f = np.where(lv == 1, float(mark), float(space))
    ph = phase + 2 * np.pi * np.cumsum(f) / rate
    a = np.where(lv == 1, amp, amp * twist)
    return a * np.cos(ph), float(ph[-1]) if n else phase


def to_s16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)
