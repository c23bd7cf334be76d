"""What the page bank's tests share (tests/test_pager.py, tests/test_gpu_pager.py): lines of POCSAG bits as soft decisions with their
sync-word records at any rate, the packing of a call's records, and the kernel's step restated in plain Python -- the
event loop from one due sample to the next, p(n) formed from the previous bit's quotient and remainder, the correction through the
table of 2048 flip masks, the open message's bits kept as bytes with a word laid down as two bytes and a nibble."""
import numpy as np

import pager_ref as gr
import pocsag_ref as pr

U32 = (1 << 32) - 1
# (rate_num, rate_den, baud): rate / baud 2, 5, 32, 11025 / 2400, and rate_num = 2^32 - 1 at both ends of the domain
RATES = {"2": (2400, 1, 1200), "5": (6000, 1, 1200), "32": (38400, 1, 1200), "11025-2400": (11025, 1, 2400), "3.5": (4200, 1, 1200),
         "wide-2": (U32, 1, U32 // 2), "wide-32": (U32, 1, (U32 + 31) // 32)}
SYNC_BITS = [(pr.SYNC >> b) & 1 for b in range(31, -1, -1)]


def line(bits, rate=(6000, 1, 1200), amp=3000, dc=0, invert=False, lead=40, tail=None):
    """(soft int16 [n], records [(k, d, corr, thr)]) of `bits` held mod / step samples each behind `lead` samples of the bare level:
    sample lead + i shows bit floor(i step / mod); a record at the middle sample of every sync word's last bit."""
    mod, step = rate[0], rate[1] * rate[2]
    bits = np.asarray(bits, np.int64)
    n = (len(bits) * mod) // step
    idx = (np.arange(n, dtype=np.int64) * step) // mod       # (n step < 2^63 for every line of the tests)
    tail = 40 * (mod // step) if tail is None else tail
    lvl = np.where(bits[idx] == 1, amp, -amp) * (-1 if invert else 1) + dc
    soft = np.concatenate([np.full(lead, dc), lvl, np.full(tail, dc)]).astype(np.int16)
    hits = []
    for i in range(len(bits) - 31):
        if bits[i:i + 32].tolist() == SYNC_BITS:
            k = lead + ((2 * (i + 31) + 1) * mod) // (2 * step)
            hits.append((k, 32 | 1 << 31 if invert else 0, (-32 if invert else 32) * amp, 32 * dc))
    return soft, hits


def pack(rows_hits, lo, n, hit_cap=16):
    """(counts uint32 [rows], records [rows, hit_cap]) of the call [lo, lo + n): every row's records in it, k_rel counted from lo"""
    counts, rec = np.zeros(len(rows_hits), np.uint32), np.zeros((len(rows_hits), hit_cap), gr.HIT_DTYPE)
    for r, hits in enumerate(rows_hits):
        mine = [(k - lo, d, c, t) for k, d, c, t in hits if lo <= k < lo + n]
        counts[r] = len(mine)
        for j, h in enumerate(mine[:hit_cap]):
            rec[r, j] = h
    return counts, rec


def stack(lines, fill=0):
    """[(soft, hits)] of different lengths -> (soft [rows, n], [hits])"""
    n = max(len(s) for s, _ in lines)
    x = np.full((len(lines), n), fill, np.int16)
    for r, (s, _) in enumerate(lines):
        x[r, :len(s)] = s
    return x, [h for _, h in lines]


# ---- the kernel's step -------------------------------------------------------------------------------------------------------------
NONE = 0xFFFFFFFF


def key(e):
    c = (e >> 1) & 0x7FFFFFFF
    for i in range(30, 9, -1):
        if (c >> i) & 1:
            c ^= pr.POLY << (i - 10)
    return (c & 0x3FF) << 1 | (bin(e).count("1") & 1)


def table(max_errors):
    """the flip masks: the error patterns in the definition's order, each at the remainder and parity it leaves on any codeword"""
    t = [NONE] * 2048
    t[key(0)] = 0
    if max_errors >= 1:
        for a in range(32):
            if t[key(1 << a)] == NONE:
                t[key(1 << a)] = 1 << a
    if max_errors >= 2:
        for a in range(32):
            for b in range(a + 1, 32):
                if t[key(1 << a | 1 << b)] == NONE:
                    t[key(1 << a | 1 << b)] = 1 << a | 1 << b
    return t


class Model:
    """One lane of fmd_pg::fmd_pager_kernel: the state of csrc/fmd_pager.hip under its names."""

    def __init__(self, rate_num, rate_den=1, baud=1200, max_errors=1):
        mod, step = rate_num, baud * rate_den
        self.r = (2 * mod + step) // (2 * step)
        self.half = self.r // 2
        self.q544 = (2 * 544 * mod + step) // (2 * step)
        self.qd, self.rd, self.rem1, self.two_step = mod // step, 2 * (mod % step), (2 * mod + step) % (2 * step), 2 * step
        assert self.two_step <= U32 and self.rd < self.two_step and self.rem1 < self.two_step
        self.table = table(max_errors)
        self.n0 = 0
        self.tail = [0] * 64
        self.window = self.locked = self.inv = self.xinv = self.best = self.open = self.cinv = False
        self.nbm1 = self.word = self.kp = self.xk = self.xthr = self.xcorr = self.thr = self.rem = self.pnext = 0
        self.c_addr = self.c_func = self.c_nbits = self.c_corr = self.c_end = 0
        self.bits = bytearray(320)
        self.messages = self.batches = self.bad = self.orph = 0
        self.behind = 0                                      # bits read behind the sample that made them due

    def info(self):
        return {"messages": self.messages, "batches": self.batches, "bad_codewords": self.bad, "orphans": self.orph,
                "locked": int(self.locked), "searching": int(not self.locked and self.window)}

    # the step's arithmetic that a kernel could get wrong on its own: tests/test_pager_domain.py derives its wrong kernels from these
    @staticmethod
    def _mag(c):
        return -c if c < 0 else c

    def _n(self, n0, i):
        return n0 + i

    def _sum(self):
        return self.rem + self.rd

    def _inside(self, n):
        return n <= self.kp + self.r

    def _near(self, n):
        return abs(n - self.kp) <= self.half

    def _pol(self, hinv):
        return hinv == self.inv

    def _close(self, out):
        if self.open:
            self.open = False
            self.messages += 1
            ln = (min(self.c_nbits, 2560) + 7) // 8
            out.append({"address": self.c_addr, "function": self.c_func, "n_bits": self.c_nbits, "bits": bytes(self.bits[:ln]),
                        "corrected": self.c_corr, "inverted": int(self.cinv), "end_sample": self.c_end})

    def _anchor(self, k, t):
        self.thr, self.nbm1, self.word, self.best = t, 0, 0, False
        self.kp, self.pnext, self.rem = k + self.q544, k + self.r, self.rem1
        self.batches += 1

    def push(self, soft, hits=()):
        soft = [int(v) for v in soft]
        hits = [tuple(int(v) for v in h) for h in hits]
        n_in, n0, cnt, out = len(soft), self.n0, len(hits), []
        busy = bool(cnt) or self.window or self.locked
        i = hi = 0
        hk = hits[0][0] if cnt else NONE
        at = False
        while busy:
            if not at:
                while hk < i:
                    hi += 1
                    hk = hits[hi][0] if hi < cnt else NONE
                dr = NONE
                if self.window or self.locked:
                    due = (self.pnext if self.nbm1 < 512 else self.kp + self.half) if self.locked else self.kp + self.r
                    if due <= n0 + i:
                        dr = i
                    elif due - n0 < n_in:
                        dr = due - n0
                nx = min(dr, hk)
                if nx >= n_in:
                    busy = False
                else:
                    i, at = nx, True
                    n = self._n(n0, i)
                    while hk <= i:
                        if hk == i:
                            _, d, hcorr, hthr = hits[hi]
                            hinv = bool(d >> 31)
                            if not self.locked:
                                if not self.window:
                                    self.window, self.xinv, self.kp, self.xk, self.xthr, self.xcorr = True, hinv, n, n, hthr, hcorr
                                elif self._inside(n) and self._mag(hcorr) > self._mag(self.xcorr):
                                    self.xinv, self.xk, self.xthr, self.xcorr = hinv, n, hthr, hcorr
                            elif self._near(n) and self._pol(hinv) and (not self.best or self._mag(hcorr) > self._mag(self.xcorr)):
                                self.best, self.xk, self.xthr, self.xcorr = True, n, hthr, hcorr
                        hi += 1
                        hk = hits[hi][0] if hi < cnt else NONE
                    if self.window and not self.locked and n >= self.kp + self.r:
                        self.window, self.locked, self.inv = False, True, self.xinv
                        self._anchor(self.xk, self.xthr)
            if busy and at:
                n = self._n(n0, i)
                leave = False
                if not self.locked:
                    leave = True
                elif self.nbm1 < 512:
                    if self.pnext > n:
                        leave = True
                    else:
                        p = self.pnext
                        assert n - 63 <= p                   # (inside the tail)
                        self.behind += int(p != n)
                        v = soft[p - n0] if p >= n0 else self.tail[(64 - (n0 - p)) & 63]
                        self.word = (self.word << 1 | (int(32 * v > self.thr) ^ int(self.inv))) & U32
                        nb = self.nbm1 + 1
                        if nb % 32 == 0:
                            m = self.table[key(self.word)]
                            cw, nfix = self.word ^ m, bin(m).count("1")
                            if m == NONE:
                                self.bad += 1
                                self._close(out)
                            elif cw == pr.IDLE:
                                self._close(out)
                            elif not cw >> 31:
                                self._close(out)
                                self.c_addr, self.c_func = ((cw >> 13) & 0x3FFFF) << 3 | ((nb // 32 - 1) >> 1), (cw >> 11) & 3
                                self.c_nbits, self.c_corr, self.c_end, self.open, self.cinv = 0, nfix, p, True, self.inv
                            elif not self.open:
                                self.orph += 1
                            else:
                                data = (cw >> 11) & 0xFFFFF
                                if self.c_nbits < 2560:
                                    b = self.c_nbits >> 3
                                    if self.c_nbits & 7 == 0:
                                        self.bits[b], self.bits[b + 1], self.bits[b + 2] = data >> 12, (data >> 4) & 255, (data << 4) & 255
                                    else:
                                        self.bits[b], self.bits[b + 1], self.bits[b + 2] = self.bits[b] | data >> 16, (data >> 8) & 255, data & 255
                                self.c_nbits += 20
                                self.c_corr += nfix
                                self.c_end = p
                            self.word = 0
                        self.nbm1 = nb
                        t = self._sum()
                        carry = t >= self.two_step
                        self.rem = t - self.two_step if carry else t
                        self.pnext += self.qd + int(carry)
                        if self.nbm1 < 512 and self.pnext > n:
                            leave = True
                elif n < self.kp + self.half:
                    leave = True
                elif self.best:
                    self._anchor(self.xk, self.xthr)
                else:
                    self.locked = False
                    self._close(out)
                    leave = True
                if leave:
                    at = False
                    i += 1
                    if i >= n_in:
                        busy = False
        keep = min(n_in, 64)
        self.tail = self.tail[keep:] + soft[n_in - keep:]
        self.n0 += n_in
        return out
