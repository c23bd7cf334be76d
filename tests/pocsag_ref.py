"""Integer definition of the POCSAG batch decoder (include/fmd.h, fmd_pocsag_decoder_*), restated for the tests, line for line what
csrc/fmd_pocsag_decode.cpp does: one row's soft decisions and sync-word records -> messages.

    mod = rate_num, step = baud * rate_den, r = (2 mod + step) // (2 step) soft samples per bit
    per sample, in this order: the sample is kept; its records are taken; a search window that is due closes; the bits and the slot
    that are due are read
    search  the first record opens a window anchored at its index k1; a later record with k <= k1 + r and strictly larger |corr|
            replaces the candidate; when sample k1 + r has arrived: lock on the candidate (k0, thr, inverted)
    locked  bit n >= 1 = (32 soft[p(n)] > thr) xor inverted, p(n) = k0 + (2 n mod + step) // (2 step); word i = bits 32 i + 1 ... 32 i +
            32, first bit highest; at sample p(544) + r // 2: of the records with |k - p(544)| <= r // 2 and the lock's polarity the
            first with the largest |corr| is the next batch's (k0, thr); with none the lock is lost and the open message closes
    word    corrected to the unique valid codeword within max_errors bits, else bad_codewords and the open message closes; idle closes;
            an address word closes and opens; a message word appends 20 bits, or counts in orphans"""

SYNC = 0x7CD215D8
IDLE = 0x7A89C197
POLY = 0x769
MAX_BITS = 2560
QUEUE = 64


def valid(w):
    c = (w >> 1) & 0x7FFFFFFF
    for i in range(30, 9, -1):
        if (c >> i) & 1:
            c ^= POLY << (i - 10)
    return c == 0 and bin(w).count("1") % 2 == 0


def correct(w, e):
    """(codeword, bits flipped) or None"""
    if valid(w):
        return w, 0
    if e >= 1:
        for a in range(32):
            if valid(w ^ (1 << a)):
                return w ^ (1 << a), 1
    if e >= 2:
        for a in range(32):
            for b in range(a + 1, 32):
                if valid(w ^ (1 << a) ^ (1 << b)):
                    return w ^ (1 << a) ^ (1 << b), 2
    return None


class _Window:
    """soft[a] during a push: the samples of the push, and the 64 before it"""

    def __init__(self, before, soft, n0):
        self.before, self.now, self.n0 = before, soft, n0

    def __getitem__(self, a):
        return self.now[a - self.n0] if a >= self.n0 else self.before[a]


class Decoder:
    def __init__(self, rate_num, rate_den, baud, max_errors=1):
        self.mod, self.step = rate_num, baud * rate_den
        assert 2 * self.step <= self.mod <= 32 * self.step and self.step >= 1 and max_errors <= 2
        self.r = (2 * self.mod + self.step) // (2 * self.step)
        self.max_errors = max_errors
        self.reset()

    def reset(self):
        self.soft = {}                                       # (everything: the C++ keeps the last 64)
        self.n = 0
        self.window = self.locked = False
        self.k1, self.cand = 0, None                         # cand: (k, thr, corr, inverted)
        self.k0 = self.p544 = self.thr = 0
        self.inv = False
        self.nb, self.word, self.best = 1, 0, None
        self.cur = None
        self.messages = self.batches = self.bad_codewords = self.orphans = 0
        self.queue = []

    def info(self):
        return {"messages": self.messages, "batches": self.batches, "bad_codewords": self.bad_codewords, "orphans": self.orphans,
                "locked": int(self.locked), "searching": int(not self.locked and self.window)}

    def _close(self):
        if self.cur is None:
            return
        m, self.cur = self.cur, None
        self.messages += 1
        nb = min(m["n_bits"], MAX_BITS)
        data = bytearray((nb + 7) // 8)
        for i, b in enumerate(m.pop("bitlist")[:nb]):
            data[i >> 3] |= b << (7 - (i & 7))
        m["bits"] = bytes(data)
        self.out.append(m)

    def _p(self, i):
        return self.k0 + (2 * i * self.mod + self.step) // (2 * self.step)

    def _anchor(self, k, thr):
        self.k0, self.thr, self.nb, self.word, self.best = k, thr, 1, 0, None
        self.p544 = self._p(544)
        self.batches += 1

    def _codeword(self, i, raw, at):
        got = correct(raw, self.max_errors)
        if got is None:
            self.bad_codewords += 1
            self._close()
            return
        cw, nfix = got
        if cw == IDLE:
            self._close()
            return
        if not cw >> 31:
            self._close()
            self.cur = {"address": ((cw >> 13) & 0x3FFFF) << 3 | (i >> 1), "function": (cw >> 11) & 3, "n_bits": 0, "bitlist": [],
                        "corrected": nfix, "inverted": int(self.inv), "end_sample": at}
            return
        if self.cur is None:
            self.orphans += 1
            return
        for b in range(19, -1, -1):
            if self.cur["n_bits"] < MAX_BITS:
                self.cur["bitlist"].append((cw >> (11 + b)) & 1)
            self.cur["n_bits"] += 1
        self.cur["corrected"] += nfix
        self.cur["end_sample"] = at

    def _record(self, k, d, corr, thr):
        inv = bool(d >> 31)
        if not self.locked:
            if not self.window:
                self.window, self.k1, self.cand = True, k, (k, thr, corr, inv)
            elif k <= self.k1 + self.r and abs(corr) > abs(self.cand[2]):
                self.cand = (k, thr, corr, inv)
            return
        if abs(k - self.p544) > self.r // 2 or inv != self.inv:
            return
        if self.best is None or abs(corr) > abs(self.best[2]):
            self.best = (k, thr, corr)

    def _advance(self):
        if not self.locked:
            if not self.window or self.n < self.k1 + self.r:
                return
            self.window, self.locked, self.inv = False, True, self.cand[3]
            self._anchor(self.cand[0], self.cand[1])
        while True:
            if self.nb <= 512:
                at = self._p(self.nb)
                if at > self.n:
                    return
                bit = int(32 * self.soft[at] > self.thr) ^ int(self.inv)
                self.word = self.word << 1 | bit
                if self.nb % 32 == 0:
                    self._codeword(self.nb // 32 - 1, self.word, at)
                    self.word = 0
                self.nb += 1
                continue
            if self.n < self.p544 + self.r // 2:
                return
            if self.best is not None:
                self._anchor(self.best[0], self.best[1])
                continue
            self.locked = False
            self._close()
            return

    def push(self, soft, hits=(), cap=None):
        """hits: records (k_rel, d, corr, thr) of this push.  Returns the messages delivered: all that closed, or with `cap` at most
        that many, the rest waiting in a queue of 64 whose oldest gives way.  Samples at which nothing is due (no record, no window
        closing, no bit, no slot) only pass, so the loop steps from one due sample to the next."""
        self.out = []
        hits = [tuple(int(v) for v in h) for h in hits]
        soft = [int(v) for v in soft]
        n0, hi, i = self.n, 0, 0
        for j, v in enumerate(soft[-64:], len(soft) - len(soft[-64:])):
            self.soft[n0 + j] = v                            # (only the last 64 of a push can be read by a later one)
        keep = dict(self.soft)
        self.soft = _Window(keep, soft, n0)
        while i < len(soft):
            while hi < len(hits) and hits[hi][0] < i:        # out of order: passed over
                hi += 1
            if self.locked:
                due = self._p(self.nb) if self.nb <= 512 else self.p544 + self.r // 2
            else:
                due = self.k1 + self.r if self.window else None
            nxt = [t for t in (None if due is None else due - n0, hits[hi][0] if hi < len(hits) else None) if t is not None]
            i = max(i, min(nxt)) if nxt else len(soft)
            if i >= len(soft):
                break
            self.n = n0 + i
            while hi < len(hits) and hits[hi][0] <= i:
                if hits[hi][0] == i:
                    self._record(self.n, hits[hi][1], hits[hi][2], hits[hi][3])
                hi += 1
            self._advance()
            i += 1
        self.n = n0 + len(soft)
        self.soft = {k: v for k, v in keep.items() if k >= self.n - 64}
        if cap is None:
            out, self.out = self.queue + self.out, []
            self.queue = []
            return out
        # the C++ order: first what waited, then straight into the caller's array while nothing waits, else into the ring
        res = []
        while len(res) < cap and self.queue:
            res.append(self.queue.pop(0))
        for m in self.out:
            if not self.queue and len(res) < cap:
                res.append(m)
            else:
                if len(self.queue) == QUEUE:
                    self.queue.pop(0)
                self.queue.append(m)
        self.out = []
        return res


def fsk_audio(rng, bits, rate, baud, amp, dc, noise=0.0, ppm=30.0, lead=0, tail=0, invert=False):
    """The int16 audio of one transmission as a discriminator gives it: +amp for a 1 and -amp for a 0 on `dc`, rectangular bits from a
    sender whose clock is `ppm` off at a random bit phase, `lead` and `tail` samples of the bare level around it, white noise of
    `noise` rms over all of it."""
    import numpy as np
    bits = np.asarray(bits, np.int64)
    per = rate / (baud * (1.0 + ppm * 1e-6))
    n = int(np.ceil(len(bits) * per)) + 1
    idx = np.floor((np.arange(n) + rng.random()) / per).astype(np.int64)
    keep = idx < len(bits)
    lvl = np.where(bits[idx[keep]] == 1, 1.0, -1.0) * (-1.0 if invert else 1.0)
    x = np.concatenate([np.zeros(lead), amp * lvl, np.zeros(tail)]) + dc
    if noise:
        x = x + rng.normal(0.0, noise, x.shape)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)
