"""The definition of the host slicer behind the pulse bank (include/fmd.h, fmd_pulse_slicer_*) in plain Python: the pulse records of
one stream in, bit packages out.

A package is a maximal run of pulses in which every pulse but the first has gap < reset.  It closes on the next record with gap >=
reset, or on idle(state, run) with state == 0 and run >= reset.  PWM: a pulse gives a 1 if |width - short| <= tol, else a 0 if |width -
long| <= tol.  PPM: every pulse but the package's first gives a bit from its gap: 0 if |gap - short| <= tol, else 1 if |gap - long| <=
tol.  A pulse that fits neither sets BAD and the rest of the package gives no bits.  256 bits are kept, MSB first; a bit beyond sets
TRUNCATED.  n_pulses counts every pulse.  start is the absolute sample of the first pulse's rise.  64 closed packages wait; one that
closes while 64 wait is dropped."""
PWM, PPM = 0, 1
BAD, TRUNCATED = 1, 2
WAITING, MAX_BITS = 64, 256


class Slicer:
    def __init__(self, modulation, short, long, tol, reset):
        assert modulation in (PWM, PPM) and short >= 1 and long >= 1 and reset >= 1
        self.modulation, self.short, self.long, self.tol, self.reset = modulation, short, long, tol, reset
        self.cur, self.waiting = None, []

    def _close(self):
        if len(self.waiting) < WAITING:
            k = dict(self.cur)
            k["bits"] = bytes(k["bits"])
            self.waiting.append(k)
        self.cur = None

    def push(self, recs, pos):
        """recs: dicts with k_rel, width, gap; pos: the absolute sample of the call's first."""
        for r in recs:
            if self.cur is not None and r["gap"] >= self.reset:
                self._close()
            first = self.cur is None
            if first:
                self.cur = {"start": max(0, pos + r["k_rel"] - r["width"]), "n_pulses": 0, "n_bits": 0, "bits": bytearray(32), "flags": 0}
            k = self.cur
            k["n_pulses"] += 1
            if k["flags"] & BAD:
                continue
            if self.modulation == PWM:
                v, ones = r["width"], (1, 0)
            elif first:
                continue
            else:
                v, ones = r["gap"], (0, 1)
            if abs(v - self.short) <= self.tol:
                bit = ones[0]
            elif abs(v - self.long) <= self.tol:
                bit = ones[1]
            else:
                k["flags"] |= BAD
                continue
            if k["n_bits"] == MAX_BITS:
                k["flags"] |= TRUNCATED
                continue
            if bit:
                k["bits"][k["n_bits"] >> 3] |= 0x80 >> (k["n_bits"] & 7)
            k["n_bits"] += 1

    def idle(self, state, run):
        if self.cur is not None and state == 0 and run >= self.reset:
            self._close()

    def take(self, cap=WAITING):
        out, self.waiting = self.waiting[:cap], self.waiting[cap:]
        return out
