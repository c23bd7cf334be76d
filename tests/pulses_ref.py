"""The definition of the pulse bank (include/fmd.h, "Pulse bank") in plain Python / numpy.  This file is the definition: the library's
kernels are held to it.  Everything is per stream; i counts samples from creation or reset and everything at a negative index is 0.

    m[i]  = ((2 b[2i] - 255)^2 + (2 b[2i+1] - 255)^2) >> 1          (exactly the Mode S bank's m)
    e[i]  = m[i] + m[i-1] + ... + m[i-W+1]                            (a box of W samples)
    s[i]  = 1 if e[i] >= hi;  0 if e[i] < lo;  else s[i-1];   s[-1] = 0
    rise at i: s[i] = 1, s[i-1] = 0.     fall at i: s[i] = 0, s[i-1] = 1.

Every fall at f gives one record, in increasing f: k_rel = f - pos; width = f - r, r the rise before f; gap = r - f_prev, f_prev the
fall before r, 0 if there has been none since creation or reset; level = e[f - 1].  width and gap saturate at 2^32 - 1.  A fall is
decided by the call that brings sample f.  Cumulative: samples, pulses (falls), rises, the current s as `state`, and `run`, the samples
since the last edge or since reset."""
import numpy as np

from modes_ref import magnitude

SAT = 2 ** 32 - 1
TAIL = 64                                                    # the largest box


class Stream:
    """One stream of the definition: run(bytes) takes a call and returns (count, records) -- every fall of the call, as dicts in
    increasing position; the caller keeps the first pulse_cap.  info is the cumulative counters with state and run."""

    def __init__(self, W=8, lo=30000, hi=60000):
        self.W, self.lo, self.hi = int(W), int(lo), int(hi)
        assert 1 <= self.W <= TAIL and 1 <= self.lo <= self.hi <= 64 * 65025
        self.reset()

    def reset(self):
        self.pos = 0
        self.tail = np.zeros(TAIL, np.int64)                 # m[pos - 64 ... pos - 1]
        self.state, self.run_len, self.gap = 0, 0, 0         # s, the samples since the last edge, the open pulse's gap
        self.info = {"samples": 0, "pulses": 0, "rises": 0, "state": 0, "run": 0}

    def box(self, b):
        """e[pos - 1 ... pos + n - 1] of the call's bytes b, as int64 [n + 1]; leaves the carried samples as they are."""
        v = np.concatenate([self.tail, magnitude(b)])        # v[64 + u] = m[pos + u]
        c = np.concatenate([[0], np.cumsum(v)])
        u = np.arange(-1, v.size - TAIL)
        return c[TAIL + 1 + u] - c[TAIL + 1 + u - self.W], v

    def run(self, b):
        b = np.asarray(b, np.uint8)
        assert b.size % 2 == 0
        n = b.size // 2
        e, v = self.box(b)                                   # e[1 + u] is the box at the call's sample u
        definite = (e[1:] >= self.hi) | (e[1:] < self.lo)
        last = np.maximum.accumulate(np.where(definite, np.arange(n), -1))       # the nearest definite sample at or below u
        s = np.where(last >= 0, e[1:][np.maximum(last, 0)] >= self.hi, self.state).astype(np.int64)
        before = np.concatenate([[self.state], s[:-1]])
        recs, at = [], 0                                     # at: the call's sample up to which run_len counts
        for u in np.nonzero(s != before)[0].tolist():
            self.run_len += u - at
            if s[u]:                                         # a rise
                self.gap = min(self.run_len, SAT) if self.info["pulses"] else 0
                self.info["rises"] += 1
            else:                                            # a fall
                recs.append({"k_rel": u, "width": min(self.run_len, SAT), "gap": self.gap, "level": int(e[u])})
                self.info["pulses"] += 1
            self.run_len, at = 0, u
        self.run_len += n - at
        if n:
            self.state = int(s[-1])
        self.tail = v[n:]
        self.pos += n
        self.info["samples"] += n
        self.info["state"], self.info["run"] = self.state, self.run_len
        return len(recs), recs


def run_bank(cfg, calls, n_streams):
    """The bank of the definition over `calls` (uint8 [n_streams, nbytes] each; an empty call leaves the results of the one before):
    a list per call of (counts [n_streams], kept records per stream) and the final info per stream.  cfg: dict with W, lo, hi,
    pulse_cap."""
    streams = [Stream(cfg["W"], cfg["lo"], cfg["hi"]) for _ in range(n_streams)]
    out, last = [], ([0] * n_streams, [[] for _ in range(n_streams)])
    for iq in calls:
        iq = np.asarray(iq, np.uint8).reshape(n_streams, -1)
        if iq.shape[1]:
            res = [st.run(iq[s]) for s, st in enumerate(streams)]
            last = ([c for c, _ in res], [r[:cfg["pulse_cap"]] for _, r in res])
        out.append(last)
    return out, [dict(st.info) for st in streams]
