"""The definition of the Mode S bank (include/fmd.h, "Mode S bank") in plain Python / numpy.  This file is the definition: the library's
kernels, its host table and its syndrome are held to it.  Everything is per stream; i counts samples from creation or reset and
everything at a negative index is 0.

    m[i]   = ((2 b[2i] - 255)^2 + (2 b[2i+1] - 255)^2) >> 1
    a_j    = m[p + j], j < 240, for a position p >= 0
    S(p)   = a0 + a2 + a7 + a9
    pre(p) = a0 > a1 and a1 < a2 and a2 > a3 and a3 < a0 and a4 < a0 and a5 < a0 and a6 < a0 and a7 > a8 and a8 < a9 and a9 > a6
             and 6 a_j < S for j in {4, 5, 11, 12, 13, 14} and S >= min_power
    bit t  = 1 iff m[p + 16 + 2t] > m[p + 17 + 2t]
    DF     = bits 0 ... 4;  n = 112 if bit 0 is 1, else 56
    syn    = remainder of bits 0 ... n-25 under 0xFFF409, XOR bits n-24 ... n-1  =  XOR over the set bits t of T_n[t]
    accept   DF in {17, 18} and syn == 0,  or  DF == 11 and df11 and (syn & 0xFFFF80) == 0,
             or  DF in {17, 18} and fix_errors and syn == T_112[t] for one t in 5 ... 111 (bit t flipped, fixed_bit = t)

Position p is decided by the call that brings sample p + 239: a call over [pos, pos + n) decides max(0, pos - 239) <= p < pos + n -
239, and a record's k_rel is p - pos."""
import numpy as np

GENERATOR = 0xFFF409
SPAN = 240                                                   # samples a position reads
QUIET = (4, 5, 11, 12, 13, 14)


def remainder(bits):
    """The 24-bit remainder of `bits` (0 / 1, first sent first) followed by 24 zeros: an MSB-first shift register from 0."""
    r = 0
    for b in list(bits) + [0] * 24:
        r = r << 1 | int(b)
        if r >> 24:
            r ^= 1 << 24 | GENERATOR
    return r


def syndrome_bits(bits):
    """syn of a whole message of 56 or 112 bits, by the shift register."""
    n = len(bits)
    assert n in (56, 112)
    return remainder(bits[:n - 24]) ^ int("".join(str(int(b)) for b in bits[n - 24:]), 2)


def table(n_bits=112):
    """T_n: the syndrome of the message whose only set bit is t."""
    out = []
    for t in range(n_bits):
        bits = [0] * n_bits
        bits[t] = 1
        out.append(syndrome_bits(bits))
    return out


T112 = table(112)
T56 = T112[56:]
_FIX = {T112[t]: t for t in range(5, 112)}


def magnitude(b):
    """m of the u8 IQ bytes b [2 n] as int64 [n]."""
    b = np.asarray(b, np.uint8).astype(np.int64)
    return ((2 * b[0::2] - 255) ** 2 + (2 * b[1::2] - 255) ** 2) >> 1


def preamble(m, min_power):
    """pre(p) for every p < len(m) - 239 of the samples m, as a bool array, and S."""
    m = np.asarray(m, np.int64)
    npos = max(0, m.size - (SPAN - 1))
    a = [m[j:j + npos] for j in range(15)]
    S = a[0] + a[2] + a[7] + a[9]
    ok = ((a[0] > a[1]) & (a[1] < a[2]) & (a[2] > a[3]) & (a[3] < a[0]) & (a[4] < a[0]) & (a[5] < a[0]) & (a[6] < a[0]) &
          (a[7] > a[8]) & (a[8] < a[9]) & (a[9] > a[6]))
    for j in QUIET:
        ok &= 6 * a[j] < S
    ok &= S >= min_power
    return ok, S


def decide(a, fix_errors, df11):
    """What the 240 samples a of a position that passed pre(p) give: None, or (n_bytes, fixed_bit, df, bytes[14])."""
    bits = [1 if a[16 + 2 * t] > a[17 + 2 * t] else 0 for t in range(112)]
    df = int("".join(map(str, bits[:5])), 2)
    n = 112 if bits[0] else 56
    syn = 0
    for t in range(n):
        if bits[t]:
            syn ^= (T112 if n == 112 else T56)[t]
    fixed = 0xFF
    if df in (17, 18):
        if syn != 0:
            if not fix_errors or syn not in _FIX:
                return None
            fixed = _FIX[syn]
            bits[fixed] ^= 1
    elif not (df == 11 and df11 and (syn & 0xFFFF80) == 0):
        return None
    data = bytes(np.packbits(np.array(bits[:n], np.uint8)).tolist()) + bytes(14 - n // 8)
    return n // 8, fixed, df, data


class Stream:
    """One stream of the definition: run(bytes) takes a call and returns (count, records) -- every acceptance of the call, as dicts
    in increasing position; the caller keeps the first msg_cap.  info is the cumulative counters."""

    def __init__(self, min_power=0, fix_errors=0, df11=0):
        self.min_power, self.fix_errors, self.df11 = int(min_power), int(fix_errors), int(df11)
        self.reset()

    def reset(self):
        self.pos = 0
        self.tail = np.zeros(SPAN - 1, np.int64)             # m[pos - 239 ... pos - 1]
        self.info = {"samples": 0, "candidates": 0, "messages": 0, "fixed": 0}

    def run(self, b):
        b = np.asarray(b, np.uint8)
        assert b.size % 2 == 0
        v = np.concatenate([self.tail, magnitude(b)])        # v[u] = m[pos - 239 + u]
        n = b.size // 2
        ok, S = preamble(v, self.min_power)                  # positions u < n: p = pos - 239 + u
        ok[:max(0, SPAN - 1 - self.pos)] = False             # p < 0
        recs = []
        for u in np.nonzero(ok)[0].tolist():
            got = decide(v[u:u + SPAN], self.fix_errors, self.df11)
            if got is None:
                continue
            nb, fixed, df, data = got
            recs.append({"k_rel": u - (SPAN - 1), "power": int(S[u]), "n_bytes": nb, "fixed_bit": fixed, "df": df, "bytes": data})
        self.info["samples"] += n
        self.info["candidates"] += int(ok.sum())
        self.info["messages"] += len(recs)
        self.info["fixed"] += sum(r["fixed_bit"] != 0xFF for r in recs)
        self.tail = v[n:]
        self.pos += n
        return len(recs), recs


def run_bank(cfg, calls, n_streams):
    """The bank of the definition over `calls` (uint8 [n_streams, nbytes] each; an empty call leaves the results of the one before):
    a list per call of (counts [n_streams], kept records per stream) and the final info per stream.  cfg: dict with min_power,
    fix_errors, df11, msg_cap."""
    streams = [Stream(cfg["min_power"], cfg["fix_errors"], cfg["df11"]) for _ in range(n_streams)]
    out, last = [], ([0] * n_streams, [[] for _ in range(n_streams)])
    for iq in calls:
        iq = np.asarray(iq, np.uint8).reshape(n_streams, -1)
        if iq.shape[1]:
            res = [st.run(iq[s]) for s, st in enumerate(streams)]
            last = ([c for c, _ in res], [r[:cfg["msg_cap"]] for _, r in res])
        out.append(last)
    return out, [dict(st.info) for st in streams]
