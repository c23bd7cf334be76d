"""The page bank's domain cases: the inputs of tests/test_gpu_pager_domain.py, pure Python and NumPy, with what the definitions make
of them held by tests/test_pager_domain.py.  A case is rows of soft decisions with every row's records, as tests/pager_cases.py lays
them out, and the cuts it is fed in.

    A  rate_rows     five rows at every rate of RATES (pager_cases.RATES and two more): clean pages in both polarities, pages with about 40 flipped bits,
                     noise with records of its own.  At "wide-a" and "wide-b" R(n) + rd passes 2^32.
    B  beyond_*      a two-batch line placed so that sample 2^32 falls inside the search window, the first codeword, an open message
                     and between the slot-16 record and slot 16; `skip` takes the definition over the zeros in front.
    C  edge_rows     2 S rows of one line, each a sample later than the one before, in calls of S samples: every sample of the line is
                     some row's first sample of a call and another's last.
    D  length_rows   a message of every word count 0 ... 130, and short_rows, a message of (w + 1) % 4 words behind it.
    E  closing_rows  lanes that close a message on the same sample after 0 ... msg_cap + 1 earlier ones in the same call.
    F  rule_rows     hand-built records at the edges of the record rules, with the outcome the definition gives (RULES).
    G  many_rows     40000 rows of 67 lines at 31 leads, and the rows the definition is run for."""
import functools

import numpy as np

import pager_cases as pc
import pager_ref as gr
import pocsag_ref as pr
from rtl_sdr_rs_amd.pocsag import POCSAG_IDLE as IDLE, pocsag_codeword as cw, pocsag_encode as encode

U32 = pc.U32
T32 = 1 << 32
I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)
CUTS = (1, 7, 1000, 333)
SYNC_BITS = np.array(pc.SYNC_BITS, np.uint8)
# pager_cases.RATES and two steps near 2^31 whose mod % step is a large part of them, so that R(n) + rd passes 2^32.  They are kept
# apart from pager_cases.RATES: at 2.86 and 2.15 samples per bit a record floored to a sample can leave a bit position on the bit's
# edge, and tests/test_pager.py holds every rate of that table to a clean 2580-bit message decoded whole.
RATES = dict(pc.RATES, **{"wide-a": (U32, 1, 1500000000), "wide-b": (U32, 1, 2000000000)})


def addr_word(address18, function):
    return cw((address18 & 0x3FFFF) << 2 | function)


def msg_word(data20):
    return cw(1 << 20 | (data20 & 0xFFFFF))


def per_bit(rate, bits):
    """soft samples that `bits` bits take, rounded up"""
    return -(-bits * rate[0] // (rate[1] * rate[2]))


def uniform(n, each):
    return [each] * (n // each)


# ---- A: every rate ---------------------------------------------------------------------------------------------------------------------
def carry_sums(name, bits=544):
    """R(n) + rd for n = 1 ... bits, as the kernel forms them"""
    mod, step = RATES[name][0], RATES[name][1] * RATES[name][2]
    rd, two_step, rem, out = 2 * (mod % step), 2 * step, (2 * mod + step) % (2 * step), []
    for _ in range(bits):
        t = rem + rd
        out.append(t)
        rem = t - two_step if t >= two_step else t
    return out


@functools.lru_cache(maxsize=None)
def rate_rows(name):
    """(x [5, n], hits): rows 0 and 1 clean pages in both polarities, 2 and 3 the pages with 40 bits off over sync, address and
    message words behind the first sync word, 4 noise with records of its own"""
    rate = RATES[name]
    rng = np.random.default_rng(sorted(RATES).index(name))
    pages = [(1234560, 0, "0123456789", "numeric"), (765437, 3, "The quick brown fox", "alpha"), (9, 1, "", "tone"),
             (77, 2, rng.integers(0, 2, 100).tolist(), "bits")]
    clean = encode(pages, preamble=64)

    def off():
        bits = clean.copy()
        bits[rng.choice(len(bits) - 96, 40, replace=False) + 96] ^= 1         # (behind the first sync word, so that the row locks)
        return bits
    q = rate[0] // (rate[1] * rate[2])
    n = 1500 * q
    soft = (np.repeat(rng.integers(0, 2, n // q + 1) * 2 - 1, q)[:n] * rng.integers(1, 30000, n)).astype(np.int16)
    ks = sorted(set(rng.integers(0, n, 14).tolist()))
    noise = [(k, int(rng.integers(0, 3)) | (int(rng.integers(0, 2)) << 31), int(rng.integers(-99999, 99999)), int(rng.integers(-9999, 9999)))
             for k in ks]
    return pc.stack([pc.line(clean, rate, dc=300), pc.line(clean, rate, dc=-200, invert=True, lead=47), pc.line(off(), rate, dc=-200),
                     pc.line(off(), rate, dc=300, invert=True, lead=33), (soft, noise)])


# ---- B: beyond 2^32 ------------------------------------------------------------------------------------------------------------------
B_RATE = RATES["5"]                                       # r = 5, half = 2, Q(544) = 2720: p(n) = k + 5 n
# where sample 2^32 lies, counted from row 0's first record: (a) inside the search window (k, k + 5], (b) inside the first codeword,
# (c) between bit 416 at k + 2080 and bit 417 at k + 2085, the words at slots 12 and 13 of the open message, (d) between the slot-16
# record at k + 2720 and slot 16 at k + 2722
B_AT = {"a": 3, "b": 55, "c": 2082, "d": 2721}
B_THIRD = 5441                                               # the first sample behind the third sync word's record


def skip(ref, m):
    """`ref` as a call of m zero samples without records leaves it, for decoders that are neither locked nor searching"""
    for d in ref.decs:
        assert not d.locked and not d.window and not d.queue
        n = d.n + m
        soft = {k: v for k, v in d.soft.items() if k >= n - 64}
        soft.update({k: 0 for k in range(max(d.n, n - 64), n)})
        d.soft, d.n, d.out = soft, n, []
    ref.pos += m
    ref.last = (np.zeros(ref.rows, np.uint32), np.zeros((ref.rows, ref.msg_cap), gr.MSG_DTYPE), [[] for _ in range(ref.rows)])


@functools.lru_cache(maxsize=None)
def beyond_rows():
    """(x [3, n], hits): two batches with a message open across the seam and another across the third sync word; the same inverted
    with one more sample of lead; an idle row"""
    rng = np.random.default_rng(32)
    m = [msg_word(int(v)) for v in rng.integers(0, 1 << 20, 11)]
    b1 = [IDLE] * 10 + [addr_word(0x2A5A5, 1)] + m[:5]
    b2 = m[5:8] + [IDLE, IDLE, addr_word(0x155, 2), m[8], m[9]] + [IDLE] * 6 + [addr_word(0x3FFFF, 3), m[10]]
    idle = np.array([(IDLE >> b) & 1 for b in range(31, -1, -1)], np.uint8)
    bits = np.concatenate([encode(None, preamble=32, words=b1 + b2), SYNC_BITS, idle])     # (the idle word closes the third message)
    return pc.stack([pc.line(bits, B_RATE), pc.line(bits, B_RATE, invert=True, lead=41), (np.zeros(10, np.int16), [])])


def beyond_runs():
    """[(name, L, cuts)]: the line starts at position 2^32 - L; with "edge" a call ends exactly at 2^32, with "inside" 2^32 is a
    call's third sample; every run has a call edge between the third sync word's record and its slot 16"""
    k = beyond_rows()[1][0][0][0]
    runs = []
    for where, at in sorted(B_AT.items()):
        L = k + at
        runs.append((where + "-edge", L, [L, k + B_THIRD - L]))
        runs.append((where + "-inside", L, [L - 2, k + B_THIRD - (L - 2)]))
    return runs


# ---- C: a call edge on every sample ----------------------------------------------------------------------------------------------------
C_RATES = ("2", "5", "wide-a")
S = 35
C_AMP, C_DC = 3000, 5000                                     # |dc| > amp: both levels on one side of zero, so a lost thr flips bits


@functools.lru_cache(maxsize=None)
def edge_line(name, lead, invert):
    """Preamble 32, two batches, the third sync word, then a batch of the bare level, in which the lock is lost inside an open
    message: the second batch ends in an address word and two message words, and the bare level reads as address words of all zeros
    or, inverted, as message words of all ones.  The first address word has one bit off and function 2; three message words lie in
    front of the batch seam and four behind it; a weaker record with a thr that reads every bit as 0 sits one sample behind every
    sync word's."""
    rate = RATES[name]
    rng = np.random.default_rng(7)
    m = [msg_word(int(v)) for v in rng.integers(0, 1 << 20, 9)]
    words = [IDLE] * 12 + [addr_word(0x1B3C7, 2)] + m[:3] + m[3:7] + [IDLE] * 9 + [addr_word(0x2D2D2, 1)] + m[7:]
    bits = encode(None, preamble=32, words=words)
    bits[32 + 32 + 32 * 12 + 9] ^= 1
    bits = np.concatenate([bits, SYNC_BITS])
    soft, hits = pc.line(bits, rate, amp=C_AMP, dc=C_DC, invert=invert, lead=lead, tail=per_bit(rate, 560))
    both = []
    for k, d, corr, thr in hits:
        both += [(k, d, corr, thr), (k + 1, d, corr // 2, thr + 64 * C_AMP)]
    return soft, both


@functools.lru_cache(maxsize=None)
def edge_rows(name, s=S, base=40):
    """(x [2 s, n], hits, cuts): row j is the line behind base + j % s samples, rows s ... 2 s - 1 inverted; calls of s samples"""
    x, hits = pc.stack([edge_line(name, base + j % s, j >= s) for j in range(2 * s)], fill=C_DC)
    return x, hits, uniform(x.shape[1], s)


@functools.lru_cache(maxsize=None)
def edge_rows_single():
    """rows 0 and S of edge_rows("2") with a call edge behind each of the first 200 samples behind row 0's first record"""
    x, hits, _ = edge_rows("2")
    return np.ascontiguousarray(x[[0, S]]), [hits[0], hits[S]], [hits[0][0][0]] + [1] * 200


# ---- D: every message length, and stale bits -----------------------------------------------------------------------------------------
D_RATE = RATES["2"]
D_WORDS = range(131)


def _message(rng, address, function, w, lead, invert):
    data = [int(v) for v in rng.integers(0, 1 << 20, max(w - 1, 0))] + [0xFFFFF] * min(w, 1)
    bits = [(v >> b) & 1 for v in data for b in range(19, -1, -1)]
    return pc.line(encode([(address, function, bits, "bits")], preamble=32), D_RATE, lead=lead, invert=invert)


@functools.lru_cache(maxsize=None)
def length_rows():
    """(x, hits, cuts): row w's message has w words (n_bits 0, 20 ... 2600), random but for the last, which is all ones; three calls"""
    rng = np.random.default_rng(131)
    x, hits = pc.stack([_message(rng, 8 * (w + 1), w % 4, w, 8 + w % 5, w % 7 == 3) for w in D_WORDS])
    return x, hits, [x.shape[1] // 3, x.shape[1] // 3]


@functools.lru_cache(maxsize=None)
def short_rows():
    """(x, hits, cuts): row w's message has (w + 1) % 4 words, to follow length_rows in the same handle: a short message behind a
    long one"""
    rng = np.random.default_rng(4)
    x, hits = pc.stack([_message(rng, 8 * (w + 200), (w + 1) % 4, (w + 1) % 4, 8 + w % 3, w % 7 == 3) for w in D_WORDS])
    return x, hits, []


def n_bytes(n_bits):
    return (min(n_bits, pr.MAX_BITS) + 7) // 8


def package(kept, n_bits, zero_behind=True, mask=True):
    """The 320 bytes of a record's bits as the wave's copy makes them from the row's kept 320 bytes: the dwords that begin in front
    of `len` bytes, the last of them masked to the bytes in front of `len`, zero behind.  `zero_behind` and `mask` False: the two
    ways to get it wrong."""
    ln, out = n_bytes(n_bits), bytearray(320)
    for b0 in range(0, 320, 4):
        if b0 < ln or not zero_behind:
            v = bytearray(kept[b0:b0 + 4])
            if mask and b0 < ln < b0 + 4:
                v[ln - b0:] = bytes(4 - (ln - b0))
            out[b0:b0 + 4] = v
    return bytes(out)


# ---- E: lanes closing together at different slots ------------------------------------------------------------------------------------
E_RATE = RATES["2"]
E_ROWS = 64 + 3
E_CUT = 260                                                  # behind the first record: between the words at slots 3 and 4


@functools.lru_cache(maxsize=None)
def closing_rows(cap):
    """(x [67, n], hits): row j has j % (cap + 2) tone-only pages at slots 0 ..., closed one by the next and the last by an idle
    word, and then, at slots 20 to 22 in every row, an address word, a message word of its own and the idle word that closes them"""
    lines = []
    for j in range(E_ROWS):
        c = j % (cap + 2)
        words = [addr_word(j * 32 + i, i % 4) for i in range(c)] + [IDLE] * (20 - c)
        words += [addr_word(0x30000 + j, 1 + j % 3), msg_word(j * 2654435761 >> 7), IDLE] + [IDLE] * 9
        lines.append(pc.line(encode(None, preamble=32, words=words), E_RATE))
    return pc.stack(lines)


def wave_slots(every, cap, one_slot=False):
    """[(row, slot, message)] the wave's copy writes for rows whose last message closes in one turn of the loop, every earlier one in
    turns of its own: the slot is the closing lane's count; `one_slot`: taken once for the wave, from its first closing lane"""
    out = []
    for r0 in range(0, len(every), 64):
        rows = range(r0, min(r0 + 64, len(every)))
        for r in rows:
            out += [(r, s, m) for s, m in enumerate(every[r][:-1]) if s < cap]
        first = len(every[r0]) - 1
        for r in rows:
            slot = first if one_slot else len(every[r]) - 1
            if slot < cap:
                out.append((r, slot, every[r][-1]))
    return out


# ---- F: the record rules --------------------------------------------------------------------------------------------------------------------
F_RATES = ("2", "5", "32")
F_AMP = 3000
F_BAD = 64 * F_AMP                                           # a thr that reads every bit of the line as 0
F_ITEMS = ["clean", "second at k1 + r", "second at k1 + r + 1", "equal, first stays", "-2^31 after 2^31 - 1", "2^31 - 1 after -2^31",
           "slot 16 - half - 1", "slot 16 - half", "slot 16 + half", "slot 16 + half + 1", "slot 16 other polarity", "thr 2^31 - 1",
           "thr -2^31", "slot 16: -2^31 after 2^31 - 1", "slot 16: 2^31 - 1 after -2^31", "slot 16: equal, first stays"]
# (batches, locked, messages) of every item's row behind the line, as the definition gives them
_RULES = [(2, 0, 2), (2, 0, 2), (2, 0, 17), (2, 0, 2), (2, 0, 2), (2, 0, 2), (1, 0, 1), (2, 0, 2), (2, 0, 2), (2, 0, 2), (1, 0, 1), (2, 0, 17),
          (2, 0, 1), (2, 0, 2), (2, 0, 2), (2, 0, 2)]
RULES = {"2": _RULES, "5": _RULES, "32": _RULES}             # (the same at the three rates)


@functools.lru_cache(maxsize=None)
def rule_rows(name):
    """(x [16, n], hits): the clean line (a page in each of two batches) in every row, with the records of F_ITEMS"""
    rate = RATES[name]
    r = (2 * rate[0] + rate[1] * rate[2]) // (2 * rate[1] * rate[2])
    half = r // 2
    one = encode([(8, 1, "rules", "alpha")], preamble=32)
    soft, h = pc.line(np.concatenate([one, one[32:]]), rate, amp=F_AMP, lead=40)
    (k0, d, corr, thr), (k1, _, _, _) = h
    h0, h1 = h
    rows = [[h0, h1],
            [(k0 - r, d, corr // 2, F_BAD), h0, h1],
            [(k0 - r - 1, d, corr // 2, F_BAD), h0, h1],
            [h0, (k0 + 1, d, -corr, F_BAD), h1],
            [(k0 - 1, d, I32_MAX, F_BAD), (k0, d, I32_MIN, thr), h1],
            [(k0, d, I32_MIN, thr), (k0 + 1, d, I32_MAX, F_BAD), h1],
            [h0, (k1 - half - 1, d, corr, thr)],
            [h0, (k1 - half, d, corr, thr)],
            [h0, (k1 + half, d, corr, thr)],
            [h0, (k1 + half + 1, d, corr, thr)],
            [h0, (k1, d ^ 1 << 31, -corr, thr)],
            [(k0, d, corr, I32_MAX), h1],
            [(k0, d, corr, I32_MIN), h1],
            [h0, (k1 - 1, d, I32_MAX, F_BAD), (k1, d, I32_MIN, thr)],
            [h0, (k1, d, I32_MIN, thr), (k1 + 1, d, I32_MAX, F_BAD)],
            [h0, h1, (k1 + 1, d, -corr, F_BAD)]]
    assert len(rows) == len(F_ITEMS)
    return np.ascontiguousarray(np.broadcast_to(soft, (len(rows), len(soft)))), rows


# ---- G: many rows -------------------------------------------------------------------------------------------------------------------------
G_RATE = RATES["2"]
G_ROWS, G_LINES, G_LEADS = 40000, 67, 31
G_CUTS = [400, 500]
G_KINDS = ("page", "inverted", "noise", "idle")


def many_kind(r):
    return G_KINDS[r % G_LINES % 4]


@functools.lru_cache(maxsize=None)
def many_lines():
    rng = np.random.default_rng(67)
    lines = []
    for i in range(G_LINES):
        kind = G_KINDS[i % 4]
        if kind in ("page", "inverted"):
            mode = ("alpha", "numeric", "tone")[i % 3]
            text = {"alpha": "line %d" % i, "numeric": "%d-%d" % (i, 7 * i + 1), "tone": ""}[mode]
            lines.append(pc.line(encode([((i * 7919 + 5) & 0x1FFFFF, i % 4, text, mode)], preamble=32), G_RATE, lead=8, invert=kind == "inverted",
                                 dc=10 * (i % 7)))
        elif kind == "noise":
            n = 900 + 3 * i
            ks = sorted(set(rng.integers(0, n, 5).tolist()))
            lines.append((rng.integers(-20000, 20000, n).astype(np.int16),
                          [(k, int(rng.integers(0, 3)) | (int(rng.integers(0, 2)) << 31), int(rng.integers(-99999, 99999)),
                            int(rng.integers(-9999, 9999))) for k in ks]))
        else:
            lines.append((rng.integers(-50, 50, 50 + i).astype(np.int16), []))        # no record: nothing is ever due
    return lines


@functools.lru_cache(maxsize=None)
def many_sample():
    rng = np.random.default_rng(40000)
    return sorted(set([0, 63, 64, 65, 39935, 39936, 39999] + rng.integers(0, G_ROWS, 193).tolist()))


def many_row(r):
    """row r: line r % 67 behind r % 31 more samples of lead"""
    soft, hits = many_lines()[r % G_LINES]
    s = r % G_LEADS
    return np.concatenate([np.zeros(s, np.int16), soft]), [(k + s, d, c, t) for k, d, c, t in hits]


@functools.lru_cache(maxsize=None)
def many_rows():
    """(x [40000, n], [(counts, records) per call]): every row, and every call's packed records"""
    n = max(len(s) for s, _ in many_lines()) + G_LEADS - 1
    x = np.zeros((G_ROWS, n), np.int16)
    rows = np.arange(G_ROWS)
    combo = (rows % G_LINES) * G_LEADS + rows % G_LEADS      # (67 and 31 are coprime: every combination occurs)
    first = {}
    for r in range(G_LINES * G_LEADS):
        first.setdefault(int(combo[r]), r)
    order = sorted(first)
    assert len(order) == G_LINES * G_LEADS
    distinct = [many_row(first[c]) for c in order]
    for c, (soft, _) in zip(order, distinct):
        x[first[c]::G_LINES * G_LEADS, :len(soft)] = soft
    calls, lo = [], 0
    for m in G_CUTS + [n]:
        m = min(m, n - lo)
        counts, rec = pc.pack([h for _, h in distinct], lo, m)
        calls.append((lo, m, counts[combo], rec[combo]))
        lo += m
    return x, calls
