"""Layout table of the tests that take a kernel's addressing beyond the 2 GiB and 4 GiB lines (tests/test_gpu_big_rows.py,
tests/test_gpu_big_banks.py, tests/test_gpu_big_demod.py), in plain integers.  tests/test_big_cases.py proves without a GPU that every case straddles the lines it
claims and that every wrong-arithmetic alias of an access lands where the GPU test looks.

The technique is a wide pitch with short calls: with a row pitch of 2^31 - delta bytes, rows 1, 2 and 4 of a buffer start delta,
2 delta and 4 delta bytes below byte 2^31, 2^32 and 2^33 of it, so a call of a few thousand samples per row reads or writes across
each line.  The buffer is never filled as a whole: only WINDOWS of it are written before and read after the call.

A LINE is the value 2^31, 2^32 or 2^33 of an offset, counted from the pointer handed to the library, in bytes and in every unit a
kernel may index with (int16, the W-sample, the packed uint32).  A row STRADDLES a line when the line lies inside the elements a call
really touches in that row, at least 64 elements from either end; a row is PAST a line when its base is at or beyond it.

The wrong-arithmetic MODELS, each in every unit u (1 byte included) and as unsigned and as signed 32-bit:
    whole    the whole element offset (row * pitch + j) taken mod 2^32
    product  the product row * pitch taken mod 2^32, then extended and added to j
The signed forms give negative offsets, so the pointer handed to the library sits 2^31 * (the largest unit) bytes inside the
allocation: a sign bug is then a failing assertion, not a fault.

Every alias lies within a few delta of a multiple of `grid` bytes (2^31 where the pitch is 2^31 - delta), so the windows are one
stretch around every multiple of `grid` inside the allocation; what they hold besides the live rows is DECOY input (valid random
samples that differ from the real ones) for a buffer the kernel loads, and SENTINEL for one it stores."""
from types import SimpleNamespace as NS

import numpy as np

import afsk_ref as ar
import agc_ref as ag
import demod_cases as dc
import resample_ref as rr

GiB = 1 << 30
MEMORY_CAP = 32 * GiB                                              # no test holds more device memory than this
SLACK = 256 << 20                                                  # handles, the small side's buffers, the allocator's rounding
EDGE = 64                                                          # elements between a straddled line and either end of the span
LINES = (31, 32, 33)
DELTAS = (1024, 1028)                                              # bytes: every row base 16-byte aligned / none but row 0 and 4
SENT = -12345


def sext32(v):
    v = np.asarray(v, dtype=np.int64) & 0xFFFFFFFF
    return np.where(v >= 1 << 31, v - (1 << 32), v)


class Geo:
    """One pitched device buffer: `rows` rows of `elem`-byte elements, `pitch` bytes apart, of which the calls touch the first
    ns[call] elements; `units` are the bytes of every unit a kernel may index it with."""

    def __init__(self, rows, elem, pitch, ns, units, delta, grid=1 << 31):
        assert pitch % elem == 0 and all(elem % u == 0 or u % elem == 0 for u in units) and all(pitch % u == 0 for u in units)
        self.rows, self.elem, self.pitch, self.ns, self.units, self.delta, self.grid = rows, elem, pitch, tuple(ns), tuple(units), delta, grid
        self.cap = pitch // elem                                   # the in_cap / out_cap handed to the library
        self.margin = (1 << 31) * max(units)                       # bytes in front of the pointer
        self.before = 16 * delta + EDGE * elem                     # window: bytes in front of a multiple of grid ...
        self.after = (max(ns) + 2 * EDGE) * elem                   # ... and behind it
        self.end = (rows - 1) * pitch + self.after                 # bytes behind the pointer
        self.size = self.margin + self.end
        self.aligned = pitch % 16 == 0

    def base(self, r):
        return r * self.pitch

    def true(self, r, j):
        """Byte offset (from the pointer) of element j of row r."""
        return r * self.pitch + np.asarray(j, dtype=np.int64) * self.elem

    def windows(self):
        """[(lo, hi)] byte offsets from the pointer, ascending and disjoint."""
        out = []
        m = -(self.margin // self.grid) * self.grid
        while m - self.before < self.end:
            lo, hi = max(m - self.before, -self.margin), min(m + self.after, self.end)
            if hi > lo:
                assert not out or lo >= out[-1][1]
                out.append((lo, hi))
            m += self.grid
        return out

    def inside(self, off):
        """Which of the byte offsets `off` lie in a window."""
        off = np.asarray(off, dtype=np.int64)
        hit = np.zeros(off.shape, bool)
        for lo, hi in self.windows():
            hit |= (off >= lo) & (off < hi)
        return hit

    def models(self):
        """{(kind, unit, signed): f(r, j) -> the byte offset a kernel with that arithmetic touches}.  In a unit wider than the element
        (the packed uint32 over int16 pairs) j counts units and the byte inside the unit is kept."""
        out = {}
        for u in sorted(set(self.units) | {1}):
            for signed in (False, True):
                wrap = sext32 if signed else (lambda v: np.asarray(v, dtype=np.int64) & 0xFFFFFFFF)

                def whole(r, j, u=u, wrap=wrap):
                    t = self.true(r, j)
                    return wrap(t // u) * u + t % u

                def product(r, j, u=u, wrap=wrap):
                    t = np.asarray(j, dtype=np.int64) * self.elem
                    return (wrap(r * self.pitch // u) + t // u) * u + t % u
                out[("whole", u, signed)] = whole
                out[("product", u, signed)] = product
        return out

    def claims(self):
        """[(row, line exponent, unit, 'straddle' | 'past')]: what the case says it crosses, from the pitch alone -- row r starts
        r * delta bytes below byte r * 2^31 (pitch 2^31 - delta), so it straddles that byte when r * 2^31 is a line of the unit, and
        every later row is past it.  Likewise at a pitch of 2^32 - delta, where row 4 reaches byte 2^34: element 2^32 of a uint32."""
        assert self.grid in (1 << 31, 1 << 32) and self.pitch == self.grid - self.delta
        out = []
        for u in sorted(set(self.units) | {1}):
            for k in LINES + ((34,) if self.grid == 1 << 32 else ()):
                line = (1 << k) * u                                # in bytes
                r = -(-line // self.grid)                          # the first row that reaches the line ...
                if r < self.rows and line % self.grid == 0:        # ... starts r * delta bytes below it
                    out.append((r, k, u, "straddle"))
                out += [(q, k, u, "past") for q in range(r + 1, self.rows)]
        return out


def watches(kind, k, signed):
    """Does the model see line 2^k?  The unsigned forms wrap at 2^32 only; a signed form turns negative from 2^31 on."""
    return signed or k >= 32


# ---- the row processors ----------------------------------------------------------------------------------------------------------

ROWS = 5
CALLS = (2400, 2304)                                               # samples per row and call: behind 4 * delta bytes + EDGE at width 1
HANDLES = ("resample", "agc", "tonesq", "afsk", "dcs")
WIDTHS = {"resample": (1, 2), "agc": (1, 2), "tonesq": (1, 2), "afsk": (1,), "dcs": (1, 2)}
RS = NS(L=3, M=2, T=8, shift=12)
AGC = ag.Cfg(block=256, target=12000, gain_max=65536, hang=2, decay=32)
AGC_CALLS = (2816, 2560)                                           # 10 blocks out per call (block j comes with block j + 1)
TQ = NS(block=256, rate=8000, freqs=(250.0, 500.0, 1000.0), guard=0, dom_shift=2, confirm=1, hang=2, ramp=64, min_power=20_000_000,
        accept=0b111)
AF = NS(rate=9600, taps=8, stride=1)
# the code squelch: every k matches some word (tol 23) and one hit decides a block, so every block confirms one of the words and all are
# accepted: the gate ramps up over block 1 and is open from block 2 on
DCS = NS(block=256, box=8, lp=(300, -200, 1023, -1023, 77), lshift=6, tap=tuple(range(0, 44, 2)) + (47,), tol=23, min_hits=1, confirm=1,
         hang=0, ramp=64, accept=(1 << 128) - 1, words=(0x2AAAAA, 0x555555, 0x0F0F0F))


def row_n_in(handle):
    return AGC_CALLS if handle == "agc" else CALLS


def row_n_out(handle):
    """Outputs per row of the two calls, from the handles' counting rules."""
    n = row_n_in(handle)
    tot = (n[0], n[0] + n[1])
    if handle == "resample":
        o = [rr.outputs(t, RS.L, RS.M, RS.T) for t in tot]
    elif handle == "agc":
        o = [ag.outputs(t, AGC.block) for t in tot]
    elif handle == "afsk":
        o = [ar.outputs(AF.taps, AF.stride, t) for t in tot]
    else:
        o = list(tot)
    return (o[0], o[1] - o[0])


def row_cases():
    """Every row processor at every width, the input pitched in one case and the output in another, at both deltas."""
    out = []
    for handle in HANDLES:
        for width in WIDTHS[handle]:
            for side in ("in", "out"):
                for delta in DELTAS:
                    ns = row_n_in(handle) if side == "in" else row_n_out(handle)
                    units = (1, 2) if width == 1 else (1, 2, 4)    # bytes, int16, the W-sample / packed uint32
                    geo = Geo(ROWS, 2 * width, (1 << 31) - delta, ns, units, delta)
                    small = max(row_n_in(handle)) * 2 * 2 * width * ROWS      # the other side, generously
                    out.append(NS(name="%s-w%d-%s-%d" % (handle, width, side, delta), handle=handle, width=width, side=side, delta=delta,
                                  geo=geo, n_in=row_n_in(handle), n_out=row_n_out(handle), peak=geo.size + small + SLACK))
    return out


# ---- DemodBank: both sides of the table prologue's switch, and the output pitched ---------------------------------------------

DEMOD_D, DEMOD_FAST, DEMOD_SLOW = 6, 5 * dc.BASE, 2 * dc.BASE      # 5 : 2, sr = 2: tiles of 2 repeat exactly, tiles of 3 do not
DEMOD_DELTAS = (256, 264)                                          # bytes: out_cap 2^30 - 128 (16-byte rows) and 2^30 - 132 samples


def _demod_case(name, nch, out_cap, kt, tiles, delta, grid):
    cases = []
    c = dc._case(cases, "big-" + name, DEMOD_D, DEMOD_FAST, DEMOD_SLOW, nch, kt,
                 [(tiles[0], {"frac": 1.0, "kind": "random"}), (tiles[1], {"frac": 0.5, "kind": "square"}), (tiles[2], {"kind": "random"})],
                 out_cap=out_cap)
    ns = [max(call.K) for call in c.calls]
    c.geo = Geo(nch, 2, 2 * out_cap, ns, (1, 2), delta, grid)
    c.name, c.out_cap = name, out_cap
    # 8 rows of 2^29 bytes (less 16): the rows past byte 2^31 are 5 ... 7 (4 ... 7 at exactly 2^29); row 4 of the first starts 64 bytes
    # under the line, too near its start to count as straddling
    c.claims = c.geo.claims() if grid == 1 << 31 else [(r, 31, 1, "past") for r in range(5 if out_cap < 1 << 28 else 4, 8)]
    c.peak = c.geo.size + nch * max(call.nbytes for call in c.calls) + SLACK
    return c


def demod_switch_cases():
    """(a) of the issue: 8 channels at out_cap 2^28 - 8 (the table prologue; the last row ends 128 bytes under byte 2^32) and at
    2^28 (exactly 2^32 bytes: the table is refused, so tiles that repeat take the closed form and tiles that do not the general
    prologue); 9 channels at a pitch of 2^31 - delta bytes, whose row 8 starts 8 delta bytes under element 2^33.  At most 32 tiles
    per call where the table is wanted; the wide cases need calls of more than 8 * delta / 2 + 64 audio samples per channel, which is
    more tiles than the table holds anyway."""
    out = []
    for kt, tag in ((3, "odd"), (2, "rep")):
        out.append(_demod_case("under-%s" % tag, 8, (1 << 28) - 8, kt, (32, 5, 32), 16, 1 << 29))
        out.append(_demod_case("exact-%s" % tag, 8, 1 << 28, kt, (32, 5, 32), 16, 1 << 29))
        for delta in DEMOD_DELTAS:
            out.append(_demod_case("wide-%s-%d" % (tag, delta), 9, ((1 << 31) - delta) // 2, kt, (1200 // kt, 1140 // kt, 1260 // kt), delta, 1 << 31))
    return out


# ---- inputs of 2^32 bytes and more: [channels][nbytes] has no pitch, so the data is really there --------------------------------

IN_CH, IN_BYTES = 65600, 65552                                     # 4.3e9 bytes; 65552 = 16 * 4097 divides neither 2^31 nor 2^32


def sampled(nch=IN_CH, nbytes=IN_BYTES):
    """The channels that are compared: the first two, the last two, and around each of byte 2^31 and 2^32 of the buffer the channel
    that straddles it and its neighbours."""
    out = {0, 1, nch - 2, nch - 1}
    for k in (31, 32):
        c = (1 << k) // nbytes
        assert (1 << k) % nbytes >= EDGE and nbytes - (1 << k) % nbytes >= EDGE and c + 1 < nch
        out |= {c - 1, c, c + 1}
    return sorted(out)


# name: (D, fast, slow, tile, what the case is there for); the tile None leaves the choice to the library (the streaming kernel)
DEMOD_INPUTS = {
    "table": (6, 10000, 4000, 70, "the table prologue, an even LDS kernel"),
    "closed": (16, 10000, 4000, 8, "the closed form, a wide LDS kernel"),
    "general": (7, 10000, 4000, 3, "the general prologue, an odd LDS kernel"),
    "classes": (10, 10000, 4000, 3, "two phase classes: the per-channel class table"),
    "stream": (4, 256000, 48000, None, "the streaming kernel"),
    "generic": (200, 5000, 5000, None, "the generic kernel (downsample 129 ... 512)"),
}
DEMOD_INPUT_MODES = {"table": 2, "closed": 1, "general": 0, "classes": 0, "stream": 2}
CLASS_PRE = 8 * 57                                                 # bytes the odd sampled channels of "classes" are ahead


def demod_input_case(name):
    """NS(D, fast, slow, kt, nch, nbytes, pre, kernels [per call], K [per call][per class], peak) of two calls."""
    D, fast, slow, kt, _ = DEMOD_INPUTS[name]
    c = NS(name=name, D=D, fast=fast, slow=slow, kt=kt, nch=IN_CH, nbytes=IN_BYTES, pre=CLASS_PRE if name == "classes" else 0, kernels=[], K=[])
    if name == "generic":
        c.kernels = ["fmd_demod_generic_kernel<true>"] * 2
        cap = IN_BYTES // 2 // D + 16
    else:
        m = dc.Model(D, fast, slow, IN_CH, kt)
        if c.pre:
            assert m.split(c.pre)
        for _ in range(2):
            assert m.legal(IN_BYTES)
            res = m.call(IN_BYTES)
            c.kernels.append(res.kernel)
            c.K.append(res.K)
        cap = max(max(k) for k in c.K) + 16
    c.peak = IN_CH * IN_BYTES + IN_CH * cap * 2 * 2 + SLACK
    return c


# ---- FirBank and FirDemodBank: the output pitched (five channels), and the same 2^32-byte input --------------------------------

FIR_T, FIR_M, FIR_SEED = 127, 8, 4                                 # 127 taps within +-2047, decimate 8: the matrix-core form
FIR_FAST, FIR_SLOW = 24000, 8000                                   # the fused bank's rates: one audio sample per 3 filter outputs
FIR_CALLS = (36864, 32768)                                         # bytes per channel: 2289 and 2048 filter outputs, 763 and 682 audio samples
FIR_DELTAS = {"fir": (1024, 1032), "fused": (256, 264)}            # (re, im) int32 pairs need pitches that are multiples of 8


def fir_counts(calls=FIR_CALLS):
    """(filter outputs, audio samples) per call, from the counting rules of tests/fir_cases.py."""
    import fir_cases as fc
    pos = i0r = 0
    md, K = [], []
    for nbytes in calls:
        m0, m1 = fc.counts(pos, FIR_T, FIR_M, nbytes // 2)
        md.append(m1 - m0)
        K.append((i0r + md[-1] * 1) // 3)                          # fr = 3, sr = 1
        i0r += md[-1] - 3 * K[-1]
        pos += nbytes // 2
    return md, K


def fir_cases():
    out = []
    md, K = fir_counts()
    for op, elem, units, ns in (("fir", 8, (1, 4, 8), md), ("fused", 2, (1, 2), K)):
        for delta in FIR_DELTAS[op]:
            geo = Geo(ROWS, elem, (1 << 31) - delta, ns, units, delta)
            out.append(NS(name="%s-out-%d" % (op, delta), op=op, delta=delta, geo=geo, ns=tuple(ns), peak=geo.size + ROWS * max(FIR_CALLS) + SLACK))
    return out


# ---- the down-converter banks: the output pitched --------------------------------------------------------------------------------

BK = NS(D=4, T=33, TU=33, TA=9, R=2, RATE=480000, FAST=120000, SLOW=30000, N=8, HOP=8, BLOCK=16, PILOT_BLOCK=1024)
BANK_CALLS = (16 * 1251, 16 * 1203)                                # bytes per stream: whole hops; 5004 and 4812 front-end outputs
BANK_DELTAS = (256, 264)
# kind: (int16 per output, outputs per front-end output m: 'm' itself, 'second' (m - TA) // R + 1, 'resample' FAST : SLOW)
BANKS = {"stations": (1, "resample"), "channelizer": (2, "m"), "stereo": (2, "second"), "rds": (2, "second"),
         "receiver-audio": (2, "second"), "receiver-rds": (2, "second"), "narrow": (1, "second"), "uniform": (2, "m"),
         "bandplan": (1, "second")}


def bank_counts(kind, calls=BANK_CALLS):
    """Outputs per row of every call, from the counting rules of the definitions (channelizer_ref, stereo_ref, rds_ref, narrow_ref;
    the station bank resamples 4 : 1 as the oracle's low_pass_real does)."""
    rule = BANKS[kind][1]
    D = BK.HOP if kind in ("uniform", "bandplan") else BK.D
    pos = m0 = n0 = i0r = 0
    out = []
    for nbytes in calls:
        pos += nbytes // 2
        m1 = (pos - BK.T) // D + 1 if pos >= BK.T else 0
        if rule == "m":
            out.append(m1 - m0)
        elif rule == "second":
            n1 = (m1 - BK.TA) // BK.R + 1 if m1 >= BK.TA else 0
            out.append(n1 - n0)
            n0 = n1
        else:
            fr, sr = BK.FAST // BK.SLOW, 1
            k = (i0r + (m1 - m0) * sr) // fr
            i0r += (m1 - m0) * sr - k * fr
            out.append(k)
        m0 = m1
    return out


def bank_cases():
    """Every bank with S x K = 5 output rows 2^31 - delta bytes apart, once as five streams of one station (delta 256: 16-byte rows) and
    once as one stream of five stations (delta 264); the banks that store packed uint32 once more at 2^32 - 256 bytes, where row 4
    passes element 2^32."""
    out = []
    for kind, (width, _) in BANKS.items():
        ns = bank_counts(kind)
        units = (1, 2) if width == 1 else (1, 2, 4)
        shapes = [(5, 1, BANK_DELTAS[0], 1 << 31), (1, 5, BANK_DELTAS[1], 1 << 31)] + ([(5, 1, BANK_DELTAS[0], 1 << 32)] if width == 2 else [])
        for S, K, delta, grid in shapes:
            geo = Geo(ROWS, 2 * width, grid - delta, ns, units, delta, grid)
            out.append(NS(name="%s-%dx%d-%s%d" % (kind, S, K, "wide-" if grid > 1 << 31 else "", delta), kind=kind, S=S, K=K, width=width,
                          delta=delta, geo=geo, ns=tuple(ns), peak=geo.size + 16 * max(BANK_CALLS) * ROWS + SLACK))
    return out


# ---- the banks' input: [streams][nbytes] has no pitch, so 65535 streams of 65552 bytes are really there ------------------------

BI = NS(D=2, T=2, TU=8, TA=2, R=2, RATE=480000, FAST=240000, SLOW=30000, N=4, HOP=8, BLOCK=16, PILOT_BLOCK=1024)
BANK_IN_S, BANK_IN_K = 65535, {"uniform": 4, "bandplan": 4}        # one station; every channel of a plan of 4
BANK_INPUTS = ("stations", "channelizer", "stereo", "rds", "receiver-audio", "narrow", "uniform", "bandplan")
SPEC = NS(N=16, HOP=8, SHIFT=5)


def bank_input_bytes(kind):
    """(input, output, the internal stage between the two passes) of one call, in bytes."""
    K = BANK_IN_K.get(kind, 1)
    m = IN_BYTES // 2 // (BI.HOP if kind in BANK_IN_K else BI.D)   # front-end outputs per row, a few more than a call completes
    width = BANKS[kind][0]
    n = {"m": m, "second": m // BI.R, "resample": m // (BI.FAST // BI.SLOW)}[BANKS[kind][1]]
    stage = BANK_IN_S * K * ((m + 3) & ~3) * 4 if BANKS[kind][1] != "m" else 0     # packed (yr, yi) or the multiplex
    return BANK_IN_S * IN_BYTES, BANK_IN_S * K * (n + 8) * 2 * width * (2 if kind.startswith("receiver") else 1), stage


def bank_input_peak(kind):
    return sum(bank_input_bytes(kind)) + (1 << 30) + SLACK         # (a GiB for the random fill and the checks on the device)


def demod_expected_modes(c):
    """The prologue every call of a switch case must run, from the issue's statement of the switch alone."""
    if c.name.startswith("under"):
        return 2
    return 1 if "-rep" in c.name else 0
