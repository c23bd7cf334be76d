"""The host's AX.25 frame decoder (include/fmd.h, fmd_ax25_decoder_*; csrc/fmd_ax25_decode.cpp) against its definition in Python
integers (tests/ax25_ref.py) where tests/test_afsk.py does not reach: the rate domain at the edge of 64-bit arithmetic, every number
of samples per bit 4 ... 64 and rational ones with jittered edges and sign noise, bit stuffing at every position, the ring of 64
frames when it overflows, and end_sample under cuts.  No GPU.  FMD_FUZZ_SEED moves the seeds."""
import ctypes as C

import numpy as np
import pytest

import ax25_ref as xr
from rows_cases import seed

UNSUPPORTED = -6
U32 = (1 << 32) - 1


# ---- the rate domain -----------------------------------------------------------------------------------------------------------------
def _new(fmd, num, den, baud):
    d = C.c_void_p()
    rc = fmd.lib().fmd_ax25_decoder_new(num, den, baud, C.byref(d))
    assert (rc == 0) == bool(d.value)
    if rc == 0:
        fmd.lib().fmd_ax25_decoder_free(d)
    else:
        assert rc == UNSUPPORTED and fmd.lib().fmd_last_error().decode() == "need 4 <= rate / baud <= 64"
    return rc == 0


def _ref_accepts(num, den, baud):
    try:
        xr.Decoder(num, den, baud)
        return True
    except ValueError:
        return False


def _agree(fmd, num, den, baud, soft):
    """Library and definition agree on whether the triple is a rate; where it is one, on what 1000 samples give."""
    ok = _ref_accepts(num, den, baud)
    assert _new(fmd, num, den, baud) == ok, (num, den, baud)
    if ok:
        dec, ref = fmd.Ax25Decoder(num, den, baud), xr.Decoder(num, den, baud)
        assert dec.push(soft) == ref.push(soft) and dec.info() == ref.info(), (num, den, baud)
    return ok


# (inside, outside) on both sides of every edge, and where baud * rate_den no longer fits what is left of 64 bits
EDGES = [((4800, 1, 1200), (4799, 1, 1200)), ((76800, 1, 1200), (76801, 1, 1200)), ((4, 1, 1), (3, 1, 1)), ((64, 1, 1), (65, 1, 1)),
         ((U32, 1, (1 << 30) - 1), (U32, 1, 1 << 30)),                       # 4 step = 2^32 - 4 against 2^32
         ((U32, 1 << 15, (1 << 15) - 1), (U32, 1 << 15, 1 << 15)),
         ((U32, 894784, 1200), (U32, 894785, 1200)), ((U32, 55925, 1200), (U32, 55924, 1200)),
         ((U32, 67108864, 1), (U32, 67108863, 1)),                           # 64 step = 2^32 against 2^32 - 64
         ((6000, 1, 1200), (6000, 0, 1200)), ((6000, 1, 1200), (6000, 1, 0)), ((6000, 1, 1200), (0, 1, 1200))]
WRAP = [(0, 1 << 31, 1 << 31), (1, 1 << 31, 1 << 31), (0, U32, U32), (U32, U32, U32), (0, 1 << 31, (1 << 31) + 1)]


def test_rate_domain_edges_and_the_wrap(fmd):
    """step = baud * rate_den reaches (2^32 - 1)^2.  At 2^62 both 4 step and 64 step are 0 in 64 bits, at 2^62 + 2^31 they are small:
    a check that forms those products accepts rates the definition refuses, and the first push then overflows the phase."""
    soft = np.where(np.arange(1000) // 7 % 2 == 0, 9000, -9000).astype(np.int16)
    for inside, outside in EDGES:
        assert _agree(fmd, *inside, soft) and not _agree(fmd, *outside, soft), (inside, outside)
    for t in WRAP:
        assert not _ref_accepts(*t) and not _new(fmd, *t), t
    assert 4 * (1 << 62) % (1 << 64) == 0 and 64 * (1 << 62) % (1 << 64) == 0 and 4 * ((1 << 62) + (1 << 31)) % (1 << 64) == 1 << 33


def test_rate_domain_sweep(fmd):
    """Seeded u32 triples with both factors of step at 2^30 and above (every one is outside: step >= 2^60), powers of two among them
    (the products that wrap to exactly 0), and triples drawn around both edges at every size of step."""
    rng = np.random.default_rng(seed(8000))
    soft = rng.integers(-32768, 32768, 1000).astype(np.int16)
    soft[100:400] = np.where(np.arange(300) // 11 % 2 == 0, 5000, -5000)
    n_in = 0
    for _ in range(400):
        den, baud = (int(v) for v in rng.integers(1 << 30, 1 << 32, 2))
        num = int(rng.integers(0, 1 << 32)) if rng.integers(0, 2) else int(rng.integers(0, 70))
        assert not _agree(fmd, num, den, baud, soft)
    for a in range(30, 32):
        for b in range(30, 32):
            for num in (0, 1, 4, 64, 1 << 31, U32):
                for da, db in ((0, 0), (1, 0), (0, 1), (-1, -1)):
                    assert not _agree(fmd, num, (1 << a) + da, (1 << b) + db, soft)
    for _ in range(400):
        den, baud = int(rng.integers(1, 1 << int(rng.integers(1, 17)))), int(rng.integers(1, 1 << int(rng.integers(1, 15))))
        step = den * baud
        k = int(rng.choice([4, 64]))
        num = k * step + int(rng.integers(-2, 3)) * int(rng.choice([1, step // 64 + 1]))
        if 0 <= num <= U32:
            n_in += _agree(fmd, num, den, baud, soft)
    assert n_in > 100


# ---- differential decoding -----------------------------------------------------------------------------------------------------------
RATIOS = [(1200 * k, 1, 1200) for k in range(4, 65)] + [(11025, 2, 1200), (22050, 4, 1200), (25600, 4, 1200), (48000, 8, 1200), (U32, 894784, 1200),
                                                          (U32, 55925, 1200)]


def _frame(rng, n=None):
    return bytes(rng.integers(0, 256, int(rng.integers(15, 40)) if n is None else n).astype(np.uint8))


def _content(rng):
    """The bits of a transmission: intact frames, a frame with a flipped bit, one cut off, one padded to a bit count that is no
    multiple of 8, an abort, two frames that share one flag.  (bits, the frames sent intact)"""
    a, b, c, d, e, f, g = (_frame(rng) for _ in range(7))
    flipped = xr.stuffed_bits(xr.with_fcs(b))
    flipped[int(rng.integers(8, len(flipped) - 8))] ^= 1
    body = xr.stuffed_bits(xr.with_fcs(c))
    padded = xr.stuffed_bits(xr.with_fcs(d)) + [0, 1, 0][:int(rng.integers(1, 4))]
    bits = (xr.frame_bits(a, flags=4) + xr.FLAG + flipped + xr.FLAG * 2 + body[:int(rng.integers(20, len(body) - 20))] + [1] * 8 +     # cut off: an abort
            xr.FLAG * 2 + padded + xr.FLAG + xr.stuffed_bits(xr.with_fcs(e)) + xr.FLAG + xr.stuffed_bits(xr.with_fcs(f)) + xr.FLAG +     # one flag between
            [1] * 12 + xr.frame_bits(g, flags=3, closing=2))
    return bits, [a, e, f, g]


def _soft(rng, bits, num, den, baud, noise=True):
    """The line levels of `bits` at num / (den * baud) samples per bit: bit k ends at sample floor((k + 1) num / (den baud)), every
    edge moved by -1, 0 or +1 samples, behind a lead of mark; amplitudes of both signs' full range, 0 (which reads as mark) among
    them, and a few bursts of one to three samples with the wrong sign."""
    lv = np.array(xr.nrzi(bits), np.int64)
    ends = (np.arange(1, len(lv) + 1, dtype=np.int64) * num) // (den * baud)             # (below 2^45)
    if noise:
        ends[:-1] += rng.integers(-1, 2, len(ends) - 1)
    runs = np.diff(np.concatenate([[0], ends]))
    assert runs.min() >= 2
    level = np.concatenate([np.ones(int(rng.integers(10, 200)), np.int64), np.repeat(lv, runs)])
    amp = rng.integers(0, 32768, level.size)
    soft = np.where(level == 1, amp, -1 - amp)
    if noise:
        for p in rng.integers(0, soft.size - 3, max(1, soft.size // 4000)):
            k = int(rng.integers(1, 4))
            soft[p:p + k] = -1 - soft[p:p + k]
    return soft.astype(np.int16)


def _both(fmd, soft, rate, cuts=None):
    """Library and definition over the same samples: frames (data, end_sample) and all four counters; the library whole, and
    again in the pieces `cuts`."""
    ref = xr.Decoder(*rate)
    want = ref.push(soft)
    for pieces in [None] + ([cuts] if cuts is not None else []):
        dec, got, lo = fmd.Ax25Decoder(*rate), [], 0
        for n in ([len(soft)] if pieces is None else list(pieces) + [len(soft)]):
            got += dec.push(soft[lo:lo + n])
            lo += n
        assert got == want and dec.info() == ref.info(), (rate, pieces)
    return want, ref.info()


@pytest.mark.parametrize("sd", range(3))
def test_every_rate_with_jitter_and_sign_noise(fmd, sd):
    """Every whole number of samples per bit 4 ... 64 and six rational ones, the two at the domain's ends among them (2^32 - 1 over
    894784 * 1200 is 4.00000004 and over 55925 * 1200 is 63.9996)."""
    total = {"frames_ok": 0, "bad_fcs": 0, "aborts": 0, "in_frame": 0}
    clean = 0
    for i, rate in enumerate(RATIOS):
        rng = np.random.default_rng([seed(8100), sd, i])
        bits, sent = _content(rng)
        soft = _soft(rng, bits, *rate)
        cuts = rng.integers(0, 3000, 40).tolist() + [0, 1, 1]
        frames, info = _both(fmd, soft, rate, cuts)
        assert all(f["end_sample"] < len(soft) for f in frames) and info["frames_ok"] == len(frames)
        for k in total:
            total[k] += info[k]
        if i % 8 == sd:                                      # without jitter and noise what was sent intact arrives, and the rest is counted
            frames, info = _both(fmd, _soft(rng, bits, *rate, noise=False), rate)
            assert [f["data"] for f in frames] == sent and info["bad_fcs"] + info["aborts"] >= 4 and info["aborts"] >= 2 and info["in_frame"] == 1, rate
            clean += 1
    assert clean >= 8 and all(v > 0 for v in total.values()), total
    assert total["frames_ok"] >= len(RATIOS)                 # (most frames survive +-1 sample of jitter at 4 samples per bit and more)


# ---- stuffing ------------------------------------------------------------------------------------------------------------------------
def _clean(fmd, bits, spb=5):
    soft = _soft(np.random.default_rng(1), bits, 1200 * spb, 1, 1200, noise=False)
    frames, info = _both(fmd, soft, (1200 * spb, 1, 1200), [1, 7, 1000, 333])
    return [f["data"] for f in frames], info


def test_runs_of_ones_ending_on_every_bit_position(fmd):
    """Runs of 1 ... 6 ones that end on each of the 8 bit positions of a byte (the longer ones start in the byte before): 5 and 6
    take a stuffed bit, at every position."""
    sent, bits = [], xr.FLAG * 3
    for run in range(1, 7):
        for pos in range(8):
            v = ((1 << run) - 1) << (8 * 9 + pos + 1 - run)  # the run's last one is bit `pos` of byte 9, LSB first
            data = v.to_bytes(20, "little")
            body = xr.stuffed_bits(xr.with_fcs(data))
            plain = [(b >> k) & 1 for b in data for k in range(8)]
            assert plain[8 * 9 + pos] == 1 and plain[8 * 9 + pos + 1] == 0 and sum(plain) == run
            assert len(xr.stuffed_bits(data)) - 160 == (1 if run >= 5 else 0)
            sent.append(data)
            bits += body + xr.FLAG
    frames, info = _clean(fmd, bits)
    assert frames == sent and info == {"frames_ok": 48, "bad_fcs": 0, "aborts": 0, "in_frame": 1}


def _search(pred, n=20, limit=20000):
    """the first seeded frame of n bytes that meets `pred` (deterministic: the candidates are seeds 0, 1, ...)"""
    for s in range(limit):
        data = bytes(np.random.default_rng(s).integers(0, 128, n).astype(np.uint8))
        if pred(data):
            return data
    raise AssertionError("no frame found")


def test_stuffed_bits_inside_the_fcs_and_directly_before_the_flag(fmd):
    def fcs_bits(d):
        c = xr.crc16_x25(d)
        return [(c >> k) & 1 for k in range(16)]

    def stuffed_in_fcs(d):                                   # a run of five 1s is completed by a bit of the FCS
        return len(xr.stuffed_bits(xr.with_fcs(d))) > len(xr.stuffed_bits(d)) + 16

    def five_before_flag(d):                                 # the FCS ends in exactly five 1s: the stuffed 0 is the last bit before the flag
        return fcs_bits(d)[10:] == [0, 1, 1, 1, 1, 1]
    a, b = _search(stuffed_in_fcs), _search(five_before_flag)
    assert xr.stuffed_bits(xr.with_fcs(b))[-7:] == [0, 1, 1, 1, 1, 1, 0] and len(xr.stuffed_bits(xr.with_fcs(b))) % 8 != 0
    c = _search(lambda d: fcs_bits(d)[11:] == [1] * 5 and fcs_bits(d)[10] == 1 and fcs_bits(d)[9] == 0)     # six 1s at the end: stuffed inside them
    bits = xr.FLAG * 2 + xr.stuffed_bits(xr.with_fcs(a)) + xr.FLAG + xr.stuffed_bits(xr.with_fcs(b)) + xr.FLAG + xr.stuffed_bits(xr.with_fcs(c)) + xr.FLAG
    frames, info = _clean(fmd, bits)
    assert frames == [a, b, c] and info == {"frames_ok": 3, "bad_fcs": 0, "aborts": 0, "in_frame": 1}
    # the same frame without its last stuffed bit: the flag's own 0 is dropped in its place, the flag is still seen (it is looked
    # for before un-stuffing), and the frame is one bit short of whole bytes
    frames, info = _clean(fmd, xr.FLAG * 2 + xr.stuffed_bits(xr.with_fcs(b))[:-1] + xr.FLAG + xr.frame_bits(a, flags=1))
    assert frames == [a] and info == {"frames_ok": 1, "bad_fcs": 1, "aborts": 0, "in_frame": 1}


def test_the_longest_stuffed_frame_is_delivered(fmd):
    """512 bytes of 0xFF and the FCS: 514 bytes, a stuffed bit behind every five of 4096 ones."""
    data = b"\xff" * 512
    bits = xr.frame_bits(data, flags=2)
    assert len(bits) >= 24 + 514 * 8 + 4096 // 5
    for spb in (4, 5, 64):
        frames, info = _clean(fmd, bits + xr.frame_bits(b"\xff" * 513, flags=1), spb)       # and one byte more is not a frame
        assert frames == [data] and info == {"frames_ok": 1, "bad_fcs": 1, "aborts": 0, "in_frame": 1}


# ---- the ring ------------------------------------------------------------------------------------------------------------------------
class _Raw:
    """fmd_ax25_decoder_push with a chosen `cap`"""

    def __init__(self, fmd, spb=5):
        from rtl_sdr_rs_amd.afsk import Ax25Frame
        self.lib, self.d, self.buf = fmd.lib(), C.c_void_p(), (Ax25Frame * 80)()
        assert self.lib.fmd_ax25_decoder_new(1200 * spb, 1, 1200, C.byref(self.d)) == 0

    def push(self, soft, cap):
        n = C.c_size_t(99)
        soft = np.ascontiguousarray(soft, np.int16)
        assert self.lib.fmd_ax25_decoder_push(self.d, soft.ctypes.data if soft.size else None, soft.size, self.buf if cap else None, cap, C.byref(n)) == 0
        assert n.value <= cap
        return [(bytes(self.buf[i].data[:self.buf[i].len]), self.buf[i].end_sample) for i in range(n.value)]

    def drain(self, cap=16):
        out = []
        while True:
            got = self.push(np.zeros(0, np.int16), cap)
            out += got
            if len(got) < cap:
                return out

    def info(self):
        from rtl_sdr_rs_amd.afsk import Ax25Info
        i = Ax25Info()
        assert self.lib.fmd_ax25_decoder_info(self.d, C.byref(i)) == 0
        return i.frames_ok, i.bad_fcs, i.aborts, int(i.in_frame)

    def close(self):
        self.lib.fmd_ax25_decoder_free(self.d)


def _train(rng, n, level=1):
    """n good frames as soft decisions at 5 per bit: (soft, the frames, the line level behind them)"""
    frames = [_frame(rng) for _ in range(n)]
    bits = []
    for f in frames:
        bits += xr.frame_bits(f, flags=2)
    lv = xr.nrzi(bits, level)
    return np.repeat(np.where(np.array(lv) == 1, 7000, -7000), 5).astype(np.int16), frames, lv[-1]


def test_the_ring_of_64_gives_up_its_oldest_frames_and_keeps_the_order(fmd):
    rng = np.random.default_rng(seed(8200))
    soft, frames, level = _train(rng, 70)
    level70 = level
    want = xr.Decoder(6000).push(soft)
    assert [f["data"] for f in want] == frames
    r = _Raw(fmd)
    assert r.push(soft, 0) == []                             # nobody takes them: 70 frames into a ring of 64
    assert r.info() == (70, 0, 0, 1)
    assert r.drain() == [(f["data"], f["end_sample"]) for f in want[6:]]       # the last 64, in order, with their own end_sample
    assert r.drain() == []
    # frames wait, and a push with room for 3 brings 4 more: the waiting ones come out first, the new ones queue up behind them
    more, frames2, level = _train(rng, 10, level)
    assert r.push(more, 0) == []
    last, frames3, _ = _train(rng, 4, level)
    got = r.push(last, 3)
    assert [g[0] for g in got] == frames2[:3]
    assert [g[0] for g in r.drain(5)] == frames2[3:] + frames3
    # room for more than wait: the waiting ones first, then the new ones straight into the caller's array
    r2 = _Raw(fmd)
    a, fa, level = _train(rng, 3)
    b, fb, _ = _train(rng, 5, level)
    assert r2.push(a, 0) == [] and [g[0] for g in r2.push(b, 6)] == fa + fb[:3] and [g[0] for g in r2.drain()] == fb[3:]
    # a full ring and a push with room for everything: the 64 that wait leave at the push's start, the new ones follow
    r3 = _Raw(fmd)
    assert r3.push(soft, 0) == []
    c, fc, _ = _train(rng, 2, level70)
    assert [g[0] for g in r3.push(c, 80)] == frames[6:] + fc
    for x in (r, r2, r3):
        x.close()


# ---- end_sample ----------------------------------------------------------------------------------------------------------------------
def test_end_sample_counts_from_the_last_reset_whatever_the_pushes(fmd):
    rng = np.random.default_rng(seed(8300))
    soft, frames, _ = _train(rng, 6)
    ref = xr.Decoder(6000)
    want = ref.push(soft)
    ends = [f["end_sample"] for f in want]
    assert [f["data"] for f in want] == frames and ends == sorted(ends) and ends[-1] < len(soft)
    # the closing flag's last bit is taken near its middle: 5 samples per bit, (k + 1) frames of known bit counts
    pos = 0
    for f, e in zip(frames, ends):
        pos += 5 * len(xr.frame_bits(f, flags=2))
        assert pos - 5 <= e < pos
    dec = fmd.Ax25Decoder(6000)
    junk = rng.integers(-32768, 32768, 777).astype(np.int16)
    for cuts in ([len(soft)], [1] * 300 + [len(soft)], rng.integers(0, 500, 60).tolist() + [len(soft)], [0, 0, 5, len(soft)]):
        dec.push(junk)                                       # whatever came before the reset does not count
        dec.reset()
        got, lo = [], 0
        for n in cuts:
            got += dec.push(soft[lo:lo + n])
            lo += n
        assert got == want, cuts[:5]
    again = dec.push(soft)                                   # without a reset the count goes on
    assert len(again) == 6 and all(len(soft) < f["end_sample"] < 2 * len(soft) for f in again)
    dec.close()
