"""Test-side definition of the RDS bank (include/fmd.h, "RDS bank"), in numpy int64: the channelizer's y (tests/channelizer_ref.py),
the stereo bank's discriminator and pilot sums (tests/stereo_ref.py), the free-running 57 kHz carrier, the FIR and the shift.
Independent of the library.  Also an RDS encoder and a synthesizer of FM stations that carry RDS, as u8 IQ bytes, for the decoder
tests: groups 0A / 0B, 2A / 2B or raw -> 26-bit blocks (checkword by polynomial division, offset word XORed in) -> differential coding ->
biphase impulse pairs -> shaping -> 57 kHz subcarrier in the multiplex -> FM -> u8 IQ."""
import numpy as np

import channelizer_ref as cr
import stations_ref as sr
import stereo_ref as st
from stations_ref import TooShort  # noqa: F401  (re-exported: a call that completes no output)

BIT_RATE = 1187.5
POLY = 0x5B9                                                 # x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
OFFSETS = {"A": 0x0FC, "B": 0x198, "C": 0x168, "C'": 0x350, "D": 0x1B4}


class RdsRef:
    """One input stream, K stations; feed() mirrors one fmd_rds call of that stream and returns int64 [K, n, 2] (ur, ui).  Keeps
    every x and q since reset (test sizes only)."""

    def __init__(self, taps, decim, incs, shift, capture_rate, rds_taps, out_decim, rds_shift, block=4096, pilot_min=0, z=None):
        self.ch = cr.ChannelizerRef(taps, decim, incs, shift, z=z)
        self.K = len(self.ch.incs)
        self.g = np.asarray(rds_taps, dtype=np.int64)
        self.Ta, self.R, self.rds_shift = self.g.size, int(out_decim), int(rds_shift)
        self.P, self.pilot_min = int(block), int(pilot_min)
        self.inc_p = st.pilot_inc(int(capture_rate), int(decim))
        self.reset()

    def reset(self):
        self.ch.reset()
        self.yprev = np.zeros((self.K, 2), dtype=np.int64)
        self.x = [np.zeros(0, np.int64) for _ in range(self.K)]
        self.qr = [np.zeros(0, np.int64) for _ in range(self.K)]
        self.qi = [np.zeros(0, np.int64) for _ in range(self.K)]
        self.x_max = self.q_max = self.v_max = 0             # max |x|, |q| and |v| since reset
        self.cuts = [0]                                      # MPX samples after every accepted call
        self.n_next = 0

    def out_after(self, m):
        return (m - self.Ta) // self.R + 1 if m >= self.Ta else 0

    def completes(self, nbytes):
        """Outputs a call of nbytes completes (0: refused)."""
        return self.out_after(self.ch.outputs_after(nbytes // 2)) - self.n_next

    # The four steps below are methods of their own so that tests/test_domain_cases.py can derive deliberately wrong variants and
    # show that the domain cases tell them from the definition.

    def carrier_index(self, m0):
        """Index of the call's first MPX sample as the carrier counts it: m since creation or reset."""
        return m0

    def shifted(self, v):
        return v >> self.rds_shift                           # arithmetic: floor

    def window(self, q, lo, hi, m0):
        """q[lo:hi], the samples the call's outputs read; those below m0 came with earlier calls."""
        return q[lo:hi]

    def block_span(self, j):
        """The samples summed for block j."""
        return j * self.P, (j + 1) * self.P

    def blocks_done(self, m):
        """Blocks complete after m MPX samples."""
        return m // self.P

    def feed(self, buf):
        b = np.asarray(buf, dtype=np.uint8)
        if self.completes(b.size) < 1:
            raise TooShort()
        y = self.ch.feed(b)                                   # [K, M, 2]
        M = y.shape[1]
        out = []
        for k in range(self.K):
            yy = np.concatenate([self.yprev[k][None, :], y[k]], axis=0)
            x = st.wrap16(st.disc_fast(yy[1:, 0], yy[1:, 1], yy[:-1, 0], yy[:-1, 1]))
            self.yprev[k] = y[k, -1]
            m0 = self.x[k].size
            self.x[k] = np.concatenate([self.x[k], x])
            self.x_max = max(self.x_max, int(np.abs(x).max()))
            phi = (np.arange(self.carrier_index(m0), self.carrier_index(m0) + M, dtype=np.uint64) * np.uint64((3 * self.inc_p) & 0xFFFFFFFF)) & 0xFFFFFFFF
            qr, qi = (x * sr.cosq(phi)) >> 14, (-x * sr.sinq(phi)) >> 14
            self.q_max = max(self.q_max, int(np.abs(qr).max()), int(np.abs(qi).max()))
            self.qr[k] = np.concatenate([self.qr[k], qr])
            self.qi[k] = np.concatenate([self.qi[k], qi])
            n1 = self.out_after(self.x[k].size)
            lo, hi = self.R * self.n_next, self.R * (n1 - 1) + self.Ta
            vr = np.correlate(self.window(self.qr[k], lo, hi, m0), self.g, "valid")[::self.R]
            vi = np.correlate(self.window(self.qi[k], lo, hi, m0), self.g, "valid")[::self.R]
            self.v_max = max(self.v_max, int(np.abs(vr).max()), int(np.abs(vi).max()))
            u = np.stack([self.shifted(vr), self.shifted(vi)], axis=1)
            assert np.abs(u).max() <= 32767                  # the int16 store is exact
            out.append(u)
        self.n_next = self.out_after(self.x[0].size)
        self.cuts.append(self.x[0].size)
        return np.stack(out)

    def pilot(self, k):
        """(present, level) of the last completed block, as StereoRef.pilot."""
        jn = self.blocks_done(self.x[k].size)
        if jn == 0:
            return False, 0
        a, b = self.block_span(jn - 1)
        m = np.arange(a, b, dtype=np.uint64)
        th = (m * np.uint64(self.inc_p)) & 0xFFFFFFFF
        x = self.x[k][a:b]
        I, Q = int((x * sr.cosq(th)).sum()), int((x * sr.sinq(th)).sum())
        present = self.pilot_min > 0 and I * I + Q * Q >= (self.pilot_min * self.P * 8192) ** 2
        return present, st.isqrt(I * I + Q * Q) // (self.P * 8192)


# ---- encoder -------------------------------------------------------------------------------------------------------------------

def remainder(v, nbits):
    """v(x) mod the generator, v of `nbits` bits."""
    for i in range(nbits - 1, 9, -1):
        if v >> i & 1:
            v ^= POLY << (i - 10)
    return v & 0x3FF


def encode_block(info, offset):
    """16 information bits -> the 26-bit block: checkword = info(x) x^10 mod g(x), then the offset word XORed in."""
    return (info << 10 | remainder(info << 10, 26)) ^ OFFSETS[offset]


def groups_0a_2a(pi, ps, rt, flag=0):
    """The station's group cycle: four 0A groups (PS, two characters each; block C carries an AF filler) and one 2A group per four
    characters of `rt` (padded with spaces to a multiple of four), interleaved 0A, 2A, 0A, 2A ... as a broadcaster does."""
    assert len(ps) == 8 and len(rt) <= 64
    rt = rt + " " * (-len(rt) % 4)
    a0 = [(pi, 0 << 12 | 0 << 11 | 1 << 3 | a, 0xE0CD, ord(ps[2 * a]) << 8 | ord(ps[2 * a + 1])) for a in range(4)]
    a2 = [(pi, 2 << 12 | 0 << 11 | flag << 4 | a, ord(rt[4 * a]) << 8 | ord(rt[4 * a + 1]), ord(rt[4 * a + 2]) << 8 | ord(rt[4 * a + 3]))
          for a in range(len(rt) // 4)]
    out = []
    for i in range(max(len(a0), len(a2))):
        if i < len(a0):
            out.append(a0[i])
        if i < len(a2):
            out.append(a2[i])
    return out


def groups_0b_2b(pi, ps, rt, flag=0):
    """The version-B cycle: four 0B groups (PS) and one 2B group per TWO characters of `rt` (at most 32, padded with spaces to an
    even count), interleaved as in groups_0a_2a.  Bit 11 of block B is set and block C repeats the PI, sent with offset C'."""
    assert len(ps) == 8 and len(rt) <= 32
    rt = rt + " " * (len(rt) % 2)
    b0 = [(pi, 0 << 12 | 1 << 11 | 1 << 3 | a, pi, ord(ps[2 * a]) << 8 | ord(ps[2 * a + 1])) for a in range(4)]
    b2 = [(pi, 2 << 12 | 1 << 11 | flag << 4 | a, pi, ord(rt[2 * a]) << 8 | ord(rt[2 * a + 1])) for a in range(len(rt) // 2)]
    out = []
    for i in range(max(len(b0), len(b2))):
        out += b0[i:i + 1] + b2[i:i + 1]
    return out


def raw_group(a, b, c, d):
    """Any group from its four 16-bit words; group_bits sends block C with offset C' when b says version B (bit 11)."""
    assert all(0 <= v < 1 << 16 for v in (a, b, c, d))
    return a, b, c, d


def group_offsets(group):
    """The offset words of the group's four blocks: C' in place of C in a version-B group."""
    return "A", "B", "C'" if group[1] >> 11 & 1 else "C", "D"


def group_bits(groups):
    """Groups (A, B, C, D) -> the transmitted bit stream (before differential coding), MSB of block A first."""
    bits = []
    for g in groups:
        for info, off in zip(g, group_offsets(g)):
            blk = encode_block(info, off)
            bits += [blk >> i & 1 for i in range(25, -1, -1)]
    return np.array(bits, dtype=np.int64)


def differential(bits):
    """e[k] = bits[k] xor e[k - 1], e[-1] = 0."""
    return np.bitwise_xor.accumulate(np.asarray(bits, dtype=np.int64))


def biphase_waveform(ebits, t, bit_rate=BIT_RATE):
    """The shaped biphase signal at the times t (seconds; bit k is centred at (k + 1/2) / bit_rate): per bit an impulse pair
    +a at the first quarter and -a at the third, a = 2 e - 1, each shaped by a raised-cosine (Hann) pulse one bit period wide.  This
    is a stand-in for the standard's cosine filter: the same +-2.4 kHz main lobe (zeros at 2 / T), no interference between the
    half-symbol centres, finite support.  The bit stream repeats cyclically.  Peak amplitude about 1."""
    T = 1.0 / bit_rate
    a = 2.0 * np.asarray(ebits, dtype=np.float64) - 1.0
    n = a.size
    r = np.zeros(t.size)
    u = t / T                                                # in bit periods
    for half, sign in ((0.25, 1.0), (0.75, -1.0)):
        for dk in (-1, 0, 1):                                # pulses within half a period of t
            k = np.floor(u).astype(np.int64) + dk
            d = u - (k + half)
            r += np.where(np.abs(d) < 0.5, sign * a[k % n] * 0.5 * (1 + np.cos(2 * np.pi * d)), 0.0)
    return r


def baseband_direct(bits, fs, f_res=0.0, phase=0.0, amp=97.0, noise=1.0, seed=0, start_bit=0.0, bit_rate=BIT_RATE):
    """The RDS bank's output without the bank: int16 [n, 2] at fs of amp * biphase_waveform(differential(bits), t) * exp(j (2 pi
    f_res t + phase)) plus white noise of `noise` per component (the defaults are about the level of the full chain's baseband of the decoder
    tests' station), from `start_bit` bit periods into the stream to its end.  Takes the
    BIT stream, so a test can damage bits before the differential coding: one flipped bit is exactly one wrong decoded bit.  Bit k
    is centred at sample ((k + 1/2 - start_bit) / bit_rate) fs."""
    n = int((len(bits) - start_bit) * fs / bit_rate)
    t = np.arange(n) / fs
    r = amp * biphase_waveform(differential(bits), t + start_bit / bit_rate, bit_rate)
    rng = np.random.default_rng(seed)
    z = r * np.exp(1j * (2 * np.pi * f_res * t + phase)) + rng.normal(0, noise, n) + 1j * rng.normal(0, noise, n)
    return np.ascontiguousarray(np.stack([np.round(z.real), np.round(z.imag)], axis=1).astype(np.int16))


def synth_rds_iq(n, fs, stations, amp=50.0, noise=0.5, seed=0, start_bit=0.0):
    """u8 IQ bytes (2 n of them) at fs.  Every station is (offset_hz, groups, pilot_hz, alpha, tone_hz): its multiplex is a 15 % audio
    tone, the pilot at 6.75 kHz deviation, and the RDS signal of `groups` (repeated cyclically) on sin(3 (theta + alpha)) at 2 kHz
    deviation, theta = 2 pi pilot_hz t; the bit clock is pilot_hz / 16, locked to the pilot as a coder's is.  FM-modulated at 75 kHz
    peak deviation scale at its offset from the centre, summed, plus white noise, quantised.  The capture starts `start_bit` bit periods
    into the group cycle (a receiver is switched on at any time)."""
    t = np.arange(n) / fs
    z = np.zeros(n, np.complex128)
    for off, groups, pilot_hz, alpha, tone_hz in stations:
        theta = 2 * np.pi * pilot_hz * t + alpha
        r = biphase_waveform(differential(group_bits(groups)), t + start_bit * 16.0 / pilot_hz, pilot_hz / 16.0)
        m = 0.15 * np.sin(2 * np.pi * tone_hz * t) + (6750.0 / 75000.0) * np.sin(theta) + (2000.0 / 75000.0) * r * np.sin(3 * theta)
        ph = 2 * np.pi * 75000.0 * np.cumsum(m) / fs
        z += amp * np.exp(1j * (2 * np.pi * off * t + ph))
    rng = np.random.default_rng(seed)
    z += rng.normal(0, noise, n) + 1j * rng.normal(0, noise, n)
    iq = np.empty(2 * n, np.uint8)
    iq[0::2] = np.clip(np.round(z.real + 127.5), 0, 255)
    iq[1::2] = np.clip(np.round(z.imag + 127.5), 0, 255)
    return iq


# ---- the decoder tests' station ------------------------------------------------------------------------------------------------
FS, D, R, T_FRONT, T_RDS = 256000, 2, 16, 64, 255
PI, PS, RT = 0xD3C2, "TEST FM ", "Now: RDS on GPU!"                  # a 16-character RadioText
PILOT_HZ = 19002.0                                           # leaves about +6 Hz at 57 kHz
# PS takes four 0A groups and 16 characters of RadioText four 2A groups: eight groups, 832 bit periods, while 0.7 s holds 831.  Block
# A of the first group is not needed (PI comes with every group), so a capture that starts inside that block -- a receiver is
# switched on at any time -- holds blocks B, C, D of all eight groups, ending 10 bit periods before the capture does.
START_BIT = 10.0


def station_capture(seconds, offsets=(40000,), seed=7, start_bit=START_BIT, alpha=0.7, fs=FS):
    """(iq bytes, groups): `seconds` of the test station at each of `offsets`."""
    groups = groups_0a_2a(PI, PS, RT)
    n = int(round(seconds * fs)) // 4 * 4
    return synth_rds_iq(n, fs, [(o, groups, PILOT_HZ, alpha, 1000.0) for o in offsets], seed=seed, start_bit=start_bit), groups


def front_taps():
    return st.lowpass(T_FRONT, 62000 / FS)
