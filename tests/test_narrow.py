"""Narrow-band bank (include/fmd.h, fmd_narrow_*) without a GPU: the test-side definition (tests/narrow_ref.py) -- its anchors to the
channelizer and the reference's discriminator, the per-sample form against the vectorised one, split invariance, the arithmetic
bounds at the domain's edges, what the operator does on synthesized AM, SSB and NFM channels next to a strong neighbour, the squelch
and the level -- the out_cap bound, the domain refusals (decided before a device is queried), the channel taps and the shipped code
objects."""
import ctypes as C
import math

import numpy as np
import pytest

import channelizer_ref as cr
import narrow_ref as nr
import stations_ref as sr
import stereo_ref as st
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

U, NODEV = -6, -8
FS, D, R, TA, P = 2400000, 10, 20, 256, 256
FA = FS / D / R                                              # 12 kHz
OFF, NEIGHBOUR = 300000, 325000                              # the channel and a strong carrier 25 kHz above it (inside the front end)


def _lib():
    import rtl_sdr_rs_amd as fmd
    return fmd, fmd.lib()


def _ref(mode, lo, hi, offs=(OFF,), squelch=0, gain=256, h=None, limit=None, block=P):
    import rtl_sdr_rs_amd as fmd
    h = st.lowpass(64, 100000 / FS) if h is None else h
    incs = [sr.phase_inc(o, FS) for o in offs]
    gr, gi = fmd.narrow_taps(FS // D, TA, lo, hi)
    shift = fmd.stations_auto_shift(h, incs, limit=16384)
    cs = fmd.narrow_auto_shift(h, incs, shift, gr, gi, mode=mode, limit=limit)
    return nr.NarrowRef(h, D, incs, shift, gr, gi, mode, R, cs, block, squelch, gain, z=sr.z_corr)


def _snr_db(a, f, fs, skip):
    """Power of the tone f in a[skip:] against everything else in it (its mean excluded), in dB."""
    v = np.asarray(a[skip:], dtype=np.float64)
    v = v - v.mean()
    n = np.arange(v.size)
    c = np.sum(v * np.exp(-2j * np.pi * f * n / fs)) * 2 / v.size
    tone = np.abs(c) ** 2 / 2
    return 10 * np.log10(tone / max(v.var() - tone, 1e-9)), np.abs(c)


# ---- anchors of the definition ---------------------------------------------------------------------------------------------------

def test_anchor_iq_is_the_channelizer_and_fm_its_discriminator():
    rng = np.random.default_rng(1)
    h = rng.integers(-2047, 2048, 40).astype(np.int16)
    incs = [int(v) for v in rng.integers(0, 1 << 32, 3)]
    import rtl_sdr_rs_amd as fmd
    shift = fmd.stations_auto_shift(h, incs, limit=256)
    b = rng.integers(0, 256, 8 * 700, dtype=np.uint8)
    y = cr.ChannelizerRef(h, 4, incs, shift).feed(b)
    iq = nr.NarrowRef(h, 4, incs, shift, [1], None, nr.IQ, 1, 0, 16, 0, 256).feed(b)
    fm = nr.NarrowRef(h, 4, incs, shift, [1], None, nr.FM, 1, 0, 16, 0, 256).feed(b)
    assert np.array_equal(iq, y)
    for k in range(3):
        yy = np.concatenate([np.zeros((1, 2), np.int64), y[k]])
        assert np.array_equal(fm[k], st.wrap16(st.disc_fast(yy[1:, 0], yy[1:, 1], yy[:-1, 0], yy[:-1, 1]))), k


@pytest.mark.parametrize("mode", [nr.IQ, nr.FM, nr.AM, nr.SSB])
def test_per_sample_form_agrees_with_the_vectorised_form(mode):
    import rtl_sdr_rs_amd as fmd
    rng = np.random.default_rng(10 + mode)
    h = rng.integers(-2047, 2048, 20).astype(np.int16)
    incs = [12345678, 4000000000]
    shift = fmd.stations_auto_shift(h, incs, limit=2048)
    gr, gi = rng.integers(-3000, 3000, 7).astype(np.int16), rng.integers(-3000, 3000, 7).astype(np.int16)
    cs = fmd.narrow_auto_shift(h, incs, shift, gr, gi, limit=300)
    b = rng.integers(0, 256, 8 * 900, dtype=np.uint8)
    b[3000:5000] = rng.integers(126, 130, 2000)
    ref = nr.NarrowRef(h, 4, incs, shift, gr, gi, mode, 3, cs, 16, 0, 700)
    rms = math.isqrt(int((ref.feed(b) if mode == nr.IQ else nr.NarrowRef(h, 4, incs, shift, gr, gi, nr.IQ, 3, cs, 16, 0, 256).feed(b))
                         .astype(np.float64).var() * 2))
    for squelch in (0, max(1, rms)):
        ref = nr.NarrowRef(h, 4, incs, shift, gr, gi, mode, 3, cs, 16, squelch, 700)
        o = np.concatenate([ref.feed(b[:2400]), ref.feed(b[2400:4992]), ref.feed(b[4992:])], axis=1)
        for k in range(2):
            d = nr.direct(ref.y[k].tolist(), gr.tolist(), gi.tolist(), mode, 3, cs, 16, squelch, 700)
            assert np.array_equal(np.array(d).reshape(o[k].shape), o[k]), (mode, k, squelch)
        if squelch:
            z = (o == 0).reshape(2, -1).mean()
            assert 0.05 < z < 0.95, z                         # the squelch both opened and closed


def test_split_invariance_of_the_definition():
    """Any cut into calls -- shorter than a block, blocks straddling calls, refused calls resent -- gives the same output."""
    rng = np.random.default_rng(2)
    n = 6 * P * R * D + 4000
    z = nr.am(n, FS, OFF, 20.0, 1000.0) * (np.arange(n) > n // 3) + nr.carrier(n, FS, NEIGHBOUR, 40.0)
    iq = nr.to_u8(z, noise=1.0, seed=2)
    for mode in (nr.AM, nr.FM, nr.IQ):
        whole = _ref(mode, -4000, 4000, squelch=100, block=64, limit=16384).feed(iq)
        part = _ref(mode, -4000, 4000, squelch=100, block=64, limit=16384)
        pieces, pos, pending, refused = [], 0, np.zeros(0, np.uint8), 0
        while pos < iq.size:
            m = min(8 * int(rng.integers(1, 400 if rng.random() < 0.7 else 9000)), iq.size - pos)
            buf = np.concatenate([pending, iq[pos:pos + m]])
            pos += m
            if part.completes(buf.size) < 1:
                with pytest.raises(nr.TooShort):
                    part.feed(buf)
                pending, refused = buf, refused + 1
                continue
            pieces.append(part.feed(buf))
            pending = np.zeros(0, np.uint8)
        got = np.concatenate(pieces, axis=1)
        assert np.array_equal(got, whole[:, :got.shape[1]]) and got.shape[1] >= whole.shape[1] - 1
        assert refused >= 1 and 0 < np.count_nonzero(got) < got.size and not got[:, :64].any()


# ---- bounds ----------------------------------------------------------------------------------------------------------------------

def test_bounds_at_the_domain_edges():
    """|v| <= B_y G < 2^30, |u| <= 16384, |u|^2 <= 2^29, a <= 23170, E_j <= 2^41, squelch^2 P < 2^41, |w gain| < 2^31; the
    integer square root at 2^29 and around perfect squares; maximal taps over bytes 0 / 255 stay inside the bounds and come within
    a factor of two of them (B_y counts |Wr| + |Wi| against both components of c at once, which no input attains)."""
    assert 16384 * 65535 < 2 ** 30 and 2 * 16384 ** 2 == 2 ** 29
    assert math.isqrt(2 ** 29) == 23170 and 23170 ** 2 <= 2 ** 29 < 23171 ** 2
    assert 4096 * 2 ** 29 == 2 ** 41 and 23170 ** 2 * 4096 < 2 ** 41 and 4096 * 23170 < 2 ** 32
    assert 23170 * 65535 < 2 ** 31 and 2 ** 14 * 65535 < 2 ** 31 and 16383 < 2 ** 23 and 16384 < 2 ** 23
    r = np.arange(0, 23171, dtype=np.int64)
    for d in (-1, 0, 1):
        x = np.clip(r * r + d, 0, 2 ** 29)
        assert np.array_equal(nr.isqrt_vec(x), [math.isqrt(int(v)) for v in x])
    x = np.concatenate([np.arange(2 ** 29 - 50000, 2 ** 29 + 1), np.random.default_rng(3).integers(0, 2 ** 29 + 1, 50000)])
    assert np.array_equal(nr.isqrt_vec(x), [math.isqrt(int(v)) for v in x])
    # B_y = 16384 exactly (sum |W| = 2^15, shift 9), G = 65535 (4 x 16383 + 3), chan_shift 16, bytes at the rails
    h = np.array([2047] * 16 + [16], np.int16)
    B = -(-256 * int(np.abs(h.astype(np.int64)).sum()) >> 9)
    assert B == 16384
    gr = np.array([16383, 16383, 16383, 16383, 3], np.int16)
    assert -(-B * 65535 >> 16) == 16384
    rng = np.random.default_rng(4)
    for gi, pat in ((None, 0), (None, 1), (np.array([0, 0, 0, 0, 0]), 2)):
        ref = nr.NarrowRef(h, 2, [0], 9, gr if pat < 2 else np.array([16383, 16383, 0, 0, 3]),
                           None if pat < 2 else np.array([0, 0, 16383, 16383, 0]), nr.AM, 1, 16, 16, 23170, 65535)
        b = np.empty(8 * 400, np.uint8)
        if pat == 0:
            b[0::2], b[1::2] = 255, 0
        else:
            b[0::2] = np.repeat(np.where(rng.random(100) < 0.5, 0, 255), 16)
            b[1::2] = np.repeat(np.where(rng.random(100) < 0.5, 0, 255), 16)
        out = ref.feed(b)
        u, a = ref.u[0], ref.a[0]
        assert ref.v_max <= B * 65535 and np.abs(u).max() <= 16384 and (u * u).sum(axis=1).max() <= 2 ** 29 and a.max() <= 23170
        assert ref.v_max > 0.49 * B * 65535, ref.v_max       # the rails reach half the bound: real W at offset 0 sees one component
        E = max(ref.block(0, j)[0] for j in range(ref.n_next // 16))
        assert E <= 16 * 2 ** 29 and np.abs(out).max() <= 32767
        if pat == 0:
            assert a.max() >= 11500 and E >= 16 * 2 ** 27 * 0.98


# ---- what the operator does ------------------------------------------------------------------------------------------------------

def _with_neighbour(sig, n, seed):
    return nr.to_u8(sig + nr.carrier(n, FS, NEIGHBOUR, 60.0), noise=1.0, seed=seed)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_am_tone_is_recovered_with_its_dc_removed(seed):
    """A 1 kHz tone at 50 % depth on a carrier of amplitude 20, a carrier of amplitude 60 25 kHz above it: after the first block the
    output's mean is within 2 % of the tone's amplitude of zero and the tone stands >= 24 dB above the rest (measured: 26.9 - 27.0 dB,
    mean / tone 0.007 over these seeds; the carrier is 328 counts of u after the worst-case chan_shift, so the floor is rounding)."""
    n = 5 * P * R * D
    ref = _ref(nr.AM, -4000, 4000)
    a = ref.feed(_with_neighbour(nr.am(n, FS, OFF, 20.0, 1000.0), n, seed))[0]
    snr, tone = _snr_db(a, 1000.0, FA, P)
    mean = a[P:].mean()
    print("AM: snr %.1f dB, tone %.0f, mean %.1f, first-block mean %.0f" % (snr, tone, mean, a[:P].mean()))
    assert snr >= 24 and abs(mean) <= 0.02 * tone
    assert a[:P].mean() > 1.5 * tone                          # block 0 still carries the carrier's level: dc_{-1} = 0
    opn, rms = ref.level(0)
    assert opn and abs(tone / rms - 0.5 / math.sqrt(1 + 0.125)) < 0.03       # depth 0.5 against the RMS of (1 + 0.5 sin)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ssb_filters_pass_their_own_sideband_only(seed):
    """A tone 1 kHz above the (suppressed) carrier passes the USB filter (300, 3000) and is rejected by the LSB filter (-3000, -300);
    1 kHz below, the reverse; a strong carrier 25 kHz away throughout.  Rejection >= 30 dB (measured: 34.7 dB over these seeds: 256
    taps at 240 kHz make a transition band about 3 kHz wide, and the rejected tone sits 1.3 kHz from the filter's edge)."""
    n = 3 * P * R * D
    res = {}
    for side, f in (("above", 1000.0), ("below", -1000.0)):
        iq = _with_neighbour(nr.ssb_tone(n, FS, OFF, 20.0, f), n, seed)
        for name, (lo, hi) in (("usb", (300, 3000)), ("lsb", (-3000, -300))):
            a = _ref(nr.SSB, lo, hi).feed(iq)[0]
            res[side, name] = st.tone_db(a, 1000.0, FA, P)
    print("SSB: " + ", ".join("%s/%s %.1f dB" % (k + (v,)) for k, v in res.items()))
    assert res["above", "usb"] - res["above", "lsb"] >= 30 and res["below", "lsb"] - res["below", "usb"] >= 30
    assert abs(res["above", "usb"] - res["below", "lsb"]) < 1


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_nfm_tone_is_recovered(seed):
    """A 1 kHz tone at 2.5 kHz deviation: its amplitude is 32768 dev / f_a in discriminator units to within 10 % and it stands >= 25 dB
    above the rest (measured: 32.7 - 33.0 dB and 4.6 % low over these seeds: the +-6 kHz filter trims the outer FM sidebands).  The
    chan_shift is chosen for |u| <= 4096: the carrier is then about 80 counts, far below where the discriminator wraps."""
    n = 3 * P * R * D
    a = _ref(nr.FM, -6000, 6000, limit=4096).feed(_with_neighbour(nr.nfm(n, FS, OFF, 20.0, 1000.0, 2500.0), n, seed))[0]
    snr, tone = _snr_db(a, 1000.0, FA, P)
    print("NFM: snr %.1f dB, tone %.0f (nominal %.0f)" % (snr, tone, 32768 * 2500 / FA))
    assert snr >= 25 and abs(tone / (32768 * 2500 / FA) - 1) < 0.10


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_squelch_mutes_noise_and_opens_one_block_after_the_carrier(seed):
    """Noise only, then a carrier from the middle of block 2 on: blocks 0 ... 2 are muted (they follow noise-only blocks), block 3
    follows a block the carrier only half fills, block 4 follows a full one and is open; `level` reads the carrier's amplitude."""
    n = 6 * P * R * D
    start = int(2.5 * P * R * D)
    sig = nr.carrier(n, FS, OFF, 20.0) * (np.arange(n) >= start)
    probe = _ref(nr.IQ, -4000, 4000)
    u = probe.feed(_with_neighbour(sig, n, seed))[0].astype(np.float64)
    rms = np.sqrt((u[:5 * P] ** 2).sum(axis=1).reshape(5, P).mean(axis=1))
    print("squelch: block rms %s" % np.round(rms, 1))
    assert rms[:2].max() * 8 < rms[3:].min()                 # (measured: noise ~ 2, carrier ~ 329)
    squelch = int(rms[3] / 4)
    ref = _ref(nr.AM, -4000, 4000, squelch=squelch)
    a = ref.feed(_with_neighbour(sig, n, seed))[0]
    assert not a[:3 * P].any() and a[4 * P:5 * P].any() and a[5 * P:].any()
    opn, level = ref.level(0)
    # the carrier's amplitude in units of u: amp x the front end's and the channel filter's DC gain over the two shifts
    nominal = 20.0 * ref.ch.h.sum() * ref.gr.sum() / 2.0 ** (ref.ch.shift + ref.chan_shift)
    print("level %d, nominal %.1f" % (level, nominal))
    assert opn and abs(level / nominal - 1) < 0.03
    quiet = _ref(nr.AM, -4000, 4000, offs=(-500000,), squelch=squelch)
    assert not quiet.feed(_with_neighbour(sig, n, seed)).any() and quiet.level(0)[0] is False


# ---- the library without a device ------------------------------------------------------------------------------------------------

def test_out_cap_bounds_every_call_and_history():
    _, lib = _lib()
    rng = np.random.default_rng(6)
    for _ in range(500):
        Dd = 2 * int(rng.integers(1, 33))
        T = int(rng.integers(1, 257))
        Ta, Rr = int(rng.integers(1, 257)), int(rng.integers(1, 33))
        pos = int(rng.integers(0, 20 * (T + Dd * (Ta + Rr))))
        nbytes = 8 * int(rng.integers(1, 200)) if rng.random() < 0.5 else 8 * int(rng.integers(1, 200000))
        cap = lib.fmd_narrow_out_cap(Dd, Rr, nbytes)
        assert cap == -(-nbytes // (2 * Dd * Rr))
        ref = nr.NarrowRef(np.ones(T, np.int64), Dd, [0], 0, np.ones(Ta, np.int64), None, nr.IQ, Rr, 0, 16, 0, 256)
        ref.ch.pos = pos
        ref.n_next = ref.audio_after(ref.ch.outputs_after(0))
        assert ref.completes(nbytes) <= cap, (Dd, T, Ta, Rr, pos, nbytes)
    assert lib.fmd_narrow_out_cap(0, 5, 64) == 0 and lib.fmd_narrow_out_cap(10, 0, 64) == 0
    assert [lib.fmd_narrow_out_width(m) for m in range(4)] == [2, 1, 1, 1]


def _new(lib, taps=None, decim=10, shift=4, incs=(0,), gr=(100,), gi=None, mode=1, R=5, cs=0, block=256, squelch=0, gain=256, n_streams=1):
    import rtl_sdr_rs_amd as fmd
    taps = np.ascontiguousarray(np.ones(8, np.int16) if taps is None else taps, dtype=np.int16)
    incs = np.ascontiguousarray(incs, dtype=np.uint32)
    gr = np.ascontiguousarray(gr, dtype=np.int16)
    gi = None if gi is None else np.ascontiguousarray(gi, dtype=np.int16)
    cfg = fmd.narrow.NarrowConfig(mode, R, cs, block, squelch, gain)
    h = C.c_void_p()
    dev = fmd.DeviceConfig(n_streams, 0, 0)
    p16 = C.POINTER(C.c_int16)
    rc = lib.fmd_narrow_new(taps.ctypes.data_as(p16), taps.size, decim, shift, incs.ctypes.data_as(C.POINTER(C.c_uint32)), incs.size,
                            gr.ctypes.data_as(p16), None if gi is None else gi.ctypes.data_as(p16), gr.size, C.byref(cfg), C.byref(dev),
                            C.byref(h))
    if rc == 0:
        lib.fmd_narrow_free(h)
    return rc


def test_domain_refusals_need_no_gpu():
    _, lib = _lib()
    assert _new(lib, decim=3) == U and _new(lib, decim=66) == U
    assert _new(lib, taps=np.ones(257, np.int16)) == U
    assert _new(lib, taps=np.full(8, 2048, np.int16)) == U
    assert _new(lib, shift=25) == U
    assert _new(lib, incs=np.zeros(33)) == U
    assert _new(lib, taps=np.full(64, 2047, np.int16), shift=0) == U          # B_y > 16384
    assert _new(lib, R=0) == U and _new(lib, R=33) == U
    msg = lib.fmd_last_error().decode()                      # this bank's own limits, not the band-plan bank's
    assert "chan_decim <= 32" in msg and "n_chan_taps <= 256" in msg, msg
    assert _new(lib, gr=np.ones(257, np.int16)) == U
    assert _new(lib, gr=[16384], cs=30) == U and _new(lib, gr=[1], gi=[-16384], cs=30) == U          # |tap| > 16383
    assert _new(lib, gr=[16383] * 4 + [4], cs=30) == U                       # G = 65536
    assert _new(lib, gr=[16383, 16383, 2], gi=[16383, -16383, 2], cs=30) == U          # G = 65536 with complex taps
    assert _new(lib, cs=31) == U
    # ones(8) at shift 4: B_y = ceil(256 * 8 / 16) = 128; G = 128 -> B_y G = 2^14: chan_shift 0 is the edge
    assert _new(lib, gr=[128], cs=0) in (0, NODEV) and _new(lib, gr=[129], cs=0) == U and _new(lib, gr=[64], gi=[65], cs=0) == U
    for blk in (8, 24, 1000, 8192):
        assert _new(lib, block=blk) == U, blk
    assert _new(lib, squelch=23171) == U
    assert _new(lib, gain=0) == U and _new(lib, gain=65536) == U
    assert _new(lib, mode=4) == U
    assert _new(lib, n_streams=65536) == U
    assert _new(lib, n_streams=0) == -1
    for kw in (dict(), dict(decim=64, block=4096, R=32, gr=np.full(256, 127, np.int16), gi=np.full(256, -128, np.int16), cs=30, squelch=23170,
                            gain=65535, mode=3),
               dict(decim=2, block=16, R=1, gr=[16383], cs=7, mode=0, gain=1), dict(gr=[16383] * 4 + [3], cs=16, mode=2),
               dict(gr=[1], gi=[0], mode=2)):
        assert _new(lib, **kw) in (0, NODEV), kw


def test_narrow_taps_meet_the_rule_and_choose_the_sideband():
    import rtl_sdr_rs_amd as fmd
    for fs, n, lo, hi in ((240000, 256, -4000, 4000), (240000, 256, 300, 3000), (240000, 255, -3000, -300), (37500, 1, -100, 100),
                          (170000, 2, 300, 3000), (37500, 63, -6000, 6000), (240000, 256, 5000, 100000)):
        gr, gi = fmd.narrow_taps(fs, n, lo, hi)
        assert gr.dtype == np.int16 and gr.size == n and (gi is None) == (lo == -hi)
        G = fmd.narrow.narrow_gain_sum(gr, gi)
        assert 0 < G <= 65535 and np.abs(gr).max() <= 16383 and (gi is None or np.abs(gi).max() <= 16383)
        if n >= 63:                                          # the response sum_t g[t] exp(j w t) at the band's centre and at its mirror
            g = gr.astype(np.float64) + (0 if gi is None else 1j * gi)
            t = np.arange(n)
            resp = lambda f: abs(np.sum(g * np.exp(2j * np.pi * f / fs * t)))
            fc = (lo + hi) / 2
            assert resp(fc) > 100 * resp(fc + 4 * (hi - lo))       # the pass band against the stop band
            if lo * hi > 0 and n >= 255:
                assert resp(fc) > 100 * resp(-fc)
    h = np.ones(10, np.int16)
    gr, gi = fmd.narrow_taps(240000, 256, -4000, 4000)
    for mode, limit in ((nr.FM, 256), (nr.AM, 16384), (nr.IQ, 16384), (nr.SSB, 16384)):
        cs = fmd.narrow_auto_shift(h, [0], 2, gr, gi, mode=mode)
        peak = fmd.narrow.narrow_y_bound(h, [0], 2) * fmd.narrow.narrow_gain_sum(gr, gi)
        assert -(-peak >> cs) <= limit and (cs == 0 or -(-peak >> (cs - 1)) > limit)


def test_null_arguments():
    _, lib = _lib()
    n, p, lv = C.c_uint64(), C.c_int(), C.c_uint32()
    assert lib.fmd_narrow_outputs(None, C.byref(n)) == -1
    assert lib.fmd_narrow_check(None) == -1
    assert lib.fmd_narrow_reset(None) == -1
    assert lib.fmd_narrow_level(None, 0, 0, C.byref(p), C.byref(lv)) == -1
    lib.fmd_narrow_free(None)


def _scalar_memory_write(op):
    """A scalar instruction that writes memory or manages the scalar data cache: none may be shipped."""
    return op.startswith("s_") and any(w in op for w in ("store", "atomic", "dcache"))


def test_code_objects_have_both_passes_without_scratch(code_objects):  # noqa: F811
    ddc = {n: k for n, k in code_objects.items() if "fmd_narrow_ddc_kernel" in n}
    chan = {n: k for n, k in code_objects.items() if "fmd_narrow_chan_kernel" in n}
    assert ddc and len(chan) == 2, sorted(code_objects)[:5]       # real and complex taps
    for n, k in ddc.items():
        assert any(i.startswith("v_mfma_i32_16x16x64_i8") for i in k["text"]), n
        assert any(i.startswith("global_load_lds_dwordx4") for i in k["text"]), n
    for n, k in chan.items():
        assert any(i.startswith("v_mad_i32_i24") for i in k["text"]), n
        assert any(i.startswith("ds_read2_b64") or i.startswith("ds_read_b64") for i in k["text"]), n
        assert any(i.startswith("s_load_dwordx8") for i in k["text"]), n     # the taps come through the scalar cache
        assert any(i.startswith("v_sqrt_f32") for i in k["text"]), n
        assert not any("f64" in i.split()[0] for i in k["text"]), n
    for n, k in list(ddc.items()) + list(chan.items()):
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert not any(i.startswith("scratch_") for i in k["text"]), n
        assert not any(_scalar_memory_write(i.split()[0]) for i in k["text"]), n
