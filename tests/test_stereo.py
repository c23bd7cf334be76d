"""Stereo station bank (include/fmd.h, fmd_stereo_*) without a GPU: the test-side definition (tests/stereo_ref.py) -- its
discriminator against pyref, split invariance, polarity and separation on synthesized stations, mono without a pilot, the
arithmetic bounds at the domain's edges -- the out_cap bound, the domain refusals (decided before a device is queried), the audio
taps and the shipped code objects."""
import ctypes as C

import numpy as np
import pytest

import pyref
import stations_ref as sr
import stereo_ref as st
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

U, NODEV = -6, -8
FS, D, R = 2400000, 10, 5


def _lib():
    import rtl_sdr_rs_amd as fmd
    return fmd, fmd.lib()


def _ref(incs, h=None, P=4096, pilot_min=None, g=None, audio_shift=None, shift=None):
    import rtl_sdr_rs_amd as fmd
    h = st.lowpass(64, 130000 / FS) if h is None else h
    g = fmd.stereo_taps(FS // D, R, 127) if g is None else g
    shift = fmd.stations_auto_shift(h, incs, limit=256) if shift is None else shift
    pmin = st.default_pilot_min(FS, D) if pilot_min is None else pilot_min
    ash = fmd.stereo.default_audio_shift(g, FS, D) if audio_shift is None else audio_shift
    return st.StereoRef(h, D, incs, shift, FS, g, R, P, pmin, ash, z=sr.z_corr)


def test_vector_discriminator_is_pyref_polar_discriminant_fast():
    rng = np.random.default_rng(1)
    for lim in (300, 16384):
        a = rng.integers(-lim, lim + 1, (4000, 2))
        b = rng.integers(-lim, lim + 1, (4000, 2))
        a[:50] = 0
        b[25:75] = 0
        got = st.disc_fast(a[:, 0], a[:, 1], b[:, 0], b[:, 1])
        exp = [pyref.polar_discriminant_fast(tuple(int(v) for v in a[i]), tuple(int(v) for v in b[i])) for i in range(a.shape[0])]
        assert np.array_equal(got, np.array(exp)), lim


def test_pilot_inc_matches_the_definition():
    _, lib = _lib()
    for rate, dec in ((2400000, 10), (1020000, 6), (106000 * 64, 64), (212000, 2), (3200000, 16)):
        inc = C.c_uint32()
        assert lib.fmd_stereo_pilot_inc(rate, dec, C.byref(inc)) == 0
        assert inc.value == st.pilot_inc(rate, dec) == ((19000 * dec * 2 ** 32 + rate // 2) // rate) % 2 ** 32
    assert lib.fmd_stereo_pilot_inc(0, 10, C.byref(inc)) == -1


def test_split_invariance_of_the_definition():
    """Any cut into calls -- shorter than a block, blocks straddling calls, refused calls resent -- gives the same audio."""
    rng = np.random.default_rng(2)
    incs = [sr.phase_inc(o, FS) for o in (-300000, 450000)]
    tone = lambda t: 0.2 * np.sin(2 * np.pi * 700 * t)
    zero = lambda t: 0 * t
    iq = st.synth_iq(3 * 1024 * D + 4000, FS, [(o, tone, zero, 1.0, True) for o in (-300000, 450000)], seed=2)
    whole = _ref(incs, P=1024).feed(iq)
    part = _ref(incs, P=1024)
    pieces, pos, pending = [], 0, np.zeros(0, np.uint8)
    while pos < iq.size:
        n = min(8 * int(rng.integers(1, 400 if rng.random() < 0.7 else 4000)), iq.size - pos)
        buf = np.concatenate([pending, iq[pos:pos + n]])
        pos += n
        if part.completes(buf.size) < 1:
            with pytest.raises(st.TooShort):
                part.feed(buf)
            pending = buf
            continue
        pieces.append(part.feed(buf))
        pending = np.zeros(0, np.uint8)
    got = np.concatenate(pieces, axis=1)
    assert np.array_equal(got, whole[:, :got.shape[1]]) and got.shape[1] >= whole.shape[1] - 1
    assert part.kc_max > 30000                                # the pilot was found: the carrier ran


@pytest.mark.parametrize("phi", [0, 90, 180, 271])
def test_polarity_and_separation(phi):
    """A 1 kHz tone on L only comes out on L; R is >= 25 dB down, at two offsets.  A swapped or inverted S fails this."""
    offs = [-400000, 300000]
    tone = lambda t: 0.15 * np.sin(2 * np.pi * 1000 * t)
    zero = lambda t: 0 * t
    iq = st.synth_iq(8 * 4096 * D, FS, [(o, tone, zero, np.deg2rad(phi), True) for o in offs], seed=phi)
    ref = _ref([sr.phase_inc(o, FS) for o in offs])
    a = ref.feed(iq)
    fa, skip = FS / D / R, 2 * 4096 // R
    for k in range(2):
        Ld, Rd = st.tone_db(a[k, :, 0], 1000, fa, skip), st.tone_db(a[k, :, 1], 1000, fa, skip)
        assert Ld - Rd >= 25, (phi, k, Ld, Rd)
        Mf, Sf = np.asarray(a[k, skip:, 0], float) + a[k, skip:, 1], np.asarray(a[k, skip:, 0], float) - a[k, skip:, 1]
        assert np.dot(Mf, Sf) > 0                            # L - R in phase with L + R: the sign of kc is right
        present, level = ref.pilot(k)
        assert present and 900 <= level <= 1600, level


def test_no_pilot_gives_identical_channels():
    tone = lambda t: 0.3 * np.sin(2 * np.pi * 1000 * t)
    zero = lambda t: 0 * t
    iq = st.synth_iq(3 * 4096 * D, FS, [(250000, tone, zero, 0.0, False)], seed=3)
    ref = _ref([sr.phase_inc(250000, FS)])
    a = ref.feed(iq)
    assert np.array_equal(a[..., 0], a[..., 1]) and ref.kc_max == 0
    assert ref.pilot(0)[0] is False


def test_pilot_min_zero_forces_mono():
    tone = lambda t: 0.3 * np.sin(2 * np.pi * 1000 * t)
    zero = lambda t: 0 * t
    iq = st.synth_iq(3 * 4096 * D, FS, [(250000, tone, zero, 0.0, True)], seed=4)
    ref = _ref([sr.phase_inc(250000, FS)], pilot_min=0)
    a = ref.feed(iq)
    assert np.array_equal(a[..., 0], a[..., 1])
    present, level = ref.pilot(0)
    assert not present and level > 500


def test_bounds_at_the_domain_edges():
    """|kc| <= 32770, |s| <= 65540 and |M +- S| < 2^31 for every estimate an i64 block sum can give.  (The table's rounding and the
    truncated c2, s2 allow 32770, one more than 2^15 + 1: (4615851610387, 1683718248746) reaches it.)"""
    rng = np.random.default_rng(5)
    lim = 1 << 43                                            # |I|, |Q| <= 32768 * 16384 * 16384
    cand = [lim, -lim, lim - 1, 1, -1, 0, 1 << 22, -(1 << 22) - 1, (1 << 23) - 1, -(1 << 23)]
    pairs = [(a, b) for a in cand for b in cand if a or b] + [tuple(int(v) for v in rng.integers(-lim, lim + 1, 2)) for _ in range(3000)]
    th = np.arange(0, 1 << 32, 1 << 22, dtype=np.uint64)    # every table index
    for I, Q in pairs:
        c2, s2 = st.angle_terms(I, Q)
        assert abs(c2) <= 16384 and abs(s2) <= 16384
        kc = (sr.sinq(th) * c2 + sr.cosq(th) * s2) >> 13
        assert np.abs(kc).max() <= 32770, (I, Q)
        for x in (32767, -32768):
            assert np.abs((x * kc) >> 14).max() <= 65540
            assert np.abs(x * kc).max() < 2 ** 31
    assert 16383 * (32768 + 65540) < 2 ** 31 and 65540 < 2 ** 23       # the FIR's sums and its 24-bit operands
    kc = (sr.sinq(th) * st.angle_terms(4615851610387, 1683718248746)[0] + sr.cosq(th) * st.angle_terms(4615851610387, 1683718248746)[1]) >> 13
    assert np.abs(kc).max() == 32770
    # presence is decided exactly at the threshold
    thr = 5 * 1024 * 8192
    assert st.estimate(thr, 0, 5, 1024)[0] and not st.estimate(thr - 1, 0, 5, 1024)[0]


def test_out_cap_bounds_every_call_and_history():
    _, lib = _lib()
    rng = np.random.default_rng(6)
    for _ in range(500):
        Dd = 2 * int(rng.integers(1, 33))
        T = int(rng.integers(1, 257))
        Ta, Rr = int(rng.integers(1, 257)), int(rng.integers(1, 33))
        pos = int(rng.integers(0, 20 * (T + Dd * (Ta + Rr))))
        nbytes = 8 * int(rng.integers(1, 200)) if rng.random() < 0.5 else 8 * int(rng.integers(1, 200000))
        cap = lib.fmd_stereo_out_cap(Dd, Rr, nbytes)
        assert cap == -(-nbytes // (2 * Dd * Rr))
        mpx = lambda s: (s - T) // Dd + 1 if s >= T else 0
        aud = lambda m: (m - Ta) // Rr + 1 if m >= Ta else 0
        assert aud(mpx(pos + nbytes // 2)) - aud(mpx(pos)) <= cap, (Dd, T, Ta, Rr, pos, nbytes)
    assert lib.fmd_stereo_out_cap(0, 5, 64) == 0 and lib.fmd_stereo_out_cap(10, 0, 64) == 0


def _new(lib, taps=None, decim=10, shift=4, incs=(0,), g=(100,), rate=2400000, block=4096, adec=5, ash=0, pmin=100, n_streams=1):
    import rtl_sdr_rs_amd as fmd
    taps = np.ascontiguousarray(np.ones(8, np.int16) if taps is None else taps, dtype=np.int16)
    incs = np.ascontiguousarray(incs, dtype=np.uint32)
    g = np.ascontiguousarray(g, dtype=np.int16)
    cfg = fmd.stereo.StereoConfig(rate, block, adec, ash, pmin)
    h = C.c_void_p()
    dev = fmd.DeviceConfig(n_streams, 0, 0)
    rc = lib.fmd_stereo_new(taps.ctypes.data_as(C.POINTER(C.c_int16)), taps.size, decim, shift, incs.ctypes.data_as(C.POINTER(C.c_uint32)),
                            incs.size, g.ctypes.data_as(C.POINTER(C.c_int16)), g.size, C.byref(cfg), C.byref(dev), C.byref(h))
    if rc == 0:
        lib.fmd_stereo_free(h)
    return rc


def test_domain_refusals_need_no_gpu():
    _, lib = _lib()
    assert _new(lib, decim=3) == U
    assert _new(lib, decim=66, rate=106000 * 66) == U
    assert _new(lib, taps=np.ones(257, np.int16)) == U
    assert _new(lib, taps=np.full(8, 2048, np.int16)) == U
    assert _new(lib, shift=25) == U
    assert _new(lib, incs=np.zeros(33)) == U
    assert _new(lib, taps=np.full(64, 2047, np.int16), shift=0) == U          # |y| bound
    assert _new(lib, rate=106000 * 10 - 1) == U                              # capture_rate < 106000 decim
    assert "106000" in lib.fmd_last_error().decode()
    for P in (512, 1000, 3000, 32768):
        assert _new(lib, block=P) == U, P
    assert _new(lib, adec=0) == U and _new(lib, adec=33) == U
    msg = lib.fmd_last_error().decode()                      # this bank's own names and limits, not the RDS bank's
    assert "audio_decim <= 32" in msg and "audio_shift <= 16" in msg and "rds" not in msg, msg
    assert _new(lib, g=np.ones(257, np.int16)) == U
    assert _new(lib, g=np.array([16383, 1], np.int16)) == U                  # sum |g| > 16383
    assert _new(lib, g=np.array([-8192, 8192], np.int16)) == U
    assert _new(lib, ash=17) == U and _new(lib, pmin=16385) == U
    assert _new(lib, n_streams=65536) == U
    assert _new(lib, n_streams=0) == -1
    assert _new(lib, g=np.array([16383], np.int16), ash=0) != U              # the RDS bank's exact-store rule is not this bank's
    for kw in (dict(), dict(decim=64, rate=106000 * 64, block=16384, adec=32, g=np.full(256, 63, np.int16), ash=16, pmin=16384),
               dict(decim=2, rate=212000, block=1024, adec=1, g=np.array([16383], np.int16), pmin=0),
               dict(g=np.array([-8191, 8192], np.int16))):
        assert _new(lib, **kw) in (0, NODEV), kw


def test_stereo_taps_meet_the_rule():
    import rtl_sdr_rs_amd as fmd
    for fs, n, tau in ((240000, 127, 75), (170000, 127, 50), (240000, 1, 75), (480000, 256, None), (106000, 2, 75)):
        g = fmd.stereo_taps(fs, 5, n, tau_us=tau)
        assert g.dtype == np.int16 and g.size == n
        assert 0 < int(np.abs(g.astype(np.int64)).sum()) <= 16383
        assert int(g.astype(np.int64).sum()) > 0


def test_null_arguments():
    _, lib = _lib()
    n, p, lv = C.c_uint64(), C.c_int(), C.c_uint32()
    assert lib.fmd_stereo_outputs(None, C.byref(n)) == -1
    assert lib.fmd_stereo_check(None) == -1
    assert lib.fmd_stereo_reset(None) == -1
    assert lib.fmd_stereo_pilot(None, 0, 0, C.byref(p), C.byref(lv)) == -1
    lib.fmd_stereo_free(None)


def test_code_objects_have_both_passes_without_scratch(code_objects):  # noqa: F811
    mpx = {n: k for n, k in code_objects.items() if "fmd_stereo_mpx_kernel" in n}
    aud = {n: k for n, k in code_objects.items() if "fmd_stereo_audio_kernel" in n}
    assert mpx and aud, sorted(code_objects)[:5]
    for n, k in mpx.items():
        assert any(i.startswith("v_mfma_i32_16x16x64_i8") for i in k["text"]), n
        assert any(i.startswith("global_load_lds_dwordx4") for i in k["text"]), n
        assert any(i.startswith("global_atomic_add_x2") for i in k["text"]), n
    for n, k in aud.items():
        assert any(i.startswith("v_mad_i32_i24") for i in k["text"]), n
    for n, k in list(mpx.items()) + list(aud.items()):
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert not any(i.startswith("scratch_") for i in k["text"]), n
