"""Power-spectrum scanner (include/fmd.h, fmd_spectrum_*) without a GPU: the integer helpers of the C ABI against the test-side
definition (tests/spectrum_ref.py), that definition against np.fft, the domain refusals (decided before a device is queried),
the station picker on a synthetic spectrum, and the shipped code object."""
import ctypes as C

import numpy as np
import pytest

import spectrum_ref as spr
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

U, INV = -6, -1


def _lib():
    import rtl_sdr_rs_amd as fmd
    return fmd, fmd.lib()


def test_hann_window_is_the_definition():
    fmd, lib = _lib()
    for N in spr.BINS:
        for A in (1, 64, 127, 128, 1000, 2047):
            got = fmd.hann_window(N, A)
            assert np.array_equal(got, spr.hann(N, A)), (N, A)
            assert got.max() <= A and got.min() >= 0
        assert spr.digits(spr.hann(N, 127)) == 1 and spr.digits(spr.hann(N, 2047)) == 2
    w = np.zeros(256, np.int16)
    p = w.ctypes.data_as(C.POINTER(C.c_int16))
    assert lib.fmd_spectrum_hann(64, 0, p) == U and lib.fmd_spectrum_hann(64, 2048, p) == U
    assert lib.fmd_spectrum_hann(48, 100, p) == U and lib.fmd_spectrum_hann(512, 100, p) == U
    assert lib.fmd_spectrum_hann(64, 100, None) == INV


def test_bin_inc_is_the_definition_and_the_bank_phase_inc():
    fmd, lib = _lib()
    inc = C.c_uint32()
    for N in spr.BINS:
        for k in range(N):
            assert lib.fmd_spectrum_bin_inc(k, N, C.byref(inc)) == 0
            assert inc.value == spr.bin_inc(k, N) == (k * (1 << 32) // N) % (1 << 32)
        # the bin's centre offset at a rate N divides tunes the station bank exactly there
        rate = 2400000 // N * N
        for k in (1, N // 4, N // 2 - 1, N // 2, 3 * N // 4, N - 1):
            off = (k if k < N // 2 else k - N) * rate // N
            assert fmd.phase_inc(off, rate) == spr.bin_inc(k, N), (N, k)
    assert lib.fmd_spectrum_bin_inc(64, 64, C.byref(inc)) == U
    assert lib.fmd_spectrum_bin_inc(0, 100, C.byref(inc)) == U
    assert lib.fmd_spectrum_bin_inc(0, 64, None) == INV


def test_frames_match_the_definition():
    _, lib = _lib()
    rng = np.random.default_rng(2)
    for _ in range(300):
        N = int(rng.choice(spr.BINS))
        hop = 8 * int(rng.integers(1, N // 8 + 1))
        nbytes = 8 * int(rng.integers(0, 4 * N))
        assert lib.fmd_spectrum_frames(N, hop, nbytes) == spr.frames(N, hop, nbytes), (N, hop, nbytes)
    assert lib.fmd_spectrum_frames(64, 64, 2 * 64) == 1 and lib.fmd_spectrum_frames(64, 64, 2 * 64 - 8) == 0
    assert lib.fmd_spectrum_frames(64, 64, 262144) == 2048 and lib.fmd_spectrum_frames(256, 8, 262144) == (131072 - 256) // 8 + 1
    for N, hop in ((64, 4), (64, 12), (64, 72), (64, 0), (48, 8), (512, 8)):
        assert lib.fmd_spectrum_frames(N, hop, 1 << 16) == 0, (N, hop)


def _new(lib, window, N, hop, shift, n_streams=1):
    import rtl_sdr_rs_amd as fmd
    h = C.c_void_p()
    dev = fmd.DeviceConfig(n_streams, 0, 0)
    wp = None if window is None else np.ascontiguousarray(window, np.int16).ctypes.data_as(C.POINTER(C.c_int16))
    rc = lib.fmd_spectrum_new(wp, N, hop, shift, C.byref(dev), C.byref(h))
    if rc == 0:
        lib.fmd_spectrum_free(h)
    return rc


def test_domain_refusals_need_no_gpu():
    _, lib = _lib()
    w = spr.hann(256, 2047)
    for N in (0, 8, 48, 100, 512):
        assert _new(lib, w, N, 8, 0) == U, N
    for hop in (0, 4, 12, 60, 72):
        assert _new(lib, w, 64, hop, 0) == U, hop
    assert _new(lib, w, 16, 24, 0) == U                       # hop > N
    assert _new(lib, w, 64, 64, 64) == U                      # shift > 63
    bad = w[:64].copy()
    bad[5] = 2048
    assert _new(lib, bad, 64, 64, 0) == U
    bad[5] = -2048
    assert _new(lib, bad, 64, 64, 0) == U
    assert _new(lib, w, 64, 64, 0, n_streams=0) == INV
    assert _new(lib, None, 64, 64, 0) == INV
    h = C.c_void_p()
    assert lib.fmd_spectrum_new(w.ctypes.data_as(C.POINTER(C.c_int16)), 64, 64, 0, None, C.byref(h)) == INV
    buf = np.zeros(64, np.uint8)
    out = np.zeros(64, np.uint64)
    assert lib.fmd_spectrum_power_batch(None, buf.ctypes.data, 64, out.ctypes.data) == INV
    assert lib.fmd_spectrum_power_device(None, buf.ctypes.data, 64, out.ctypes.data, 0, None) == INV
    assert lib.fmd_spectrum_check(None) == INV


def _tone(N, k0, n, amp=100.0):
    t = np.arange(n)
    x = amp * np.exp(2j * np.pi * k0 * t / N)
    iq = np.empty(2 * n, np.uint8)
    iq[0::2] = np.round(x.real + 127)
    iq[1::2] = np.round(x.imag + 127)
    return iq


@pytest.mark.parametrize("N", spr.BINS)
def test_definition_agrees_with_numpy_fft_on_a_tone(N):
    rng = np.random.default_rng(N)
    for A in (127, 2047):
        w = spr.hann(N, A)
        for k0 in (int(rng.integers(1, N // 2)), N // 4):
            for k in (k0, N - k0):                                 # +f0 and -f0
                hop = N // 2
                iq = _tone(N, k, 8 * N)
                P = spr.power(w, hop, 0, iq)[0]
                assert int(np.argmax(P)) == k, (N, A, k)
                # the same frames through np.fft: |P_ref^1/2 - P_fft^1/2| <= ||z_ref - z_fft||_2 <= sqrt(F) N max|dW| max|c|
                c = (iq[0::2].astype(np.float64) - 127) + 1j * (iq[1::2].astype(np.float64) - 127)
                F = spr.frames(N, hop, iq.size)
                fr = np.stack([c[f * hop:f * hop + N] for f in range(F)]) * w
                Pf = (np.abs(np.fft.fft(fr, axis=1)) ** 2).sum(axis=0)
                tol = np.sqrt(F) * N * 0.75 * np.abs(c).max()
                assert np.all(np.abs(np.sqrt(P.astype(np.float64)) - np.sqrt(Pf)) <= tol), (N, A, k)
                assert np.sqrt(P[k]) > 20 * tol                     # the check above is not vacuous at the peak


def test_definition_is_exact_at_full_scale_and_wraps_mod_2_64():
    N = 256
    w = np.full(N, 2047, np.int16)
    iq = np.tile(np.array([255, 0], np.uint8), 4 * N)            # c = 128 - 127 j ...: |z| < 2^31
    P = spr.power(w, 8, 0, iq)
    wr, wi = spr.taps(w)
    c = np.full(N, 128, np.int64) + 1j * np.full(N, -127, np.int64)
    z = (wr + 1j * wi) @ c
    p = [int(round(v.real)) ** 2 + int(round(v.imag)) ** 2 for v in z]
    F = spr.frames(N, 8, iq.size)
    assert [int(x) for x in P[0]] == [(F * v) % (1 << 64) for v in p]


def test_find_stations_on_a_synthetic_spectrum():
    import rtl_sdr_rs_amd as fmd
    N, rate = 256, 2400000
    df = rate / N
    f = np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N) * df
    rng = np.random.default_rng(3)
    p = rng.uniform(0.8, 1.2, N) * 1e6
    truth = [-700000.0, -300000.0, 50000.0, 610000.0]
    for c in truth:                                              # a tone-modulated FM station: two horns at +-75 kHz
        p += 1e9 * (np.exp(-0.5 * ((f - c - 75000) / 6000) ** 2) + np.exp(-0.5 * ((f - c + 75000) / 6000) ** 2))
    offs, bins = fmd.find_stations(p.astype(np.uint64), rate, count=8)
    assert offs.size == len(truth)
    assert np.all(np.abs(offs - np.array(truth)) < df), offs
    assert np.array_equal(bins, np.round(np.array(truth) / df).astype(np.int64) % N)
    offs2, _ = fmd.find_stations(p, rate, count=2)
    assert offs2.size == 2
    assert fmd.find_stations(np.ones(N), rate, count=4)[0].size == 0


def test_code_object_has_the_spectrum_kernel_on_the_matrix_cores(code_objects):  # noqa: F811
    ks = {n: k for n, k in code_objects.items() if "fmd_spectrum" in n}
    assert len(ks) == 4, sorted(ks)                              # one per K-chunk count: N = 16/32, 64, 128, 256
    for n, k in ks.items():
        assert any(i.startswith("v_mfma_i32_16x16x64_i8") or i.startswith("v_mfma_i32_32x32x32_i8") for i in k["text"]), n
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert not any(i.startswith("scratch_") for i in k["text"]), n
        assert not any(bad in n for bad in ("fmd_stations", "fmd_demod_tile_kernel", "fmd_demod_stream_kernel", "fmd_fir")), n


@pytest.mark.parametrize("N,hop", [(16, 8), (32, 24), (64, 40), (128, 120), (256, 248), (256, 8)])
def test_chunked_power_equals_the_direct_form(N, hop):
    """spr.power_chunked (long calls) against spr.power, bit for bit: random and full-scale windows and bytes, chunks that split
    the frames unevenly, and a sum that wraps modulo 2^64 at shift 0."""
    rng = np.random.default_rng(300 + N + hop)
    nbytes = 2 * (N + hop * 700 + int(rng.integers(0, hop)))
    nbytes += (-nbytes) % 8
    wins = [rng.integers(-2047, 2048, N).astype(np.int16), np.where(rng.random(N) < 0.5, -2047, 2047).astype(np.int16),
            spr.hann(N, 127)]
    data = [rng.integers(0, 256, (2, nbytes), dtype=np.uint8), np.where(rng.random((2, nbytes)) < 0.5, 0, 255).astype(np.uint8)]
    for w in wins:
        for b in data:
            for shift in (0, 7):
                want = spr.power(w, hop, shift, b)
                for chunk in (97, 1 << 14):
                    assert np.array_equal(spr.power_chunked(w, hop, shift, b, chunk=chunk), want), (chunk, shift)
