"""Station bank (include/fmd.h, fmd_stations_*) without a GPU: the test-side definition's anchor to the reference chain, the
integer helpers of the C ABI, the domain refusals (decided before a device is queried) and the shipped code object."""
import ctypes as C

import numpy as np
import pytest

import stations_ref as sr
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)


def _lib():
    import rtl_sdr_rs_amd as fmd
    return fmd, fmd.lib()


@pytest.mark.parametrize("D", [2, 6, 10, 16, 64])
def test_reference_anchor_inc0_on_rotated_bytes_is_the_oracle_chain(oracle, D):
    """inc = 0, h = 1...1, T = D, shift = 0 on rot(B) is Demod::demodulate(B), over ragged and full-scale calls."""
    rng = np.random.default_rng(100 + D)
    d = oracle.new(oracle.config(D, 240000, 32000))
    ref = sr.StationsRef(oracle, np.ones(D, np.int16), D, [0], 240000, 32000, 0)
    calls = [rng.integers(0, 256, n, dtype=np.uint8) for n in (8 * D * 2, 8 * 37, 8 * (5 * D + 3), 65536)]
    calls += [np.full(8 * 40 * D, 255, np.uint8), np.zeros(8 * 40 * D, np.uint8), np.tile(np.array([255, 0], np.uint8), 4 * 40 * D)]
    for B in calls:
        assert np.array_equal(ref.feed(sr.rot90(B))[0], oracle.demodulate(d, B))
        assert ref.state(0)["demod_pre"] == oracle.state_of(d)["demod_pre"]
        assert ref.state(0)["now_lpr"] == oracle.state_of(d)["now_lpr"]


def test_numpy_rotate_90_is_the_oracles(oracle):
    b = np.random.default_rng(7).integers(0, 256, 4096, dtype=np.uint8)
    o = b.copy()
    assert oracle.lib.fmo_rotate_90(o.ctypes.data_as(C.POINTER(C.c_uint8)), o.size) == 0
    assert np.array_equal(sr.rot90(b), o)


def test_nco_table_matches_numpy():
    _, lib = _lib()
    tab = np.zeros(1024, np.int16)
    assert lib.fmd_stations_nco_table(tab.ctypes.data_as(C.POINTER(C.c_int16))) == 0
    assert np.array_equal(tab.astype(np.int64), sr.nco_table())
    # no entry within 3.9e-4 of a rounding tie: any libm gives this table
    v = 16384.0 * np.cos(2.0 * np.pi * np.arange(1024) / 1024.0)
    assert np.min(np.abs(np.abs(v - np.floor(v)) - 0.5)) > 3.9e-4


def test_phase_inc_is_exact_integer_arithmetic():
    fmd, lib = _lib()
    rng = np.random.default_rng(3)
    cases = [(0, 2400000), (1, 2400000), (-1, 2400000), (1200000, 2400000), (-1200000, 2400000), (300000, 2400000),
             (-300000, 2400000), (1, 3), (-1, 3), (7, 15), (-7, 15), (2147483647 // 2, 4294967295), (-(4294967295 // 2), 4294967295)]
    for _ in range(200):
        rate = int(rng.integers(1, 1 << 32))
        cases.append((int(rng.integers(-(rate // 2), rate // 2 + 1)), rate))
    for off, rate in cases:
        assert fmd.phase_inc(off, rate) == sr.phase_inc(off, rate), (off, rate)
    inc = C.c_uint32()
    assert lib.fmd_stations_phase_inc(1200001, 2400000, C.byref(inc)) == -6      # FMD_ERR_UNSUPPORTED
    assert lib.fmd_stations_phase_inc(-1200001, 2400000, C.byref(inc)) == -6
    assert lib.fmd_stations_phase_inc(0, 0, C.byref(inc)) == -4                  # FMD_ERR_BAD_RATES
    assert lib.fmd_stations_phase_inc(0, 100, None) == -1


def test_out_cap_bounds_every_call(oracle):
    _, lib = _lib()
    rng = np.random.default_rng(5)
    for _ in range(30):
        D = int(rng.choice([2, 4, 6, 10, 16, 64]))
        fast = int(rng.integers(32000, 300000))
        slow = int(rng.integers(1000, fast + 1))
        nbytes = 8 * int(rng.integers(1, 20000))
        cap = lib.fmd_stations_out_cap(D, fast, slow, nbytes)
        most = (nbytes // 2 // D + 1) * slow // fast + 1          # at most one audio sample per rate_out / rate_resample outputs, + 1 carried
        assert cap >= most
        assert cap == lib.fmd_firdemod_out_cap(D, fast, slow, nbytes)
    assert lib.fmd_stations_out_cap(0, 1, 1, 64) == 0 and lib.fmd_stations_out_cap(2, 0, 1, 64) == 0


def _new(lib, taps, decim, shift, incs, K, fast, slow, n_streams=1):
    import rtl_sdr_rs_amd as fmd
    taps = np.ascontiguousarray(taps, dtype=np.int16)
    incs = np.ascontiguousarray(incs, dtype=np.uint32)
    h = C.c_void_p()
    dev = fmd.DeviceConfig(n_streams, 0, 0)
    rc = lib.fmd_stations_new(taps.ctypes.data_as(C.POINTER(C.c_int16)), taps.size, decim, shift,
                              incs.ctypes.data_as(C.POINTER(C.c_uint32)), K, fast, slow, C.byref(dev), C.byref(h))
    if rc == 0:
        lib.fmd_stations_free(h)
    return rc


def test_domain_refusals_need_no_gpu():
    _, lib = _lib()
    ones = np.ones(8, np.int16)
    z = np.zeros(32, np.uint32)
    U, R = -6, -4
    assert _new(lib, ones, 3, 0, z, 1, 240000, 32000) == U                       # odd decim
    assert _new(lib, ones, 66, 0, z, 1, 240000, 32000) == U                      # decim > 64
    assert _new(lib, ones, 0, 0, z, 1, 240000, 32000) == U
    assert _new(lib, np.ones(257, np.int16), 10, 0, z, 1, 240000, 32000) == U    # T > 256
    assert _new(lib, np.ones(0, np.int16), 10, 0, z, 1, 240000, 32000) == U      # T == 0
    assert _new(lib, ones, 8, 0, np.zeros(33, np.uint32), 33, 240000, 32000) == U   # K > 32
    assert _new(lib, ones, 8, 0, z, 0, 240000, 32000) == U                       # K == 0
    assert _new(lib, np.full(8, 2048, np.int16), 8, 10, z, 1, 240000, 32000) == U   # |h| > 2047
    assert _new(lib, ones, 8, 25, z, 1, 240000, 32000) == U                      # shift > 24
    assert _new(lib, ones, 8, 0, z, 1, 32000, 48000) == R                        # rate_out < rate_resample
    assert _new(lib, ones, 8, 0, z, 1, 32000, 0) == R
    # the gain bound: ceil(256 G / 2^shift) <= 16384 -- at inc = 0, G = sum|h|
    h = np.full(64, 100, np.int16)                                              # G = 6400: 256 G = 1638400 -> shift >= 7
    assert _new(lib, h, 8, 6, z, 1, 240000, 32000) == U
    inc = np.array([sr.phase_inc(300000, 2400000)], np.uint32)
    g = sr.max_gain(h, inc)
    s = 0
    while -(-256 * g >> s) > 16384:
        s += 1
    assert _new(lib, h, 8, s - 1, inc, 1, 240000, 32000) == U


def test_auto_shift_matches_the_definition():
    import rtl_sdr_rs_amd as fmd
    rng = np.random.default_rng(9)
    h = rng.integers(-2047, 2048, 64).astype(np.int16)
    incs = [sr.phase_inc(int(o), 2400000) for o in (-900000, -300000, 0, 450000)]
    s = fmd.stations_auto_shift(h, incs)
    g = sr.max_gain(h, incs)
    assert -(-256 * g >> s) <= 2048 < -(-256 * g >> (s - 1))


def test_code_object_has_the_station_kernel_on_the_matrix_cores(code_objects):  # noqa: F811
    ks = {n: k for n, k in code_objects.items() if "fmd_stations" in n}
    assert ks, sorted(code_objects)[:5]
    for n, k in ks.items():
        assert any(re_i.startswith("v_mfma_i32_16x16x64_i8") or re_i.startswith("v_mfma_i32_32x32x32_i8") for re_i in k["text"]), n
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert not any(i.startswith("scratch_") for i in k["text"]), n
        assert not any(bad in n for bad in ("fmd_demod_tile_kernel<", "fmd_demod_stream_kernel<", "fmd_fir_", "fmd_firdemod")), n
        assert any(i.startswith("global_load_lds_dwordx4") for i in k["text"]), n


@pytest.mark.parametrize("D,T,K", [(2, 1, 1), (2, 3, 2), (4, 27, 3), (6, 5, 1), (10, 64, 8), (30, 59, 4), (64, 256, 2), (64, 26, 5)])
def test_correlation_path_equals_the_gather_form(oracle, D, T, K):
    """sr.z_corr (production-size calls) against sr.z_direct, bit for bit, over random and full-scale bytes and taps, and the
    whole StationsRef chain fed the same calls through either."""
    rng = np.random.default_rng(7000 + 100 * D + T)
    for h in (rng.integers(-2047, 2048, T), np.where(rng.random(T) < 0.5, -2047, 2047)):
        incs = [int(x) for x in rng.integers(0, 1 << 32, K)]
        w = [sr.complex_taps(h, i) for i in incs]
        wr, wi = np.stack([a for a, _ in w]), np.stack([b for _, b in w])
        for b in (rng.integers(0, 256, 2 * (40 * D + T + 9)), np.where(rng.random(2 * (40 * D + T + 9)) < 0.5, 0, 255)):
            cr, ci = b[0::2].astype(np.int64) - 127, b[1::2].astype(np.int64) - 127
            for first, M in ((0, 1), (3, 17), (7, 40)):
                zd, zc = sr.z_direct(cr, ci, wr, wi, D, first, M), sr.z_corr(cr, ci, wr, wi, D, first, M)
                assert all(np.array_equal(a, c) and a.dtype == c.dtype for a, c in zip(zd, zc)), (first, M)
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    incs = [int(x) for x in rng.integers(0, 1 << 32, K)]
    shift = 0
    while -(-256 * sr.max_gain(h, incs) >> shift) > 16384:
        shift += 1
    a = sr.StationsRef(oracle, h, D, incs, 240000, 32000, shift)
    c = sr.StationsRef(oracle, h, D, incs, 240000, 32000, shift, z=sr.z_corr)
    for n in (8 * (T + 2 * D), 8 * 5, 8 * 700, 8 * (T // 4 + 1)):
        b = np.where(rng.random(n) < 0.3, 0, 255).astype(np.uint8) if n == 8 * 700 else rng.integers(0, 256, n, dtype=np.uint8)
        try:
            ea = a.feed(b)
        except sr.TooShort:
            with pytest.raises(sr.TooShort):
                c.feed(b)
            continue
        ec = c.feed(b)
        assert all(np.array_equal(x, y) for x, y in zip(ea, ec))
        assert [a.state(k) for k in range(K)] == [c.state(k) for k in range(K)]


def accepted_rates(D, T, K, rate_out, rate_resample):
    """The rate rule of include/fmd.h (station bank, "Rates"), restated: the reduced terms, then one audio sample per tile."""
    import math
    g = math.gcd(rate_out, rate_resample)
    fr, srr = rate_out // g, rate_resample // g
    if fr > 1 << 24 or 3 * srr >= 1 << 24:
        return False
    c = -(-rate_out // rate_resample)
    cap = 2 * c + 3
    if cap > 256:
        return False
    groups = -(-cap // 64)                                   # 16-column groups of a wave
    nkc = -(-(12 + 2 * T) // 64)
    raw = max(12 + 6 * D + 8 * D * (16 * groups - 1) + 64 * nkc, 12 + 2 * D * (cap - 1) + 2 * T + 15)
    raw = -(-raw // 16) * 16
    return raw + 2048 + 4 * K * cap + 24 <= 65536


def test_rate_ratio_rule_is_what_the_library_refuses():
    """The bank refuses exactly the rate ratios the documented rule refuses: accepted shows up as FMD_ERR_NO_DEVICE without a GPU
    (the sizing is decided before a device is queried), and as a handle with one."""
    _, lib = _lib()
    U, NODEV = -6, -8
    rng = np.random.default_rng(17)
    cases = [(2, 8, 1, 1260000, 10000), (2, 8, 1, 1260001, 10000), (64, 256, 32, 1160000, 10000), (64, 256, 32, 1161000, 10000),
             (2, 64, 8, 1200000, 8000), (10, 64, 8, 240000, 32000), (2, 1, 1, 48000, 48000), (64, 256, 32, 48000, 48000),
             (2, 8, 1, 1 << 24, 1), (2, 8, 1, (1 << 24) + 1, 1), (2, 8, 1, (1 << 24) - 1, 5592405), (2, 8, 1, (1 << 24) - 1, 5592406),
             (2, 8, 1, 16777213, 16777212), (2, 8, 1, 4000037, 3999971)]
    for c in (110, 116, 117, 120, 125, 126, 127):
        for D, T, K in ((64, 256, 32), (64, 256, 1), (2, 256, 32), (64, 1, 32), (30, 128, 17), (62, 200, 24)):
            cases.append((D, T, K, c * 10000, 10000))
            cases.append((D, T, K, (c - 1) * 10007 + 1, 10007))
    for _ in range(120):
        D = 2 * int(rng.integers(1, 33))
        T, K = int(rng.integers(1, 257)), int(rng.integers(1, 33))
        slow = int(rng.integers(1, 200000))
        fast = int(slow * rng.uniform(1.0, 140.0))
        cases.append((D, T, K, fast, slow))
    seen = set()
    for D, T, K, fast, slow in cases:
        want = accepted_rates(D, T, K, fast, slow)
        seen.add(want)
        rc = _new(lib, np.ones(T, np.int16), D, 24, np.zeros(K, np.uint32), K, fast, slow)
        assert rc in ((0, NODEV) if want else (U,)), (D, T, K, fast, slow, rc)
    assert seen == {True, False}
    # the limits the header quotes
    assert all(accepted_rates(64, 256, 32, 116 * r, r) for r in (1, 7, 10000))
    assert not accepted_rates(64, 256, 32, 117 * 10000, 10000)
    assert all(accepted_rates(D, T, K, 126 * 10000, 10000) for D, T, K in ((2, 8, 1), (10, 64, 8), (64, 1, 1)))
    assert not accepted_rates(2, 1, 1, 126 * 10000 + 1, 10000)
