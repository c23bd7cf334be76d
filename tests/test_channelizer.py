"""Channelizer (include/fmd.h, fmd_channelizer_*) without a GPU: the test-side definition composed with the oracle's fm_demod +
low_pass_real is the station bank's definition, the out_cap bound, the domain refusals (decided before a device is queried), the
shift rule and the shipped code object."""
import ctypes as C

import numpy as np
import pytest

import channelizer_ref as cr
import stations_ref as sr
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

U, NODEV = -6, -8


def _lib():
    import rtl_sdr_rs_amd as fmd
    return fmd, fmd.lib()


def _shift_for(h, incs, limit=16384):
    g, s = sr.max_gain(h, incs), 0
    while -(-256 * g >> s) > limit:
        s += 1
    return s


@pytest.mark.parametrize("seed", range(6))
def test_definition_then_oracle_demod_is_the_station_bank_definition(oracle, seed):
    """channelizer_ref + the oracle's fm_demod + low_pass_real per call == StationsRef, bit for bit, over random shapes and cuts."""
    rng = np.random.default_rng(300 + seed)
    D = int(rng.choice([2, 4, 6, 10, 16, 30, 64]))
    T = int(rng.integers(1, 257)) if seed % 2 else int(rng.integers(1, D + 1))        # odd seeds: any T; even: T <= decim
    K = int(rng.integers(1, 6))
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    incs = [int(x) for x in rng.integers(0, 1 << 32, K)]
    shift = _shift_for(h, incs)
    fast = int(rng.integers(80000, 400000)) // D * D
    slow = int(rng.integers(8000, fast // 2))
    ref = sr.StationsRef(oracle, h, D, incs, fast, slow, shift, z=sr.z_corr)
    ch = cr.ChannelizerRef(h, D, incs, shift, z=sr.z_corr)
    demods = [oracle.new(oracle.config(D, fast, slow)) for _ in incs]
    fed = 0
    for _ in range(8):
        n = 8 * int(rng.integers(1, 3000))
        b = rng.integers(0, 256, n, dtype=np.uint8)
        if rng.random() < 0.3:
            b = np.where(rng.random(n) < 0.5, 0, 255).astype(np.uint8)
        if ch.outputs_after(n // 2) - ch.m_next < 2:         # the bank refuses such a call and changes nothing
            with pytest.raises(sr.TooShort):
                ref.feed(b)
            continue
        exp = ref.feed(b)
        got = cr.oracle_chain(oracle, demods, ch.feed(b))
        fed += 1
        for k in range(K):
            assert np.array_equal(got[k], exp[k]), (D, T, K, k)
    assert fed > 0
    for k in range(K):
        assert oracle.state_of(demods[k]) == ref.state(k)


def test_definition_carries_history_and_m_across_any_cut():
    rng = np.random.default_rng(8)
    for D, T in ((2, 1), (4, 3), (10, 64), (6, 5), (64, 256), (64, 20)):
        h = rng.integers(-2047, 2048, T)
        incs = [int(x) for x in rng.integers(0, 1 << 32, 3)]
        s = _shift_for(h, incs)
        data = rng.integers(0, 256, 8 * (40 * D + T), dtype=np.uint8)
        whole = cr.ChannelizerRef(h, D, incs, s).feed(data)
        part = cr.ChannelizerRef(h, D, incs, s)
        pieces, pos, pending = [], 0, np.zeros(0, np.uint8)
        while pos < data.size:
            n = min(8 * int(rng.integers(1, 2 * D + T // 2 + 2)), data.size - pos)
            buf = np.concatenate([pending, data[pos:pos + n]])
            pos += n
            if part.outputs_after(buf.size // 2) - part.m_next < 1:
                state = (part.pos, part.m_next, part.base, part.cr.size)
                with pytest.raises(cr.TooShort):              # refused: nothing changes, the caller sends the bytes again
                    part.feed(buf)
                assert (part.pos, part.m_next, part.base, part.cr.size) == state
                pending = buf
                continue
            pieces.append(part.feed(buf))
            pending = np.zeros(0, np.uint8)
        assert np.array_equal(np.concatenate(pieces, axis=1), whole), (D, T)
        assert np.abs(whole).max() <= 16384


def test_out_cap_bounds_every_call_and_history():
    _, lib = _lib()
    rng = np.random.default_rng(5)
    for _ in range(400):
        D = 2 * int(rng.integers(1, 33))
        T = int(rng.integers(1, 257)) if rng.random() < 0.7 else int(rng.integers(1, D + 1))
        pos = int(rng.integers(0, 5 * (T + D)))               # samples already consumed
        nbytes = 8 * int(rng.integers(1, 200)) if rng.random() < 0.5 else 8 * int(rng.integers(1, 20000))
        cap = lib.fmd_channelizer_out_cap(D, nbytes)
        assert cap == -(-nbytes // (2 * D))
        before = (pos - T) // D + 1 if pos >= T else 0
        after = (pos + nbytes // 2 - T) // D + 1 if pos + nbytes // 2 >= T else 0
        assert after - before <= cap, (D, T, pos, nbytes)
    # the bound is reached: nbytes = 2 D n from a state that starts on a window edge
    assert lib.fmd_channelizer_out_cap(10, 8 * 25) == 10
    assert lib.fmd_channelizer_out_cap(0, 64) == 0


def _new(lib, taps, decim, shift, incs, K, n_streams=1):
    import rtl_sdr_rs_amd as fmd
    taps = np.ascontiguousarray(taps, dtype=np.int16)
    incs = np.ascontiguousarray(incs, dtype=np.uint32)
    h = C.c_void_p()
    dev = fmd.DeviceConfig(n_streams, 0, 0)
    rc = lib.fmd_channelizer_new(taps.ctypes.data_as(C.POINTER(C.c_int16)), taps.size, decim, shift,
                                 incs.ctypes.data_as(C.POINTER(C.c_uint32)), K, C.byref(dev), C.byref(h))
    if rc == 0:
        lib.fmd_channelizer_free(h)
    return rc


def test_domain_refusals_need_no_gpu():
    _, lib = _lib()
    ones = np.ones(8, np.int16)
    z = np.zeros(32, np.uint32)
    assert _new(lib, ones, 3, 0, z, 1) == U                       # odd decim
    assert _new(lib, ones, 66, 0, z, 1) == U                      # decim > 64
    assert _new(lib, ones, 0, 0, z, 1) == U
    assert _new(lib, np.ones(257, np.int16), 10, 0, z, 1) == U    # T > 256
    assert _new(lib, np.ones(0, np.int16), 10, 0, z, 1) == U      # T == 0
    assert _new(lib, ones, 8, 0, np.zeros(33, np.uint32), 33) == U   # K > 32
    assert _new(lib, ones, 8, 0, z, 0) == U                       # K == 0
    assert _new(lib, np.full(8, 2048, np.int16), 8, 10, z, 1) == U   # |h| > 2047
    assert _new(lib, np.full(8, -2048, np.int16), 8, 10, z, 1) == U
    assert _new(lib, ones, 8, 25, z, 1) == U                      # shift > 24
    assert _new(lib, ones, 8, 0, z, 1, n_streams=65536) == U      # n_streams > 65535
    assert _new(lib, ones, 8, 0, z, 1, n_streams=0) == -1         # FMD_ERR_INVALID_ARG
    # inside the domain: a handle, or no device -- never a domain error (no rate parameters at all)
    for D, T, K in ((2, 1, 1), (64, 256, 32), (10, 64, 8), (64, 1, 32), (2, 256, 32)):
        assert _new(lib, np.ones(T, np.int16), D, 24, np.zeros(K, np.uint32), K) in (0, NODEV), (D, T, K)
    # the gain bound: ceil(256 G / 2^shift) <= 16384, at the edge
    rng = np.random.default_rng(12)
    for _ in range(6):
        T, K = int(rng.integers(1, 257)), int(rng.integers(1, 33))
        h = rng.integers(-2047, 2048, T).astype(np.int16)
        incs = rng.integers(0, 1 << 32, K).astype(np.uint32)
        s = _shift_for(h, incs)
        assert _new(lib, h, 10, s, incs, K) in (0, NODEV)
        if s > 0:
            assert _new(lib, h, 10, s - 1, incs, K) == U


def test_auto_shift_meets_the_16384_rule():
    import rtl_sdr_rs_amd as fmd
    _, lib = _lib()
    rng = np.random.default_rng(9)
    for T in (1, 7, 64, 256):
        h = rng.integers(-2047, 2048, T).astype(np.int16)
        incs = [sr.phase_inc(int(o), 2400000) for o in (-900000, -300000, 0, 450000)]
        s = fmd.stations_auto_shift(h, incs, limit=16384)
        g = sr.max_gain(h, incs)
        assert -(-256 * g >> s) <= 16384
        assert s == 0 or -(-256 * g >> (s - 1)) > 16384
        assert _new(lib, h, 10, s, np.array(incs, np.uint32), 4) in (0, NODEV)


def test_as_complex_and_null_arguments():
    fmd, lib = _lib()
    x = np.array([[[1, -2], [16384, -16384]]], np.int16)
    c = fmd.as_complex(x)
    assert c.dtype == np.complex64 and c.shape == (1, 2)
    assert c[0, 0] == 1 - 2j and c[0, 1] == 16384 - 16384j
    with pytest.raises(ValueError):
        fmd.as_complex(np.zeros((3, 3), np.int16))
    n = C.c_uint64()
    assert lib.fmd_channelizer_outputs(None, C.byref(n)) == -1
    assert lib.fmd_channelizer_check(None) == -1
    assert lib.fmd_channelizer_reset(None) == -1
    lib.fmd_channelizer_free(None)


def test_code_object_has_the_channelizer_kernel_on_the_matrix_cores(code_objects):  # noqa: F811
    ks = {n: k for n, k in code_objects.items() if "fmd_channelizer" in n}
    assert ks, sorted(code_objects)[:5]
    for n, k in ks.items():
        assert any(i.startswith("v_mfma_i32_16x16x64_i8") for i in k["text"]), n
        assert any(i.startswith("global_load_lds_dwordx4") for i in k["text"]), n
        assert any(i.startswith("global_store_dwordx4") for i in k["text"]), n
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert not any(i.startswith("scratch_") for i in k["text"]), n
