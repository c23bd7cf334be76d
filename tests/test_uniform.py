"""Uniform channelizer (include/fmd.h, fmd_uniform_*) without a GPU: the integer helpers of the C ABI against the formulas, the
domain refusals (decided before a device is queried), the Python helpers, that the definition (tests/uniform_ref.py) separates
the channels of a band plan, and the shipped code object."""
import ctypes as C

import numpy as np
import pytest

import stations_ref as sr
import uniform_ref as ur
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

U, INV = -6, -1


def _lib():
    import rtl_sdr_rs_amd as fmd
    return fmd, fmd.lib()


def test_channel_inc_is_the_formula_and_the_scanner_bin_inc():
    fmd, lib = _lib()
    inc, inc2 = C.c_uint32(), C.c_uint32()
    for N in range(2, 257):
        for k in range(N):
            assert lib.fmd_uniform_channel_inc(k, N, C.byref(inc)) == 0
            want = ((k * (1 << 33) // N + 1) // 2) % (1 << 32)
            assert inc.value == want == ur.channel_inc(k, N), (k, N)
            assert abs(inc.value - k * (1 << 32) / N) <= 0.5
            if N in (16, 32, 64, 128, 256):
                assert lib.fmd_spectrum_bin_inc(k, N, C.byref(inc2)) == 0 and inc2.value == inc.value, (k, N)
        assert lib.fmd_uniform_channel_inc(N, N, C.byref(inc)) == U
    assert fmd.uniform_channel_inc(37, 96) == ur.channel_inc(37, 96)
    for k, N in ((0, 1), (0, 0), (0, 257), (300, 256)):
        assert lib.fmd_uniform_channel_inc(k, N, C.byref(inc)) == U, (k, N)
    assert lib.fmd_uniform_channel_inc(0, 16, None) == INV


def test_out_cap():
    _, lib = _lib()
    assert lib.fmd_uniform_out_cap(0, 4096) == 0
    assert lib.fmd_uniform_out_cap(8, 262144) == 16384 and lib.fmd_uniform_out_cap(256, 262144) == 512
    assert lib.fmd_uniform_out_cap(48, 96 * 7) == 7 and lib.fmd_uniform_out_cap(48, 96 * 7 - 16) == 6 and lib.fmd_uniform_out_cap(48, 0) == 0
    rng = np.random.default_rng(1)
    for _ in range(200):
        hop, nbytes = 8 * int(rng.integers(1, 33)), int(rng.integers(0, 1 << 20))
        assert lib.fmd_uniform_out_cap(hop, nbytes) == nbytes // (2 * hop)


def _new(lib, taps, N, hop, shift, channels=None, n_sel=None, n_streams=1, dev=True, out=True):
    """fmd_uniform_new with a device config that is never opened: the device it names does not exist, so a shape inside the domain
    ends in FMD_ERR_NO_DEVICE and one outside it in its refusal, which comes first."""
    import rtl_sdr_rs_amd as fmd
    h = C.c_void_p()
    cfg = fmd.DeviceConfig(n_streams, 1 << 20, 0)
    tp = None if taps is None else np.ascontiguousarray(taps, np.int16).ctypes.data_as(C.POINTER(C.c_int16))
    sel = None if channels is None else np.ascontiguousarray(channels, np.uint32)
    sp = None if sel is None else sel.ctypes.data_as(C.POINTER(C.c_uint32))
    ns = (0 if sel is None else sel.size) if n_sel is None else n_sel
    rc = lib.fmd_uniform_new(tp, 0 if taps is None else len(taps), N, hop, shift, sp, ns, C.byref(cfg) if dev else None,
                             C.byref(h) if out else None)
    if rc == 0:
        lib.fmd_uniform_free(h)
    return rc


INSIDE = (-8,)                  # FMD_ERR_NO_DEVICE: the arguments passed every domain check


def test_domain_edges_both_sides():
    _, lib = _lib()
    h = np.full(64, 100, np.int16)
    s = ur.min_shift(h, ur.channel_incs(16))
    for N, ok in ((1, False), (2, True), (256, True), (257, False)):
        assert (_new(lib, h, N, 8, 24) in INSIDE) == ok and (ok or _new(lib, h, N, 8, 24) == U), N
    for hop, ok in ((0, False), (8, True), (12, False), (256, True), (264, False), (4, False)):
        assert (_new(lib, h, 16, hop, 24) in INSIDE) == ok and (ok or _new(lib, h, 16, hop, 24) == U), hop
    assert _new(lib, np.zeros(0, np.int16), 16, 8, 24) == U                    # T = 0
    assert _new(lib, np.ones(1, np.int16), 16, 8, 24) in INSIDE                # T = 1
    assert _new(lib, np.ones(2048, np.int16), 16, 8, 24) in INSIDE             # T = 2048
    assert _new(lib, np.ones(2049, np.int16), 16, 8, 24) == U
    for v, ok in ((2047, True), (-2047, True), (2048, False), (-2048, False)):
        g = h.copy()
        g[7] = v
        assert (_new(lib, g, 16, 8, 24) in INSIDE) == ok and (ok or _new(lib, g, 16, 8, 24) == U), v
    assert _new(lib, h, 16, 8, 24) in INSIDE and _new(lib, h, 16, 8, 25) == U
    assert _new(lib, h, 16, 8, s, n_streams=65535) in INSIDE and _new(lib, h, 16, 8, s, n_streams=65536) == U


@pytest.mark.parametrize("N,hop,T,amp,sel", [(16, 8, 64, 2047, None), (96, 48, 768, 2047, None), (12, 8, 72, 127, [0, 5, 11]),
                                             (4, 64, 2048, 2047, None), (4, 64, 2048, 2047, [1])])
def test_the_16384_rule_at_the_smallest_shift_and_one_below(N, hop, T, amp, sel):
    _, lib = _lib()
    h = np.full(T, amp, np.int16) if N == 4 else np.random.default_rng(T).integers(-amp, amp + 1, T).astype(np.int16)
    incs = ur.channel_incs(N, sel)
    s = ur.min_shift(h, incs)
    assert 0 < s <= 24 and -(-256 * sr.max_gain(h, incs) >> s) <= 16384 < -(-256 * sr.max_gain(h, incs) >> (s - 1))
    assert _new(lib, h, N, hop, s, channels=sel) in INSIDE
    assert _new(lib, h, N, hop, s - 1, channels=sel) == U


def test_selection_refusals_and_nulls():
    _, lib = _lib()
    h = np.full(64, 100, np.int16)
    assert _new(lib, h, 16, 8, 24, channels=[0, 3, 15]) in INSIDE
    assert _new(lib, h, 16, 8, 24, channels=list(range(16))) in INSIDE
    assert _new(lib, h, 16, 8, 24, channels=[3, 1]) == U                       # unsorted
    assert _new(lib, h, 16, 8, 24, channels=[1, 1]) == U                       # duplicated
    assert _new(lib, h, 16, 8, 24, channels=[0, 16]) == U                      # >= N
    assert _new(lib, h, 16, 8, 24, channels=[0, 1], n_sel=0) == U              # n_selected 0
    assert _new(lib, h, 16, 8, 24, channels=list(range(17)), n_sel=17) == U    # n_selected > N
    assert _new(lib, h, 16, 8, 24, channels=None, n_sel=0) in INSIDE           # NULL: all N
    assert _new(lib, None, 16, 8, 24) == INV
    assert _new(lib, h, 16, 8, 24, dev=False) == INV
    assert _new(lib, h, 16, 8, 24, out=False) == INV
    assert _new(lib, h, 16, 8, 24, n_streams=0) == INV
    buf = np.zeros(64, np.uint8)
    n = C.c_size_t()
    assert lib.fmd_uniform_run_batch(None, buf.ctypes.data, 64, buf.ctypes.data, 1, C.byref(n)) == INV
    assert lib.fmd_uniform_run_device(None, buf.ctypes.data, 64, buf.ctypes.data, 1, C.byref(n), None) == INV
    assert lib.fmd_uniform_check(None) == INV and lib.fmd_uniform_reset(None) == INV
    assert lib.fmd_uniform_outputs(None, None) == INV and lib.fmd_uniform_tap_digits(None) == INV
    assert lib.fmd_uniform_kernel_name(None, None, 0) == INV
    lib.fmd_uniform_free(None)


def test_uniform_taps_is_the_formula_and_respects_the_amplitude():
    fmd, _ = _lib()
    for N, P, A in ((16, 8, 2047), (96, 8, 2047), (12, 6, 127), (128, 8, 1000), (256, 8, 2047), (5, 3, 1)):
        h = fmd.uniform_taps(N, P, A)
        T = N * P
        t = np.arange(T)
        s = np.sinc((t - (T - 1) / 2) / N) * np.hamming(T)
        assert h.dtype == np.int16 and h.size == T
        assert np.array_equal(h, np.floor(A * s / np.abs(s).max() + 0.5).astype(np.int16)) and np.array_equal(h, ur.taps(N, P, A))
        assert np.abs(h).max() == A
    assert np.array_equal(fmd.uniform_taps(16, 8), fmd.uniform_taps(16, 8, 2047))
    for bad in (0, 2048):
        with pytest.raises(ValueError):
            fmd.uniform_taps(16, 8, bad)
    offs = fmd.uniform_channel_offsets(2400000, 96)
    assert offs[0] == 0 and offs[1] == 25000 and offs[47] == 47 * 25000 and offs[48] == -48 * 25000 and offs[95] == -25000


def test_auto_shift_is_the_smallest_admissible():
    fmd, _ = _lib()
    for N, P, sel in ((16, 8, None), (96, 8, None), (12, 6, [0, 5, 11]), (256, 8, [0, 1, 127, 128, 255])):
        h = fmd.uniform_taps(N, P)
        incs = [fmd.uniform_channel_inc(k, N) for k in (range(N) if sel is None else sel)]
        s = fmd.uniform_auto_shift(h, N, sel)
        g = sr.max_gain(h, incs)
        assert s == ur.min_shift(h, incs) and -(-256 * g >> s) <= 16384 and (s == 0 or -(-256 * g >> (s - 1)) > 16384)


# channel k0 over the largest other channel, mean power in dB: measured on the definition with uniform_taps; the
# assertion sits 3 dB below, which covers the seed-to-seed spread of a 400-output estimate
SEPARATION = {(16, 8, 8, 5): 42.7, (96, 48, 8, 37): 49.8, (128, 64, 8, 100): 51.1, (12, 8, 6, 7): 41.9}


def separation(N, hop, P, k0, seed=0):
    """A tone at the centre of channel k0 (amplitude 50 of 127, noise sigma 1) through the definition, 400 outputs of all channels:
    (dB of channel k0 over the largest other channel, y of channel k0)."""
    h = ur.taps(N, P)
    T, M = h.size, 400
    n = T + hop * (M - 1)
    rng = np.random.default_rng(seed)
    x = 50.0 * np.exp(2j * np.pi * k0 * np.arange(n) / N) + rng.normal(0, 1.0, n) + 1j * rng.normal(0, 1.0, n)
    iq = np.empty(2 * n, np.uint8)
    iq[0::2] = np.clip(np.round(x.real + 127), 0, 255)
    iq[1::2] = np.clip(np.round(x.imag + 127), 0, 255)
    pad = (-iq.size) % (2 * hop)
    iq = np.concatenate([iq, np.full(pad, 127, np.uint8)])
    incs = ur.channel_incs(N)
    y = ur.UniformRef(h, N, hop, ur.min_shift(h, incs)).feed(iq)[:, :M]
    yc = y[..., 0].astype(np.float64) + 1j * y[..., 1].astype(np.float64)
    p = (np.abs(yc) ** 2).mean(axis=1)
    others = np.delete(p, k0)
    return 10 * np.log10(p[k0] / others.max()), yc[k0]


@pytest.mark.parametrize("N,hop,P,k0", sorted(SEPARATION))
def test_the_definition_separates_the_channels(N, hop, P, k0):
    db, y = separation(N, hop, P, k0)
    print("N %d hop %d P %d k0 %d: %.1f dB" % (N, hop, P, k0, db))
    assert db >= SEPARATION[(N, hop, P, k0)] - 3.0, db
    rms = np.sqrt((np.abs(y) ** 2).mean())
    assert abs(np.abs(y.mean()) - rms) <= 0.02 * rms           # the tone lands at DC of its channel


def test_code_object_kernels_have_no_scratch_and_no_spills(code_objects):  # noqa: F811
    ks = {n: k for n, k in code_objects.items() if "fmd_uv::" in n}
    assert len(ks) == 6, sorted(ks)                              # R in {1, 2, 4} row tiles per batch x G in {4, 8} column groups
    for n, k in ks.items():
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
