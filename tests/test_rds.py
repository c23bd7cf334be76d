"""RDS bank (include/fmd.h, fmd_rds_*) and RDS decoder (fmd_rds_decoder_*) without a GPU: the arithmetic bounds of the definition at
the domain's corners, call-cut invariance of the test-side definition (tests/rds_ref.py), the domain refusals (decided before a
device is queried), the encoder against the block check, the host decoder on the definition's baseband of a synthesized station,
and the shipped code object."""
import ctypes as C

import numpy as np
import pytest

import rds_ref as rr
import stations_ref as sr
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

U, NODEV = -6, -8


def _lib():
    import rtl_sdr_rs_amd as fmd
    return fmd, fmd.lib()


def test_definition_bounds_at_the_domain_corners():
    th = np.arange(0, 1 << 32, 1 << 22, dtype=np.uint64)    # every table index
    qmax = 0
    for x in (32767, -32768):
        qr, qi = (x * sr.cosq(th)) >> 14, (-x * sr.sinq(th)) >> 14
        assert np.abs(x * sr.cosq(th)).max() <= 2 ** 29
        qmax = max(qmax, int(np.abs(qr).max()), int(np.abs(qi).max()))
    assert qmax == 32768 and qmax < 2 ** 23                  # |q| <= 32768: a 24-bit operand
    gsum = 16383                                             # the largest allowed sum |g|
    assert gsum < 2 ** 23 and 32768 * gsum < 2 ** 29         # |v| < 2^29
    # the smallest allowed rds_shift at the largest sum |g| (and at every other sum): both extremes of v fit int16 after the floor
    for gs in (16383, 16382, 8192, 8191, 4096, 1000, 3, 1):
        s = 0
        while -(-32768 * gs >> s) > 32767:
            s += 1
        assert s <= 24
        for v in (32768 * gs, -32768 * gs):
            assert -32768 <= v >> s <= 32767, (gs, s)
        if s:
            assert (32768 * gs) >> (s - 1) > 32767 or -(-32768 * gs >> (s - 1)) > 32767   # one less is refused for a reason
    assert rr_shift(16383) == 14
    # ... and the definition run on the extreme itself: g = [16383], x alternating between the int16 extremes
    fmd, _ = _lib()
    g = np.array([16383], np.int16)
    assert fmd.rds.rds_shift_for(g) == 14


def rr_shift(gs):
    s = 0
    while -(-32768 * gs >> s) > 32767:
        s += 1
    return s


def _ref(incs, T=64, Ta=255, R=16, seed=0, g=None):
    rng = np.random.default_rng(seed)
    import rtl_sdr_rs_amd as fmd
    h = rr.front_taps() if T == 64 else rng.integers(-2047, 2048, T).astype(np.int16)
    if g is None:
        g = rng.integers(-200, 201, Ta)
        g = (np.sign(g) * (np.abs(g) * 16383 // max(1, int(np.abs(g).sum())))).astype(np.int16)
    shift = fmd.stations_auto_shift(h, incs, limit=2048)
    return rr.RdsRef(h, rr.D, incs, shift, rr.FS, g, R, fmd.rds.rds_shift_for(g), block=1024, pilot_min=1, z=sr.z_corr)


def test_call_cut_invariance_of_the_definition():
    """One call against the same bytes cut at 8-byte multiples: cuts inside a front-end window, inside an RDS filter window (every
    cut is, with 255 taps), calls that complete nothing (refused, resent with the next bytes)."""
    rng = np.random.default_rng(11)
    incs = [sr.phase_inc(40000, rr.FS), 0]
    iq = rng.integers(0, 256, 8 * 2500, dtype=np.uint8)
    whole = _ref(incs).feed(iq)
    assert whole.shape[1] > 250
    part = _ref(incs)
    cuts = [8 * 75, 8 * 143, 8, 8 * 3, 8 * 600, 8 * 1, 8 * 777, 8 * 2, 8 * 898]      # 8 * 75 alone completes no output
    assert sum(cuts) == iq.size
    pieces, pos, pending, refused = [], 0, np.zeros(0, np.uint8), 0
    for n in cuts:
        buf = np.concatenate([pending, iq[pos:pos + n]])
        pos += n
        if part.completes(buf.size) < 1:
            with pytest.raises(rr.TooShort):
                part.feed(buf)
            pending, refused = buf, refused + 1
            continue
        pieces.append(part.feed(buf))
        pending = np.zeros(0, np.uint8)
    got = np.concatenate(pieces, axis=1)
    assert refused >= 1 and pending.size == 0
    assert np.array_equal(got, whole)
    assert part.q_max <= 32768 and part.v_max < 2 ** 29


def _new(lib, taps=None, decim=10, shift=4, incs=(0,), g=(100,), rate=2400000, block=4096, R=32, rshift=8, pmin=100, n_streams=1):
    import rtl_sdr_rs_amd as fmd
    taps = np.ascontiguousarray(np.ones(8, np.int16) if taps is None else taps, dtype=np.int16)
    incs = np.ascontiguousarray(incs, dtype=np.uint32)
    g = np.ascontiguousarray(g, dtype=np.int16)
    cfg = fmd.rds.RdsConfig(rate, block, R, rshift, pmin)
    h = C.c_void_p()
    dev = fmd.DeviceConfig(n_streams, 0, 0)
    rc = lib.fmd_rds_new(taps.ctypes.data_as(C.POINTER(C.c_int16)), taps.size, decim, shift, incs.ctypes.data_as(C.POINTER(C.c_uint32)),
                         incs.size, g.ctypes.data_as(C.POINTER(C.c_int16)), g.size, C.byref(cfg), C.byref(dev), C.byref(h))
    if rc == 0:
        lib.fmd_rds_free(h)
    return rc


def test_domain_refusals_need_no_gpu():
    _, lib = _lib()
    assert _new(lib, decim=3) == U
    assert _new(lib, decim=66, rate=120000 * 66) == U
    assert _new(lib, taps=np.ones(257, np.int16)) == U
    assert _new(lib, taps=np.full(8, 2048, np.int16)) == U
    assert _new(lib, shift=25) == U
    assert _new(lib, incs=np.zeros(33)) == U
    assert _new(lib, taps=np.full(64, 2047, np.int16), shift=0) == U          # |y| bound
    assert _new(lib, rate=120000 * 10 - 1) == U                              # capture_rate < 120000 decim
    assert "120000" in lib.fmd_last_error().decode()
    for P in (512, 1000, 3000, 32768):
        assert _new(lib, block=P) == U, P
    assert _new(lib, R=0) == U and _new(lib, R=33) == U
    msg = lib.fmd_last_error().decode()                      # this bank's own names and limits, not the stereo bank's
    assert "out_decim <= 32" in msg and "rds_shift <= 24" in msg, msg
    assert _new(lib, g=np.ones(257, np.int16), rshift=14) == U
    assert _new(lib, g=np.array([16383, 1], np.int16), rshift=24) == U       # sum |g| > 16383
    assert _new(lib, g=np.array([-8192, 8192], np.int16), rshift=24) == U
    assert _new(lib, rshift=25) == U
    assert _new(lib, g=np.array([16383], np.int16), rshift=13) == U          # the int16 store would not be exact
    assert _new(lib, g=np.array([100], np.int16), rshift=6) == U             # ceil(32768 * 100 / 64) = 51200
    assert _new(lib, pmin=16385) == U
    assert _new(lib, n_streams=65536) == U
    assert _new(lib, n_streams=0) == -1
    for kw in (dict(), dict(decim=64, rate=120000 * 64, block=16384, R=32, g=np.full(256, 63, np.int16), rshift=24, pmin=16384),
               dict(decim=2, rate=240000, block=1024, R=1, g=np.array([16383], np.int16), rshift=14, pmin=0),
               dict(g=np.array([-8191, 8192], np.int16), rshift=14), dict(g=np.array([100], np.int16), rshift=7)):
        assert _new(lib, **kw) in (0, NODEV), kw
    assert lib.fmd_rds_out_cap(10, 32, 262144) == -(-262144 // 640) and lib.fmd_rds_out_cap(0, 32, 64) == 0
    n, p, lv = C.c_uint64(), C.c_int(), C.c_uint32()
    assert lib.fmd_rds_outputs(None, C.byref(n)) == -1 and lib.fmd_rds_check(None) == -1 and lib.fmd_rds_reset(None) == -1
    assert lib.fmd_rds_pilot(None, 0, 0, C.byref(p), C.byref(lv)) == -1
    lib.fmd_rds_free(None)
    d = C.c_void_p()
    for num, den in ((3999, 1), (32001, 1), (256000, 65)):
        assert lib.fmd_rds_decoder_new(num, den, C.byref(d)) == U
    assert lib.fmd_rds_decoder_new(8000, 0, C.byref(d)) == -1


def test_rds_taps_meet_the_rule():
    fmd, _ = _lib()
    for fs, n in ((128000, 255), (240000, 255), (120000, 1), (170000, 256), (480000, 64)):
        g, s = fmd.rds_taps(fs, 16, n)
        total = int(np.abs(g.astype(np.int64)).sum())
        assert g.dtype == np.int16 and g.size == n and 0 < total <= 16383 and int(g.astype(np.int64).sum()) > 0
        assert s <= 24 and -(-32768 * total >> s) <= 32767 and (s == 0 or -(-32768 * total >> (s - 1)) > 32767)


def test_encoder_and_block_check_are_self_consistent():
    """Every encoded block leaves, divided by the generator, its own offset word and no other."""
    rng = np.random.default_rng(3)
    assert rr.POLY == sum(1 << i for i in (10, 8, 7, 5, 4, 3, 0))
    infos = [0, 0xFFFF, rr.PI, 0x2003] + [int(v) for v in rng.integers(0, 1 << 16, 200)]
    for info in infos:
        for name, word in rr.OFFSETS.items():
            blk = rr.encode_block(info, name)
            assert blk >> 10 == info and blk < 1 << 26
            syn = rr.remainder(blk, 26)
            assert syn == word and [n for n, w in rr.OFFSETS.items() if w == syn] == [name]
    bits = rr.group_bits(rr.groups_0a_2a(rr.PI, rr.PS, rr.RT))
    assert bits.size == 8 * 104
    e = rr.differential(bits)
    assert np.array_equal(e[1:] ^ e[:-1], bits[1:]) and e[0] == bits[0]


@pytest.fixture(scope="module")
def baseband():
    """The definition's baseband (int16 [n, 2]) of 0.7 s of the test station: capture_rate 256000, D = 2, R = 16 (8 kHz), 64 + 255
    taps, pilot at 19002 Hz (about +6 Hz left at 57 kHz)."""
    fmd, _ = _lib()
    iq, groups = rr.station_capture(0.7)
    h = rr.front_taps()
    incs = [sr.phase_inc(40000, rr.FS)]
    g, rs = fmd.rds_taps(rr.FS // rr.D, rr.R, rr.T_RDS)
    ref = rr.RdsRef(h, rr.D, incs, fmd.stations_auto_shift(h, incs, limit=256), rr.FS, g, rr.R, rs, z=sr.z_corr)
    u = ref.feed(iq)[0]
    assert g.size == 255 and h.size == 64 and iq.size == 2 * 179200
    return np.ascontiguousarray(u.astype(np.int16)), groups


def _decode(fmd, u, pieces=None):
    dec = fmd.RdsDecoder(rr.FS, rr.D * rr.R)
    groups, pos = [], 0
    for n in pieces or [u.shape[0]]:
        groups += dec.push(u[pos:pos + n])
        pos += n
    assert pos == u.shape[0]
    return groups, dec.info()


def test_decoder_reads_pi_ps_and_radiotext_from_0_7_s(baseband):
    fmd, _ = _lib()
    u, sent = baseband
    groups, info = _decode(fmd, u)
    print("groups %d, info %r" % (len(groups), info))
    assert info["pi"] == rr.PI
    assert info["ps"] == rr.PS
    assert len(rr.RT) == 16 and info["rt"] == rr.RT
    assert info["synced"] and info["blocks_bad"] == 0
    spg = 104 * rr.FS / (rr.D * rr.R) / (rr.PILOT_HZ / 16)   # samples per group
    assert groups and groups[0]["first_sample"] < 3 * spg     # lock within the first 3 groups
    assert all(g["ok_mask"] == 15 for g in groups[1:]) and info["groups_ok"] >= len(groups) - 1
    # every delivered group is one that was sent, in the order sent
    first = sent.index(groups[1]["blocks"]) - 1
    for i, g in enumerate(groups[1:], 1):
        assert g["blocks"] == sent[(first + i) % len(sent)], i
    assert [b for b, ok in zip(groups[0]["blocks"], range(4)) if groups[0]["ok_mask"] >> ok & 1] == \
           [b for b, ok in zip(sent[first % len(sent)], range(4)) if groups[0]["ok_mask"] >> ok & 1]


def test_decoder_does_not_depend_on_how_the_baseband_is_pushed(baseband):
    fmd, _ = _lib()
    u, _ = baseband
    rng = np.random.default_rng(5)
    whole = _decode(fmd, u)
    pieces = [1, 2, 3, 0, 701]
    while sum(pieces) < u.shape[0]:
        pieces.append(min(int(rng.integers(1, 900)), u.shape[0] - sum(pieces)))
    assert _decode(fmd, u, pieces) == whole


def test_python_decoder_is_the_c_abi_decoder(baseband):
    fmd, lib = _lib()
    u, _ = baseband
    groups, info = _decode(fmd, u)
    d = C.c_void_p()
    assert lib.fmd_rds_decoder_new(rr.FS, rr.D * rr.R, C.byref(d)) == 0
    buf, n = (fmd.rds.RdsGroup * 4)(), C.c_size_t()
    got = []
    assert lib.fmd_rds_decoder_push(d, u.ctypes.data, u.shape[0], buf, 4, C.byref(n)) == 0
    while n.value:                                           # a small buffer: the rest stays queued
        got += [(tuple(buf[i].block), buf[i].ok_mask, buf[i].first_sample) for i in range(n.value)]
        assert lib.fmd_rds_decoder_push(d, None, 0, buf, 4, C.byref(n)) == 0
    assert got == [(g["blocks"], g["ok_mask"], g["first_sample"]) for g in groups] and len(got) > 4
    i = fmd.rds.RdsInfo()
    assert lib.fmd_rds_decoder_info(d, C.byref(i)) == 0
    assert (i.pi, i.ps.decode(), i.rt.decode(), i.groups_ok, i.blocks_bad, bool(i.synced)) == \
           (info["pi"], info["ps"], info["rt"], info["groups_ok"], info["blocks_bad"], info["synced"])
    assert lib.fmd_rds_decoder_reset(d) == 0
    assert lib.fmd_rds_decoder_info(d, C.byref(i)) == 0 and (i.pi, i.ps.decode(), i.rt.decode(), i.synced) == (0, " " * 8, "", 0)
    lib.fmd_rds_decoder_free(d)


def test_decoder_finds_nothing_in_noise():
    fmd, _ = _lib()
    rng = np.random.default_rng(9)
    u = rng.integers(-200, 201, (8000, 2)).astype(np.int16)
    groups, info = _decode(fmd, u)
    assert not groups and not info["synced"] and info["pi"] == 0 and info["groups_ok"] == 0


def test_code_object_has_the_baseband_pass_without_scratch(code_objects):  # noqa: F811
    bb = {n: k for n, k in code_objects.items() if "fmd_rds_baseband_kernel" in n}
    assert len(bb) == 1, sorted(code_objects)[:5]
    assert sum("fmd_stereo_mpx_kernel" in n for n in code_objects) == 1      # pass 0 is shared, not forked
    for n, k in bb.items():
        assert any(i.startswith("v_mad_i32_i24") for i in k["text"]), n
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert not any(i.startswith("scratch_") for i in k["text"]), n
