"""FM receiver bank (include/fmd.h, fmd_receiver_*) without a GPU: the exported symbols, null arguments, the domain refusals (decided
before a device is queried) with the text of the bank whose rule fires, the capacities against the definition over a seeded sequence
of cuts, the test-side definition's own refusal rule and call-cut invariance (tests/receiver_ref.py), and the shipped code object."""
import ctypes as C
import re

import numpy as np
import pytest

import receiver_ref as rxr
import rds_ref as rr
import stations_ref as sr
from test_host_logic import header_functions
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

INVALID, U, NODEV = -1, -6, -8
ENTRY_POINTS = ["new", "free", "reset", "check", "run_device", "run_batch", "outputs", "pilot", "kernel_name"]


def _lib():
    import rtl_sdr_rs_amd as fmd
    return fmd, fmd.lib()


def test_every_receiver_symbol_is_declared_exported_and_bound():
    fmd, lib = _lib()
    names = [n for n in header_functions() if n.startswith("fmd_receiver_")]
    assert sorted(names) == sorted("fmd_receiver_" + e for e in ENTRY_POINTS)
    from rtl_sdr_rs_amd import _ffi
    for n in names:
        assert hasattr(lib, n) and n in _ffi.PROTOTYPES, n
    assert fmd.ReceiverBank._prefix == "receiver" and callable(fmd.receive_stations)
    assert C.sizeof(fmd.receiver.ReceiverConfig) == 28       # seven u32 fields, the header's order
    hdr = open(fmd._ffi.ROOT + "/include/fmd.h").read()
    fields = re.search(r"typedef struct fmd_receiver_config \{(.*?)\}", hdr, flags=re.S).group(1)
    assert re.findall(r"uint32_t (\w+);", fields) == [f[0] for f in fmd.receiver.ReceiverConfig._fields_]


def _new(lib, taps=None, decim=10, shift=4, incs=(0,), ga=(100,), gr=(100,), rate=2400000, block=4096, pmin=100, Ra=5, ashift=3, Rr=32,
         rshift=8, n_streams=1, null=()):
    """fmd_receiver_new's status (a handle it returned is freed); `null` names the pointers passed as NULL."""
    import rtl_sdr_rs_amd as fmd
    taps = np.ascontiguousarray(np.ones(8, np.int16) if taps is None else taps, dtype=np.int16)
    incs = np.ascontiguousarray(incs, dtype=np.uint32)
    ga, gr = np.ascontiguousarray(ga, dtype=np.int16), np.ascontiguousarray(gr, dtype=np.int16)
    cfg = fmd.receiver.ReceiverConfig(rate, block, pmin, Ra, ashift, Rr, rshift)
    h = C.c_void_p()
    dev = fmd.DeviceConfig(n_streams, 0, 0)
    p16, pu = C.POINTER(C.c_int16), C.POINTER(C.c_uint32)
    a = dict(taps=taps.ctypes.data_as(p16), incs=incs.ctypes.data_as(pu), ga=ga.ctypes.data_as(p16), gr=gr.ctypes.data_as(p16),
             cfg=C.byref(cfg), dev=C.byref(dev), out=C.byref(h))
    for n in null:
        a[n] = None
    rc = lib.fmd_receiver_new(a["taps"], taps.size, decim, shift, a["incs"], incs.size, a["ga"], ga.size, a["gr"], gr.size, a["cfg"],
                              a["dev"], a["out"])
    if rc == 0:
        lib.fmd_receiver_free(h)
    return rc


def test_null_arguments():
    _, lib = _lib()
    for n in ("taps", "incs", "ga", "gr", "cfg", "dev", "out"):
        assert _new(lib, null=(n,)) == INVALID, n
        assert "null" in lib.fmd_last_error().decode()
    assert _new(lib, n_streams=0) == INVALID
    a, r, p, lv, n = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint32(), C.c_size_t()
    buf = C.create_string_buffer(64)
    assert lib.fmd_receiver_outputs(None, C.byref(a), C.byref(r)) == INVALID
    assert lib.fmd_receiver_check(None) == INVALID and lib.fmd_receiver_reset(None) == INVALID
    assert lib.fmd_receiver_pilot(None, 0, 0, C.byref(p), C.byref(lv)) == INVALID
    assert lib.fmd_receiver_kernel_name(None, 0, buf, 64) == INVALID
    assert lib.fmd_receiver_run_batch(None, buf, 64, buf, 1, C.byref(n), buf, 1, C.byref(n)) == INVALID
    assert lib.fmd_receiver_run_device(None, buf, 64, buf, 1, C.byref(n), buf, 1, C.byref(n), None) == INVALID
    lib.fmd_receiver_free(None)


def _msg(lib):
    return lib.fmd_last_error().decode()


def test_domain_refusals_need_no_gpu_and_keep_the_banks_texts():
    fmd, lib = _lib()
    # the front end's
    assert _new(lib, decim=3) == U and "even 2 <= decim <= 64" in _msg(lib)
    assert _new(lib, taps=np.ones(257, np.int16)) == U
    assert _new(lib, taps=np.full(8, 2048, np.int16)) == U and "|tap| > 2047" in _msg(lib)
    assert _new(lib, shift=25) == U and _new(lib, incs=np.zeros(33)) == U and _new(lib, n_streams=65536) == U
    assert _new(lib, taps=np.full(64, 2047, np.int16), shift=0) == U and "filter gain too large" in _msg(lib)
    # the rate floor is the RDS bank's: 120000 decim, where the stereo bank's 106000 decim would have passed
    rate = 106000 * 10 + 5000
    assert _new(lib, rate=rate) == U and _msg(lib) == "need capture_rate >= 120000 * decim"
    scfg = fmd.stereo.StereoConfig(rate, 4096, 5, 3, 100)
    t, i, g = np.ones(8, np.int16), np.zeros(1, np.uint32), np.array([100], np.int16)
    h, dev = C.c_void_p(), fmd.DeviceConfig(1, 0, 0)
    p16 = C.POINTER(C.c_int16)
    rc = lib.fmd_stereo_new(t.ctypes.data_as(p16), 8, 10, 4, i.ctypes.data_as(C.POINTER(C.c_uint32)), 1, g.ctypes.data_as(p16), 1,
                            C.byref(scfg), C.byref(dev), C.byref(h))
    assert rc in (0, NODEV)                                  # the stereo bank's domain holds this rate
    if rc == 0:
        lib.fmd_stereo_free(h)
    assert _new(lib, rate=120000 * 10 - 1) == U and _new(lib, rate=120000 * 10) in (0, NODEV)
    for P in (512, 1000, 3000, 32768):
        assert _new(lib, block=P) == U and _msg(lib) == "block must be a power of two in [1024, 16384]", P
    # the audio stage's, in the stereo bank's words
    audio = "need 1 <= audio_decim <= 32, 1 <= n_audio_taps <= 256, audio_shift <= 16, pilot_min <= 16384"
    for kw in (dict(Ra=0), dict(Ra=33), dict(ga=np.ones(257, np.int16)), dict(ashift=17), dict(pmin=16385)):
        assert _new(lib, **kw) == U and _msg(lib) == audio, kw
    assert _new(lib, ga=np.array([16383, 1], np.int16)) == U and _msg(lib) == "sum |audio_taps| > 16383"
    assert _new(lib, ga=np.array([-8192, 8192], np.int16)) == U
    # the RDS stage's, in the RDS bank's words
    rds = "need 1 <= out_decim <= 32, 1 <= n_rds_taps <= 256, rds_shift <= 24, pilot_min <= 16384"
    for kw in (dict(Rr=0), dict(Rr=33), dict(gr=np.ones(257, np.int16), rshift=14), dict(rshift=25)):
        assert _new(lib, **kw) == U and _msg(lib) == rds, kw
    assert _new(lib, gr=np.array([16383, 1], np.int16), rshift=24) == U and _msg(lib) == "sum |rds_taps| > 16383"
    store = "rds_shift too small: need ceil(32768 * sum |rds_taps| / 2^rds_shift) <= 32767"
    assert _new(lib, gr=np.array([16383], np.int16), rshift=13) == U and _msg(lib) == store
    assert _new(lib, gr=np.array([100], np.int16), rshift=6) == U and _msg(lib) == store      # ceil(32768 * 100 / 64) = 51200
    # the same texts as the banks themselves give
    import test_rds
    assert test_rds._new(lib, g=np.array([100], np.int16), rshift=6) == U and _msg(lib) == store
    assert test_rds._new(lib, R=33) == U and _msg(lib) == rds
    # accepted corners: a device, or only then its absence
    for kw in (dict(),
               dict(decim=64, rate=120000 * 64, block=16384, pmin=16384, Ra=32, ga=np.full(256, 63, np.int16), ashift=16, Rr=32,
                    gr=np.full(256, 63, np.int16), rshift=24),
               dict(decim=2, rate=240000, block=1024, pmin=0, Ra=1, ga=np.array([16383], np.int16), ashift=0, Rr=1,
                    gr=np.array([16383], np.int16), rshift=14),
               dict(gr=np.array([100], np.int16), rshift=7)):
        assert _new(lib, **kw) in (0, NODEV), kw


def _ref(incs, Ta=127, Ra=5, Tr=255, Rr=16):
    """The definition at the issue case's shape; the library's domain holds these arguments."""
    fmd, lib = _lib()
    h = rr.front_taps()
    ga = fmd.stereo_taps(rr.FS // rr.D, Ra, Ta)
    gr, rs = fmd.rds_taps(rr.FS // rr.D, Rr, Tr)
    shift = fmd.stations_auto_shift(h, incs, limit=2048)
    assert _new(lib, taps=h, decim=rr.D, shift=shift, incs=incs, ga=ga, gr=gr, rate=rr.FS, block=1024, pmin=1, Ra=Ra, ashift=4, Rr=Rr,
                rshift=rs) in (0, NODEV)
    return rxr.ReceiverRef(h, rr.D, incs, shift, rr.FS, ga, Ra, 4, gr, Rr, rs, block=1024, pilot_min=1, z=sr.z_corr)


def _cuts(rng, total, lo, hi):
    """Seeded call lengths (multiples of 8) that sum to `total`."""
    cuts = []
    while sum(cuts) < total:
        cuts.append(min(8 * int(rng.integers(lo, hi)), total - sum(cuts)))
    return cuts


def test_out_caps_bound_every_call_of_a_seeded_sequence_of_cuts():
    """ReceiverBank.out_caps -- fmd_stereo_out_cap and fmd_rds_out_cap, no third function -- against the definition's counts: they
    bound the first call, a call behind any history, and refused calls' bytes resent with the next ones."""
    fmd, lib = _lib()
    for D, T, Ta, Ra, Tr, Rr, seed in ((2, 64, 127, 5, 255, 16, 1), (10, 33, 1, 1, 255, 32, 2), (64, 256, 256, 32, 1, 1, 3), (4, 7, 16, 3, 40, 7, 4)):
        rng = np.random.default_rng(seed)
        bank = object.__new__(fmd.ReceiverBank)             # out_caps needs no handle
        bank.decim, bank.audio_decim, bank.rds_decim = D, Ra, Rr
        pos = na = nr = 0
        out_a = lambda m: (m - Ta) // Ra + 1 if m >= Ta else 0      # noqa: E731
        out_r = lambda m: (m - Tr) // Rr + 1 if m >= Tr else 0      # noqa: E731
        mpx = lambda p: (p - T) // D + 1 if p >= T else 0            # noqa: E731
        pending = 0
        for n in _cuts(rng, 8 * 60000, 1, 4000):
            nbytes = pending + n
            ca, cr_ = bank.out_caps(nbytes)
            assert (ca, cr_) == (lib.fmd_stereo_out_cap(D, Ra, nbytes), lib.fmd_rds_out_cap(D, Rr, nbytes))
            m = mpx(pos + nbytes // 2)
            da, dr = out_a(m) - na, out_r(m) - nr
            assert 0 <= da <= ca and 0 <= dr <= cr_, (D, n, da, ca, dr, cr_)
            if min(da, dr) < 1:
                pending = nbytes                             # refused: resent with the next bytes
                continue
            pos, na, nr, pending = pos + nbytes // 2, na + da, nr + dr, 0
        assert na > 10 and nr > 10


def test_the_definition_refuses_and_keeps_state_when_either_stage_completes_nothing():
    rng = np.random.default_rng(21)
    incs = [sr.phase_inc(40000, rr.FS), 0]
    # audio R = 1 with one tap completes an output with every multiplex sample, the RDS stage one in 32
    fmd, _ = _lib()
    h = rr.front_taps()
    gr, rs = fmd.rds_taps(rr.FS // rr.D, 32, 255)
    _, lib = _lib()                                          # the library's domain holds these arguments
    sh = fmd.stations_auto_shift(h, incs, limit=2048)
    assert _new(lib, taps=h, decim=rr.D, shift=sh, incs=incs, ga=[16383], gr=gr, rate=rr.FS, block=1024, pmin=1, Ra=1, ashift=14, Rr=32,
                rshift=rs) in (0, NODEV)
    ref = rxr.ReceiverRef(h, rr.D, incs, sh, rr.FS, np.array([16383], np.int16), 1, 14, gr, 32, rs, block=1024, pilot_min=1, z=sr.z_corr)
    one = rxr.ReceiverRef(h, rr.D, incs, sh, rr.FS, np.array([16383], np.int16), 1, 14, gr, 32, rs, block=1024, pilot_min=1, z=sr.z_corr)
    iq = rng.integers(0, 256, 8 * 1200, dtype=np.uint8)
    whole = one.feed(iq)
    with pytest.raises(rxr.TooShort):                        # neither stage: fewer samples than the front end's taps
        ref.feed(iq[:8 * 4])
    a0 = ref.completes(8 * 100)
    assert a0[0] >= 1 and a0[1] == 0                         # audio outputs, but no RDS output yet
    with pytest.raises(rxr.TooShort):
        ref.feed(iq[:8 * 100])
    assert ref.outputs() == (0, 0) and ref.stereo.ch.pos == 0 and ref.rds.x[0].size == 0
    first = 8 * 400
    a, u = ref.feed(iq[:first])
    na, nr = ref.completes(8 * 4)
    assert na >= 1 and nr == 0                               # 16 samples, 8 multiplex samples: short of the next RDS output
    before = ref.outputs()
    with pytest.raises(rxr.TooShort):
        ref.feed(iq[first:first + 8 * 4])
    assert ref.outputs() == before
    a2, u2 = ref.feed(iq[first:])                            # the same bytes again, as the head of a longer call
    assert np.array_equal(np.concatenate([a, a2], axis=1), whole[0]) and np.array_equal(np.concatenate([u, u2], axis=1), whole[1])


def test_call_cut_invariance_of_the_definition():
    """One call against the same bytes cut at seeded 8-byte multiples, none of them refused: cuts inside a front-end window and
    inside both filter windows (every cut is, with 127 and 255 taps)."""
    rng = np.random.default_rng(12)
    incs = [sr.phase_inc(40000, rr.FS), 0]
    iq = rng.integers(0, 256, 8 * 2500, dtype=np.uint8)
    whole = _ref(incs).feed(iq)
    assert whole[0].shape[1] > 900 and whole[1].shape[1] > 250
    for seed in (1, 2, 3):
        part = _ref(incs)
        # the first call completes an output of each stage (64 + 2 * 254 = 572 samples: 8 * 143 B); later ones carry >= 16 multiplex
        # samples, one RDS output
        cuts = [8 * 150] + _cuts(np.random.default_rng(seed), iq.size - 8 * 150, 8, 500)
        pos, aa, uu = 0, [], []
        for n in cuts:
            assert min(part.completes(n)) >= 1, (seed, n)    # the set holds no refused call
            a, u = part.feed(iq[pos:pos + n])
            aa.append(a); uu.append(u)
            pos += n
            assert np.array_equal(np.concatenate(aa, axis=1), whole[0][:, :part.outputs()[0]]), (seed, n)
            assert np.array_equal(np.concatenate(uu, axis=1), whole[1][:, :part.outputs()[1]]), (seed, n)
        assert pos == iq.size and len(cuts) > 5 and part.outputs() == (whole[0].shape[1], whole[1].shape[1])
        assert part.pilot(0) == _pilot_of(whole, incs, iq)


def _pilot_of(whole, incs, iq):
    one = _ref(incs)
    one.feed(iq)
    return one.pilot(0)


def _lds_bytes(symbol_part):
    """group_segment_fixed_size of the library's kernels whose symbol holds `symbol_part`, from the code objects' metadata notes.
    (A kernel's entry lists its keys in alphabetical order, so this one comes before the entry's .name.)"""
    import os, shutil, subprocess, tempfile
    from test_isa_invariants import LIB, LLVM
    tmp = tempfile.mkdtemp(prefix="fmd_rx_")
    try:
        shutil.copy(LIB, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        found = []
        for co in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], cwd=tmp, check=True, capture_output=True, text=True).stdout
            for entry in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:       # one kernel each: .agpr_count is an entry's first key
                name = re.search(r"\n\s*\.name:\s*(\S+)", entry).group(1)
                if symbol_part in name:
                    found.append(int(re.search(r"\n\s*\.group_segment_fixed_size:\s*(\d+)", entry).group(1)))
        return found
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_code_object_has_one_multiplex_pass_and_the_fused_second_pass_within_its_limits(code_objects):  # noqa: F811
    assert sum("fmd_stereo_mpx_kernel" in n for n in code_objects) == 1      # pass 0 is shared, not forked
    fused = {n: k for n, k in code_objects.items() if "fmd_receiver_second_kernel" in n}
    assert len(fused) == 1, sorted(n for n in code_objects if "receiver" in n)
    assert sum("fmd_receiver" in n for n in code_objects) == 1               # no A/B form left in the shipped library
    for n, k in fused.items():
        m = k["meta"]
        lds = _lds_bytes("fmd_receiver_second_kernel")
        assert len(lds) == 1 and 16384 < lds[0] <= 20480, lds  # one pair buffer, not one per side: two workgroups per 40 KiB
        assert m["vgpr_count"] <= 64, m                      # 512 / 8 waves
        assert m.get("private_segment_fixed_size") == 0 and m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, m
        assert not any(i.startswith("scratch_") for i in k["text"]), n
        assert any(i.startswith("v_mad_i32_i24") for i in k["text"]), n
