"""Band-plan bank (include/fmd.h, fmd_bandplan_*) without a GPU: the two statements of the definition agree, the domain refusals
(decided before a device is queried), fmd_bandplan_out_cap, the Python helpers, the shipped code object, and that the definition
(tests/bandplan_ref.py) does the job: squelched AM, NFM and SSB audio out of a band plan."""
import ctypes as C
import re

import numpy as np
import pytest

import bandplan_ref as br
import narrow_ref as nr
import stations_ref as sr
import uniform_ref as ur
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

U, INV, NO_DEVICE = -6, -1, -8


def _lib():
    import rtl_sdr_rs_amd as fmd
    return fmd, fmd.lib()


# ---- the definition ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [br.IQ, br.FM, br.AM, br.SSB])
def test_the_two_statements_of_the_definition_agree(mode):
    """BandPlanRef (vectorised, fed in calls that cut blocks and windows) against narrow_ref.direct over the whole y of each row."""
    rng = np.random.default_rng(40 + mode)
    N, hop, T, sel = 12, 8, 72, [1, 5, 6, 11]
    R, Ta, P = 3, 7, 16
    h = rng.integers(-2047, 2048, T).astype(np.int64)
    gr = rng.integers(-3000, 3001, Ta)
    gi = rng.integers(-3000, 3001, Ta) if mode in (br.IQ, br.SSB) else None
    shift = ur.min_shift(h, ur.channel_incs(N, sel))
    cs = br.min_chan_shift(h, N, shift, gr, gi, sel)
    yref = ur.UniformRef(h, N, hop, shift, channels=sel)
    data = rng.integers(0, 256, 2 * hop * 260, dtype=np.uint8)
    y = yref.feed(data)
    # a squelch at the median block RMS of an always-open run, so that blocks fall on both sides of it
    probe = br.BandPlanRef(h, N, hop, shift, gr, gi, mode, R, cs, P, 0, 700, channels=sel)
    probe.feed(data)
    sq = int(np.median([np.sqrt(probe.block(i, j)[0] / P) for i in range(len(sel)) for j in range(probe.n_next // P)]))
    assert 0 < sq <= 23170
    ref = br.BandPlanRef(h, N, hop, shift, gr, gi, mode, R, cs, P, sq, 700, channels=sel)
    parts, at, pending, refused = [], 0, np.zeros(0, np.uint8), 0
    for hops in (T // hop + 3, 1, 37, 2, 1, 260 - (T // hop + 3) - 41):
        pending = np.concatenate([pending, data[2 * hop * at:2 * hop * (at + hops)]])
        at += hops
        try:
            parts.append(ref.feed(pending))
            pending = pending[:0]
        except br.TooShort:                                    # a refused call changes nothing, stage one included: the same
            refused += 1                                       # bytes come again in front of the next ones
    assert at == 260 and pending.size == 0 and refused >= 1
    got = np.concatenate(parts, axis=1)
    assert got.shape[1] == (y.shape[1] - Ta) // R + 1 > 4 * P
    for i in range(len(sel)):
        want = nr.direct(y[i].tolist(), gr.tolist(), None if gi is None else gi.tolist(), mode, R, cs, P, sq, 700)
        assert got[i].tolist() == [list(w) for w in want] if mode == br.IQ else got[i].tolist() == want, (mode, i)
    assert np.abs(got).max() > 0 and (got == 0).any()              # the squelch both opened and closed


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------

def test_out_cap():
    _, lib = _lib()
    assert lib.fmd_bandplan_out_cap(0, 4, 4096) == 0 and lib.fmd_bandplan_out_cap(48, 0, 4096) == 0
    assert lib.fmd_bandplan_out_cap(48, 4, 262144) == 683 and lib.fmd_bandplan_out_cap(64, 2, 262144) == 1024
    assert lib.fmd_bandplan_out_cap(8, 1, 16) == 1 and lib.fmd_bandplan_out_cap(8, 8, 16) == 1 and lib.fmd_bandplan_out_cap(8, 8, 0) == 0
    rng = np.random.default_rng(2)
    for _ in range(200):
        hop, R, nbytes = 8 * int(rng.integers(1, 33)), int(rng.integers(1, 9)), int(rng.integers(0, 1 << 20))
        assert lib.fmd_bandplan_out_cap(hop, R, nbytes) == br.out_cap(hop, R, nbytes) == -(-nbytes // (2 * hop * R))


H = np.full(64, 100, np.int16)
G = np.full(8, 100, np.int16)


def _new(lib, taps=H, N=16, hop=8, shift=24, channels=None, n_sel=None, gr=G, gi=None, n_chan=None, mode=1, R=2, chan_shift=30,
         block=256, squelch=0, gain=256, n_streams=1, cfg=True, dev=True, out=True):
    """fmd_bandplan_new with a device config that is never opened: the device it names does not exist, so arguments inside the
    domain end in FMD_ERR_NO_DEVICE and arguments outside it in their refusal, which comes first."""
    import rtl_sdr_rs_amd as fmd
    from rtl_sdr_rs_amd.narrow import NarrowConfig
    h = C.c_void_p()
    dc = fmd.DeviceConfig(n_streams, 1 << 20, 0)
    p16 = C.POINTER(C.c_int16)
    tp = None if taps is None else np.ascontiguousarray(taps, np.int16).ctypes.data_as(p16)
    sel = None if channels is None else np.ascontiguousarray(channels, np.uint32)
    sp = None if sel is None else sel.ctypes.data_as(C.POINTER(C.c_uint32))
    ns = (0 if sel is None else sel.size) if n_sel is None else n_sel
    gra = None if gr is None else np.ascontiguousarray(gr, np.int16)
    gia = None if gi is None else np.ascontiguousarray(gi, np.int16)
    nc = NarrowConfig(mode, R, chan_shift, block, squelch, gain)
    rc = lib.fmd_bandplan_new(tp, 0 if taps is None else len(taps), N, hop, shift, sp, ns, None if gra is None else gra.ctypes.data_as(p16),
                              None if gia is None else gia.ctypes.data_as(p16), (0 if gra is None else gra.size) if n_chan is None else n_chan,
                              C.byref(nc) if cfg else None, C.byref(dc) if dev else None, C.byref(h) if out else None)
    if rc == 0:
        lib.fmd_bandplan_free(h)
    return rc


def _edge(lib, ok, **kw):
    rc = _new(lib, **kw)
    assert rc == (NO_DEVICE if ok else U), (kw, rc)


def test_stage_one_domain_edges_both_sides():
    _, lib = _lib()
    for N, ok in ((1, False), (2, True), (256, True), (257, False)):
        _edge(lib, ok, N=N)
    for hop, ok in ((0, False), (8, True), (12, False), (256, True), (264, False), (4, False)):
        _edge(lib, ok, hop=hop)
    _edge(lib, False, taps=np.zeros(0, np.int16))
    _edge(lib, True, taps=np.ones(2048, np.int16))
    _edge(lib, False, taps=np.ones(2049, np.int16))
    for v, ok in ((2047, True), (-2047, True), (2048, False), (-2048, False)):
        g = H.copy()
        g[7] = v
        _edge(lib, ok, taps=g)
    _edge(lib, True, shift=24)
    _edge(lib, False, shift=25)
    _edge(lib, True, n_streams=65535)
    _edge(lib, False, n_streams=65536)
    _edge(lib, True, channels=[0, 3, 15])
    for bad in ([3, 1], [1, 1], [0, 16]):
        _edge(lib, False, channels=bad)
    _edge(lib, False, channels=[0, 1], n_sel=0)
    _edge(lib, False, channels=list(range(17)), n_sel=17)
    # the 16384 rule of stage one at the smallest shift and one below, over the SELECTED channels
    h = np.random.default_rng(3).integers(-2047, 2048, 72).astype(np.int16)
    for sel in (None, [0, 5, 11]):
        s = ur.min_shift(h, ur.channel_incs(12, sel))
        assert s > 0
        _edge(lib, True, taps=h, N=12, shift=s, channels=sel)
        _edge(lib, False, taps=h, N=12, shift=s - 1, channels=sel)


def test_stage_two_domain_edges_both_sides():
    _, lib = _lib()
    for R, ok in ((0, False), (1, True), (8, True), (9, False), (32, False)):
        _edge(lib, ok, R=R)
    _edge(lib, False, R=9)
    msg = lib.fmd_last_error().decode()                          # this bank's own limits, not the narrow-band bank's
    assert "chan_decim <= 8" in msg and "n_chan_taps <= 64" in msg, msg
    for Ta, ok in ((1, True), (64, True), (65, False), (256, False)):
        _edge(lib, ok, gr=np.full(Ta, 10, np.int16))
    _edge(lib, False, n_chan=0)
    for mode, ok in ((0, True), (3, True), (4, False)):
        _edge(lib, ok, mode=mode)
    for cs, ok in ((30, True), (31, False)):
        _edge(lib, ok, chan_shift=cs)
    for P, ok in ((8, False), (16, True), (4096, True), (8192, False), (48, False)):
        _edge(lib, ok, block=P)
    for q, ok in ((23170, True), (23171, False)):
        _edge(lib, ok, squelch=q)
    for g, ok in ((0, False), (1, True), (65535, True), (65536, False)):
        _edge(lib, ok, gain=g)
    for v, ok in ((16383, True), (-16383, True), (16384, False), (-16384, False)):
        g = G.copy()
        g[3] = v
        _edge(lib, ok, gr=g)
        _edge(lib, ok, gi=g)
    # sum |gr| + |gi| <= 65535
    _edge(lib, True, gr=np.array([16383, 16383, 16383, 16383, 3], np.int16))
    _edge(lib, False, gr=np.array([16383, 16383, 16383, 16383, 4], np.int16))
    _edge(lib, False, gr=np.array([16383, 16383, 2], np.int16), gi=np.array([16383, 16383, 2], np.int16))


@pytest.mark.parametrize("sel", [None, [0, 5, 11]])
def test_the_stage_two_gain_rule_at_the_smallest_chan_shift_and_one_below(sel):
    """ceil(B_y sum(|gr| + |gi|) / 2^chan_shift) <= 16384 with B_y the uniform channelizer's bound over the selected channels."""
    _, lib = _lib()
    rng = np.random.default_rng(4)
    h = rng.integers(-2047, 2048, 72).astype(np.int16)
    gr, gi = rng.integers(-900, 901, 33).astype(np.int16), rng.integers(-900, 901, 33).astype(np.int16)
    s = ur.min_shift(h, ur.channel_incs(12, sel))
    cs = br.min_chan_shift(h, 12, s, gr, gi, sel)
    by = br.y_bound(h, 12, s, sel)
    assert cs > 0 and -(-by * br.gain_sum(gr, gi) >> cs) <= 16384 < -(-by * br.gain_sum(gr, gi) >> (cs - 1))
    _edge(lib, True, taps=h, N=12, shift=s, channels=sel, gr=gr, gi=gi, chan_shift=cs)
    _edge(lib, False, taps=h, N=12, shift=s, channels=sel, gr=gr, gi=gi, chan_shift=cs - 1)


def test_nulls():
    _, lib = _lib()
    assert _new(lib) == NO_DEVICE
    assert _new(lib, taps=None) == INV and _new(lib, gr=None) == INV and _new(lib, cfg=False) == INV
    assert _new(lib, dev=False) == INV and _new(lib, out=False) == INV and _new(lib, n_streams=0) == INV
    buf = np.zeros(64, np.uint8)
    n = C.c_size_t()
    assert lib.fmd_bandplan_run_batch(None, buf.ctypes.data, 64, buf.ctypes.data, 1, C.byref(n)) == INV
    assert lib.fmd_bandplan_run_device(None, buf.ctypes.data, 64, buf.ctypes.data, 1, C.byref(n), None) == INV
    assert lib.fmd_bandplan_check(None) == INV and lib.fmd_bandplan_reset(None) == INV
    assert lib.fmd_bandplan_outputs(None, None) == INV and lib.fmd_bandplan_levels(None, None, None) == INV
    assert lib.fmd_bandplan_kernel_name(None, 0, None, 0) == INV
    lib.fmd_bandplan_free(None)
    assert lib.fmd_version() == 3


def test_auto_shifts_are_the_smallest_admissible():
    fmd, _ = _lib()
    for N, P, sel, mode in ((16, 8, None, br.AM), (96, 8, [5, 37, 38, 90], br.AM), (96, 8, [5, 37, 38, 90], br.FM), (12, 6, [0, 5, 11], br.IQ)):
        h = fmd.uniform_taps(N, P)
        gr, gi = fmd.narrow_taps(50000, 32, 300, 3000) if mode == br.IQ else fmd.narrow_taps(50000, 32, -4000, 4000)
        s, cs = fmd.bandplan_auto_shifts(h, N, sel, gr, gi, mode)
        limit = 256 if mode == br.FM else 16384
        assert s == ur.min_shift(h, ur.channel_incs(N, sel)) and cs == br.min_chan_shift(h, N, s, gr, gi, sel, limit=limit)
        assert fmd.bandplan_auto_shifts(h, N, sel, gr, gi, mode, shift=s + 2)[0] == s + 2


# ---- the shipped code object ------------------------------------------------------------------------------------------------------

def test_code_object_kernels_no_f64_no_scratch_no_spills(code_objects):  # noqa: F811
    ks = {n: k for n, k in code_objects.items() if "fmd_bp::" in n}
    assert len(ks) == 2, sorted(ks)                              # real and complex taps
    for n, k in ks.items():
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        f64 = [ins for ins in k["text"] if re.search(r"_f64|f64_", ins.split()[0])]
        assert not f64, (n, f64[:4])
        assert any(ins.startswith("v_dot2") for ins in k["text"]), n   # the FIR is on the packed dot product


# ---- the definition does the job --------------------------------------------------------------------------------------------------

FS, N_PLAN, HOP, SEL = 2400000, 96, 48, [5, 37, 38, 90]
P_BLK = 256


def _offset(k, n=N_PLAN):
    return (k if 2 * k < n else k - n) * FS / n


def _run_job(signal, mode, hop, R, gr, gi, squelch, seed, blocks=6, limit=16384):
    """`signal(n)` (complex, full scale 127) plus noise sigma 1 through the definition with the smallest legal shifts: the audio of
    SEL [4, n] (IQ: [4, n, 2]), the levels [(open, rms)] of the last block, and the output rate."""
    h = ur.taps(N_PLAN, 8)
    T = h.size
    M = R * (blocks * P_BLK - 1) + len(gr)                       # y outputs that complete `blocks` blocks
    n = T + hop * (M - 1)
    n += (-n) % hop
    iq = nr.to_u8(signal(n), noise=1.0, seed=seed)
    shift = ur.min_shift(h, ur.channel_incs(N_PLAN, SEL))
    cs = br.min_chan_shift(h, N_PLAN, shift, gr, gi, SEL, limit=limit)
    ref = br.BandPlanRef(h, N_PLAN, hop, shift, gr, gi, mode, R, cs, P_BLK, squelch, 256, channels=SEL)
    out = ref.feed(iq)
    assert out.shape[1] == blocks * P_BLK
    return out, [ref.level(i) for i in range(len(SEL))], FS / hop / R


def _tone_db(x, rate, tone_hz, skip=P_BLK):
    """Power of the tone's bin over all the other bins but DC, in dB, of x[skip:] cut to whole periods of the tone's bin grid."""
    x = np.asarray(x[skip:], np.float64)
    per = int(round(rate / np.gcd(int(rate), int(tone_hz))))     # samples after which the tone's phase repeats
    x = x[:x.size // per * per]
    X = np.abs(np.fft.rfft(x)) ** 2
    b = int(round(tone_hz * x.size / rate))
    rest = X[1:].sum() - X[b]
    return 10 * np.log10(X[b] / rest)


def am_job(seed):
    """The issue's case: an AM tone (1 kHz, 50 %, amplitude 20) in channel 37, a carrier of amplitude 60 in channel 90."""
    import rtl_sdr_rs_amd as fmd
    gr, _ = fmd.narrow_taps(FS / HOP, 32, -4000, 4000)
    sig = lambda n: nr.am(n, FS, _offset(37), 20, 1000.0, 0.5) + nr.carrier(n, FS, _offset(90), 60)
    out, lv, rate = _run_job(sig, br.AM, HOP, 4, gr, None, 40, seed)
    return out, lv, _tone_db(out[1], rate, 1000)


def nfm_job(seed):
    """An NFM tone (1 kHz, deviation 2.5 kHz, amplitude 20) in channel 37, the same carrier in channel 90; chan_shift keeps
    |u| <= 2048 (at the 256 of the auto shift a signal of amplitude 20 is left with an RMS of 5 units)."""
    import rtl_sdr_rs_amd as fmd
    gr, _ = fmd.narrow_taps(FS / HOP, 32, -5000, 5000)
    sig = lambda n: nr.nfm(n, FS, _offset(37), 20, 1000.0, 2500.0) + nr.carrier(n, FS, _offset(90), 60)
    out, lv, rate = _run_job(sig, br.FM, HOP, 4, gr, None, 20, seed, limit=2048)
    return out, lv, _tone_db(out[1], rate, 1000)


def ssb_job(seed, upper):
    """A tone 1 kHz above and another 1.5 kHz below a suppressed carrier at channel 37's centre, both of amplitude 20; USB taps
    (300 ... 3000 Hz) or LSB taps (-3000 ... -300 Hz), 64 of them at hop 96 (25 kHz), R = 2."""
    import rtl_sdr_rs_amd as fmd
    gr, gi = fmd.narrow_taps(FS / 96, 64, 300, 3000) if upper else fmd.narrow_taps(FS / 96, 64, -3000, -300)
    sig = lambda n: nr.ssb_tone(n, FS, _offset(37), 20, 1000.0) + nr.ssb_tone(n, FS, _offset(37), 20, -1500.0)
    out, lv, rate = _run_job(sig, br.SSB, 96, 2, gr, gi, 40, seed)
    return out, lv, _tone_db(out[1], rate, 1000 if upper else 1500)


# tone over the rest of channel 37's audio in dB, seeds 0 ... 3, measured on the definition; the assertion sits 3 dB
# below the lowest
MEASURED = {"am": (34.6, 35.4, 35.2, 34.6), "nfm": (22.3, 22.4, 22.4, 22.4), "usb": (51.1, 51.3, 51.0, 50.7), "lsb": (51.1, 50.9, 50.8, 50.5)}
JOBS = {"am": am_job, "nfm": nfm_job, "usb": lambda s: ssb_job(s, True), "lsb": lambda s: ssb_job(s, False)}


@pytest.mark.parametrize("kind", sorted(JOBS))
def test_the_definition_does_the_job(kind):
    out, lv, db = JOBS[kind](0)
    print("%s seed 0: levels %s, tone %.1f dB over the rest" % (kind, lv, db))
    opened = [o for o, _ in lv]
    if kind in ("am", "nfm"):
        assert opened == [False, True, False, True], lv         # 37 and 90 only
        assert lv[0][1] < 10 and lv[2][1] < 10 and lv[3][1] > 2 * lv[1][1] > 0, lv
    else:
        assert opened == [False, True, False, False], lv
    assert not out[0].any() and not out[2].any()                # the silent neighbours came out all zero
    assert not out[1][:P_BLK].any() and out[1][P_BLK:].any()    # block 0 is decided by block -1: closed
    assert db >= min(MEASURED[kind]) - 3.0, db
