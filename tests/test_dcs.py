"""CPU checks of the code squelch (include/fmd.h, fmd_dcs_*): the symbols, the refusals that need no device, the test-side
definition's own cut invariance and stepping rule (tests/dcs_ref.py), the code words and the designer in Python against C++, what the
definition decides on a DCS code under voice and noise at five rates, dcs_gpu's argument handling, and the resources of the shipped
kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dcs_ref as dr
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rtl-sdr-rs_amd")
CLI = os.path.join(PKG, "dcs_gpu")

INVALID_ARG, CAPACITY, UNSUPPORTED, NO_DEVICE = -1, -5, -6, -8
SYMBOLS = ["new", "free", "reset", "check", "outputs", "status", "kernel_name", "out_cap", "run_batch", "run_device"]
OK_CFG = dict(block=256, box=8, lp=[3, -5, 7], lshift=2, tap=list(range(23)), tol=1, min_hits=8, confirm=1, hang=1, ramp=64,
              accept=(1 << 128) - 1)


def test_every_symbol_is_declared_exported_and_bound(fmd):
    from rtl_sdr_rs_amd import _ffi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fmd_dcs_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted("fmd_dcs_" + s for s in SYMBOLS)
    for name in declared:
        assert name in _ffi.PROTOTYPES and hasattr(fmd.lib(), name), name
    assert fmd.CodeSquelch._prefix == "dcs" and issubclass(fmd.CodeSquelch, _ffi.RowProcessor)
    assert callable(fmd.code_squelched) and callable(fmd.dcs_word) and callable(fmd.dcs_design) and len(fmd.DCS_CODES) == 104
    assert fmd.lib().fmd_version() == 3
    from rtl_sdr_rs_amd.dcs import CodeSquelchConfig
    assert C.sizeof(CodeSquelchConfig) == 272 and CodeSquelchConfig.accept.offset == 256 and CodeSquelchConfig.tap.offset == 144


def _cfg(**kw):
    from rtl_sdr_rs_amd.dcs import CodeSquelchConfig
    c = dict(OK_CFG, **kw)
    cfg = CodeSquelchConfig()
    cfg.block, cfg.box, cfg.n_taps, cfg.lshift = c["block"], c["box"], c.get("n_taps", len(c["lp"])), c["lshift"]
    cfg.lp[:len(c["lp"])] = c["lp"]
    cfg.tap[:] = c["tap"]
    cfg.tol, cfg.min_hits, cfg.confirm, cfg.hang, cfg.ramp = c["tol"], c["min_hits"], c["confirm"], c["hang"], c["ramp"]
    cfg.accept[0], cfg.accept[1] = c["accept"] & ((1 << 64) - 1), c["accept"] >> 64
    return cfg


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def test_null_arguments_are_refused(fmd):
    lib = fmd.lib()
    cfg, dev, h = _cfg(), fmd.DeviceConfig(1, -1, 0), C.c_void_p()
    words = np.array([1, 2], np.uint32)
    buf = np.zeros(8, np.int16)
    i32, u32, u64, u8, sz = C.c_int32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint8(0), C.c_size_t(0)
    assert lib.fmd_dcs_new(None, _u32(words), 2, 1, C.byref(dev), C.byref(h)) == INVALID_ARG
    assert lib.fmd_dcs_new(C.byref(cfg), None, 2, 1, C.byref(dev), C.byref(h)) == INVALID_ARG
    assert lib.fmd_dcs_new(C.byref(cfg), _u32(words), 2, 1, None, C.byref(h)) == INVALID_ARG
    assert lib.fmd_dcs_new(C.byref(cfg), _u32(words), 2, 1, C.byref(dev), None) == INVALID_ARG
    assert lib.fmd_dcs_reset(None) == INVALID_ARG and lib.fmd_dcs_check(None) == INVALID_ARG
    assert lib.fmd_dcs_outputs(None, C.byref(u64), C.byref(u64)) == INVALID_ARG
    assert lib.fmd_dcs_status(None, C.byref(i32), C.byref(u32), C.byref(u8)) == INVALID_ARG
    assert lib.fmd_dcs_kernel_name(None, C.create_string_buffer(8), 8) == INVALID_ARG
    assert lib.fmd_dcs_run_batch(None, buf.ctypes.data, 1, 1, buf.ctypes.data, 1, C.byref(sz)) == INVALID_ARG
    assert lib.fmd_dcs_run_device(None, buf.ctypes.data, 1, 1, buf.ctypes.data, 1, C.byref(sz), None) == INVALID_ARG
    lib.fmd_dcs_free(None)                                   # a no-op


def _new(fmd, width=1, rows=1, words=2, word=None, **kw):
    """fmd_dcs_new's status and error text; a handle that a device granted is freed.  `word`: the value of the last table word."""
    cfg, dev, h = _cfg(**kw), fmd.DeviceConfig(rows, -1, 0), C.c_void_p()
    tab = np.arange(max(1, words), dtype=np.uint32)
    if word is not None:
        tab[-1] = word
    rc = fmd.lib().fmd_dcs_new(C.byref(cfg), _u32(tab), words, width, C.byref(dev), C.byref(h))
    text = fmd.lib().fmd_last_error().decode()
    if rc == 0:
        fmd.lib().fmd_dcs_free(h)
    return rc, text


BLOCK, BOX, NTAPS, LP, LSHIFT = ("need block a multiple of 64 in [64, 32768]", "need box a power of two in [1, 64]", "need 1 <= n_taps <= 64",
                                 "|lp entry| > 1023", "need lshift <= 31")
TAP, WORDS, WORD, TOL, MINHITS = ("need tap[0] = 0, tap non-decreasing, tap[22] <= 511", "need 1 <= n_words <= 128",
                                  "need every word below 2^23", "need tol <= 23", "need min_hits >= 1")
CONFIRM, HANG, RAMP = "need 1 <= confirm <= 255", "need hang <= 65535", "need ramp a power of two in [1, block]"


def _taps(last, first=0):
    return [first] + [last // 2] * 11 + [last] * 11


# (inside, outside, the refusal's text): keyword arguments of _new on both sides of every rule's edge
EDGES = [
    (dict(width=1), dict(width=0), "need width 1 or 2"),
    (dict(width=2), dict(width=3), "need width 1 or 2"),
    (dict(block=64), dict(block=0, ramp=1), BLOCK),
    (dict(block=32768), dict(block=32832), BLOCK),
    (dict(block=192), dict(block=200), BLOCK),
    (dict(box=1), dict(box=0), BOX),
    (dict(box=64), dict(box=128), BOX),
    (dict(box=2), dict(box=3), BOX),
    (dict(lp=[1]), dict(lp=[1], n_taps=0), NTAPS),
    (dict(lp=[1] * 64), dict(lp=[1] * 64, n_taps=65), NTAPS),
    (dict(lp=[1023, -1023]), dict(lp=[1, 1024]), LP),
    (dict(lp=[-1023]), dict(lp=[-1024]), LP),
    (dict(lp=[1, 5000], n_taps=1), dict(lp=[1, 5000], n_taps=2), LP),      # entries behind n_taps are not looked at
    (dict(lshift=31), dict(lshift=32), LSHIFT),
    (dict(tap=_taps(511)), dict(tap=_taps(512)), TAP),
    (dict(tap=[0] * 23), dict(tap=_taps(9, 1)), TAP),
    (dict(tap=[0] * 22 + [3]), dict(tap=[0, 2, 1] + [3] * 20), TAP),
    (dict(words=1), dict(words=0), WORDS),
    (dict(words=128), dict(words=129), WORDS),
    (dict(word=(1 << 23) - 1), dict(word=1 << 23), WORD),
    (dict(tol=23), dict(tol=24), TOL),
    (dict(min_hits=1), dict(min_hits=0), MINHITS),
    (dict(confirm=1), dict(confirm=0), CONFIRM),
    (dict(confirm=255), dict(confirm=256), CONFIRM),
    (dict(hang=65535), dict(hang=65536), HANG),
    (dict(ramp=1), dict(ramp=0), RAMP),
    (dict(ramp=256), dict(ramp=512), RAMP),
    (dict(ramp=128, block=192), dict(ramp=256, block=192), RAMP),
    (dict(ramp=32), dict(ramp=48), RAMP),
    (dict(rows=1), dict(rows=0), "need n_rows >= 1"),
]


@pytest.mark.parametrize("inside,outside,text", EDGES, ids=["%d" % i for i in range(len(EDGES))])
def test_domain_edges_are_decided_without_a_device(fmd, inside, outside, text):
    rc, msg = _new(fmd, **inside)
    assert rc in (0, NO_DEVICE), (rc, msg)                   # the arguments passed: only the device is left to ask
    assert _new(fmd, **outside) == (UNSUPPORTED, text)
    if not set(outside) & {"rows", "width", "words", "word", "n_taps"}:    # the Python class passes the library's refusal on
        c = dict(OK_CFG, **outside)
        with pytest.raises(fmd.FmdError) as e:
            fmd.CodeSquelch([1, 2], c["block"], c["box"], c["lp"], c["lshift"], c["tap"], tol=c["tol"], min_hits=c["min_hits"],
                            confirm=c["confirm"], hang=c["hang"], ramp=c["ramp"])
        assert e.value.status == UNSUPPORTED and text in str(e.value)


def test_out_cap_is_n_in(fmd):
    assert [fmd.lib().fmd_dcs_out_cap(n) for n in (0, 1, 655, 4096, 1 << 28)] == [0, 1, 655, 4096, 1 << 28]


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def _noise(rng, rows, n, width, amp=3000):
    return rng.integers(-amp, amp + 1, (rows, n, width)).astype(np.int16)


@pytest.mark.parametrize("width", [1, 2])
def test_reference_is_cut_invariant_and_equals_the_plain_integer_definition(width):
    """P = 192, B = 4, 5 random taps, 5 random words at tol 7 and min_hits 3, so that noise opens and closes the gate: the cuts 1 |
    7 | 1000 | 333 | rest equal one call, and both equal dcs_row's sample-by-sample Python integers, outputs and reports."""
    rng = np.random.default_rng(3 + width)
    P, F = 192, 5
    words = rng.integers(0, 1 << 23, F).astype(np.uint32)
    tap = [0, 0, 1, 2, 2, 3, 5, 6, 7, 9, 9, 10, 12, 13, 14, 15, 17, 18, 19, 20, 22, 23, 25]
    cfg = dr.Cfg(P, 4, [1023, -700, 300, 55, -1023], 9, tap, 7, 3, 1, 1, 64, 0b10110)
    x = _noise(rng, 3, 9 * P + 77, width, 32767)
    x[:, 17] = -32768
    whole = dr.CodeSquelch(words, cfg)
    y = whole.push(x)
    ref, got, lo = dr.CodeSquelch(words, cfg), [], 0
    for n in (1, 7, 1000, 333, x.shape[1]):
        hi = min(x.shape[1], lo + n)
        got.append(ref.push(x[:, lo:hi]))
        lo = hi
    assert np.array_equal(np.concatenate(got, axis=1), y) and ref.status() == whole.status() and ref.hits == whole.hits
    seen = set()
    for r in range(3):
        out, reports, _, _ = dr.dcs_row(x[r], words, cfg)
        assert np.array_equal(np.array(out, np.int64), y[r].astype(np.int64))
        assert [(h, n) for b, row, h, f, n in whole.hits if row == r] == [(rep[0], rep[2]) for rep in reports]
        assert (whole.status()[0][r], whole.status()[1][r], whole.status()[2][r]) == (reports[-1][1], reports[-1][2], reports[-1][3] != 0)
        seen |= {rep[3] for rep in reports}
    assert seen == {0, 256}                                  # the gate was both open and closed


HITS = [5, 5, 5, -1, -1, -1, 5, 7, 7, 7, -1]
STEPS = {(1, 0): [5, 5, 5, -1, -1, -1, 5, 7, 7, 7, -1], (1, 2): [5, 5, 5, 5, 5, -1, 5, 7, 7, 7, 7],
         (3, 0): [-1, -1, 5, -1, -1, -1, -1, -1, -1, 7, -1], (3, 2): [-1, -1, 5, 5, 5, -1, -1, -1, -1, 7, 7]}


@pytest.mark.parametrize("confirm,hang", sorted(STEPS))
def test_stepping_rule_on_a_hand_made_hit_sequence(confirm, hang):
    cfg = dr.Cfg(256, 8, [1], 0, [0] * 23, 1, 8, confirm, hang, 64, (1 << 5) | (1 << 100))
    state, ts, ss = (dr.NONE, dr.NONE, 0, 0), [], []
    for hit in HITS:
        state, s = dr.step(state, hit, cfg)
        ts.append(state[0])
        ss.append(s)
    assert ts == STEPS[(confirm, hang)]
    assert ss == [256 if t == 5 else 0 for t in ts]          # of 5 and 7, only word 5 is accepted
    assert dr.step((dr.NONE, 100, 9, 0), 100, cfg)[1] == 256                # a bit of the second accept word
    state = (dr.NONE, 5, 65534, 0)
    for _ in range(3):
        state, _ = dr.step(state, 5, cfg)
    assert state[2] == 65535                                 # the count saturates


def test_out_equals_x_under_an_open_gate():
    """One word of all ones at tol 23 and min_hits 1: every k hits, so block 0 opens block 1 over Q samples, and from block 2 on
    the output is the input bit for bit."""
    P, Q = 128, 32
    cfg = dr.Cfg(P, 2, [5, 5], 1, list(range(23)), 23, 1, 1, 0, Q, 1)
    rng = np.random.default_rng(11)
    x = rng.integers(-32768, 32768, (2, 4 * P + 5, 2)).astype(np.int16)
    ref = dr.CodeSquelch([0x7FFFFF], cfg)
    y = ref.push(x).astype(np.int64)
    xi = x.astype(np.int64)
    assert [h[2:] for h in ref.hits if h[1] == 0] == [(0, 0, P // 2)] * 4
    assert not y[:, :P].any() and np.array_equal(y[:, 2 * P:], xi[:, 2 * P:])
    up = (256 * (np.minimum(np.arange(P), Q - 1) + 1)) >> 5
    assert np.array_equal(y[:, P:2 * P], (xi[:, P:2 * P] * up[None, :, None]) >> 8)


# ---- the designer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe_exe(fmd, tmp_path_factory):
    fmd.lib()
    exe = str(tmp_path_factory.mktemp("probe") / "dcs_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "dcs_probe.cpp"), "-o", exe, "-L", PKG, "-lfmd_hip", "-Wl,-rpath," + PKG],
                   check=True, timeout=300)
    return exe


def _rotations(w):
    return {((w << s) | (w >> (23 - s))) & 0x7FFFFF for s in range(23)}


def test_code_words(fmd, probe_exe):
    from rtl_sdr_rs_amd import dcs
    codes = fmd.DCS_CODES
    assert len(codes) == len(set(codes)) == 104 and list(codes) == sorted(codes) and (codes[0], codes[-1]) == (0o023, 0o754)
    assert fmd.dcs_codeword(0o023) == 0x763813 and fmd.dcs_word(0o023) == 0x640E37
    cw = [fmd.dcs_codeword(c) for c in codes]
    for c, w in zip(codes, cw):
        assert w & 0xFFF == 0x800 | c and w < 1 << 23 and dcs.dcs_remainder(w) == 0          # divisible by the polynomial
        assert fmd.dcs_word(c) == int(format(w, "023b")[::-1], 2) == sum(((w >> (22 - j)) & 1) << j for j in range(23))
        assert fmd.dcs_word(c, True) == fmd.dcs_word(c) ^ 0x7FFFFF
    rots = [_rotations(w) for w in cw]
    for a in range(104):                                     # no word is a rotation of another
        assert sum(cw[a] in rots[b] for b in range(104)) == 1
    for a in range(104):                                     # the complement of every word is a rotation of one of the 104
        assert sum((cw[a] ^ 0x7FFFFF) in rots[b] for b in range(104)) == 1
    assert (cw[codes.index(0o023)] ^ 0x7FFFFF) in rots[codes.index(0o047)]
    out = subprocess.run([probe_exe, "words"], check=True, capture_output=True, timeout=120).stdout.decode().split()
    cpp = np.array([int(v) for v in out], np.int64).reshape(104, 4)
    assert cpp.tolist() == [[c, fmd.dcs_codeword(c), fmd.dcs_word(c), fmd.dcs_word(c, True)] for c in codes]


@pytest.mark.parametrize("rate", [8000, 9600, 12000, 12500, 16000, 24000, 44100, 48000, 95000])
def test_design_in_cpp_and_python(fmd, probe_exe, rate):
    d = fmd.dcs_design(rate)
    out = subprocess.run([probe_exe, "design", str(rate)], check=True, capture_output=True, timeout=120).stdout.decode().split()
    cpp = [int(v) for v in out]
    assert cpp == [d.block, d.box, len(d.lp), d.lshift, d.tol, d.min_hits, d.confirm, d.hang, d.ramp] + d.lp.tolist() + d.tap.tolist()
    assert np.abs(d.lp.astype(np.int64)).max() == 1023 and len(d.lp) == 32 and d.lshift == 13
    assert 1 << (d.lshift - 1) < np.abs(d.lp.astype(np.int64)).sum() <= 1 << d.lshift
    assert d.box in (1, 2, 4, 8, 16, 32, 64) and abs(rate / d.box - 1500) <= min(abs(rate / b - 1500) for b in (1, 2, 4, 8, 16, 32, 64))
    assert d.block % 64 == 0 and 0 <= d.block - 46 * rate / 134.4 < 64 and d.tap[0] == 0 and d.tap[22] <= 511
    assert (d.tol, d.min_hits, d.confirm, d.hang, d.ramp) == (1, 8, 1, 1, 64)


def test_design_at_the_issues_rates(fmd):
    assert [fmd.dcs_design(r).box for r in (9600, 12000, 16000, 24000, 48000)] == [8, 8, 8, 16, 32]
    assert fmd.dcs_design(12000).block == 4160 and fmd.dcs_design(12000).tap.tolist()[:4] == [0, 11, 22, 33]
    with pytest.raises(ValueError):
        fmd.dcs_design(200000)


def test_cpp_code_squelch_passes_the_librarys_argument_checks_on(probe_exe):
    out = subprocess.run([probe_exe], check=True, capture_output=True, timeout=120).stdout.decode()
    probe = {line.split()[0]: int(line.split()[1]) for line in out.splitlines()}
    inside = {k: v for k, v in probe.items() if k in ("defaults", "block_32768", "largest")}
    assert len(inside) == 3 and all(v in (0, NO_DEVICE) for v in inside.values()), probe
    outside = {k: v for k, v in probe.items() if k not in inside}
    assert sorted(outside) == ["block_4100", "box_3", "confirm_256", "hang_65536", "lp_1024", "lshift_32", "min_hits_0", "n_taps_65",
                               "ramp_48", "rows_0", "tap_512", "tol_24", "width_3", "words_129"]
    assert all(v == UNSUPPORTED for v in outside.values()), probe


# ---- what the definition decides --------------------------------------------------------------------------------------------------
VOICE = ((310, 2500), (440, 3000), (950, 2500), (1730, 2000), (2900, 1500))


def _voice(rng, rate, n):
    t = np.arange(n, dtype=np.float64)
    x = rng.normal(0.0, 200.0, n)
    for hz, amp in VOICE:
        x += amp * np.cos(2 * np.pi * hz * t / rate)
    return x


def _code_signal(fmd, rate, n, code, phase, dc):
    """NRZ at 134.4 bit/s, bit 0 of the codeword first, amplitude 300 on the DC `dc`, starting `phase` bits into the word."""
    c = fmd.dcs_codeword(code)
    bit = np.floor(np.arange(n) * 134.4 / rate + phase).astype(np.int64) % 23
    return dc + 300.0 * (2.0 * ((c >> bit) & 1) - 1.0)


@pytest.mark.parametrize("rate", [9600, 12000, 16000, 24000, 48000])
def test_every_fourth_code_is_found_under_voice_and_noise_and_no_code_is_never_a_hit(fmd, rate):
    """dcs_design(rate) over the table of all 104 words: a code at amplitude 300, at a random bit phase, on a DC of +-2500, under five
    voice-band cosines (310, 440, 950, 1730, 2900 Hz at 2500, 3000, 2500, 2000, 1500) and Gaussian noise of 200 rms is a hit on its own
    index in every block from the third on, for every fourth of the 104 codes, and no other index reaches min_hits in any block; the
    voice mix without a code never reaches it over 40 blocks, nor does white noise of 3000 rms.
    Measured worst values (own hits from the third block on / largest foreign count / voice only / noise only):
    9600: 14 / 1 / 1 / 1;  12000: 19 / 1 / 1 / 1;  16000: 26 / 0 / 2 / 2;  24000: 18 / 1 / 2 / 2;  48000: 19 / 0 / 1 / 1."""
    rng = np.random.default_rng(20261020 + rate)
    codes = fmd.DCS_CODES
    words = [fmd.dcs_word(c) for c in codes]
    d = fmd.dcs_design(rate)
    cfg = dr.Cfg(d.block, d.box, d.lp, d.lshift, d.tap, d.tol, d.min_hits, d.confirm, d.hang, d.ramp, (1 << 104) - 1)
    P, nblk = d.block, 6
    tested = list(range(0, 104, 4))
    x = np.stack([_voice(rng, rate, nblk * P) + _code_signal(fmd, rate, nblk * P, codes[f], rng.uniform(0, 23), rng.choice([-2500.0, 2500.0]))
                  for f in tested])
    x = np.rint(x).clip(-32768, 32767).astype(np.int16)[:, :, None]
    own, foreign = None, 0
    ref = dr.CodeSquelch(words, cfg)
    for j in range(nblk):
        ref.push(x[:, j * P:(j + 1) * P - 1])
        counts = ref.cnt.copy()                              # (the block's counters, one sample before its end)
        ref.push(x[:, (j + 1) * P - 1:(j + 1) * P])
        for row, f in enumerate(tested):
            if j >= 2:
                own = int(counts[row, f]) if own is None else min(own, int(counts[row, f]))
            counts[row, f] = 0
        foreign = max(foreign, int(counts.max()))
    quiet = {}
    for name, sig in (("voice", _voice(rng, rate, 40 * P)), ("noise", rng.normal(0.0, 3000.0, 40 * P))):
        q = dr.CodeSquelch(words, cfg)
        q.push(np.rint(sig).clip(-32768, 32767).astype(np.int16)[None, :, None])
        quiet[name] = (max(h[4] for h in q.hits), [h[2] for h in q.hits])
    print("rate %d: worst own hits %d, largest foreign count %d, voice only %d, noise only %d" % (rate, own, foreign, quiet["voice"][0],
                                                                                               quiet["noise"][0]))
    for j in range(2, nblk):
        assert [h[2] for h in ref.hits if h[0] == j] == tested, j
    assert foreign < d.min_hits <= own
    assert quiet["voice"][1] == [dr.NONE] * 40 and quiet["noise"][1] == [dr.NONE] * 40
    assert quiet["voice"][0] < d.min_hits and quiet["noise"][0] < d.min_hits


# ---- the tool -----------------------------------------------------------------------------------------------------------------------
USAGE = """usage: %s -r rate [-c 1|2] [-a code,...] [-i] [in.s16 [out.s16]]
       (code squelch: raw s16 in, mono or interleaved pairs (-c 2), raw s16 of the same length, muted unless an accepted DCS code is sent)
"""
MISSING = "/nonexistent-dir/in.s16"
NO_DEVICE_TEXT = "error: no usable gfx950 device: "

# (arguments, exit code, stderr)
EARLY = [
    (["-h"], 0, USAGE % CLI),
    (["--help"], 0, USAGE % CLI),
    ([os.devnull], 2, "need -r rate\n"),
    (["-r", "0", os.devnull], 2, "need -r rate\n"),
    (["-r", "12000", "-c", "3", os.devnull], 2, "bad -c: need 1 or 2\n"),
    (["-r", "x", os.devnull], 2, "bad -r: x\n"),
    (["-r", "12000", "-a", "024", os.devnull], 2, "bad -a: 024\n"),
    (["-r", "12000", "-a", "23.0", os.devnull], 2, "bad -a: 23.0\n"),
    (["-r", "12000", "-a", "089", os.devnull], 2, "bad -a: 089\n"),
    (["-r", "12000", "-a", "023,", os.devnull], 2, "bad -a: 023,\n"),
    (["-r", "12000", "-a", "", os.devnull], 2, "bad -a: \n"),
    ([os.devnull, "-r"], 2, "-r needs a value\n"),
    ([os.devnull, "-a"], 2, "-a needs a value\n"),
    (["-r", "12000", os.devnull, "a.s16", "b.s16"], 2, "too many files\n"),
    (["-r", "12000", MISSING], 2, MISSING + ": No such file or directory\n"),
]
NEED_DEVICE = [[], ["-c", "2", "-a", "023,754", "-i"], ["-a", "23"]]


def run_cli(args, cwd):
    assert os.path.exists(CLI), "dcs_gpu not built (run __graft_entry__.build())"
    p = subprocess.run([CLI] + args, stdin=subprocess.DEVNULL, capture_output=True, cwd=str(cwd), timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


@pytest.mark.parametrize("args,code,stderr", EARLY, ids=[" ".join(c[0]) for c in EARLY])
def test_cli_early_exits(args, code, stderr, tmp_path):
    assert run_cli(args, tmp_path) == (code, b"", stderr)
    assert list(tmp_path.iterdir()) == []


def test_cli_refuses_a_rate_outside_the_designers_range_without_a_device(tmp_path):
    code, stdout, stderr = run_cli(["-r", "200000", os.devnull, "out.s16"], tmp_path)
    assert (code, stdout) == (1, b"") and stderr.startswith("error: ") and stderr.count("\n") == 1
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("args", NEED_DEVICE, ids=[" ".join(c) or "defaults" for c in NEED_DEVICE])
def test_cli_no_device_is_exit_1_with_the_library_message(fmd, args, tmp_path):
    code, stdout, stderr = run_cli(["-r", "12000"] + args + [os.devnull], tmp_path)
    if fmd.device_count() > 0:                               # with a device the empty input is an empty output
        assert (code, stdout, stderr) == (0, b"", "")
    else:
        assert (code, stdout) == (1, b"") and stderr.startswith(NO_DEVICE_TEXT)
        assert stderr.count("\n") == 1 and stderr.endswith("\n")


def test_code_object_kernels_fit_what_the_design_states(code_objects):  # noqa: F811
    """both widths, no scratch, no spills, at most 128 VGPRs (four waves per SIMD by registers), and static LDS (the b
    ring, two chunks of m and of the samples as they are, the counters, the state, the constant) that with the largest soft ring
    (16 rows x 1024 int16 of dynamic LDS) stays inside 64 KiB."""
    ks = {n: k for n, k in code_objects.items() if "fmd_dc::" in n}
    assert sorted(n.split("fmd_dc::")[1].split("(")[0] for n in ks) == ["fmd_dcs_kernel<1>", "fmd_dcs_kernel<2>"], sorted(ks)
    for n, k in ks.items():
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert m["vgpr_count"] <= 128, (n, m)
    from test_receiver import _lds_bytes
    lds = sorted(_lds_bytes("fmd_dcs_kernel"))
    assert len(lds) == 2 and lds[1] + 16 * 1024 * 2 <= 65536 and lds[1] - lds[0] == 4096, lds
