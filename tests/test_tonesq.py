"""CPU checks of the tone squelch (include/fmd.h, fmd_tonesq_*): the symbols, the refusals that need no device, the test-side
definition's own cut invariance, stepping rule and ramp (tests/tonesq_ref.py), the table designer in Python against C++, what the
definition decides on a CTCSS tone under voice and noise, tonesq_gpu's argument handling, and the resources of the shipped kernels."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import tonesq_ref as tr
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rtl-sdr-rs_amd")
CLI = os.path.join(PKG, "tonesq_gpu")

INVALID_ARG, CAPACITY, UNSUPPORTED, NO_DEVICE = -1, -5, -6, -8
SYMBOLS = ["new", "free", "reset", "check", "outputs", "status", "kernel_name", "out_cap", "run_batch", "run_device"]
OK_CFG = dict(block=256, guard=1, dom_shift=3, confirm=2, hang=2, ramp=64, min_power=20_000_000, accept=(1 << 64) - 1)


def test_every_symbol_is_declared_exported_and_bound(fmd):
    from rtl_sdr_rs_amd import _ffi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fmd_tonesq_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted("fmd_tonesq_" + s for s in SYMBOLS)
    for name in declared:
        assert name in _ffi.PROTOTYPES and hasattr(fmd.lib(), name), name
    assert fmd.ToneSquelch._prefix == "tonesq" and issubclass(fmd.ToneSquelch, _ffi.RowProcessor)
    assert callable(fmd.tone_squelched) and callable(fmd.tone_table) and len(fmd.CTCSS_TONES) == 38
    assert fmd.lib().fmd_version() == 3


def _cfg(**kw):
    from rtl_sdr_rs_amd.tonesq import ToneSquelchConfig
    c = dict(OK_CFG, **kw)
    return ToneSquelchConfig(c["block"], c["guard"], c["dom_shift"], c["confirm"], c["hang"], c["ramp"], c["min_power"], c["accept"])


def _table(F, P, fill=7):
    return np.full((F, P, 2), fill, np.int16)


def _i16(a):
    return a.ctypes.data_as(C.POINTER(C.c_int16))


def test_null_arguments_are_refused(fmd):
    lib = fmd.lib()
    cfg, dev, h = _cfg(), fmd.DeviceConfig(1, -1, 0), C.c_void_p()
    tab = _table(2, 256)
    buf = np.zeros(8, np.int16)
    i32, u64, u8, sz = C.c_int32(0), C.c_uint64(0), C.c_uint8(0), C.c_size_t(0)
    assert lib.fmd_tonesq_new(None, _i16(tab), 2, 1, C.byref(dev), C.byref(h)) == INVALID_ARG
    assert lib.fmd_tonesq_new(C.byref(cfg), None, 2, 1, C.byref(dev), C.byref(h)) == INVALID_ARG
    assert lib.fmd_tonesq_new(C.byref(cfg), _i16(tab), 2, 1, None, C.byref(h)) == INVALID_ARG
    assert lib.fmd_tonesq_new(C.byref(cfg), _i16(tab), 2, 1, C.byref(dev), None) == INVALID_ARG
    assert lib.fmd_tonesq_reset(None) == INVALID_ARG and lib.fmd_tonesq_check(None) == INVALID_ARG
    assert lib.fmd_tonesq_outputs(None, C.byref(u64), C.byref(u64)) == INVALID_ARG
    assert lib.fmd_tonesq_status(None, C.byref(i32), C.byref(u64), C.byref(u8)) == INVALID_ARG
    assert lib.fmd_tonesq_kernel_name(None, C.create_string_buffer(8), 8) == INVALID_ARG
    assert lib.fmd_tonesq_run_batch(None, buf.ctypes.data, 1, 1, buf.ctypes.data, 1, C.byref(sz)) == INVALID_ARG
    assert lib.fmd_tonesq_run_device(None, buf.ctypes.data, 1, 1, buf.ctypes.data, 1, C.byref(sz), None) == INVALID_ARG
    lib.fmd_tonesq_free(None)                                # a no-op


def _new(fmd, width=1, rows=1, tones=2, entry=None, **kw):
    """fmd_tonesq_new's status and error text; a handle that a device granted is freed.  `entry`: the value of one table entry."""
    cfg, dev, h = _cfg(**kw), fmd.DeviceConfig(rows, -1, 0), C.c_void_p()
    P = dict(OK_CFG, **kw)["block"]
    tab = _table(max(1, tones), P if 1 <= P <= 16384 else 64)
    if entry is not None:
        tab[-1, -1, 1] = entry
    rc = fmd.lib().fmd_tonesq_new(C.byref(cfg), _i16(tab), tones, width, C.byref(dev), C.byref(h))
    text = fmd.lib().fmd_last_error().decode()
    if rc == 0:
        fmd.lib().fmd_tonesq_free(h)
    return rc, text


BLOCK, TONES, PRODUCT, ENTRY = ("need block a power of two in [64, 8192]", "need 1 <= n_tones <= 64", "need n_tones * block <= 262144",
                                "|table entry| > 1023")
GUARD, DOM, POWER, CONFIRM, HANG, RAMP = ("need guard <= 63", "need dom_shift <= 32", "need min_power >= 1", "need 1 <= confirm <= 255",
                                          "need hang <= 65535", "need ramp a power of two in [1, block]")
# (inside, outside, the refusal's text): keyword arguments of _new on both sides of every rule's edge
EDGES = [
    (dict(width=1), dict(width=0), "need width 1 or 2"),
    (dict(width=2), dict(width=3), "need width 1 or 2"),
    (dict(block=64), dict(block=32, ramp=32), BLOCK),
    (dict(block=8192), dict(block=16384), BLOCK),
    (dict(block=128), dict(block=96), BLOCK),
    (dict(tones=1), dict(tones=0), TONES),
    (dict(tones=64), dict(tones=65), TONES),
    (dict(tones=32, block=8192), dict(tones=33, block=8192), PRODUCT),
    (dict(tones=64, block=4096), dict(tones=63, block=8192), PRODUCT),
    (dict(entry=1023), dict(entry=1024), ENTRY),
    (dict(entry=-1023), dict(entry=-1024), ENTRY),
    (dict(guard=63), dict(guard=64), GUARD),
    (dict(dom_shift=32), dict(dom_shift=33), DOM),
    (dict(min_power=1), dict(min_power=0), POWER),
    (dict(confirm=1), dict(confirm=0), CONFIRM),
    (dict(confirm=255), dict(confirm=256), CONFIRM),
    (dict(hang=65535), dict(hang=65536), HANG),
    (dict(ramp=1), dict(ramp=0), RAMP),
    (dict(ramp=256), dict(ramp=512), RAMP),
    (dict(ramp=32), dict(ramp=48), RAMP),
    (dict(rows=1), dict(rows=0), "need n_rows >= 1"),
]


@pytest.mark.parametrize("inside,outside,text", EDGES, ids=["%s|%s" % (a, b) for a, b, _ in EDGES])
def test_domain_edges_are_decided_without_a_device(fmd, inside, outside, text):
    rc, msg = _new(fmd, **inside)
    assert rc in (0, NO_DEVICE), (rc, msg)                   # the arguments passed: only the device is left to ask
    assert _new(fmd, **outside) == (UNSUPPORTED, text)
    if not set(outside) & {"rows", "width", "tones", "entry", "block"}:   # the Python class passes the library's refusal on
        with pytest.raises(fmd.FmdError) as e:
            fmd.ToneSquelch(_table(2, 256), **outside)
        assert e.value.status == UNSUPPORTED and text in str(e.value)


def test_out_cap_is_n_in(fmd):
    assert [fmd.lib().fmd_tonesq_out_cap(n) for n in (0, 1, 655, 4096, 1 << 28)] == [0, 1, 655, 4096, 1 << 28]


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def _noise(rng, rows, n, width, amp=3000):
    return rng.integers(-amp, amp + 1, (rows, n, width)).astype(np.int16)


def _random_table(rng, F, P):
    t = rng.integers(-1023, 1024, (F, P, 2)).astype(np.int16)
    t[0, :3] = [[1023, -1023], [-1023, 1023], [0, 0]]
    return t


@pytest.mark.parametrize("width", [1, 2])
def test_reference_is_cut_invariant_and_equals_the_plain_integer_definition(width):
    """P = 256, a random table of 5 tones, thresholds low enough that noise opens and closes the gate: the cuts 1 | 7 | 1000 | 333 |
    rest equal one call, and both equal tonesq_row's sample-by-sample Python integers, outputs and reports."""
    rng = np.random.default_rng(3 + width)
    P, F = 256, 5
    tab = _random_table(rng, F, P)
    cfg = tr.Cfg(P, 0, 0, 1, 1, 64, 1, 0b10110)
    x = _noise(rng, 3, 9 * P + 77, width, 32767)
    x[:, 17] = -32768
    whole = tr.ToneSquelch(tab, cfg)
    y = whole.push(x)
    ref, got, lo = tr.ToneSquelch(tab, cfg), [], 0
    for n in (1, 7, 1000, 333, x.shape[1]):
        hi = min(x.shape[1], lo + n)
        got.append(ref.push(x[:, lo:hi]))
        lo = hi
    assert np.array_equal(np.concatenate(got, axis=1), y) and ref.status() == whole.status() and ref.hits == whole.hits
    opened = 0
    for r in range(3):
        out, reports = tr.tonesq_row(x[r], tab, cfg)
        assert np.array_equal(np.array(out, np.int64), y[r].astype(np.int64))
        assert [h for b, row, h in whole.hits if row == r] == [rep[0] for rep in reports]
        assert (whole.status()[0][r], whole.status()[1][r], whole.status()[2][r]) == (reports[-1][1], reports[-1][2], reports[-1][3] != 0)
        opened += len({rep[3] for rep in reports})
    assert opened > 3                                        # some row saw the gate both open and closed


HITS = [5, 5, 5, -1, -1, -1, 5, 7, 7, 7, -1]
STEPS = {(1, 0): [5, 5, 5, -1, -1, -1, 5, 7, 7, 7, -1], (1, 2): [5, 5, 5, 5, 5, -1, 5, 7, 7, 7, 7],
         (3, 0): [-1, -1, 5, -1, -1, -1, -1, -1, -1, 7, -1], (3, 2): [-1, -1, 5, 5, 5, -1, -1, -1, -1, 7, 7]}


@pytest.mark.parametrize("confirm,hang", sorted(STEPS))
def test_stepping_rule_on_a_hand_made_hit_sequence(confirm, hang):
    cfg = tr.Cfg(256, 1, 3, confirm, hang, 64, 1, 1 << 5)
    state, ts, ss = (tr.NONE, tr.NONE, 0, 0), [], []
    for hit in HITS:
        state, s = tr.step(state, hit, cfg)
        ts.append(state[0])
        ss.append(s)
    assert ts == STEPS[(confirm, hang)]
    assert ss == [256 if t == 5 else 0 for t in ts]          # only tone 5 is accepted
    state = (tr.NONE, 5, 65534, 0)
    for _ in range(3):
        state, _ = tr.step(state, 5, cfg)
    assert state[2] == 65535                                 # the count saturates


@pytest.mark.parametrize("Q", [1, 64, 256])
def test_ramp_and_open_gate(Q):
    """One tone row of all +1023 and a constant input: block 0 hits, so block 1 ramps up over Q samples, block 2 passes x bit for
    bit; then silence: block 3 is still open (its decision comes at its end), block 4 ramps down, block 5 is zeros."""
    P = 256
    tab = np.zeros((1, P, 2), np.int16)
    tab[0, :, 0] = 1023
    cfg = tr.Cfg(P, 0, 0, 1, 0, Q, 1, 1)
    rng = np.random.default_rng(Q)
    x = rng.integers(-32768, 32768, (1, 6 * P, 2)).astype(np.int16)
    x[0, :3 * P] = np.abs(x[0, :3 * P].astype(np.int64)).clip(1, 32767)     # a positive m in blocks 0 ... 2
    x[0, 3 * P:, 0] = x[0, 3 * P:, 0].clip(-32767, 32767)
    x[0, 3 * P:, 1] = -x[0, 3 * P:, 0]                                       # m = 0 in blocks 3 ... 5
    ref = tr.ToneSquelch(tab, cfg)
    y = ref.push(x).astype(np.int64)
    xi = x.astype(np.int64)
    assert [h for _, _, h in ref.hits] == [0, 0, 0, tr.NONE, tr.NONE, tr.NONE]
    assert not y[0, :P].any()
    k = np.minimum(np.arange(P), Q - 1) + 1
    up = (256 * k) >> (Q.bit_length() - 1)
    assert up[Q - 1] == 256 and (Q == 1 or up[0] == 256 // Q)
    assert np.array_equal(y[0, P:2 * P], (xi[0, P:2 * P] * up[:, None]) >> 8)
    assert np.array_equal(y[0, 2 * P:4 * P], xi[0, 2 * P:4 * P])             # an open gate passes x bit for bit
    down = 256 + ((-256 * k) >> (Q.bit_length() - 1))
    assert down[Q - 1] == 0 and np.array_equal(y[0, 4 * P:5 * P], (xi[0, 4 * P:5 * P] * down[:, None]) >> 8)
    assert not y[0, 5 * P:].any()


# ---- the designer ---------------------------------------------------------------------------------------------------------------
def _build_probe(fmd, tmp_path_factory):
    fmd.lib()
    exe = str(tmp_path_factory.mktemp("probe") / "tonesq_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "tonesq_probe.cpp"), "-o", exe, "-L", PKG, "-lfmd_hip", "-Wl,-rpath," + PKG],
                   check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def probe_exe(fmd, tmp_path_factory):
    return _build_probe(fmd, tmp_path_factory)


def test_ctcss_list_and_table_entries_in_cpp_and_python(fmd, probe_exe):
    tones = fmd.CTCSS_TONES
    assert len(tones) == 38 and list(tones) == sorted(tones) and (tones[0], tones[11], tones[-1]) == (67.0, 100.0, 250.3)
    for rate, P, freqs in ((12000, 4096, tones), (12500, 1024, tones), (8000, 64, (67.0, 250.3)), (48000, 8192, (100.0, 203.5))):
        tab = fmd.tone_table(rate, freqs, P)
        assert tab.shape == (len(freqs), P, 2) and tab.dtype == np.int16 and np.abs(tab.astype(np.int64)).max() <= 1023
        out = subprocess.run([probe_exe, "table", str(rate), str(P)] + [repr(float(f)) for f in freqs], check=True, capture_output=True,
                             timeout=120).stdout.decode().split()
        cpp = np.array([int(v) for v in out], np.int64).reshape(len(freqs), P, 2)
        assert np.array_equal(cpp, tab.astype(np.int64)), (rate, P)
    tab = fmd.tone_table(12000, tones, 4096).astype(np.int64)
    assert np.abs(tab).max() >= 1020                         # the window's top reaches the bound
    r = 2047
    w = 0.5 - 0.5 * math.cos(2 * math.pi * (r + 0.5) / 4096)
    assert tab[11, r, 0] == round(1023 * w * math.cos(2 * math.pi * 100.0 * r / 12000))


def test_cpp_tonesq_passes_the_librarys_argument_checks_on(probe_exe):
    out = subprocess.run([probe_exe], check=True, capture_output=True, timeout=120).stdout.decode()
    probe = {line.split()[0]: int(line.split()[1]) for line in out.splitlines()}
    inside = {k: v for k, v in probe.items() if k in ("defaults", "block_8192", "largest")}
    assert len(inside) == 3 and all(v in (0, NO_DEVICE) for v in inside.values()), probe
    outside = {k: v for k, v in probe.items() if k not in inside}
    assert sorted(outside) == ["block_48", "confirm_256", "dom_shift_33", "guard_64", "hang_65536", "min_power_0", "product_33", "ramp_48",
                               "rows_0", "tones_65", "width_3"]
    assert all(v == UNSUPPORTED for v in outside.values()), probe


# ---- what the definition decides --------------------------------------------------------------------------------------------------
RATE, P_B = 12000, 4096
VOICE = ((310, 2500), (440, 3000), (950, 2500), (1730, 2000), (2900, 1500))


def _mix(rng, n, tone_hz=None, phase=0.0):
    t = np.arange(n, dtype=np.float64)
    x = rng.normal(0.0, 200.0, n)
    for hz, amp in VOICE:
        x += amp * np.cos(2 * np.pi * hz * t / RATE)
    if tone_hz is not None:
        x += 300.0 * np.cos(2 * np.pi * tone_hz * t / RATE + phase)
    return np.rint(x).astype(np.int16)


def test_every_ctcss_tone_is_found_under_voice_and_noise_and_no_tone_is_never_a_hit(fmd):
    """Rate 12000, P 4096, the 38-tone table, guard 1, dom_shift 3, min_power 2e7: a tone of amplitude 300 under five voice-band
    cosines (310, 440, 950, 1730, 2900 Hz at 2500, 3000, 2500, 2000, 1500) and Gaussian noise of 200 rms is hit with its own index,
    each of the 38 tones at two phases; the same mix without a tone never hits over 60 blocks."""
    rng = np.random.default_rng(20261019)
    tones = fmd.CTCSS_TONES
    tab = fmd.tone_table(RATE, tones, P_B)
    cfg = tr.Cfg(P_B, 1, 3, 2, 2, 64, 20_000_000, (1 << 38) - 1)
    x = np.stack([_mix(rng, P_B, hz, ph) for hz in tones for ph in (0.0, math.pi / 3)])[:, :, None]
    worst_w, worst_ratio = None, None
    ref = tr.ToneSquelch(tab, cfg)
    ref.push(x)
    hits = {row: h for _, row, h in ref.hits}
    for row in range(x.shape[0]):
        f = row // 2
        re_im = (tr.mono(x[row]).astype(np.float64) @ ref.mat).astype(np.int64) >> 14
        W = [int(re_im[2 * k]) ** 2 + int(re_im[2 * k + 1]) ** 2 for k in range(38)]
        rest = max([W[k] for k in range(38) if abs(k - f) > 1], default=0)
        worst_w = W[f] if worst_w is None else min(worst_w, W[f])
        worst_ratio = W[f] / max(rest, 1) if worst_ratio is None else min(worst_ratio, W[f] / max(rest, 1))
    quiet = tr.ToneSquelch(tab, cfg)
    q = _mix(rng, 60 * P_B)[None, :, None]
    quiet.push(q)
    largest = 0
    for j in range(60):
        re_im = (tr.mono(q[0, j * P_B:(j + 1) * P_B]).astype(np.float64) @ quiet.mat).astype(np.int64) >> 14
        largest = max(largest, max(int(re_im[2 * k]) ** 2 + int(re_im[2 * k + 1]) ** 2 for k in range(38)))
    print("worst W_f* with a tone %.3g, worst W_f* / rest %.1f, largest W without a tone %.3g" % (worst_w, worst_ratio, largest))
    assert [hits[row] for row in range(x.shape[0])] == [row // 2 for row in range(x.shape[0])]
    assert [h for _, _, h in quiet.hits] == [tr.NONE] * 60
    assert worst_w >= 20_000_000 > largest and worst_ratio >= 8


# ---- the tool -----------------------------------------------------------------------------------------------------------------------
USAGE = """usage: %s -r rate [-c 1|2] [-b block] [-a tone_hz,...] [in.s16 [out.s16]]
       (tone squelch: raw s16 in, mono or interleaved pairs (-c 2), raw s16 of the same length, muted unless an accepted CTCSS tone is sent)
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
    (["-r", "12000", "-b", "-256", os.devnull], 2, "bad -b: -256\n"),
    (["-r", "12000", "-a", "100.1", os.devnull], 2, "bad -a: 100.1\n"),
    (["-r", "12000", "-a", "100.0,", os.devnull], 2, "bad -a: 100.0,\n"),
    (["-r", "12000", "-a", "", os.devnull], 2, "bad -a: \n"),
    ([os.devnull, "-r"], 2, "-r needs a value\n"),
    ([os.devnull, "-a"], 2, "-a needs a value\n"),
    (["-r", "12000", os.devnull, "a.s16", "b.s16"], 2, "too many files\n"),
    (["-r", "12000", MISSING], 2, MISSING + ": No such file or directory\n"),
]
# values outside the domain: the library's refusal, before a device is asked and before the output file exists
REFUSED = [(["-b", "48"], BLOCK), (["-b", "32"], BLOCK), (["-b", "0"], BLOCK), (["-b", "16384"], BLOCK), (["-b", "8192"], PRODUCT)]
NEED_DEVICE = [[], ["-c", "2", "-b", "64", "-a", "67.0,250.3"], ["-b", "4096", "-a", "100"]]


def run_cli(args, cwd):
    assert os.path.exists(CLI), "tonesq_gpu not built (run __graft_entry__.build())"
    p = subprocess.run([CLI] + args, stdin=subprocess.DEVNULL, capture_output=True, cwd=str(cwd), timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


@pytest.mark.parametrize("args,code,stderr", EARLY, ids=[" ".join(c[0]) for c in EARLY])
def test_cli_early_exits(args, code, stderr, tmp_path):
    assert run_cli(args, tmp_path) == (code, b"", stderr)
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("args,text", REFUSED, ids=[" ".join(c[0]) for c in REFUSED])
def test_cli_refuses_values_outside_the_domain_without_a_device(args, text, tmp_path):
    code, stdout, stderr = run_cli(["-r", "12000"] + args + [os.devnull, "out.s16"], tmp_path)
    assert (code, stdout) == (1, b"") and stderr.startswith("error: ") and stderr.endswith(": " + text + "\n")
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
    """both widths, no scratch, no spills, at most 168 VGPRs (three waves per SIMD) and 28160 / 32256 bytes of static
    LDS (the table chunk, m, the samples as they are, the state), of which five workgroups fit a CU."""
    ks = {n: k for n, k in code_objects.items() if "fmd_tq::" in n}
    assert sorted(n.split("fmd_tq::")[1].split("(")[0] for n in ks) == ["fmd_tonesq_kernel<1>", "fmd_tonesq_kernel<2>"], sorted(ks)
    for n, k in ks.items():
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert m["vgpr_count"] <= 168, (n, m)
    from test_receiver import _lds_bytes
    assert sorted(_lds_bytes("fmd_tonesq_kernel")) == [28160, 32256]
