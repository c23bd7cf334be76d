"""CPU checks of the rational resampler (include/fmd.h, fmd_resample_*): the symbols, the refusals that need no device, the ratio
and capacity helpers, the test-side definition's own call semantics (tests/resample_ref.py), the tap designer in Python and C++, and
resample_gpu's argument handling."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rtl-sdr-rs_amd")
CLI = os.path.join(PKG, "resample_gpu")

INVALID_ARG, TOO_SHORT, CAPACITY, UNSUPPORTED, NO_DEVICE = -1, -3, -5, -6, -8
SYMBOLS = ["ratio", "new", "free", "reset", "check", "outputs", "kernel_name", "out_cap", "run_batch", "run_device"]
# (L, M, T) of the issue: identity, plain FIR, the audio ratios, up and down to the limits
SHAPES = [(1, 1, 1), (1, 1, 256), (15, 16, 32), (3, 16, 64), (441, 512, 24), (160, 147, 48), (6, 1, 8), (1, 32, 256), (1024, 1023, 16)]


def test_every_symbol_is_declared_exported_and_bound(fmd):
    from rtl_sdr_rs_amd import _ffi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fmd_resample_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted("fmd_resample_" + s for s in SYMBOLS)
    for name in declared:
        assert name in _ffi.PROTOTYPES and hasattr(fmd.lib(), name), name
    assert fmd.Resampler._prefix == "resample" and issubclass(fmd.Resampler, _ffi.BankHandle)


def test_null_arguments_are_refused(fmd):
    lib = fmd.lib()
    g = np.array([1], np.int16)
    gp = g.ctypes.data_as(C.POINTER(C.c_int16))
    dev = fmd.DeviceConfig(1, -1, 0)
    h = C.c_void_p()
    u32, u64, sz = C.c_uint32(0), C.c_uint64(0), C.c_size_t(0)
    assert lib.fmd_resample_new(None, 1, 1, 1, 0, 1, C.byref(dev), C.byref(h)) == INVALID_ARG
    assert lib.fmd_resample_new(gp, 1, 1, 1, 0, 1, None, C.byref(h)) == INVALID_ARG
    assert lib.fmd_resample_new(gp, 1, 1, 1, 0, 1, C.byref(dev), None) == INVALID_ARG
    assert lib.fmd_resample_ratio(51200, 1, 48000, None, C.byref(u32)) == INVALID_ARG
    assert lib.fmd_resample_ratio(51200, 1, 48000, C.byref(u32), None) == INVALID_ARG
    assert lib.fmd_resample_reset(None) == INVALID_ARG and lib.fmd_resample_check(None) == INVALID_ARG
    assert lib.fmd_resample_outputs(None, C.byref(u64), C.byref(u64)) == INVALID_ARG
    assert lib.fmd_resample_kernel_name(None, C.create_string_buffer(8), 8) == INVALID_ARG
    assert lib.fmd_resample_run_batch(None, g.ctypes.data, 1, 1, g.ctypes.data, 1, C.byref(sz)) == INVALID_ARG
    assert lib.fmd_resample_run_device(None, g.ctypes.data, 1, 1, g.ctypes.data, 1, C.byref(sz), None) == INVALID_ARG
    lib.fmd_resample_free(None)                              # a no-op


def _new(fmd, g, L, M, T, shift, width, rows=1):
    """fmd_resample_new's status and error text; a handle that a device granted is freed."""
    g = np.ascontiguousarray(g, dtype=np.int16)
    dev = fmd.DeviceConfig(rows, -1, 0)
    h = C.c_void_p()
    rc = fmd.lib().fmd_resample_new(g.ctypes.data_as(C.POINTER(C.c_int16)), L, M, T, shift, width, C.byref(dev), C.byref(h))
    text = fmd.lib().fmd_last_error().decode()
    if rc == 0:
        fmd.lib().fmd_resample_free(h)
    return rc, text


def _phase(T, mag):
    """T taps with sum |g| == mag, both signs"""
    g = np.zeros(T, np.int64)
    g[0] = mag - (T - 1)
    g[1:] = -1
    return g


# (inside, outside, the refusal's text): (L, M, T, shift, width) on both sides of every rule's edge
EDGES = [
    ((1024, 1024, 16, 0, 1), (1025, 1024, 15, 0, 1), "need 1 <= L <= 1024 and 1 <= M <= 1024"),
    ((1024, 1024, 16, 0, 1), (1024, 1025, 16, 0, 1), "need 1 <= L <= 1024 and 1 <= M <= 1024"),
    ((1, 1, 1, 0, 1), (0, 1, 1, 0, 1), "need 1 <= L <= 1024 and 1 <= M <= 1024"),
    ((1, 1, 1, 0, 1), (1, 0, 1, 0, 1), "need 1 <= L <= 1024 and 1 <= M <= 1024"),
    ((1, 1, 256, 0, 1), (1, 1, 257, 0, 1), "need 1 <= T <= 256"),
    ((1, 1, 1, 0, 1), (1, 1, 0, 0, 1), "need 1 <= T <= 256"),
    ((64, 64, 256, 0, 2), (113, 113, 145, 0, 2), "need L T <= 16384"),
    ((1, 32, 4, 0, 1), (1, 33, 4, 0, 1), "need M <= 32 L"),
    ((3, 96, 4, 0, 1), (3, 97, 4, 0, 1), "need M <= 32 L"),
    ((8, 1, 4, 0, 1), (9, 1, 4, 0, 1), "need L <= 8 M"),
    ((24, 3, 4, 0, 2), (25, 3, 4, 0, 2), "need L <= 8 M"),
    ((2, 3, 4, 24, 1), (2, 3, 4, 25, 1), "need shift <= 24"),
    ((2, 3, 4, 0, 1), (2, 3, 4, 0, 0), "need width 1 or 2"),
    ((2, 3, 4, 0, 2), (2, 3, 4, 0, 3), "need width 1 or 2"),
]


@pytest.mark.parametrize("inside,outside,text", EDGES, ids=["%s|%s" % (a, b) for a, b, _ in EDGES])
def test_domain_edges_are_decided_without_a_device(fmd, inside, outside, text):
    for (L, M, T, shift, width), ok in ((inside, True), (outside, False)):
        g = np.ones(max(1, L * T), np.int16)
        rc, msg = _new(fmd, g, L, M, T, shift, width)
        if ok:
            assert rc in (0, NO_DEVICE), (rc, msg)           # the arguments passed: only the device is left to ask
        else:
            assert rc == UNSUPPORTED and msg == text, (rc, msg)


def test_gain_rule_and_rows_are_decided_without_a_device(fmd):
    L, T = 3, 5
    g = np.stack([_phase(T, 100), _phase(T, 32767), _phase(T, 7)])
    assert np.abs(g).sum(axis=1).tolist() == [100, 32767, 7]
    assert _new(fmd, g, L, 2, T, 0, 1)[0] in (0, NO_DEVICE)
    g[1, 0] += 1                                             # sum |g| = 32768 in one phase
    assert _new(fmd, g, L, 2, T, 0, 1) == (UNSUPPORTED, "need sum |g| <= 32767 in every phase")
    g[1] = -g[1]
    assert _new(fmd, g, L, 2, T, 0, 1) == (UNSUPPORTED, "need sum |g| <= 32767 in every phase")
    assert _new(fmd, np.ones(4, np.int16), 1, 1, 4, 0, 1, rows=0) == (UNSUPPORTED, "need n_rows >= 1")
    with pytest.raises(ValueError):
        fmd.Resampler(np.ones(7, np.int16), 2, 1, 0)         # not [L, T]


def test_ratio_against_fractions(fmd):
    cases = [(51200, 48000), (Fraction(1020000, 6), 48000), ((2400000, 40), 48000), ((2048000, 40), 48000), (44100, 48000),
             (256000, 48000), (Fraction(512000, 9), 48000), (8000, 48000), (1536000, 48000), (48000, 48000), (170000, 32000),
             (60000, 7500)]
    for rate_in, rate_out in cases:
        f = Fraction(rate_out) / (Fraction(*rate_in) if isinstance(rate_in, tuple) else Fraction(rate_in))
        assert fmd.resample_ratio(rate_in, rate_out) == (f.numerator, f.denominator), (rate_in, rate_out)
    assert fmd.resample_ratio(51200, 48000) == (15, 16) and fmd.resample_ratio(256000, 48000) == (3, 16)
    # reduced, but out of the domain: on L, on M, on M <= 32 L, on L <= 8 M; and zero rates
    for rate_in, rate_out, text in [(48000, 48001, "need 1 <= L <= 1024 and 1 <= M <= 1024"),      # 48001 / 48000
                                    (48001, 32000, "need 1 <= L <= 1024 and 1 <= M <= 1024"),      # 32000 / 48001
                                    (48000, 1000, "need M <= 32 L"), (1000, 9000, "need L <= 8 M"),
                                    (0, 48000, "need non-zero rates, rate_in_den and rate_out below 2^32"),
                                    (48000, 0, "need non-zero rates, rate_in_den and rate_out below 2^32")]:
        with pytest.raises(fmd.FmdError) as e:
            fmd.resample_ratio(rate_in, rate_out)
        assert e.value.status == UNSUPPORTED and text in str(e.value), (rate_in, rate_out)


def test_out_cap_bounds_every_call(fmd):
    rng = np.random.default_rng(5)
    lib = fmd.lib()
    assert lib.fmd_resample_out_cap(0, 1, 100) == 0 and lib.fmd_resample_out_cap(1, 0, 100) == 0
    for L, M, T in SHAPES + [(1, 32, 8), (8, 1, 1)]:
        N = 0
        for _ in range(300):
            n = int(rng.integers(0, 40)) if rng.random() < 0.5 else int(rng.integers(0, 5000))
            made = rr.outputs(N + n, L, M, T) - rr.outputs(N, L, M, T)
            assert made <= lib.fmd_resample_out_cap(L, M, n), (L, M, T, N, n)
            N += n


def feed(push, x, cuts):
    """The stream x [rows, N, width] through push() in pieces of `cuts` samples and then the rest; a piece that completes no
    output is refused and not taken, so it is handed over again in front of the next one.  Returns the outputs and the calls made."""
    out, calls, lo, pos = [], 0, 0, 0
    for n in list(cuts) + [x.shape[1]]:
        pos = min(x.shape[1], pos + n)
        if pos == lo:
            continue
        try:
            out.append(push(x[:, lo:pos]))
        except rr.TooShort:
            continue
        calls += 1
        lo = pos
    return np.concatenate(out, axis=1), calls


@pytest.mark.parametrize("L,M,T", [(15, 16, 32), (3, 16, 64), (441, 512, 24), (160, 147, 48), (6, 1, 8), (1, 32, 8), (1, 1, 5)])
def test_reference_is_cut_invariant_and_keeps_at_most_T_minus_1(L, M, T):
    rng = np.random.default_rng(L * 1000 + M)
    g = rng.integers(-32767 // T, 32767 // T + 1, (L, T))
    x = rng.integers(-32768, 32768, (2, 3000, 2)).astype(np.int16)
    whole = rr.resample_all(x, g, L, M, 9)
    assert whole.shape[1] == rr.outputs(3000, L, M, T)
    for cuts in ([7, 1000, 333], [5] * 200, [T, 1, 1, 2, 3, 900]):
        ref = rr.Resampler(g, L, M, 9)
        hist = []

        def push(piece):
            y = ref.push(piece)
            hist.append((ref.hist.shape[1], ref.history()))
            return y
        got, calls = feed(push, x, cuts)
        assert np.array_equal(got, whole), cuts
        assert calls > 1 and all(a == b and a <= T - 1 for a, b in hist)
    if M > L * T:                                            # the next output starts beyond what has arrived: inputs are skipped
        ref = rr.Resampler(g, L, M, 9)
        ref.push(x[:, :T + 2])
        assert ref.history() == 0 and rr.outputs(ref.N, L, M, T) * M // L > ref.N


@pytest.mark.parametrize("L,M,T", SHAPES)
def test_taps_sum_to_a_power_of_two_and_pass_dc(fmd, L, M, T):
    g, shift = fmd.resample_taps(L, M, T)
    assert g.shape == (L, T) and g.dtype == np.int16 and shift <= 14
    assert (g.astype(np.int64).sum(axis=1) == 1 << shift).all()
    assert np.abs(g.astype(np.int64)).sum(axis=1).max() <= 32767
    if shift < 14:                                           # the largest such shift: at one more, some phase breaks the gain rule
        h = np.array(fmd.resample.resample_prototype(L, M, T))
        phases = np.stack([[h[L * (T - 1 - t) + p] for t in range(T)] for p in range(L)])
        rounded = np.floor(phases / phases.sum(axis=1, keepdims=True) * (2 << shift) + 0.5)
        assert np.abs(rounded).sum(axis=1).max() > 32767 + T   # (the exact-sum correction moves one tap by less than T)
    for dc in (-32768, -1, 0, 1234, 32767):
        x = np.full((1, 600 + 40 * M // L, 1), dc, np.int16)
        y = rr.resample_all(x, g, L, M, shift)
        assert y.shape[1] > 0 and (y == dc).all()
    if (L, M, T) == (1, 1, 1):
        assert g.tolist() == [[16384]] and shift == 14       # the identity


# (L, M, T, rate_in): the audio cases of the issue; measured residuals (int16 taps, float64 taps) in LSB rms: 15/16 at 51.2 kHz
# 11.18, 10.88; 3/16 at 256 kHz 3.05, 3.30; 441/512 at 512/9 kHz 12.36, 12.34; 160/147 at 44.1 kHz 4.92, 3.02
TONES = [(15, 16, 32, 51200.0), (3, 16, 64, 256000.0), (441, 512, 24, 512000.0 / 9), (160, 147, 48, 44100.0)]


def _tone_residual(y, rate, skip):
    """rms of y minus its least-squares fit by a 1 kHz sinusoid and a constant, and the fitted amplitude"""
    n = np.arange(y.size)
    A = np.stack([np.cos(2 * np.pi * 1000 * n / rate), np.sin(2 * np.pi * 1000 * n / rate), np.ones(y.size)], axis=1)[skip:]
    c = np.linalg.lstsq(A, y[skip:], rcond=None)[0]
    return float(np.sqrt(np.mean((A @ c - y[skip:]) ** 2))), float(np.hypot(c[0], c[1]))


@pytest.mark.parametrize("L,M,T,rate_in", TONES)
def test_tone_at_1_khz_comes_out_at_1_khz(fmd, L, M, T, rate_in):
    """A 1 kHz tone of amplitude 16000 at rate_in comes out as a 1 kHz tone at rate_in L / M: what is left after the best fit of a
    1 kHz sinusoid is at most twice what a float64 evaluation of the same prototype (per-phase normalised, unrounded taps, unrounded
    output) leaves on the same input.  The factor 2 is the margin for the int16 rounding of the taps.  Measured (integer, float64) in
    LSB rms: 15/16: 11.18, 10.88; 3/16: 3.05, 3.30; 441/512: 12.36, 12.34; 160/147: 4.92, 3.02.  (At 1/32 and at the identity the
    float residual, 0.04 and 0.27 LSB, is below the rounding of the int16 OUTPUT alone, which the margin does not cover: those are
    not tone cases.)"""
    g, shift = fmd.resample_taps(L, M, T)
    x = np.floor(16000 * np.sin(2 * np.pi * 1000 * np.arange(20000) / rate_in + 0.3) + 0.5).astype(np.int16)
    y = rr.resample_all(x[None, :, None], g, L, M, shift)[0, :, 0].astype(np.float64)
    h = np.array(fmd.resample.resample_prototype(L, M, T))
    gf = np.stack([[h[L * (T - 1 - t) + p] for t in range(T)] for p in range(L)])
    gf /= gf.sum(axis=1, keepdims=True)
    n = np.arange(y.size)
    yf = (x[(n * M // L)[:, None] + np.arange(T)[None, :]] * gf[n * M % L]).sum(axis=1)
    (res_i, amp_i), (res_f, amp_f) = _tone_residual(y, rate_in * L / M, T), _tone_residual(yf, rate_in * L / M, T)
    print("tone %d/%d T=%d: residual int16 taps %.3f, float64 taps %.3f LSB rms; amplitude %.1f, %.1f" % (L, M, T, res_i, res_f, amp_i, amp_f))
    assert abs(amp_i - 16000) < 160 and abs(amp_f - 16000) < 160          # within 1 % (0.09 dB): the passband at 1 kHz
    assert res_i <= 2 * res_f


@pytest.fixture(scope="module")
def probe(fmd, tmp_path_factory):
    """{name: [int, ...]} as tests/cpp/resample_probe.cpp prints it."""
    fmd.lib()
    exe = str(tmp_path_factory.mktemp("probe") / "resample_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "resample_probe.cpp"), "-o", exe, "-L", PKG, "-lfmd_hip", "-Wl,-rpath," + PKG],
                   check=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, timeout=120).stdout.decode()
    return {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out.splitlines()}


def test_cpp_designer_and_ratio_match_python(fmd, probe):
    seen = 0
    for L, M, T in SHAPES:
        if (L, M, T) == (1, 1, 256):
            continue
        g, shift = fmd.resample_taps(L, M, T)
        assert probe["taps_%d_%d_%d" % (L, M, T)] == [shift] + g.ravel().tolist(), (L, M, T)
        seen += 1
    assert seen == 8
    for num, den, out in [(51200, 1, 48000), (1020000, 6, 48000), (2400000, 40, 48000), (2048000, 40, 48000), (44100, 1, 48000)]:
        assert tuple(probe["ratio_%d_%d_%d" % (num, den, out)]) == fmd.resample_ratio((num, den), out)


USAGE = """usage: %s -i rate_in[/den] -r rate_out [-c 1|2] [-T taps_per_phase] <in.s16 | ->
       (rational resampler: raw s16 in, mono or interleaved pairs (-c 2), raw s16 at rate_out on stdout)
"""
NEED = "need -i rate_in[/den] and a non-zero -r rate_out\n"
MISSING = "/nonexistent-dir/in.s16"
NO_DEVICE_TEXT = "error: no usable gfx950 device: "

# (arguments, exit code, stderr)
EARLY = [
    (["-h"], 0, USAGE % CLI),
    (["--help"], 0, USAGE % CLI),
    ([], 2, NEED),
    ([os.devnull], 2, NEED),
    (["-i", "51200", os.devnull], 2, NEED),
    (["-r", "48000", os.devnull], 2, NEED),
    (["-i", "51200", "-r", "0", os.devnull], 2, NEED),
    (["-i", "x", "-r", "48000", os.devnull], 2, "bad -i rate: x\n"),
    (["-i", "0", "-r", "48000", os.devnull], 2, "bad -i rate: 0\n"),
    (["-i", "1020000/", "-r", "48000", os.devnull], 2, "bad -i rate: 1020000/\n"),
    (["-i", "1020000/0", "-r", "48000", os.devnull], 2, "bad -i rate: 1020000/0\n"),
    (["-i", "1020000/6x", "-r", "48000", os.devnull], 2, "bad -i rate: 1020000/6x\n"),
    (["-i", "51200", "-r", "48000", "-c", "3", os.devnull], 2, "bad -c: need 1 or 2\n"),
    (["-i", "51200", "-r", "48000", "-T", "0", os.devnull], 2, "bad -T: need 1 ... 256\n"),
    (["-i", "51200", "-r", "48000", "-T", "257", os.devnull], 2, "bad -T: need 1 ... 256\n"),
    (["-i", "51200", "-r", "48000"], 2, "missing input file (use - for stdin)\n"),
    (["-i", "51200", "-r", "48000", MISSING], 2, MISSING + ": No such file or directory\n"),
]
# ratios outside the domain: the library's refusal, before a device is asked
REFUSED = [(["-i", "48000", "-r", "1000"], "need M <= 32 L"), (["-i", "1000", "-r", "9000"], "need L <= 8 M"),
           (["-i", "48000", "-r", "48001"], "need 1 <= L <= 1024 and 1 <= M <= 1024"), (["-i", "44100", "-r", "48000", "-T", "256"], "need L T <= 16384")]
NEED_DEVICE = [["-i", "51200", "-r", "48000"], ["-i", "1020000/6", "-r", "48000", "-c", "2"], ["-i", "256000", "-r", "48000", "-T", "64", "-c", "1"]]


def run_cli(args, cwd):
    assert os.path.exists(CLI), "resample_gpu not built (run __graft_entry__.build())"
    p = subprocess.run([CLI] + args, stdin=subprocess.DEVNULL, capture_output=True, cwd=str(cwd), timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


@pytest.mark.parametrize("args,code,stderr", EARLY, ids=[" ".join(c[0]) or "none" for c in EARLY])
def test_cli_early_exits(args, code, stderr, tmp_path):
    assert run_cli(args, tmp_path) == (code, b"", stderr)
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("args,text", REFUSED, ids=[" ".join(c[0]) for c in REFUSED])
def test_cli_refuses_ratios_outside_the_domain_without_a_device(args, text, tmp_path):
    code, stdout, stderr = run_cli(args + [os.devnull], tmp_path)
    assert (code, stdout) == (1, b"") and stderr.startswith("error: ") and stderr.endswith(": " + text + "\n")


@pytest.mark.parametrize("args", NEED_DEVICE, ids=[" ".join(c) for c in NEED_DEVICE])
def test_cli_no_device_is_exit_1_with_the_library_message(fmd, args, tmp_path):
    code, stdout, stderr = run_cli(args + [os.devnull], tmp_path)
    if fmd.device_count() > 0:                               # with a device the empty input is a run of no blocks
        assert (code, stdout) == (0, b"") and "error" not in stderr and stderr.startswith("resample: L / M = ")
    else:
        assert (code, stdout) == (1, b"") and stderr.startswith(NO_DEVICE_TEXT)
        assert stderr.count("\n") == 1 and stderr.endswith("\n")
