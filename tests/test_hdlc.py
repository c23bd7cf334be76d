"""The frame bank (include/fmd.h, fmd_hdlc_*) without a GPU: the plumbing (symbols, NULL arguments, every domain edge with its text and
no device), the test-side definition tests/hdlc_ref.py (packaging, cut invariance), the kernel's per-bit step -- the CRC that runs
with the bits, seven bits late, and the X.25 residue at the flag -- restated in plain Python and held to
ax25_ref.Decoder frame for frame and counter for counter, the frames-per-call bound of the header, afsk_gpu -G's arguments, and the
code object's resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ax25_ref as xr
import hdlc_ref as hr
from digital_cases import CASES, WANT, Model, _body, _find, _soft, cases  # noqa: F401  (the lines and the per-bit step live there)
from test_ax25_domain import EDGES as RATE_EDGES, WRAP
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rtl-sdr-rs_amd")
CLI = os.path.join(PKG, "afsk_gpu")
INVALID_ARG, CAPACITY, UNSUPPORTED, NO_DEVICE = -1, -5, -6, -8
SYMBOLS = ["new", "free", "reset", "check", "kernel_name", "run_batch", "run_device", "inputs", "counts", "frames", "info"]
RATE, CAP, ROWS = "need 4 <= rate / baud <= 64", "need 1 <= frame_cap <= 16", "need n_rows >= 1"


def test_every_symbol_is_declared_exported_and_bound(fmd):
    from rtl_sdr_rs_amd import _ffi, afsk
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fmd_hdlc_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted("fmd_hdlc_" + s for s in SYMBOLS)
    for name in declared:
        assert name in _ffi.PROTOTYPES and hasattr(fmd.lib(), name), name
    assert fmd.Ax25Framer._prefix == "hdlc" and issubclass(fmd.Ax25Framer, _ffi.BankHandle)
    assert callable(fmd.framed) and callable(fmd.decode_rows_gpu) and callable(fmd.decode_rows)
    assert fmd.lib().fmd_version() == 3
    assert C.sizeof(afsk.Ax25Frame) == hr.FRAME_DTYPE.itemsize == 528 and afsk.Ax25Frame.end_sample.offset == 520
    rust = open(os.path.join(ROOT, "rust", "fmd-gpu", "src", "lib.rs")).read()
    assert sorted(set(re.findall(r"pub fn (fmd_hdlc_[a-z0-9_]+)\(", rust))) == declared


def test_null_arguments_are_refused(fmd):
    lib = fmd.lib()
    dev, h = fmd.DeviceConfig(1, -1, 0), C.c_void_p()
    buf = np.zeros(8, np.int16)
    assert lib.fmd_hdlc_new(6000, 1, 1200, 4, None, C.byref(h)) == INVALID_ARG
    assert lib.fmd_hdlc_new(6000, 1, 1200, 4, C.byref(dev), None) == INVALID_ARG
    assert lib.fmd_hdlc_reset(None) == INVALID_ARG and lib.fmd_hdlc_check(None) == INVALID_ARG
    assert lib.fmd_hdlc_inputs(None, C.byref(C.c_uint64(0))) == INVALID_ARG
    assert lib.fmd_hdlc_counts(None, buf.ctypes.data) == INVALID_ARG
    assert lib.fmd_hdlc_frames(None, buf.ctypes.data, 0, buf.ctypes.data) == INVALID_ARG
    assert lib.fmd_hdlc_info(None, buf.ctypes.data) == INVALID_ARG
    assert lib.fmd_hdlc_kernel_name(None, C.create_string_buffer(8), 8) == INVALID_ARG
    assert lib.fmd_hdlc_run_batch(None, buf.ctypes.data, 1, 1) == INVALID_ARG
    assert lib.fmd_hdlc_run_device(None, buf.ctypes.data, 1, 1, None) == INVALID_ARG
    lib.fmd_hdlc_free(None)                                  # a no-op


def _new(fmd, num=6000, den=1, baud=1200, frame_cap=4, rows=1):
    """fmd_hdlc_new's status and error text; a handle that a device granted is freed."""
    dev, h = fmd.DeviceConfig(rows, -1, 0), C.c_void_p(1)
    rc = fmd.lib().fmd_hdlc_new(num, den, baud, frame_cap, C.byref(dev), C.byref(h))
    text = fmd.lib().fmd_last_error().decode()
    assert (rc == 0) == bool(h.value)                        # *out is cleared by every refusal
    if rc == 0:
        fmd.lib().fmd_hdlc_free(h)
    return rc, text


def _rate(t):
    return dict(num=t[0], den=t[1], baud=t[2])


EDGES = [(_rate(i), _rate(o), RATE) for i, o in RATE_EDGES] + [
    (dict(frame_cap=1), dict(frame_cap=0), CAP),
    (dict(frame_cap=16), dict(frame_cap=17), CAP),
    (dict(frame_cap=16), dict(frame_cap=(1 << 32) - 1), CAP),
    (dict(rows=1), dict(rows=0), ROWS),
]


@pytest.mark.parametrize("inside,outside,text", EDGES, ids=["%d" % i for i in range(len(EDGES))])
def test_domain_edges_are_decided_without_a_device(fmd, inside, outside, text):
    rc, msg = _new(fmd, **inside)
    assert rc in (0, NO_DEVICE), (rc, msg)                   # the arguments passed: only the device is left to ask
    assert _new(fmd, **outside) == (UNSUPPORTED, text)
    if "rows" not in outside:                                # the Python class passes the library's refusal on
        a = dict(dict(num=6000, den=1, baud=1200, frame_cap=4), **outside)
        with pytest.raises(fmd.FmdError) as e:
            fmd.Ax25Framer(a["num"], a["den"], a["baud"], a["frame_cap"])
        assert e.value.status == UNSUPPORTED and text in str(e.value)


def test_the_u64_wrap_tuples_and_the_order_of_the_refusals(fmd):
    for t in WRAP:                                           # step at 2^62 and above: 4 step and 64 step wrap in 64 bits
        assert _new(fmd, *t) == (UNSUPPORTED, RATE), t
    assert _new(fmd, 100, 1, 1200, 0, 0) == (UNSUPPORTED, RATE)
    assert _new(fmd, 6000, 1, 1200, 0, 0) == (UNSUPPORTED, CAP)
    assert _new(fmd, 6000, 1, 1200, 4, 0) == (UNSUPPORTED, ROWS)


# ---- the kernel's per-bit step (tests/digital_cases.py: cases, Model) over the lines ---------------------------------
def _hold(name, soft, num, den, cuts=(1, 7, 1000, 333)):
    ref, mod = xr.Decoder(num, den), Model(num, den)
    lo, total = 0, []
    for m in list(cuts) + [len(soft)]:
        want, got = ref.push(soft[lo:lo + m]), mod.push(soft[lo:lo + m])
        assert got == want and mod.info() == ref.info(), (name, lo, m)
        total += want
        lo += m
    return total, ref.info()


@pytest.mark.parametrize("name", sorted(CASES))
def test_per_bit_step_model_equals_the_definition(name):
    total, info = _hold(name, _soft(CASES[name]), 6000, 1)
    total2, info2 = _hold(name, _soft(CASES[name], 11025, 2400), 11025, 2)      # 4.59375 samples per bit
    assert [f["data"] for f in total] == [f["data"] for f in total2] and info == info2
    want = WANT
    if name in want:
        assert (info["frames_ok"], info["bad_fcs"], info["aborts"]) == want[name], info
    if name == "ff-514":
        assert total[0]["data"] == b"\xff" * 512


def test_per_bit_step_model_equals_the_definition_on_noise():
    rng = np.random.default_rng(77)
    for num, den in ((4800, 1), (6000, 1), (76800, 1), (11025, 2), ((1 << 32) - 1, 894784)):
        soft = rng.integers(-32768, 32768, 60000).astype(np.int16)
        soft[20000:40000] = np.repeat(rng.integers(0, 2, 20000 // 4) * 2 - 1, 4) * 5000     # bit-like noise: flags, aborts, stuffing
        total, info = _hold("noise", soft, num, den)
        if num == 4800:
            assert info["bad_fcs"] > 10 and info["aborts"] > 10 and not total


def test_x25_residue_is_f0b8_exactly_for_the_right_fcs():
    rng = np.random.default_rng(3)

    def reg(body):
        crc = 0xFFFF
        for b in body:
            crc ^= b
            for _ in range(8):
                crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
        return crc
    for n in list(range(1, 40)) + [512]:
        d = _body(rng, n)
        good = xr.with_fcs(d)
        assert reg(good) == 0xF0B8
        for k in rng.integers(0, 8 * len(good), 8).tolist():
            bad = bytearray(good)
            bad[k >> 3] ^= 1 << (k & 7)
            assert reg(bad) != 0xF0B8


# ---- the definition's packaging ----------------------------------------------------------------------------------------------------
def test_packaging_count_beyond_frame_cap_and_zeros_behind_len():
    rng = np.random.default_rng(5)
    a, b = _body(rng, 15), _body(rng, 40)
    bits = xr.FLAG * 3 + xr.stuffed_bits(xr.with_fcs(a)) + xr.FLAG + xr.stuffed_bits(xr.with_fcs(b)) + xr.FLAG * 2
    soft = np.stack([_soft(bits), -_soft(bits), np.zeros(5 * len(bits), np.int16)])
    one, four = hr.Framer(6000, frame_cap=1, rows=3), hr.Framer(6000, frame_cap=4, rows=3)
    c1, r1, e1 = one.run(soft)
    c4, r4, e4 = four.run(soft)
    assert c1.tolist() == c4.tolist() == [2, 2, 0] and one.info() == four.info()        # (NRZI: the inverted row reads the same)
    assert r1.shape == (3, 1) and r4.shape == (3, 4) and np.array_equal(r1[:, 0], r4[:, 0])
    assert bytes(r4[0, 0]["data"][:15]) == a and not r4[0, 0]["data"][15:].any() and r4[0, 0]["len"] == 15
    assert bytes(r4[0, 1]["data"][:40]) == b and not r4[0, 1]["data"][40:].any()
    assert r4[0, 0]["end_sample"] < r4[0, 1]["end_sample"] and not r4[0, 2:].view(np.uint8).any() and not r4[2].view(np.uint8).any()
    assert one.info()[0]["frames_ok"] == 2 and one.pos == soft.shape[1]
    assert one.run(soft[:, :0])[0] is c1                     # a call of no samples leaves the last call's
    one.reset()
    assert one.pos == 0 and one.info()[0]["frames_ok"] == 0 and not one.last[0].any()


def test_reference_is_cut_invariant():
    rng = np.random.default_rng(6)
    bits = []
    for k in range(6):
        bits += xr.frame_bits(_body(rng, 15 + 30 * k), flags=2 + k, closing=1)
    soft = np.stack([_soft(bits), _soft(bits[40:] + bits[:40]), rng.integers(-9000, 9000, 5 * len(bits)).astype(np.int16)])
    whole = hr.Framer(6000, frame_cap=16, rows=3)
    counts, rec, every = whole.run(soft)
    assert counts[0] == 6 and counts[1] >= 4
    cut = hr.Framer(6000, frame_cap=16, rows=3)
    got, lo = [[] for _ in range(3)], 0
    for m in (1, 7, 1000, 333, soft.shape[1]):
        c, r, e = cut.run(soft[:, lo:lo + m])
        for row in range(3):
            got[row] += e[row]
            assert len(e[row]) == c[row]
        lo += m
    assert got == every and cut.info() == whole.info() and cut.pos == whole.pos


# ---- how many frames a call can complete -------------------------------------------------------------------------------------------
class Counting(xr.Decoder):
    def __init__(self, *a):
        super().__init__(*a)
        self.takes = []

    def _bit(self, bit, frames):
        self.takes.append(self.n)
        super()._bit(bit, frames)


@pytest.mark.parametrize("num,den,baud", [(4800, 1, 1200), (6000, 1, 1200), (11025, 2, 1200), (76800, 1, 1200), ((1 << 32) - 1, 1, (1 << 30) - 1)])
def test_frames_per_call_bound(fmd, num, den, baud):
    """The header's B(n) bounds the bits any n consecutive samples take, whatever the phase in front of them -- under the input that
    pulls the clock forward at every sample, under noise and under a clean signal -- and (B(n) + 143) / 144 the frames they complete,
    on a line of the shortest frames sharing their flags at the fastest clock."""
    mod, step = num, baud * den
    rng = np.random.default_rng(num % 1000)
    n_all = 6000
    streams = [np.where(np.arange(n_all) % 2 == 0, 1, -1), rng.integers(-5, 5, n_all), np.where(np.arange(n_all) // 3 % 2 == 0, 1, -1)]
    lens = (1, 2, 3, 7, 64, 145, 443, 1000)
    for s in streams:
        d = Counting(num, den, baud)
        d.push(s.astype(np.int16))
        cum = np.zeros(n_all + 1, np.int64)
        cum[np.asarray(d.takes, np.int64) + 1] = 1
        cum = np.cumsum(cum)
        for n in lens:
            B = min(n, (mod - 1 + n * (step + (mod // 2 + 3) // 4)) // mod)
            assert (cum[n:] - cum[:-n]).max() <= B, (n, B)
    assert len(Counting(num, den, baud).takes) == 0
    # the frames: 17-byte frames with no stuffed bit, one flag between two
    one = xr.stuffed_bits(xr.with_fcs(_find(rng, 15, lambda d, s: len(s) == 136)))
    bits = xr.FLAG * 2 + (one + xr.FLAG) * 30
    soft = hr.levels_to_soft(xr.nrzi(bits), mod, step)
    d = xr.Decoder(num, den, baud)
    ends = np.array([f["end_sample"] for f in d.push(soft)], np.int64)
    assert len(ends) == 30
    for n in (1, 144, 145, 443, 600, 2000, 5000):
        worst = max(int(((ends >= a) & (ends < a + n)).sum()) for a in ends)     # the window that starts on a closing sample
        assert worst <= fmd.ax25_max_frames(num, den, baud, n), n
    assert fmd.ax25_max_frames(6000, 1, 1200, 1) == 1 and fmd.ax25_max_frames(6000, 1, 1200, 0) == 0


# ---- afsk_gpu -G ---------------------------------------------------------------------------------------------------------------------
TAPS = "need 2 <= T <= 64"
EARLY = [(["-G", os.devnull], 2, "need -r rate\n"), (["-G", "-r"], 2, "-r needs a value\n"),
         (["-r", "12000", "-G", os.devnull, "b.s16"], 2, "too many files\n"), (["-G", "-r", "12000", "-D", "0", os.devnull], 2, "bad -D: 0\n")]


def run_cli(args, cwd):
    assert os.path.exists(CLI), "afsk_gpu not built (run __graft_entry__.build())"
    p = subprocess.run([CLI] + args, stdin=subprocess.DEVNULL, capture_output=True, cwd=str(cwd), timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


@pytest.mark.parametrize("args,code,stderr", EARLY, ids=[" ".join(c[0]) for c in EARLY])
def test_cli_g_early_exits(args, code, stderr, tmp_path):
    assert run_cli(args, tmp_path) == (code, b"", stderr)
    assert list(tmp_path.iterdir()) == []


def test_cli_g_refusals_and_no_device(fmd, tmp_path):
    for args in (["-r", "1200", "-G"], ["-G", "-r", "96000"]):
        code, stdout, stderr = run_cli(args + [os.devnull], tmp_path)
        assert (code, stdout) == (1, b"") and stderr.startswith("error: ") and stderr.endswith(": " + TAPS + "\n")
    for args in (["-r", "12000", "-G"], ["-G", "-r", "48000", "-D", "8"]):
        code, stdout, stderr = run_cli(args + [os.devnull], tmp_path)
        if fmd.device_count() > 0:                           # with a device the empty input is no frame
            assert (code, stdout, stderr) == (0, b"", "frames_ok 0 bad_fcs 0 aborts 0\n")
        else:
            assert (code, stdout) == (1, b"") and stderr.startswith("error: no usable gfx950 device: ") and stderr.count("\n") == 1


# ---- the code object -----------------------------------------------------------------------------------------------------------------
def test_code_object_kernel_fits_what_the_design_states(code_objects):  # noqa: F811
    """one kernel, no scratch, no spills, at most 64 VGPRs (eight waves per SIMD by registers), no AGPRs, 8448 bytes of
    static LDS (64 rows x 33 dwords), and no floating-point instruction."""
    ks = {n: k for n, k in code_objects.items() if "fmd_hd::" in n}
    assert sorted(n.split("fmd_hd::")[1].split("(")[0] for n in ks) == ["fmd_hdlc_kernel"], sorted(ks)
    for n, k in ks.items():
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert m["vgpr_count"] <= 64 and m.get("agpr_count", 0) == 0, (n, m)
        ops = [t.split()[0] for t in k["text"]]
        assert not [o for o in ops if re.search(r"_f(16|32|64)\b|_f(16|32|64)_", o)], n
        assert any(o.startswith("ds_read") or o.startswith("ds_load") for o in ops) and any(o.startswith("global_store_byte") for o in ops), n
    from test_receiver import _lds_bytes
    assert _lds_bytes("fmd_hdlc_kernel") == [64 * 33 * 4]
