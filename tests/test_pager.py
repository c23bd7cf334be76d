"""The page bank (include/fmd.h, fmd_pager_*) without a GPU: the plumbing (symbols, NULL arguments, every domain edge with its text,
no device, and the order of the refusals), the test-side definition tests/pager_ref.py (packaging, cut invariance), the messages-per-call
bound of the header, the kernel's table of 2048 flip masks against fmd_pocsag_correct, the kernel's step -- the event loop, p(n) formed
from the previous bit's quotient and remainder, the table, the bits laid down as bytes and nibbles (tests/pager_cases.py)
-- restated in plain Python and held to pocsag_ref.Decoder message for message and counter for counter over the rate domain,
pocsag_gpu -G's arguments, and the code object's resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pager_cases as pc
import pager_ref as gr
import pocsag_ref as pr
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rtl-sdr-rs_amd")
CLI = os.path.join(PKG, "pocsag_gpu")
INVALID_ARG, CAPACITY, UNSUPPORTED, NO_DEVICE = -1, -5, -6, -8
SYMBOLS = ["new", "free", "reset", "check", "kernel_name", "run_batch", "run_device", "inputs", "counts", "msgs", "info", "table",
           "max_messages", "fsk_hits"]
RATE, ERRORS, CAP, ROWS = "need 2 <= rate / baud <= 32", "need max_errors <= 2", "need 1 <= msg_cap <= 16", "need n_rows >= 1"
U32 = pc.U32
R5 = pc.RATES["5"]


def test_every_symbol_is_declared_exported_and_bound(fmd):
    from rtl_sdr_rs_amd import _ffi, pocsag
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fmd_pager_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted("fmd_pager_" + s for s in SYMBOLS)
    for name in declared:
        assert name in _ffi.PROTOTYPES and hasattr(fmd.lib(), name), name
    assert fmd.Pager._prefix == "pager" and issubclass(fmd.Pager, _ffi.BankHandle)
    for name in ("paged", "decode_pages_gpu", "decode_pages", "pocsag_max_messages"):
        assert callable(getattr(fmd, name)), name
    assert callable(fmd.FskDemod.hits_device)
    assert fmd.lib().fmd_version() == 3
    assert C.sizeof(pocsag.PocsagMsg) == gr.MSG_DTYPE.itemsize == 352 and gr.MSG_DTYPE.fields["end_sample"][1] == 344
    assert gr.MSG_DTYPE.fields["bits"][1] == 12 and gr.MSG_DTYPE.fields["corrected"][1] == 332 and gr.HIT_DTYPE.itemsize == 16
    rust = open(os.path.join(ROOT, "rust", "fmd-gpu", "src", "lib.rs")).read()
    assert sorted(set(re.findall(r"pub fn (fmd_pager_[a-z0-9_]+)\(", rust))) == declared
    hpp = open(os.path.join(PKG, "csrc", "demod.hpp")).read()
    assert "class Pager" in hpp and "fmd_pager_run_batch" in hpp


def test_null_arguments_are_refused(fmd):
    lib = fmd.lib()
    dev, h = fmd.DeviceConfig(1, -1, 0), C.c_void_p()
    buf = np.zeros(16, np.int16)
    p = buf.ctypes.data
    assert lib.fmd_pager_new(6000, 1, 1200, 1, 4, None, C.byref(h)) == INVALID_ARG
    assert lib.fmd_pager_new(6000, 1, 1200, 1, 4, C.byref(dev), None) == INVALID_ARG
    assert lib.fmd_pager_reset(None) == INVALID_ARG and lib.fmd_pager_check(None) == INVALID_ARG
    assert lib.fmd_pager_inputs(None, C.byref(C.c_uint64(0))) == INVALID_ARG
    assert lib.fmd_pager_counts(None, p) == INVALID_ARG
    assert lib.fmd_pager_msgs(None, p, 0, p) == INVALID_ARG
    assert lib.fmd_pager_info(None, p) == INVALID_ARG
    assert lib.fmd_pager_kernel_name(None, C.create_string_buffer(8), 8) == INVALID_ARG
    assert lib.fmd_pager_run_batch(None, p, 1, 1, p, p, 1) == INVALID_ARG
    assert lib.fmd_pager_run_device(None, p, 1, 1, p, p, 1, None) == INVALID_ARG
    assert lib.fmd_pager_fsk_hits(None, C.byref(h), C.byref(h)) == INVALID_ARG
    assert lib.fmd_pager_table(1, None) == INVALID_ARG
    assert lib.fmd_pager_table(3, p) == UNSUPPORTED and lib.fmd_last_error().decode() == ERRORS
    lib.fmd_pager_free(None)                                 # a no-op


def _new(fmd, num=6000, den=1, baud=1200, max_errors=1, msg_cap=4, rows=1):
    """fmd_pager_new's status and error text; a handle that a device granted is freed."""
    dev, h = fmd.DeviceConfig(rows, -1, 0), C.c_void_p(1)
    rc = fmd.lib().fmd_pager_new(num, den, baud, max_errors, msg_cap, C.byref(dev), C.byref(h))
    text = fmd.lib().fmd_last_error().decode()
    assert (rc == 0) == bool(h.value)                        # *out is cleared by every refusal
    if rc == 0:
        fmd.lib().fmd_pager_free(h)
    return rc, text


def _rate(num, den, baud):
    return dict(num=num, den=den, baud=baud)


EDGES = [
    (_rate(2400, 1, 1200), _rate(2399, 1, 1200), RATE),
    (_rate(38400, 1, 1200), _rate(38401, 1, 1200), RATE),
    (_rate(11025, 2, 1200), _rate(4800, 0, 1200), RATE),
    (_rate(U32, U32 // 2400, 1200), _rate(4800, 1, 0), RATE),
    (_rate(U32, 1, U32 // 2), _rate(U32, 1, U32 // 2 + 1), RATE),                 # step > mod / 2
    (_rate(U32, 1, (U32 + 31) // 32), _rate(U32, 1, (U32 + 31) // 32 - 1), RATE),   # mod > 32 step
    (dict(max_errors=0), dict(max_errors=3), ERRORS),
    (dict(max_errors=2), dict(max_errors=U32), ERRORS),
    (dict(msg_cap=1), dict(msg_cap=0), CAP),
    (dict(msg_cap=16), dict(msg_cap=17), CAP),
    (dict(msg_cap=16), dict(msg_cap=U32), CAP),
    (dict(rows=1), dict(rows=0), ROWS),
]


@pytest.mark.parametrize("inside,outside,text", EDGES, ids=["%d" % i for i in range(len(EDGES))])
def test_domain_edges_are_decided_without_a_device(fmd, inside, outside, text):
    rc, msg = _new(fmd, **inside)
    assert rc in (0, NO_DEVICE), (rc, msg)                   # the arguments passed: only the device is left to ask
    assert _new(fmd, **outside) == (UNSUPPORTED, text)
    if "rows" not in outside:                                # the Python class passes the library's refusal on
        a = dict(dict(num=6000, den=1, baud=1200, max_errors=1, msg_cap=4), **outside)
        with pytest.raises(fmd.FmdError) as e:
            fmd.Pager(a["num"], a["den"], a["baud"], a["max_errors"], a["msg_cap"])
        assert e.value.status == UNSUPPORTED and text in str(e.value)


def test_the_u64_wrap_tuples_and_the_order_of_the_refusals(fmd):
    for t in ((0, 1 << 31, 1 << 31), (U32, U32, U32), (U32, 1 << 31, 1 << 31), (1, U32, U32)):     # step up to 2^64 - 2^33 + 1
        assert _new(fmd, *t) == (UNSUPPORTED, RATE), t
    assert _new(fmd, 100, 1, 1200, 3, 0, 0) == (UNSUPPORTED, RATE)
    assert _new(fmd, 6000, 1, 1200, 3, 0, 0) == (UNSUPPORTED, ERRORS)
    assert _new(fmd, 6000, 1, 1200, 1, 0, 0) == (UNSUPPORTED, CAP)
    assert _new(fmd, 6000, 1, 1200, 1, 4, 0) == (UNSUPPORTED, ROWS)


# ---- the definition's packaging ----------------------------------------------------------------------------------------------------
def _tones(fmd, n, rate=R5, **kw):
    from rtl_sdr_rs_amd.pocsag import POCSAG_IDLE as IDLE, pocsag_codeword as cw
    words = [cw((100 + i) << 2 | i % 4) for i in range(n)] + [IDLE]
    return pc.line(fmd.pocsag_encode(None, preamble=32, words=words + [IDLE] * (-len(words) % 16)), rate, **kw)


def test_packaging_count_beyond_msg_cap_and_zeros_behind_the_bits(fmd):
    rng = np.random.default_rng(5)
    data = rng.integers(0, 2, 60).tolist()
    x, hits = pc.stack([_tones(fmd, 3), _tones(fmd, 3, invert=True), (np.zeros(10, np.int16), []),
                        pc.line(fmd.pocsag_encode([(9, 1, data, "bits")], preamble=32), R5)])
    counts, rec = pc.pack(hits, 0, x.shape[1])
    one, four = gr.Pager(*R5, msg_cap=1, rows=4), gr.Pager(*R5, msg_cap=4, rows=4)
    c1, r1, e1 = one.run(x, counts, rec)
    c4, r4, e4 = four.run(x, counts, rec)
    assert c1.tolist() == c4.tolist() == [3, 3, 0, 1] and one.info() == four.info()      # three closes in one call, msg_cap 1
    assert r1.shape == (4, 1) and r4.shape == (4, 4) and np.array_equal(r1[:, 0], r4[:, 0])
    assert [int(m["address"]) >> 3 for m in r4[0, :3]] == [100, 101, 102] and not r4[0, 3:].view(np.uint8).any()
    assert r4[1, 0]["inverted"] == 1 and not r4[2].view(np.uint8).any()
    m = r4[3, 0]
    assert m["n_bits"] == 60 and np.unpackbits(m["bits"][:8])[:60].tolist() == data
    assert not m["bits"][8:].any() and m["bits"][7] & 0x0F == 0          # zero behind (60 + 7) / 8 bytes, and behind the bits in the last
    assert one.info()[0]["messages"] == 3 and one.pos == x.shape[1]
    assert one.run(x[:, :0])[0] is c1                        # a call of no samples leaves the last call's
    one.reset()
    assert one.pos == 0 and one.info()[0]["messages"] == 0 and not one.last[0].any()


def _cut(ref, x, hits, cuts):
    got, lo = [[] for _ in range(x.shape[0])], 0
    for m in list(cuts) + [x.shape[1]]:
        part = x[:, lo:lo + m]
        counts, rec = pc.pack(hits, lo, part.shape[1])
        c, r, e = ref.run(part, counts, rec)
        for row in range(x.shape[0]):
            got[row] += e[row]
            assert len(e[row]) == c[row]
        lo += part.shape[1]
    return got


def test_reference_is_cut_invariant(fmd):
    rng = np.random.default_rng(6)
    pages = [(int(rng.integers(0, 1 << 21)), int(rng.integers(0, 4)), "page %d of the cut test" % k, "alpha") for k in range(5)]
    x, hits = pc.stack([pc.line(fmd.pocsag_encode(pages, preamble=64), R5), pc.line(fmd.pocsag_encode(pages[::-1], preamble=40), R5, invert=True),
                        (rng.integers(-9000, 9000, 3000).astype(np.int16), [(700, 1, 40000, 10), (1405, 1 << 31, -50000, 0)])])
    whole, cut = gr.Pager(*R5, msg_cap=16, rows=3), gr.Pager(*R5, msg_cap=16, rows=3)
    every = _cut(whole, x, hits, [])
    assert [len(e) for e in every[:2]] == [5, 5]
    assert _cut(cut, x, hits, (1, 7, 1000, 333)) == every and cut.info() == whole.info() and cut.pos == whole.pos


# ---- how many messages a call can complete -----------------------------------------------------------------------------------------
class Closing(pr.Decoder):
    """the decoder, noting the sample at which every message closes"""

    def reset(self):
        super().reset()
        self.closes = []

    def _close(self):
        if self.cur is not None:
            self.closes.append(self.n)
        super()._close()


def _worst(closes, total, n):
    """the most closes in any n consecutive samples"""
    cum = np.zeros(total + 1, np.int64)
    np.add.at(cum, np.asarray(closes, np.int64) + 1, 1)
    cum = np.cumsum(cum)
    return int((cum[n:] - cum[:-n]).max()) if n <= total else int(cum[-1])


BOUND_RATES = [pc.RATES["2"], pc.RATES["3.5"], (11025, 1, 2400), pc.RATES["5"], pc.RATES["32"]]


@pytest.mark.parametrize("rate", BOUND_RATES, ids=["2", "3.5", "4.59", "5", "32"])
def test_messages_per_call_bound(fmd, rate):
    """M(n) of the header bounds the messages that close in any n consecutive samples -- whatever lies in front of them -- on lines
    of nothing but address words with and without the next sync word, on lines that lose and regain the lock, and on noise with
    records of its own."""
    from rtl_sdr_rs_amd.pocsag import pocsag_codeword as cw
    rng = np.random.default_rng(rate[0] % 1000)
    addr = [cw(int(v) << 2 | int(v) % 4) for v in rng.integers(0, 1 << 18, 64)]
    with_sync = fmd.pocsag_encode(None, preamble=32, words=addr)                                  # four batches on end
    one = fmd.pocsag_encode(None, preamble=32, words=addr[:16])
    gaps = np.concatenate([one, np.zeros(100, np.uint8), one[16:], np.zeros(37, np.uint8), one, one[32:]])   # loses and regains the lock
    lines = [pc.line(with_sync, rate), pc.line(one, rate), pc.line(gaps, rate, invert=True)]
    n_noise = 6000 * (rate[0] // (rate[1] * rate[2]))
    noise = np.repeat(rng.integers(0, 2, n_noise // 2 + 1) * 2 - 1, 2)[:n_noise] * 5000
    lines.append((noise.astype(np.int16), [(int(k), 0, 50000, 0) for k in range(50, n_noise, 577 * (rate[0] // (rate[1] * rate[2])))]))
    q = rate[0] // (rate[1] * rate[2])
    sizes = sorted(set(list(range(1, 70)) + [32 * q - 1, 32 * q, 32 * q + 1, 64 * q, 100, 256, 512 * q, 544 * q, 1000, 2048, 4096]))
    seen = 0.0
    for soft, hits in lines:
        d = Closing(*rate, 1)
        d.push(soft, hits)
        assert d.messages == len(d.closes)
        for n in sizes:
            w = _worst(d.closes, len(soft), n)
            m = gr.max_messages(*rate, n)
            assert w <= m, (n, w, m)
            seen = max(seen, w / m)
            assert fmd.pocsag_max_messages(*rate, n) == m
    assert seen >= 0.5                                       # (the lines do press on the bound)
    assert fmd.pocsag_max_messages(6000, 1, 1200, 256) == 3 and fmd.pocsag_max_messages(6000, 1, 1200, 0) == 1
    assert fmd.pocsag_max_messages(100, 1, 1200, 256) == 0
    assert fmd.pocsag_max_messages(6000, 1, 1200, 2400) == 16 and fmd.pocsag_max_messages(6000, 1, 1200, 2401) == 17


# ---- the correction table ------------------------------------------------------------------------------------------------------------
def _lib_table(fmd, e):
    t = np.zeros(2048, np.uint32)
    assert fmd.lib().fmd_pager_table(e, t.ctypes.data) == 0
    return t.tolist()


@pytest.mark.parametrize("e", [0, 1, 2])
def test_correction_table_equals_fmd_pocsag_correct(fmd, e):
    """Every entry: a word with that remainder and parity is corrected by the library's definition to what the flip mask gives, or
    to nothing where the mask is `none`; and every single and double flip of sync, idle and 50 random codewords."""
    from rtl_sdr_rs_amd.pocsag import POCSAG_IDLE, POCSAG_SYNC, pocsag_codeword, pocsag_correct
    t = _lib_table(fmd, e)
    assert t == pc.table(e)
    rng = np.random.default_rng(e)
    base = pocsag_codeword(int(rng.integers(0, 1 << 21)))
    for s in range(1024):                                    # a word for every syndrome and parity: the codeword with those bits flipped
        for par in (0, 1):
            w = base ^ (s << 1)                              # the check bits carry the remainder as it is
            if (bin(w).count("1") & 1) != par:
                w ^= 1
            assert pc.key(w) == s << 1 | par
            m = t[s << 1 | par]
            got = pocsag_correct(w, e)
            assert got == (None if m == pc.NONE else (w ^ m, bin(m).count("1"))), (s, par)
            assert got == pr.correct(w, e)
    words = [POCSAG_SYNC, POCSAG_IDLE] + [pocsag_codeword(int(v)) for v in rng.integers(0, 1 << 21, 50)]
    for cw in words:
        for a in range(32):
            for b in range(a, 32):
                w = cw ^ (1 << a) ^ (1 << b) if b > a else cw ^ (1 << a)
                m = t[pc.key(w)]
                flips = 1 if a == b else 2
                assert (m != pc.NONE and w ^ m == cw) == (flips <= e), (hex(cw), a, b)
                assert pocsag_correct(w, e) == (None if m == pc.NONE else (w ^ m, bin(m).count("1")))
    assert sum(1 for m in t if m != pc.NONE) == (1, 33, 33 + 496)[e]


# ---- the kernel's step over the rate domain ------------------------------------------------------------------------------------------------
def _hold(rate, e, soft, hits, cuts=(1, 7, 1000, 333)):
    """The model and the definition over the same pushes.  It also holds that every bit is read at the sample that makes it due:
    p(1) of a new batch is never behind the sample that anchors it (k + r >= k1 + r after a search; best_k + r >= p544 + r / 2 at slot
    16, since best_k >= p544 - r / 2), so the 64 samples in front of a call, which the handle carries as the definition keeps them,
    are never read."""
    ref, mod = pr.Decoder(rate[0], rate[1], rate[2], e), pc.Model(rate[0], rate[1], rate[2], e)
    lo, total = 0, []
    for m in list(cuts) + [len(soft)]:
        part = soft[lo:lo + m]
        h = [(k - lo, d, c, t) for k, d, c, t in hits if lo <= k < lo + len(part)]
        want, got = ref.push(part, h), mod.push(part, h)
        assert got == want and mod.info() == ref.info() and mod.behind == 0, (rate, e, lo, m)
        total += want
        lo += len(part)
    return total, ref.info()


@pytest.mark.parametrize("name", sorted(pc.RATES))
def test_kernel_step_model_equals_the_definition(fmd, name):
    rate = pc.RATES[name]
    rng = np.random.default_rng(len(name))
    pages = [(1234560, 0, "0123456789", "numeric"), (765437, 3, "The quick brown fox jumps over the lazy dog", "alpha"), (9, 1, "", "tone"),
             (77, 2, rng.integers(0, 2, 2580).tolist(), "bits")]
    clean = fmd.pocsag_encode(pages, preamble=64)
    for e in (0, 1, 2):
        total, info = _hold(rate, e, *pc.line(clean, rate, dc=300, invert=e == 1))
        assert [(m["address"], m["n_bits"]) for m in total] == [(1234560, 40), (765437, 320), (9, 0), (77, 2580)], (name, e)
        bits = clean.copy()
        bits[rng.choice(len(bits) - 64, 40, replace=False) + 64] ^= 1                    # sync words, addresses and message words off
        _hold(rate, e, *pc.line(bits, rate, dc=-200, invert=e == 2), cuts=(333, 1, 1, 2000))
    # noise, with records of its own: windows, locks on nothing, lost locks
    q = rate[0] // (rate[1] * rate[2])
    n = 3000 * q
    soft = (np.repeat(rng.integers(0, 2, n // q + 1) * 2 - 1, q)[:n] * rng.integers(1, 30000, n)).astype(np.int16)
    ks = sorted(set(rng.integers(0, n, 40).tolist()))
    hits = [(k, int(rng.integers(0, 3)) | (int(rng.integers(0, 2)) << 31), int(rng.integers(-99999, 99999)), int(rng.integers(-9999, 9999))) for k in ks]
    total, info = _hold(rate, 1, soft, hits, cuts=(1, 7, 1000, 333))
    assert info["batches"] >= 1


# ---- pocsag_gpu -G ---------------------------------------------------------------------------------------------------------------------
EARLY = [(["-G"], 2, "need -r rate\n"), (["-G", "-r"], 2, "-r needs a value\n"), (["-r", "12000", "-G", os.devnull, "b.s16"], 2, "too many files\n"),
         (["-G", "-r", "12000", "-b", "0", os.devnull], 2, "bad -b: 0\n"), (["-G", "-r", "12000", "-m", "hex"], 2, "bad -m: hex\n")]


def run_cli(args, cwd):
    assert os.path.exists(CLI), "pocsag_gpu not built (run __graft_entry__.build())"
    p = subprocess.run([CLI] + args, stdin=subprocess.DEVNULL, capture_output=True, cwd=str(cwd), timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


@pytest.mark.parametrize("args,code,stderr", EARLY, ids=[" ".join(c[0]) for c in EARLY])
def test_cli_g_early_exits(args, code, stderr, tmp_path):
    assert run_cli(args, tmp_path) == (code, b"", stderr)
    assert list(tmp_path.iterdir()) == []


def test_cli_g_refusals_and_no_device(fmd, tmp_path):
    for args, text in ((["-r", "12000", "-G", "-e", "3"], ERRORS), (["-G", "-r", "12000", "-b", "7000"], None)):
        code, stdout, stderr = run_cli(args + [os.devnull], tmp_path)
        assert (code, stdout) == (1, b"") and stderr.startswith("error: ") and stderr.count("\n") == 1
        assert text is None or stderr.endswith(": " + text + "\n")
        assert run_cli([a for a in args if a != "-G"] + [os.devnull], tmp_path) == (code, stdout, stderr)      # the same refusal without -G
    for args in (["-r", "12000", "-G"], ["-G", "-r", "24000", "-b", "2400", "-e", "0"]):
        code, stdout, stderr = run_cli(args + [os.devnull], tmp_path)
        if fmd.device_count() > 0:                           # with a device the empty input gives no line and zero counters
            assert (code, stdout, stderr) == (0, b"", "messages 0 batches 0 bad_codewords 0 orphans 0\n")
        else:
            assert (code, stdout) == (1, b"") and stderr.startswith("error: no usable gfx950 device: ") and stderr.count("\n") == 1


# ---- the code object -----------------------------------------------------------------------------------------------------------------
def test_code_object_kernel_fits_what_the_design_states(code_objects):  # noqa: F811
    """one kernel, no scratch, no spills, at most 128 VGPRs (four waves per SIMD by registers), no AGPRs, 8192 bytes of
    static LDS (the table), and no floating-point instruction."""
    ks = {n: k for n, k in code_objects.items() if "fmd_pg::" in n}
    assert sorted(n.split("fmd_pg::")[1].split("(")[0] for n in ks) == ["fmd_pager_kernel"], sorted(ks)
    for n, k in ks.items():
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert m["vgpr_count"] <= 128 and m.get("agpr_count", 0) == 0, (n, m)
        ops = [t.split()[0] for t in k["text"]]
        assert not [o for o in ops if re.search(r"_f(16|32|64)\b|_f(16|32|64)_", o)], n
        assert any(o.startswith("ds_read") or o.startswith("ds_load") for o in ops) and any(o.startswith("global_store_byte") for o in ops), n
    from test_receiver import _lds_bytes
    assert _lds_bytes("fmd_pager_kernel") == [2048 * 4]
