"""FSK front end of the pager decoder (include/fmd.h, fmd_fsk_*) without a GPU: the plumbing (symbols, NULL arguments, every domain
edge with its text and no device, out_cap), the test-side definition tests/fsk_ref.py against a plain-integer restatement and against
itself under cuts, the equality cases of the rule, the designer in C++ and Python, and the code object's resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fsk_ref as fr
from test_isa_invariants import code_objects  # noqa: F401  (module fixture: the library's gfx950 code objects)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rtl-sdr-rs_amd")
INVALID_ARG, CAPACITY, UNSUPPORTED, NO_DEVICE = -1, -5, -6, -8
SYMBOLS = ["new", "free", "reset", "check", "outputs", "hits", "kernel_name", "out_cap", "run_batch", "run_device"]
SYNC = 0x7CD215D8
OK_CFG = dict(D=2, W=5, shift=4, tap=[5 * j for j in range(32)], sync=SYNC, tol=2, min_corr=1024, hit_cap=16)
PAIRS = [(9600, 1200), (11025, 1200), (12000, 512), (12000, 1200), (12000, 2400), (16000, 1200), (22050, 2400), (24000, 512),
         (24000, 1200), (25600, 2400), (48000, 512), (48000, 2400)]


def test_every_symbol_is_declared_exported_and_bound(fmd):
    from rtl_sdr_rs_amd import _ffi, pocsag
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fmd_fsk_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted("fmd_fsk_" + s for s in SYMBOLS)
    for name in declared:
        assert name in _ffi.PROTOTYPES and hasattr(fmd.lib(), name), name
    assert fmd.FskDemod._prefix == "fsk" and issubclass(fmd.FskDemod, _ffi.RowProcessor)
    assert callable(fmd.fsk_design) and callable(fmd.pages)
    assert fmd.lib().fmd_version() == 3
    assert C.sizeof(pocsag.FskConfig) == 156 and pocsag.FskConfig.tap.offset == 12 and pocsag.FskConfig.sync.offset == 140
    assert C.sizeof(pocsag.FskHit) == 16


def _cfg(**kw):
    from rtl_sdr_rs_amd.pocsag import FskConfig
    c = dict(OK_CFG, **kw)
    cfg = FskConfig()
    cfg.D, cfg.W, cfg.shift, cfg.sync, cfg.tol, cfg.min_corr, cfg.hit_cap = c["D"], c["W"], c["shift"], c["sync"], c["tol"], c["min_corr"], c["hit_cap"]
    cfg.tap[:] = c["tap"]
    return cfg


def test_null_arguments_are_refused(fmd):
    lib = fmd.lib()
    cfg, dev, h = _cfg(), fmd.DeviceConfig(1, -1, 0), C.c_void_p()
    buf = np.zeros(8, np.int16)
    u64, sz = C.c_uint64(0), C.c_size_t(0)
    assert lib.fmd_fsk_new(None, 1, C.byref(dev), C.byref(h)) == INVALID_ARG
    assert lib.fmd_fsk_new(C.byref(cfg), 1, None, C.byref(h)) == INVALID_ARG
    assert lib.fmd_fsk_new(C.byref(cfg), 1, C.byref(dev), None) == INVALID_ARG
    assert lib.fmd_fsk_reset(None) == INVALID_ARG and lib.fmd_fsk_check(None) == INVALID_ARG
    assert lib.fmd_fsk_outputs(None, C.byref(u64), C.byref(u64)) == INVALID_ARG
    assert lib.fmd_fsk_hits(None, None, None) == INVALID_ARG
    assert lib.fmd_fsk_kernel_name(None, C.create_string_buffer(8), 8) == INVALID_ARG
    assert lib.fmd_fsk_run_batch(None, buf.ctypes.data, 1, 1, buf.ctypes.data, 1, C.byref(sz)) == INVALID_ARG
    assert lib.fmd_fsk_run_device(None, buf.ctypes.data, 1, 1, buf.ctypes.data, 1, C.byref(sz), None) == INVALID_ARG
    lib.fmd_fsk_free(None)                                   # a no-op


def _new(fmd, width=1, rows=1, **kw):
    """fmd_fsk_new's status and error text; a handle that a device granted is freed."""
    cfg, dev, h = _cfg(**kw), fmd.DeviceConfig(rows, -1, 0), C.c_void_p()
    rc = fmd.lib().fmd_fsk_new(C.byref(cfg), width, C.byref(dev), C.byref(h))
    text = fmd.lib().fmd_last_error().decode()
    if rc == 0:
        fmd.lib().fmd_fsk_free(h)
    return rc, text


DTEXT, WTEXT, SHIFT, TAP = "need 1 <= D <= 64", "need 1 <= W <= 16", "need shift <= 10 and D W <= 2^shift", "need tap[0] = 0, tap non-decreasing, tap[31] <= 255"
TOL, CORR, CAP = "need tol <= 15", "need 0 <= min_corr <= 2^20", "need 1 <= hit_cap <= 64"


def _taps(last, first=0):
    return [first] + [last // 2] * 15 + [last] * 16


# (inside, outside, the refusal's text): keyword arguments of _new on both sides of every rule's edge
EDGES = [
    (dict(width=1), dict(width=2), "need width 1"),
    (dict(width=1), dict(width=0), "need width 1"),
    (dict(D=1), dict(D=0), DTEXT),
    (dict(D=64, W=16, shift=10), dict(D=65, W=1, shift=10), DTEXT),
    (dict(W=1), dict(W=0), WTEXT),
    (dict(D=1, W=16, shift=4), dict(D=1, W=17, shift=10), WTEXT),
    (dict(shift=10), dict(shift=11), SHIFT),
    (dict(D=2, W=4, shift=3), dict(D=3, W=3, shift=3), SHIFT),
    (dict(D=1, W=1, shift=0), dict(D=2, W=1, shift=0), SHIFT),
    (dict(D=64, W=16, shift=10), dict(D=64, W=16, shift=9), SHIFT),
    (dict(tap=_taps(255)), dict(tap=_taps(256)), TAP),
    (dict(tap=[0] * 32), dict(tap=_taps(9, 1)), TAP),
    (dict(tap=[0] * 31 + [3]), dict(tap=[0, 2, 1] + [3] * 29), TAP),
    (dict(tol=15), dict(tol=16), TOL),
    (dict(min_corr=0), dict(min_corr=-1), CORR),
    (dict(min_corr=1 << 20), dict(min_corr=(1 << 20) + 1), CORR),
    (dict(hit_cap=1), dict(hit_cap=0), CAP),
    (dict(hit_cap=64), dict(hit_cap=65), CAP),
    (dict(rows=1), dict(rows=0), "need n_rows >= 1"),
]


@pytest.mark.parametrize("inside,outside,text", EDGES, ids=["%d" % i for i in range(len(EDGES))])
def test_domain_edges_are_decided_without_a_device(fmd, inside, outside, text):
    rc, msg = _new(fmd, **inside)
    assert rc in (0, NO_DEVICE), (rc, msg)                   # the arguments passed: only the device is left to ask
    assert _new(fmd, **outside) == (UNSUPPORTED, text)
    if not set(outside) & {"rows", "width"}:                 # the Python class passes the library's refusal on
        c = dict(OK_CFG, **outside)
        with pytest.raises(fmd.FmdError) as e:
            fmd.FskDemod(c["D"], c["W"], c["shift"], c["tap"], c["sync"], c["tol"], c["min_corr"], c["hit_cap"])
        assert e.value.status == UNSUPPORTED and text in str(e.value)


def test_out_cap_bounds_a_calls_outputs_from_every_stream_position(fmd):
    lib = fmd.lib()
    assert [lib.fmd_fsk_out_cap(0, n) for n in (0, 5)] == [0, 0]
    for D in (1, 2, 3, 19, 64):
        for n in (0, 1, D - 1, D, D + 1, 655, 1024, 4097):
            cap = lib.fmd_fsk_out_cap(D, n)
            assert cap == -(-n // D) + 1
            assert max((p + n) // D - p // D for p in range(2 * D)) == -(-n // D) < cap


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def _cfgs():
    rng = np.random.default_rng(5)
    for D, W, last in ((1, 1, 31), (2, 4, 155), (3, 5, 40), (9, 5, 255), (64, 16, 90)):
        yield fr.random_cfg(rng, D, W, last)


@pytest.mark.parametrize("cfg", list(_cfgs()), ids=lambda c: "D%d-W%d" % (c.D, c.W))
def test_reference_is_cut_invariant_and_equals_the_plain_integer_definition(cfg):
    rng = np.random.default_rng(cfg.D * 100 + cfg.W)
    rows, n = 3, min(40000, 900 * cfg.D + 7)
    x = fr.laid_signal(rng, cfg, rows, n)
    x[2] = rng.integers(-32768, 32768, n)
    whole = fr.FskDemod(cfg, rows)
    out, counts, rec = whole.run(x)
    total = 0
    for r in range(rows):
        soft, hits = fr.fsk_row(x[r], cfg)
        assert out[r].tolist() == soft and counts[r] == len(hits)
        assert [tuple(int(v) for v in h) for h in rec[r, :min(len(hits), cfg.hit_cap)]] == hits[:cfg.hit_cap]
        assert not rec[r, len(hits):].view(np.uint32).any()
        total += len(hits)
    assert total >= 4 and whole.outputs() == n // cfg.D
    cut = fr.FskDemod(cfg, rows)
    parts, hits, lo, k, sums = [], [[] for _ in range(rows)], 0, 0, np.zeros(rows, np.int64)
    for m in (1, 7, 1000, 333, n):
        o, c, rc = cut.run(x[:, lo:lo + m])
        sums += c
        for r in range(rows):
            hits[r] += [(int(h["k_rel"]) + k, int(h["d"]), int(h["corr"]), int(h["thr"])) for h in rc[r, :int(c[r])]]
        parts.append(o)
        lo, k = lo + m, k + o.shape[1]
    assert np.array_equal(np.concatenate(parts, axis=1), out)
    assert sums.tolist() == counts.tolist()
    for r in range(rows):                                    # (the uncut call kept its first hit_cap records: a prefix of the cut calls')
        want = [tuple(int(v) for v in h) for h in rec[r, :min(int(counts[r]), cfg.hit_cap)]]
        assert hits[r][:len(want)] == want and (len(hits[r]) == counts[r] or counts[r] > cfg.hit_cap)


def _one(cfg, soft):
    """the definition's verdict on the newest k of a row whose soft decisions are `soft` (D = W = 1, shift 0: x is soft)"""
    d = fr.FskDemod(cfg, 1)
    out, counts, rec = d.run(np.asarray(soft, np.int16)[None])
    last = [h for h in rec[0, :counts[0]] if h["k_rel"] == len(soft) - 1]
    return (int(last[0]["d"]), int(last[0]["corr"]), int(last[0]["thr"])) if last else None


def test_the_equality_cases_of_the_rule():
    tap = np.arange(32, dtype=np.uint32)
    word = lambda w, a, b=None: [a if (w >> (31 - i)) & 1 else (-a if b is None else b) for i in range(32)]   # noqa: E731
    cfg = fr.Cfg(1, 1, 0, tap, SYNC, 2, 1024, 64)
    ones = bin(SYNC).count("1")
    # C == min_corr hits, min_corr - 1 does not: soft +-a gives C = 32 a
    assert _one(cfg, word(SYNC, 32)) == (0, 1024, 32 * (2 * ones - 32)) and _one(cfg._replace(min_corr=1025), word(SYNC, 32)) is None
    # d == tol hits, tol + 1 does not; the same from the other side at 32 - tol
    two, three = SYNC ^ 0x00010001, SYNC ^ 0x00010101
    assert _one(cfg, word(two, 1000))[0] == 2 and _one(cfg, word(three, 1000)) is None
    inv = _one(cfg, word(two ^ 0xFFFFFFFF, 1000))
    assert inv[0] == 30 | 1 << 31 and inv[1] < 0 and _one(cfg, word(three ^ 0xFFFFFFFF, 1000)) is None
    assert _one(cfg._replace(tol=3), word(three ^ 0xFFFFFFFF, 1000))[0] == 29 | 1 << 31
    # 32 soft == thr gives bit 0: 16 samples at +a, 15 at -a and one at exactly the mean, 32 v = sum -> v = a / 31, a = 31 * 8
    w16 = 0xFFFF0000
    soft = word(w16, 248)
    soft[16] = 8                                             # a sample whose 32-fold is the sum: 16 * 248 - 15 * 248 + 8 = 256 = 32 * 8
    c = fr.Cfg(1, 1, 0, tap, w16, 0, 0, 64)
    assert sum(soft) == 32 * 8 and _one(c, soft) == (0, 16 * 248 + 15 * 248 - 8, 256)
    soft[16] = 9                                             # above the mean: bit 1, one bit off
    assert _one(c, soft) is None and _one(c._replace(tol=1), soft)[0] == 1


def test_hit_cap_1_under_four_hits_and_the_inverted_signal():
    rng = np.random.default_rng(9)
    tap = (5 * np.arange(32)).astype(np.uint32)
    cfg = fr.Cfg(2, 5, 4, tap, SYNC, 2, 35000, 1)            # (five soft samples see the word; the weakest stays below min_corr)
    bits = [(SYNC >> b) & 1 for b in range(31, -1, -1)]
    x = np.concatenate([np.zeros(100), np.repeat(np.where(np.array(bits) == 1, 3000, -3000), 10), np.zeros(100)]) + 500
    x = (x + rng.normal(0, 200, x.shape)).astype(np.int16)
    out, counts, rec = fr.FskDemod(cfg, 1).run(x[None])
    allr = fr.FskDemod(cfg._replace(hit_cap=16), 1).run(x[None])
    assert counts[0] == allr[1][0] == 4
    assert rec.shape == (1, 1) and rec[0, 0] == allr[2][0, 0] and not rec[0, 0]["d"] >> 31
    ks = allr[2][0, :counts[0]]["k_rel"].astype(np.int64)
    assert (np.diff(ks) == 1).all()                          # one sync word: consecutive k around the bit's centre
    inv = fr.FskDemod(cfg._replace(hit_cap=16), 1).run((1000 - x.astype(np.int64)).astype(np.int16)[None])
    assert inv[1][0] == counts[0] and (inv[2][0, :counts[0]]["d"] >> 31).all()
    assert np.abs(inv[2][0]["corr"].astype(np.int64) + allr[2][0]["corr"]).max() <= 32     # (the shift floors: not an exact mirror)
    assert np.array_equal(inv[2][0]["k_rel"], allr[2][0]["k_rel"])


# ---- the designer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe_exe(fmd, tmp_path_factory):
    fmd.lib()
    exe = str(tmp_path_factory.mktemp("probe") / "pocsag_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "pocsag_probe.cpp"), "-o", exe, "-L", PKG, "-lfmd_hip", "-Wl,-rpath," + PKG],
                   check=True, timeout=300)
    return exe


@pytest.mark.parametrize("rate,baud", PAIRS, ids=["%d-%d" % p for p in PAIRS])
def test_design_in_cpp_and_python(fmd, probe_exe, rate, baud):
    d = fmd.fsk_design(rate, baud)
    out = subprocess.run([probe_exe, "design", str(rate), str(baud)], check=True, capture_output=True, timeout=120).stdout.decode().split()
    assert [int(v) for v in out] == [d.D, d.W, d.shift, d.sync, d.tol, d.min_corr, d.hit_cap] + d.tap.tolist()
    assert (d.sync, d.tol, d.min_corr, d.hit_cap) == (SYNC, 2, 1024, 16)
    assert d.D == max(1, int(rate / (5 * baud) + 0.5)) and abs(d.D * d.W - rate / baud) <= d.D / 2
    assert 1 << d.shift >= d.D * d.W > (1 << d.shift) // 2 and d.tap[0] == 0 and d.tap[31] <= 255
    assert np.abs(d.tap - np.arange(32) * rate / (baud * d.D)).max() <= 0.5
    rc, msg = _new(fmd, D=d.D, W=d.W, shift=d.shift, tap=d.tap.tolist())
    assert rc in (0, NO_DEVICE), msg


def test_design_at_chosen_pairs_and_its_refusals(fmd, probe_exe):
    assert [tuple(fmd.fsk_design(r, b)[:3]) for r, b in ((9600, 1200), (12000, 2400), (24000, 1200), (48000, 512))] == [
        (2, 4, 3), (1, 5, 3), (4, 5, 5), (19, 5, 7)]
    assert fmd.fsk_design(12000).tap.tolist()[:4] == [0, 5, 10, 15]
    for rate, baud in ((200000, 512), (1000, 2400), (500000, 1200)):
        with pytest.raises(ValueError):
            fmd.fsk_design(rate, baud)
        out = subprocess.run([probe_exe, "design", str(rate), str(baud)], check=True, capture_output=True, timeout=120).stdout.decode()
        assert out == "refused\n"
    with pytest.raises(ValueError):
        fmd.fsk_design(0)


def test_cpp_fsk_demod_passes_the_librarys_argument_checks_on(probe_exe):
    out = subprocess.run([probe_exe], check=True, capture_output=True, timeout=120).stdout.decode()
    probe = {line.split()[0]: int(line.split()[1]) for line in out.splitlines()}
    inside = {k: v for k, v in probe.items() if k in ("defaults", "largest")}
    assert len(inside) == 2 and all(v in (0, NO_DEVICE) for v in inside.values()), probe
    outside = {k: v for k, v in probe.items() if k not in inside}
    assert sorted(outside) == ["D_65", "W_17", "hit_cap_65", "min_corr_neg", "rows_0", "shift_11", "shift_2", "tap_256", "tol_16", "width_2"]
    assert all(v == UNSUPPORTED for v in outside.values()), probe


def test_code_object_kernel_fits_what_the_design_states(code_objects):  # noqa: F811
    """one kernel, no scratch, no spills, at most 128 VGPRs (four waves per SIMD by registers), and static LDS (the two
    rings of four rows, the taps and signs) that with the largest staging buffer (4 rows x 64 x 64 int16 of dynamic LDS) stays
    inside 64 KiB."""
    ks = {n: k for n, k in code_objects.items() if "fmd_fk::" in n}
    assert sorted(n.split("fmd_fk::")[1].split("(")[0] for n in ks) == ["fmd_fsk_kernel"], sorted(ks)
    for n, k in ks.items():
        m = k["meta"]
        assert m.get("private_segment_fixed_size") == 0, (n, m)
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, (n, m)
        assert m["vgpr_count"] <= 128, (n, m)
    from test_receiver import _lds_bytes
    lds = sorted(_lds_bytes("fmd_fsk_kernel"))
    assert len(lds) == 1 and lds[0] + 4 * 64 * 64 * 2 <= 65536, lds
