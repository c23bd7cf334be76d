"""The case table of the FIR and fused FIR-demod kernels (tests/fir_cases.py) without a GPU: the table's planner constants are the
sources', its kernel names are the shipped code object's, every class the domain sweep finds has a case, every (family, edge) pair
of the table contains what it claims, and two independent references agree on every case -- the C oracle against an int64 numpy
convolution of the rotated, centred stream (and, for the fused chain, that convolution -> floor shift -> tests/pyref.py's
discriminator and resampler, fed call by call).  tests/test_gpu_fir_domain.py then holds the kernels to the claims."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import fir_cases as fc
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-sdr-rs_amd", "csrc")
LIB = os.path.join(ROOT, "rtl-sdr-rs_amd", "libfmd_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
FIR, FUSED = fc.deterministic()
PYREF_MAX = 12000                                                  # filter outputs per case and channel that the per-sample Python loop still takes


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def shipped(text):
    """The text without its `#ifdef FMD_EXPERIMENT ... #endif` blocks (an #else branch is the shipped one and stays)."""
    out, skip, depth = [], False, 0
    for ln in text.splitlines():
        s = ln.strip()
        if s.startswith("#ifdef FMD_EXPERIMENT"):
            skip, depth = True, 1
            continue
        if skip and s.startswith(("#if", "#ifdef", "#ifndef")):
            depth += 1
        elif skip and s.startswith("#else") and depth == 1:
            skip = False
            continue
        elif s.startswith("#endif") and (skip or depth):
            depth -= 1
            if depth == 0:
                skip = False
            continue
        if not skip:
            out.append(ln)
    return "\n".join(out)


# ---- the table matches the sources ------------------------------------------------------------------------------------------------------

def test_table_matches_the_sources():
    fir, fd = src("fmd_fir.hip"), src("fmd_firdemod.hip")
    cases = [(int(a), int(b)) for a, b in re.findall(r"case (\d+): launch_mfma<(\d+)>", fir)]
    assert all(a == b for a, b in cases) and "default: launch_mfma<8>" in fir
    assert tuple(sorted({a for a, _ in cases} | {8})) == fc.NKU
    cases = [(int(a), int(b)) for a, b in re.findall(r"case (\d+): launch<(\d+)>", fd)]
    assert all(a == b for a, b in cases) and "default: launch<8>" in fd
    assert tuple(sorted({a for a, _ in cases} | {8})) == fc.NKU
    # the column parameters and mappings launch<> dispatches to in the shipped library
    body = fd[fd.index("void launch(const FirDemodLaunch& L"):fd.index("struct fmd_firdemod {")]
    assert "FMD_EXPERIMENT" in body
    body = shipped(body)
    regx = {}
    for k, n in re.findall(r"FD_REGX\(fmd_firdemod_(\w+)_kernel, (\d+)\)", body):
        regx.setdefault(k, set()).add(int(n))
    assert regx == {"regs": set(fc.FD_NG["regs"]), "reg1s": set(fc.FD_NG["reg1s"])}
    assert {int(n) for n in re.findall(r"FD_REG\((\d+)\)", body)} == set(fc.FD_NG["reg"])
    assert {int(n) for n in re.findall(r"fmd_firdemod_kernel<NKU, (\d)>", body)} == set(fc.FD_RS)
    # the digit forms of the FIR
    assert {int(n) for n in re.findall(r"launch_mfma_d<NKU, (\d)>", fir)} | {int(n) for n in re.findall(r"fmd_fir_mfma_kernel<NKU, false, (\d)>", fir)} == {1, 2, 3}
    assert int(re.search(r"constexpr uint32_t kFdRows = (\d+);", fd).group(1)) == fc.FD_ROWS
    assert int(re.search(r"constexpr int kFirGroupsPerWave = (\d+);", fir).group(1)) == fc.FIR_GROUPS_PER_WAVE
    row = re.search(r"static const uint32_t budget\[13\] = \{([^}]*)\};", fd).group(1)
    assert tuple(int(x) for x in row.split(",")) == fc.FD_BUDGET
    assert int(re.search(r"size_t lds_budget = (\d+);", fd).group(1)) == fc.FD_LDS
    assert re.search(r"constexpr uint32_t kMaxOutputs = 64u \* 4u \* kGroupsPerWave;", fd) and re.search(r"constexpr int kGroupsPerWave = 4;", fd)
    assert fc.FD_MAX_OUTPUTS == 1024
    # the launch bounds that make instantiations different code: NKU 7 in the FIR, the table flag and NG 6 in the register forms
    assert "NKU <= 6 ? 8 : (NKU == 7 ? 6 : 4)" in fir and "fd_reg_blocks(NKU, NG, ROWS)" in fd


def shipped_kernel_names():
    """The demangled kernel names of the gfx950 code objects in the shipped library, read as tests/test_isa_invariants.py reads them."""
    if not os.path.exists(LIB):
        pytest.fail("libfmd_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    tmp = tempfile.mkdtemp(prefix="fmd_fir_names_")
    try:
        shutil.copy(LIB, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        cos = sorted(f for f in os.listdir(tmp) if "gfx950" in f)
        assert cos, "no gfx950 code object in the library"
        syms = set()
        for co in cos:
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], cwd=tmp, check=True, capture_output=True, text=True).stdout
            syms |= {m.group(1) for m in re.finditer(r"^\s*-?\s*\.name:\s*(_Z\S+)\s*$", notes, re.M)}
        syms = sorted(syms)
        return subprocess.run(["c++filt"] + syms, capture_output=True, text=True, check=True).stdout.splitlines()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def unreachable():
    """Kernels the shipped library instantiates (every launch<> / launch_mfma<> arm exists for every NKU) and no shape of the domain
    reaches -- by the sweep, and for these reasons."""
    out = set()
    # the conflict-free LDS layout: launch_mfma_d compiles both arms, fmd_fir::swz is a knob of the experiment build
    out |= {"fmd_fir_mfma_kernel<%d, true, %d>" % (n, d) for n in fc.NKU for d in (1, 2)}
    # eight outputs per column at decimation >= 8 span at least two K chunks
    out |= {"fmd_fir_mfma_kernel<1, false, 3>"}
    for rows in ("true", "false"):
        out |= {"fmd_firdemod_%s_kernel<1, %d, %s>" % (k, ng, rows) for k in ("regs", "reg1s") for ng in (4, 6, 8)}
        # the dense kernel takes an EVEN column parameter only when the split / one-digit plan does not fit one K pass: 201 ... 232 taps,
        # which are 8 K chunks -- fmd_firdemod_reg_kernel<5, 8, true>, which tests/test_isa_invariants.py names, is one of these
        out |= {"fmd_firdemod_reg_kernel<%d, %d, %s>" % (n, ng, rows) for n in range(1, 8) for ng in (4, 6, 8)}
    return out


def sampled_tableless(claimed):
    """Reachable, and claimed by sample only: the table-less twin <..., false> of every register-form kernel runs on a call of more than
    160 tiles (megabytes per channel).  The table runs it per family at the smallest and the largest column parameter."""
    return {n.replace(", true>", ", false>") for n in claimed if n.endswith(", true>")} - claimed


def test_table_matches_the_shipped_code_object():
    """An instantiation added later without a case fails here; so does a case whose kernel the library does not contain."""
    names = set()
    for n in shipped_kernel_names():
        m = re.search(r"\(anonymous namespace\)::(fmd_fir(?:demod)?_\w*kernel(?:<[^>]*>)?)\(", n)
        if m:
            names.add(m.group(1))
    assert len(names) > 100, len(names)
    claimed = {k.kernel.split("::")[-1] for c in FIR + FUSED for k in c.calls}
    helper = {"fmd_fir_hist_kernel"}                               # the history copy behind the vector-pipe kernel and behind calls that emit nothing
    assert "fmd_firdemod_reg_kernel<5, 8, true>" in names and "fmd_firdemod_reg_kernel<5, 8, true>" in unreachable()
    assert not claimed & unreachable()
    extra = sampled_tableless(claimed)
    assert len({n for n in claimed if n.endswith(", false>")}) == 8 and extra
    assert names == claimed | unreachable() | extra | helper, (sorted(names - claimed - unreachable() - extra - helper),
                                                               sorted((claimed | unreachable() | extra | helper) - names))


# ---- every class, every edge ------------------------------------------------------------------------------------------------------------

def test_every_class_of_the_sweep_has_a_case():
    sf, sd = fc.sweep_fir(), fc.sweep_fused()
    old_fir, old_fused = fc.legacy_reach()
    got_fir = {c.sel.cls for c in FIR if "class" in c.tags}
    got_fused = {c.sel.cls for c in FUSED if "class" in c.tags}
    print("FIR: %d reachable classes (%d matrix-core + the vector-pipe kernel), the named shapes reached %d, the table reaches %d" % (
        len(sf), len(sf) - 1, len(old_fir & set(sf)), len(got_fir)))
    for fam in fc.FD_FAMILIES:
        print("fused %s: %d reachable classes" % (fam, sum(c[0] == fam for c in sd)))
    print("fused: %d reachable classes, the named shapes reached %d, the table reaches %d" % (len(sd), len(old_fused & set(sd)), len(got_fused)))
    assert got_fir == set(sf) and got_fused == set(sd)
    assert len(sf) == 32 and len(sd) == 77
    # what the lists of launch<> imply: every NKU in every family, except where the plan cannot be that short
    assert {c[1] for c in sf if c[0] == "mfma1"} == set(fc.NKU) and {c[1] for c in sf if c[0] == "mfma3"} == set(fc.NKU[1:])
    assert {(c[1], c[2]) for c in sd if c[0] == "reg"} == {(n, g) for n in fc.NKU for g in (5, 7)} | {(8, g) for g in (4, 6, 8)}
    for fam in ("regs", "reg1s"):
        assert {(c[1], c[2]) for c in sd if c[0] == fam} == {(n, g) for n in fc.NKU[1:] for g in fc.FD_NG[fam]}
    # the class case sits at the smallest shape of its class
    for c in FIR:
        if "class" in c.tags:
            assert (c.T, c.M) == sf[c.sel.cls][0][:2], fc.describe(c)
    # the sparse form's clamp of the groups per tile (> 8 -> 8) cannot bind inside the domain: decimation 8 gives exactly 8
    assert max(c.sel.groups for c in FIR if c.sel.form == 3) == 8 and all(16384 // (256 * M) <= 8 for M in range(8, 65, 2))


def zero_run(taps):
    best = run = 0
    for v in taps:
        run = run + 1 if v == 0 else 0
        best = max(best, run)
    return best


def taps_hold(case):
    t, k = case.taps.astype(np.int64), case.tapkind
    if k == "pm127":
        return t.max() == 127 and t.min() == (-127 if case.T > 1 else 127)
    if k == "pm2047":
        return t.max() == 2047 and t.min() == (-2047 if case.T > 1 else 2047)
    if k == "p128":
        return t.max() == 128 and t.min() >= -127
    if k == "m128":
        return t.min() == -128 and t.max() <= 127
    if k == "split":
        return set(fc.SPLIT_EDGES) <= set(t.tolist())
    if k in ("pos8", "pos12"):
        return t.min() > 0 and t.max() == (127 if k == "pos8" else 2047)
    if k in ("neg8", "neg12"):
        return t.max() < 0 and t.min() == (-127 if k == "neg8" else -2047)
    if k in ("runs8", "runs12"):
        # (a class of one or two K chunks has no room for a run longer than a chunk: there, every tap between the ends is zero)
        return zero_run(t) > 32 or (case.T < 48 and zero_run(t) == case.T - 2)
    if k == "ones":
        return case.T == case.M and np.all(t == 1)
    return k == "bound"


def test_fir_edges_per_family():
    sf = fc.sweep_fir()
    for fam in fc.FIR_FAMILIES:
        nkus = fc.family_nkus(sf, fam)
        for nku in {nkus[0], nkus[-1]}:
            mine = [c for c in FIR if c.sel.family == fam and c.sel.nku == nku and "edge" in c.tags]
            assert {c.nch for c in mine} == set(fc.CHANNELS), (fam, nku)
            kinds = fc.TAPS8 if fam == "mfma1" else fc.TAPS12 if fam != "valu" else fc.TAPS8 + fc.TAPS12
            assert {c.tapkind for c in mine} == set(kinds), (fam, nku)
            # both window parities, wherever the class has at least 6 taps at such a decimation: the highest NKU always has, the lowest
            # not always (one K chunk of the one-digit form: 7 M + T <= 32, decimation 2 alone; two of the split form: decimation 8 alone)
            assert {(c.M // 2) % 2 for c in mine} == {p for p in (0, 1) if fc.fir_pick(fam, nku, bool(p))} >= ({0, 1} if nku == nkus[-1] else set()), (fam, nku)
            assert mine
            for c in mine:
                assert taps_hold(c) and c.T >= 6, fc.describe(c)
                assert (fam == "mfma1") == (np.abs(c.taps.astype(np.int64)).max() <= 127) or fam == "valu", fc.describe(c)
                by = {k.label: k for k in c.calls}
                ot = c.sel.out_tile
                assert by["nothing"].n_out == 0 and by["nothing"].nbytes == 8 and by["one"].n_out == 1, fc.describe(c)
                if c.M >= 4:
                    assert (by["tile-1"].n_out, by["tile"].n_out, by["tile+1"].n_out) == (ot - 1, ot, ot + 1), fc.describe(c)
                    assert (by["tile-1"].tiles, by["tile"].tiles, by["tile+1"].tiles) == (1, 1, 2)
                assert by["three-tiles"].tiles == 3 and by["three-tiles"].n_out % ot, fc.describe(c)
                assert by["short"].nbytes == 8 and by["short"].n_out >= 1 and by["short"].short and 4 * c.sel.Hw > 8, fc.describe(c)
                assert {k.kind for k in c.calls} == set(fc.KINDS)
                emitting = [k for k in c.calls if k.n_out]
                if (c.M // 2) % 2:
                    assert {k.par_first for k in emitting} == {0, 1} and all(k.par_step == 1 for k in emitting), fc.describe(c)
                else:
                    assert {k.par_first for k in emitting} == {0} and all(k.par_step == 0 for k in emitting)
            assert any(c.M >= 4 for c in mine) or (fam, nku) == ("mfma1", 1)       # (one K chunk with >= 6 taps: decimation 2 only)
    # same-sign taps meet the all-0 and all-255 streams: the centring constants and the accumulators at their extremes
    assert all({"zeros", "ones"} <= {k.kind for k in c.calls if k.n_out > 1} for c in FIR if c.tapkind.startswith(("pos", "neg")))
    box = [c for c in FIR if "boxcar" in c.tags]
    assert {c.sel.family for c in box} == {"mfma1", "valu"} and all(taps_hold(c) for c in box) and len({c.sel.nku for c in box}) >= 4
    assert {c.sel.family for c in FIR if c.device} == set(fc.FIR_FAMILIES)
    # one digit up to +-127, two from +128 / -128 on
    assert all(c.sel.digits == 1 for c in FIR if c.tapkind == "pm127" and c.M <= 64)
    assert all(c.sel.digits == 2 for c in FIR if c.tapkind in ("p128", "m128") and c.M <= 64)


def test_fused_edges_per_family():
    sd = fc.sweep_fused()
    for fam in fc.FD_FAMILIES:
        nkus = fc.family_nkus(sd, fam)
        for nku in {nkus[0], nkus[-1]}:
            mine = [c for c in FUSED if c.sel.family == fam and c.sel.nku == nku and "edge" in c.tags]
            assert {c.nch for c in mine} == set(fc.CHANNELS), (fam, nku)
            kinds = set(fc.TAPS8) if fam == "reg1s" else set(fc.TAPS12)
            assert {c.tapkind for c in mine} >= kinds, (fam, nku, {c.tapkind for c in mine})
            if fam == "lds0":
                assert {(c.M // 2) % 2 for c in mine} == {0, 1}
            exact = 0
            for c in mine:
                assert taps_hold(c) and c.T >= 6, fc.describe(c)
                by = {k.label: k for k in c.calls}
                kt = c.sel.kt
                first = by["min"]                                  # the shortest legal call: 8 bytes less would hold fewer than 2 windows
                assert all(k.M >= 2 for k in c.calls) and (first.nbytes == 8 or fc.counts(0, c.T, c.M, first.nbytes // 2 - 4)[1] < 2), fc.describe(c)
                if (by["tile-1"].K, by["tile"].K, by["tile+1"].K) == (kt - 1, kt, kt + 1):
                    exact += 1
                    want = (1, 2, 2) if c.sel.ng else (1, 1, 2)    # register form: the trailing partial group counts as a group
                    assert (by["tile-1"].nt, by["tile"].nt, by["tile+1"].nt) == want, fc.describe(c)
                else:
                    assert c.M == 2
                assert by["three-tiles"].nt == 3 and by["three-tiles"].K % kt, fc.describe(c)
                assert by["short"].M in (2, 3) and by["short"].nbytes == 8 * -(-(c.M + 1) // 4), fc.describe(c)
                # ... shorter than the carried history wherever the class has the taps for that (1 - 2 K chunks at decimation 8 have at most 8)
                assert by["short"].short or (nku == nkus[0] and c.M == 8 and c.T <= 8), fc.describe(c)
                assert {k.kind for k in c.calls} == set(fc.KINDS) and all(k.rows for k in c.calls)
                if (c.M // 2) % 2:
                    assert {k.par_first for k in c.calls} == {0, 1}, fc.describe(c)
            assert exact >= len(mine) - 3 and exact >= 2
            # lp_bound exactly 2048 and 2049 for the same filter (sum|h| 2048 and 2049 at shift 7)
            pairs = [c for c in FUSED if "bound2048" in c.tags and c.sel.family == fam and "nku%d" % nku in c.tags]
            if fam == "reg1s" and nku == nkus[0]:
                assert not pairs and 127 * max(m[0] for m in fc.members(sd, fam, nku)) < 2048      # 8 taps of 8 bits cannot sum to 2048
                pairs = [c for c in FUSED if "bound2048" in c.tags and c.sel.family == fam]
            assert pairs, (fam, nku)
            for a in pairs:
                b = FUSED[a.twin]
                assert (a.lp_bound, b.lp_bound, a.shift, b.shift) == (2048, 2049, 7, 7) and a.sel.f32 and not b.sel.f32
                assert np.count_nonzero(a.taps != b.taps) == 1 and (a.T, a.M, a.fast, a.slow) == (b.T, b.M, b.fast, b.slow)
                assert b.sel.family == (fam if fam == "lds0" else "lds1"), fc.describe(b)
    assert all({"zeros", "ones"} <= {k.kind for k in c.calls} for c in FUSED if c.tapkind.startswith(("pos", "neg")))
    # every column parameter at fa == 4 NG exactly and at 4 NG + 3
    ng = {(c.sel.fa, c.sel.small): c.sel for c in FUSED if "ng-edge" in c.tags}
    for n in range(4, 9):
        for plus in (0, 3):
            assert ng[(4 * n + plus, False)].ng == n and ng[(4 * n + plus, False)].family == ("regs" if n % 2 == 0 else "reg")
            assert ng[(4 * n + plus, True)].ng == n - n % 2 and ng[(4 * n + plus, True)].family == "reg1s"
    # reduced resample rates that are a power of two and that are not, inside and outside the register forms; the range condition on sr
    for tag, pow2 in (("sr-pow2", True), ("sr-other", False)):
        got = [c.sel for c in FUSED if tag in c.tags]
        assert all((s.sr & (s.sr - 1) == 0) == pow2 and s.sr > 1 for s in got) and {bool(s.ng) for s in got} == {True, False}
    assert all(c.sel.fa >= 32 and c.sel.ng == 0 and c.sel.family == "lds1" and c.sel.sr * 64 * 30 >= 1 << 24 for c in FUSED if "sr-range" in c.tags)
    assert {c.sel.family for c in FUSED if "ratio-one" in c.tags} == {"lds0", "lds1"} and all(c.fast == c.slow for c in FUSED if "ratio-one" in c.tags)
    # 200 / 201 / 232 / 233 taps at decimation 8
    tb = {(c.sel.small, c.T, c.sel.fa // 4): c.sel for c in FUSED if "tap-boundary" in c.tags}
    assert (tb[(True, 200, 8)].cls, tb[(True, 201, 8)].cls) == (("reg1s", 8, 8), ("reg", 8, 8))
    assert (tb[(True, 200, 7)].cls, tb[(True, 201, 7)].cls) == (("reg1s", 8, 6), ("reg", 8, 7))           # 7 -> 6 only while one digit fits
    assert [tb[(False, T, 8)].cls for T in (200, 201, 232, 233)] == [("regs", 8, 8), ("reg", 8, 8), ("reg", 8, 8), ("lds0", 5, 0)]
    assert [tb[(False, T, 7)].cls for T in (200, 201, 232, 233)] == [("reg", 7, 7), ("reg", 8, 7), ("reg", 8, 7), ("lds0", 5, 0)]    # (the dense plan of 200 taps: 7 K chunks)
    assert tb[(True, 232, 8)].cls == ("reg", 8, 8) and tb[(True, 233, 8)].cls == ("lds0", 5, 0)
    box = [c for c in FUSED if "boxcar" in c.tags]
    assert {c.sel.family for c in box} >= {"lds0", "lds1", "reg1s"} and all(taps_hold(c) and c.shift == 0 for c in box)
    assert {c.sel.family for c in FUSED if c.device} == set(fc.FD_FAMILIES) == {c.sel.family for c in FUSED if c.ckpt}


def test_tableless_cases():
    tl = [c for c in FUSED if "tableless" in c.tags]
    want = {("lds0", 0), ("lds1", 1), ("regs", 4), ("regs", 8), ("reg1s", 4), ("reg1s", 8), ("reg", 5), ("reg", 7), ("reg", 4), ("reg", 8)}
    assert {(c.sel.family, c.sel.cls[2]) for c in tl} == want and len(tl) == len(want)
    for c in tl:
        assert c.nch == 1 and [k.nt for k in c.calls[1:3]] == [fc.FD_ROWS, fc.FD_ROWS + 1] and [k.rows for k in c.calls] == [True, True, False, True]
        assert c.calls[2].kernel.endswith(", false>") == bool(c.sel.ng) and c.calls[3].kernel == c.calls[0].kernel
        # the lowest rate ratio the form admits keeps the calls as short as they can be
        assert c.sel.fa == (4 * c.sel.ng if c.sel.ng else 1)
        print("table-less %-5s NG / RS %d: tile %4d audio samples, %7d and %7d bytes" % (c.sel.family, c.sel.cls[2], c.sel.kt, c.calls[1].nbytes, c.calls[2].nbytes))
        assert 600000 < c.calls[1].nbytes < c.calls[2].nbytes < 5 << 20
    assert all(k.rows for c in FUSED if "tableless" not in c.tags for k in c.calls)
    assert max(k.nbytes * c.nch for c in FIR + FUSED if "tableless" not in c.tags for k in c.calls) < 3 << 20      # these are the only large cases


def test_which_lds_budgets_decide_a_tile():
    """budget[NG] one allocation granule (1280 bytes) smaller changes the tile at NG 5 and 8 only -- there the GPU test sees it in
    tiling(); at NG 4, 6 and 7 the column length (64 (4 NG - 2) - 3 filter outputs) ends the tile search below the budget, so for
    those rows the comparison with the sources above is the check."""
    base = fc.FD_BUDGET
    try:
        for ng in range(4, 9):
            changed = n = 0
            for T in (1, 41, 105, 169, 200, 201, 232):
                for small in (True, False):
                    for fa in range(4 * ng, 4 * ng + 4 if ng < 8 else 40, 1 if ng < 8 else 7):
                        s = fc.fused_select(T, 8, small, True, 8000 * fa, 8000)
                        if s.ng != ng:
                            continue
                        assert s.lds <= base[ng]
                        fc.FD_BUDGET = base[:ng] + (base[ng] - 1280,) + base[ng + 1:]
                        changed += fc.fused_select(T, 8, small, True, 8000 * fa, 8000).kt != s.kt
                        fc.FD_BUDGET = base
                        n += 1
            assert n >= 20 and (changed > n // 2) == (ng in (5, 8)) and (changed == 0) == (ng in (4, 6, 7)), (ng, n, changed)
    finally:
        fc.FD_BUDGET = base
    # the table holds tiles that the budget itself cut: within one granule of it
    assert {c.sel.ng for c in FUSED if c.sel.ng and c.sel.lds > base[c.sel.ng] - 1280} >= {5, 8}


# ---- the references ---------------------------------------------------------------------------------------------------------------------

def check_fir_case(case, oracle):
    """The C oracle against the numpy convolution, on one channel in rotation and the last."""
    chs = sorted({case.i % case.nch, case.nch - 1})
    nps = {ch: fc.FirNp(case.taps, case.M) for ch in chs}
    for ci, iq, exp in fc.reference_fir(case, oracle):
        call = case.calls[ci]
        assert iq.shape == (case.nch, call.nbytes)
        assert all(e.shape == (call.n_out, 2) for e in exp), (fc.describe(case), ci)
        for ch in chs:
            want = nps[ch].feed(iq[ch])
            assert np.abs(want).max(initial=0) < 1 << 31, fc.describe(case)                    # no sum comes near a wrap
            assert np.array_equal(want, exp[ch]), (fc.describe(case), ci, ch)


@pytest.mark.parametrize("fam", fc.FIR_FAMILIES)
def test_fir_references_agree(oracle, fam):
    cases = [c for c in FIR if c.sel.family == fam]
    assert cases
    for case in cases:
        check_fir_case(case, oracle)


def check_fused_case(case, oracle, use_pyref=None):
    """The oracle's composition against numpy convolution -> floor shift -> discriminator + resampler, on one channel in rotation and the
    last: pyref's per-sample loop (on the first of the two) where the case is short enough for it, and fir_cases.ChainNp (the same steps on arrays) on every case --
    so ChainNp is held to pyref wherever both run, and carries the long calls."""
    chs = sorted({case.i % case.nch, case.nch - 1})
    if use_pyref is None:
        use_pyref = sum(k.M for k in case.calls) <= PYREF_MAX
    firs = {ch: fc.FirNp(case.taps, case.M) for ch in chs}
    pds = {ch: pyref.Demod(case.M, case.fast, case.slow) for ch in chs}
    nps = {ch: fc.ChainNp(case.fast, case.slow) for ch in chs}
    panics0 = oracle.lib.fmo_would_panic()
    for ci, iq, audio, states in fc.reference_fused(case, oracle):
        call = case.calls[ci]
        assert iq.shape == (case.nch, call.nbytes)
        assert all(a.size == call.K for a in audio), (fc.describe(case), ci, [a.size for a in audio], call.K)
        for ch in chs:
            y = firs[ch].feed(iq[ch])
            assert y.shape == (call.M, 2) and np.abs(y).max() < 1 << 31                # no sum comes near a wrap
            lp = y >> case.shift                                                       # floor
            assert np.abs(lp).max() <= case.lp_bound <= 16384, fc.describe(case)
            got = nps[ch].feed(lp)
            assert np.array_equal(got, audio[ch]), (fc.describe(case), ci, ch)
            assert nps[ch].state() == states[ch], (fc.describe(case), ci, ch, nps[ch].state(), states[ch])
            if use_pyref and ch == chs[0]:
                pd = pds[ch]
                out = pd.low_pass_real(pd.fm_demod([(int(a), int(b)) for a, b in lp]))
                assert np.array_equal(np.array(out, np.int16), audio[ch]), (fc.describe(case), ci, ch)
                assert (pd.now_lpr, pd.prev_lpr_index, list(pd.demod_pre)) == states[ch], (fc.describe(case), ci, ch)
    assert oracle.lib.fmo_would_panic() == panics0, fc.describe(case)
    return use_pyref


@pytest.mark.parametrize("fam", fc.FD_FAMILIES)
def test_fused_references_agree(oracle, fam):
    cases = [c for c in FUSED if c.sel.family == fam]
    assert cases
    n_py = sum(check_fused_case(case, oracle) for case in cases)
    assert n_py * 2 >= len(cases), (fam, n_py, len(cases))                             # pyref itself ran on most cases of the family


def test_vector_chain_is_pyrefs_on_the_extremes():
    """fir_cases.fast_atan2_np against pyref.fast_atan2 where they could part: zeros, axes, diagonals, the i32 wrap of 4096 * (x -+ |y|)."""
    v = [0, 1, -1, 2, -2, 4095, 4096, -4096, 1 << 18, (1 << 19) - 1, 1 << 19, -(1 << 19), 1 << 27, 2 * 16384 * 16384, -2 * 16384 * 16384, (1 << 29) + 12345]
    ys, xs = np.meshgrid(np.array(v, np.int64), np.array(v, np.int64))
    got = fc.fast_atan2_np(ys.ravel(), xs.ravel())
    assert got.tolist() == [pyref.fast_atan2(int(y), int(x)) for y, x in zip(ys.ravel(), xs.ravel())]


# ---- the random leg -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ["fir", "fused"])
def test_random_leg_is_reproducible_and_inside_the_domain(oracle, op):
    n, source = fc.fuzz_source(op)
    a = [next(source) for _ in range(n)]
    n2, source2 = fc.fuzz_source(op)
    b = [next(source2) for _ in range(n2)]
    assert n >= 40 and [fc.describe(c) for c in a] == [fc.describe(c) for c in b]
    assert all(np.array_equal(x.taps, y.taps) for x, y in zip(a, b))
    assert len({c.sel.cls for c in a}) >= 20 and len({c.sel.family for c in a}) >= (4 if op == "fir" else 5)
    for c in a:
        assert 1 <= c.nch <= 18 and len(c.calls) >= 3 and all(k.nbytes % 8 == 0 for k in c.calls)
        assert 1 <= c.T <= 1024 and c.M % 2 == 0 and np.abs(c.taps.astype(np.int64)).max() <= 2047
        if op == "fused":
            assert 2 <= c.M <= 64 and c.slow <= c.fast and (128 * int(np.abs(c.taps.astype(np.int64)).sum())) >> c.shift <= 16384
            assert all(k.M >= 2 for k in c.calls) and c.shift <= 24
    for c in a[:8]:                                                # the references take the random cases as they take the table's
        check_fir_case(c, oracle) if op == "fir" else check_fused_case(c, oracle, use_pyref=False)
