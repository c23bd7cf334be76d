"""The package bank without a GPU: the definition (tests/packages_ref.py) against the slicer's definition it is built on and against
the shipped host slicer, the bound of R + 1 packages per call, the declarations, the library's refusals that are decided before a
device is touched, the kernel's budget from the shipped code object, and the case table of tests/test_gpu_packages.py checking
itself."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import packages_cases as kc
import packages_ref as ref
import pulse_slice_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED, NO_DEVICE = -1, -6, -8


def random_call(rng, short, long, tol, reset, n):
    pick = lambda: int(rng.choice([short, long, short + tol, long + tol + 1, max(0, short - tol), rng.integers(0, 300), reset, 2 ** 32 - 1]))
    recs = [{"k_rel": int(k), "width": pick(), "gap": pick(), "level": 0} for k in np.sort(rng.integers(0, 5000, n))]
    return recs, {"samples": 0, "state": int(rng.integers(0, 2)), "run": int(rng.integers(0, 400))}


def test_definition_is_the_slicers_definition_and_the_shipped_slicer(fmd):
    """A stream of the bank against a pulse_slice_ref.Slicer and an fmd_pulse_slicer that are emptied after every call (so their 64
    places never fill): the same packages in the same order, with min_bits = 0; min_bits only removes packages."""
    rng = np.random.default_rng(21)
    for trial in range(40):
        modulation = trial % 2
        short, long, tol, reset = int(rng.integers(1, 40)), int(rng.integers(1, 80)), int(rng.integers(0, 8)), int(rng.integers(1, 200))
        min_bits = int(rng.integers(1, 6))
        st, cut = ref.Stream(modulation, short, long, tol, reset), ref.Stream(modulation, short, long, tol, reset, min_bits, 3)
        plain, lib_s = sref.Slicer(modulation, short, long, tol, reset), fmd.PulseSlicer(modulation, short, long, tol, reset)
        samples, seen, short_ones = 0, 0, 0
        for call in range(10):
            n = int(rng.integers(0, 60))
            recs, tot = random_call(rng, short, long, tol, reset, n)
            samples += 5000
            tot["samples"] = samples
            count, got = st.run(n + (5 if call % 4 == 3 else 0), recs + [{"k_rel": 1, "width": 1, "gap": reset, "level": 0}] * 5, n + 5, tot, 5000)
            want = []
            for s in (plain, lib_s):
                s.push(recs, samples - 5000)
                if call % 4 == 3:
                    s.push([{"k_rel": 1, "width": 1, "gap": reset, "level": 0}] * 5, samples - 5000)
                s.idle(tot["state"], tot["run"])
                want.append(s.take())
            assert want[0] == want[1] and len(want[0]) < 64
            assert count == len(got) and got == want[0], (trial, call)
            c2, g2 = cut.run(n + (5 if call % 4 == 3 else 0), recs + [{"k_rel": 1, "width": 1, "gap": reset, "level": 0}] * 5, n + 5, tot, 5000)
            long_enough = [k for k in got if k["n_bits"] >= min_bits]
            assert c2 == len(long_enough) and g2 == long_enough[:3]
            seen += count
            short_ones += len(got) - len(long_enough)
        assert seen and st.info["packages"] == seen and st.info["records"] == cut.info["records"]
        assert cut.info["packages"] == seen and cut.info["skipped"] == short_ones
        assert st.info["open"] == int(plain.cur is not None) and st.info["open_pulses"] == (plain.cur["n_pulses"] if plain.cur else 0)


def test_a_call_of_r_records_closes_at_most_r_plus_one():
    """3000 random configurations: the carried package closes at record 0, each record's own at the next, the last by idle."""
    rng = np.random.default_rng(22)
    worst = -10
    for trial in range(3000):
        modulation, reset = trial % 2, int(rng.integers(1, 50))
        st = ref.Stream(modulation, int(rng.integers(1, 20)), int(rng.integers(1, 40)), int(rng.integers(0, 5)), reset)
        for call in range(3):
            n = int(rng.integers(0, 12))
            recs = [{"k_rel": i, "width": int(rng.integers(0, 40)), "gap": int(rng.choice([0, reset - 1, reset, reset + 5])), "level": 0} for i in range(n)]
            count, got = st.run(n, recs, max(1, n), {"samples": 100, "state": int(rng.integers(0, 2)), "run": int(rng.choice([0, reset]))}, 100)
            assert count == len(got) <= ref.packages_max(n)
            worst = max(worst, count - n)
    assert worst == 1


def test_n_pulses_saturates_on_the_definition():
    """On the definition only: a device test would need 2^32 records."""
    st = ref.Stream(ref.PWM, 10, 30, 3, 100)
    st.run(1, [{"k_rel": 5, "width": 10, "gap": 200, "level": 0}], 1, {"samples": 10, "state": 1, "run": 0}, 10)
    st.slicer.cur["n_pulses"] = 2 ** 32 - 2
    assert st.info["open_pulses"] == 2 ** 32 - 2
    recs = [{"k_rel": 5, "width": 10, "gap": 20, "level": 0}] * 3
    count, got = st.run(3, recs, 3, {"samples": 20, "state": 0, "run": 100}, 10)
    assert count == 1 and got[0]["n_pulses"] == ref.SAT and got[0]["n_bits"] == 4


def test_symbols_and_struct_sizes(fmd):
    from rtl_sdr_rs_amd import _ffi
    rust = open(os.path.join(ROOT, "rust", "fmd-gpu", "src", "lib.rs")).read()
    names = ["fmd_packages_" + n for n in ("new", "free", "reset", "check", "run_batch", "run_bank", "flush", "counts", "pkgs", "info", "kernel_name", "max")]
    for name in names:
        assert name in _ffi.PROTOTYPES and hasattr(fmd.lib(), name) and "pub fn %s(" % name in rust, name
    p = fmd.packages
    assert C.sizeof(fmd.pulses.PulsePackage) == 56 and C.sizeof(p.PackagesTotals) == 40 and C.sizeof(p.PackagesConfig) == 28
    assert "pub struct fmd_packages_config" in rust and "pub struct fmd_packages_totals" in rust
    assert fmd.packages_max(0) == 1 and fmd.packages_max(1024) == 1025 == ref.packages_max(1024)
    assert fmd.PackageBank is p.PackageBank and callable(fmd.sliced)


def test_refusals_in_their_order_before_a_device(fmd):
    lib, P, S = fmd.lib(), fmd.packages.PackagesConfig, fmd.pulses.PulseSlicerConfig
    dev, none, h = fmd.DeviceConfig(2, -1, 0), fmd.DeviceConfig(0, -1, 0), C.c_void_p()
    # each line is wrong in its own place and in every place behind it: the first wrong place decides
    order = [(P(S(2, 0, 0, 0, 0), 257, 0), none, "need modulation 0 (PWM) or 1 (PPM)"),
             (P(S(1, 0, 1, 0, 0), 257, 0), none, "need short_w and long_w >= 1"),
             (P(S(1, 1, 0, 0, 0), 257, 0), none, "need short_w and long_w >= 1"),
             (P(S(0, 1, 1, 0, 0), 257, 0), none, "need reset >= 1"),
             (P(S(0, 1, 1, 0, 1), 257, 0), none, "need min_bits <= 256"),
             (P(S(0, 1, 1, 0, 1), 256, 0), none, "need 1 <= pkg_cap <= 1025"),
             (P(S(0, 1, 1, 0, 1), 256, 1026), none, "need 1 <= pkg_cap <= 1025"),
             (P(S(0, 1, 1, 2 ** 32 - 1, 1), 256, 1025), none, "need n_streams >= 1")]
    for bad, d, text in order:
        assert lib.fmd_packages_new(C.byref(bad), C.byref(d), C.byref(h)) == UNSUPPORTED and not h
        assert lib.fmd_last_error().decode() == text
    # the slicer's texts are the host slicer's
    for bad in (S(2, 0, 0, 0, 0), S(1, 0, 1, 0, 0), S(0, 1, 1, 0, 0)):
        assert lib.fmd_pulse_slicer_new(C.byref(bad), C.byref(h)) == UNSUPPORTED
        text = lib.fmd_last_error().decode()
        assert lib.fmd_packages_new(C.byref(P(bad, 0, 1)), C.byref(dev), C.byref(h)) == UNSUPPORTED and lib.fmd_last_error().decode() == text
    good = P(S(1, 1, 1, 0, 1), 0, 1)
    assert lib.fmd_packages_new(None, C.byref(dev), C.byref(h)) == INVALID_ARG
    assert lib.fmd_packages_new(C.byref(good), None, C.byref(h)) == INVALID_ARG
    assert lib.fmd_packages_new(C.byref(good), C.byref(dev), None) == INVALID_ARG
    buf = (C.c_uint8 * 64)()
    assert lib.fmd_packages_run_batch(None, buf, buf, 1, buf, 8) == INVALID_ARG and lib.fmd_packages_run_bank(None, None, None) == INVALID_ARG
    assert lib.fmd_packages_flush(None, None) == INVALID_ARG and lib.fmd_packages_check(None) == INVALID_ARG
    assert lib.fmd_packages_counts(None, buf) == INVALID_ARG and lib.fmd_packages_info(None, buf) == INVALID_ARG
    assert lib.fmd_packages_pkgs(None, None, 0, None) == INVALID_ARG and lib.fmd_packages_reset(None) == INVALID_ARG
    assert lib.fmd_packages_kernel_name(None, None, 0) == INVALID_ARG
    lib.fmd_packages_free(None)
    if fmd.device_count() == 0:
        assert lib.fmd_packages_new(C.byref(good), C.byref(dev), C.byref(h)) == NO_DEVICE and not h
        with pytest.raises(fmd.FmdError) as ei:
            fmd.PackageBank(2, "pwm", 10, 30, 3, 100)
        assert ei.value.status == NO_DEVICE
    with pytest.raises(ValueError):
        fmd.PackageBank(2, "fsk", 10, 30, 3, 100)


def test_kernel_fits_its_budget():
    """no scratch memory or spills, at most 64 VGPRs, no AGPRs, and no LDS at all: the open package's 256 bits stand in
    eight lanes of the wave."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_digest.py"), "--src", "fmd_packages.hip"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    ks = {r["name"].split("(")[0]: r for r in map(json.loads, p.stdout.splitlines()) if "kernel" in r["name"]}
    assert sorted(ks) == ["fmd_pk::fmd_packages_kernel"]
    k = ks["fmd_pk::fmd_packages_kernel"]
    assert k["scratch"] == 0 and k["vgpr"] <= 64 and k.get("agpr", 0) == 0 and k["lds"] == 0, k
    assert k["static_mix"].get("lds", 0) == 0, k                  # (no LDS instruction either: no cross-lane permute through it)
    src = open(os.path.join(ROOT, "tools", "isa_digest.py")).read()
    assert '"fmd_packages.hip"' in src.split("DEFAULT =")[1].split("]")[0]


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_case_table_checks_itself(name):
    assert kc.case(name).name == name
    kc.check_case(name)


def test_case_names_are_the_cases():
    assert [c.name for c in kc.all_cases()] == kc.CASE_NAMES
