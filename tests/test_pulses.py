"""The pulse bank and its slicer without a GPU: the definition (tests/pulses_ref.py) against hand-worked streams and against the loop it
restates, the library's refusals that are decided before a device is touched, the kernels' budget from the shipped code object, the
host slicer against its definition (tests/pulse_slice_ref.py) and under the sanitizers, the sender, the thresholds, and the case table
of tests/test_gpu_pulses.py checking itself."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pulse_slice_ref as sref
import pulses_cases as pc
import pulses_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_LENGTH, UNSUPPORTED, NO_DEVICE = -1, -2, -6, -8


def literal(b, W, lo, hi):
    """The definition as the loop it is written as, over one whole stream: (records in absolute positions, info)."""
    m = ref.magnitude(b).tolist()
    s, run, gap, recs, rises = 0, 0, 0, [], 0
    e_prev = 0
    for i in range(len(m)):
        e = sum(m[max(0, i - W + 1):i + 1])
        new = 1 if e >= hi else 0 if e < lo else s
        if new != s:
            if new:
                gap = min(run, ref.SAT) if recs else 0
                rises += 1
            else:
                recs.append({"p": i, "width": min(run, ref.SAT), "gap": gap, "level": e_prev})
            run, s = 0, new
        run += 1
        e_prev = e
    return recs, {"samples": len(m), "pulses": len(recs), "rises": rises, "state": s, "run": run}


def stream_of_m(values):
    """u8 IQ whose m are the given ones of {1, 1861, 7321}."""
    i_of = {pc.M_QUIET: pc.QUIET, pc.M_MEDIUM: pc.MEDIUM, pc.M_STRONG: pc.STRONG}
    iq = np.full(2 * len(values), 128, np.uint8)
    iq[0::2] = [i_of[v] for v in values]
    return iq


def absolute(st, calls):
    out, pos = [], 0
    for b in calls:
        out += [dict({k: v for k, v in r.items() if k != "k_rel"}, p=pos + r["k_rel"]) for r in st.run(b)[1]]
        pos += len(b) // 2
    return out


def test_symbols_are_declared_everywhere(fmd):
    from rtl_sdr_rs_amd import _ffi
    rust = open(os.path.join(ROOT, "rust", "fmd-gpu", "src", "lib.rs")).read()
    names = ["fmd_pulses_" + n for n in ("new", "free", "reset", "run_batch", "run_device", "check", "counts", "recs", "info", "kernel_name", "tile")]
    names += ["fmd_pulse_slicer_" + n for n in ("new", "free", "push", "idle", "take")]
    for name in names:
        assert name in _ffi.PROTOTYPES and hasattr(fmd.lib(), name) and "pub fn %s(" % name in rust, name
    p = fmd.pulses
    assert C.sizeof(p.PulseRec) == 16 and C.sizeof(p.PulsesTotals) == 40 and C.sizeof(p.PulsesConfig) == 16
    assert C.sizeof(p.PulsePackage) == 56 and C.sizeof(p.PulseSlicerConfig) == 20
    assert pc.M_STRONG == int(ref.magnitude([pc.STRONG, 128])[0]) and pc.M_MEDIUM == int(ref.magnitude([pc.MEDIUM, 128])[0])
    assert int(ref.magnitude([128, 128])[0]) == pc.M_QUIET and int(ref.magnitude([255, 255])[0]) == 65025


def test_hand_worked_stream_at_the_equalities():
    """W = 2, lo = 3722, hi = 9182: e == hi sets, e == lo keeps, e == lo - 1 clears.  m: 1 1 1861 7321 1861 1861 1 1 ..."""
    q, md, sg = pc.M_QUIET, pc.M_MEDIUM, pc.M_STRONG
    b = stream_of_m([q, q, md, sg, md, md, q, q, q, sg, sg, q])
    # e:          1  2  1862 9182 9182 3722 1862 2 2 7322 14642 7322
    st = ref.Stream(2, 3722, 9182)
    count, recs = st.run(b)
    # e[3] == hi: a rise at 3; e[5] == lo: keep; e[6] == lo - 1860 < lo: a fall at 6, level e[5] = 3722; e[9] = 7322 keeps (state 0);
    # e[10] = 14642 rises at 10; e[11] = 7322 keeps: the pulse is open at the end
    assert count == 1 and recs == [{"k_rel": 6, "width": 3, "gap": 0, "level": 3722}]
    assert st.info == {"samples": 12, "pulses": 1, "rises": 2, "state": 1, "run": 2}
    assert ref.Stream(2, 3722, 9183).run(b)[0] == 0          # e == hi - 1 does not set: (then e[10] is the only rise)
    st = ref.Stream(2, 3723, 9182)                           # e[5] == lo - 1 now: the fall comes a sample sooner
    assert st.run(b)[1] == [{"k_rel": 5, "width": 2, "gap": 0, "level": 9182}]
    assert literal(b, 2, 3722, 9182)[0] == [{"p": 6, "width": 3, "gap": 0, "level": 3722}]


def test_lo_equal_hi_and_the_first_gap():
    q, sg = pc.M_QUIET, pc.M_STRONG
    b = stream_of_m([q, q, sg, sg, sg, q, q, sg, q, q])
    st = ref.Stream(1, 5000, 5000)
    count, recs = st.run(b)
    assert recs == [{"k_rel": 5, "width": 3, "gap": 0, "level": sg}, {"k_rel": 8, "width": 1, "gap": 2, "level": sg}]
    assert st.info == {"samples": 10, "pulses": 2, "rises": 2, "state": 0, "run": 2}
    count, recs = st.run(stream_of_m([q, sg, q, q]))          # the gap counts across the call: 2 + 1 samples since the fall at 8
    assert recs == [{"k_rel": 2, "width": 1, "gap": 3, "level": sg}] and st.info["run"] == 2
    st.reset()
    assert st.info == {"samples": 0, "pulses": 0, "rises": 0, "state": 0, "run": 0} and st.run(b)[1][0]["gap"] == 0


def test_box_of_one_and_of_sixty_four():
    q, sg = pc.M_QUIET, pc.M_STRONG
    b = stream_of_m([q] * 10 + [sg] * 100 + [q] * 100)
    assert ref.Stream(1, 1000, 5000).run(b)[1] == [{"k_rel": 110, "width": 100, "gap": 0, "level": sg}]
    # W = 64: e >= 400000 needs 55 strong samples (54 sg + 10 = 395344): the rise at 10 + 54; e < 100000 at 13 strong ones left
    # (13 sg + 51 = 95224): the fall at 110 + 50, with 14 sg + 50 in front of it
    assert ref.Stream(64, 100000, 400000).run(b)[1] == [{"k_rel": 160, "width": 96, "gap": 0, "level": 14 * sg + 50}]
    for W, lo, hi in pc.SETTINGS.values():
        got = absolute(ref.Stream(W, lo, hi), [b])
        assert got == literal(b, W, lo, hi)[0] and len(got) == 1, W


def test_definition_restates_the_loop_and_ignores_the_cuts():
    iq = pc.traffic(5000, 3)[0]
    rng = np.random.default_rng(4)
    for W, lo, hi in [(1, 5000, 5000), (8, 30000, 60000), (64, 100000, 400000), (3, 1, 195075), (8, 10000, 30000)]:
        want, info = literal(iq, W, lo, hi)
        one = ref.Stream(W, lo, hi)
        assert absolute(one, [iq]) == want and one.info == info, (W, lo, hi)
        cuts = sorted(set((rng.integers(1, 2500, 30) * 2).tolist()))
        some = ref.Stream(W, lo, hi)
        assert absolute(some, np.split(iq, cuts)) == want and some.info == info
        four = ref.Stream(W, lo, hi)
        assert absolute(four, np.split(iq, np.arange(8, iq.size, 8))) == want and four.info == info
    assert len(literal(iq, 8, 30000, 60000)[0]) >= 10


def test_width_and_gap_saturate():
    """On the definition only: a device test would need 2^32 samples."""
    q, sg = pc.M_QUIET, pc.M_STRONG
    st = ref.Stream(1, 5000, 5000)
    st.run(stream_of_m([sg, q, q, q]))                       # one pulse, so that a gap is counted
    st.run_len = 2 ** 32 + 5
    count, recs = st.run(stream_of_m([q, sg, q, q]))
    assert recs == [{"k_rel": 2, "width": 1, "gap": ref.SAT, "level": sg}]
    st.run(stream_of_m([q, sg, sg, sg]))
    st.run_len = 2 ** 32 + 7
    assert st.run(stream_of_m([sg, q, q, q]))[1] == [{"k_rel": 1, "width": ref.SAT, "gap": 3, "level": sg}]
    st.run_len = 2 ** 32 - 4                                 # one short of it: 2^32 - 2 samples since the fall
    assert st.run(stream_of_m([q, q, sg, q]))[1] == [{"k_rel": 3, "width": 1, "gap": ref.SAT - 1, "level": sg}]


def test_definition_does_not_depend_on_the_cuts_of_the_cases():
    c = pc.case("cuts_one")
    per_call, info = pc.expected("cuts_one")
    want = pc.absolute(per_call, c.calls, 0)
    for how in ("random", "four"):
        o = pc.case("cuts_" + how)
        other, oinfo = pc.expected("cuts_" + how)
        assert pc.absolute(other, o.calls, 0) == want and oinfo == info, how
    assert pc.absolute(*[x for x in (pc.expected("long_calls")[0], pc.case("long_calls").calls)], 0) == \
        pc.absolute(pc.expected("long_one")[0], pc.case("long_one").calls, 0)


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_case_table_checks_itself(name):
    assert pc.case(name).name == name
    pc.check_case(name)


def test_case_names_are_the_cases():
    assert [c.name for c in pc.all_cases()] == pc.CASE_NAMES


def test_domain_errors_are_decided_before_a_device(fmd):
    lib, cfgs = fmd.lib(), fmd.pulses.PulsesConfig
    dev, h = fmd.DeviceConfig(2, -1, 0), C.c_void_p()
    E = 64 * 65025
    for bad, text in ((cfgs(0, 1, 2, 4), "W"), (cfgs(65, 1, 2, 4), "W"), (cfgs(8, 0, 2, 4), "lo"), (cfgs(8, 3, 2, 4), "lo <= hi"),
                      (cfgs(8, 1, E + 1, 4), "hi"), (cfgs(8, 1, 2, 0), "pulse_cap"), (cfgs(8, 1, 2, 1025), "pulse_cap")):
        assert lib.fmd_pulses_new(C.byref(bad), C.byref(dev), C.byref(h)) == UNSUPPORTED and not h
        assert text in lib.fmd_last_error().decode()
    good = cfgs(64, E, E, 1024)
    assert lib.fmd_pulses_new(C.byref(good), C.byref(fmd.DeviceConfig(0, -1, 0)), C.byref(h)) == UNSUPPORTED and not h
    assert "n_streams" in lib.fmd_last_error().decode()
    assert lib.fmd_pulses_new(None, C.byref(dev), C.byref(h)) == INVALID_ARG
    assert lib.fmd_pulses_new(C.byref(good), None, C.byref(h)) == INVALID_ARG
    assert lib.fmd_pulses_new(C.byref(good), C.byref(dev), None) == INVALID_ARG
    buf = (C.c_uint8 * 64)()
    assert lib.fmd_pulses_run_batch(None, buf, 8, 8) == INVALID_ARG and lib.fmd_pulses_run_device(None, buf, 8, 8, None) == INVALID_ARG
    assert lib.fmd_pulses_counts(None, buf) == INVALID_ARG and lib.fmd_pulses_info(None, buf) == INVALID_ARG
    assert lib.fmd_pulses_recs(None, None, 0, None) == INVALID_ARG and lib.fmd_pulses_check(None) == INVALID_ARG
    assert lib.fmd_pulses_reset(None) == INVALID_ARG and lib.fmd_pulses_kernel_name(None, 0, None, 0) == INVALID_ARG
    lib.fmd_pulses_free(None)
    if fmd.device_count() == 0:
        assert lib.fmd_pulses_new(C.byref(good), C.byref(dev), C.byref(h)) == NO_DEVICE and not h
        with pytest.raises(fmd.FmdError) as ei:
            fmd.PulseBank(2)
        assert ei.value.status == NO_DEVICE
    assert fmd.pulses_tile() % 8 == 0 and fmd.pulses_tile() >= 512 and (fmd.pulses_tile() + 64) * 65025 < 2 ** 32


def test_kernels_fit_their_budget():
    """both passes without scratch memory or spills, at most 64 VGPRs (eight waves per SIMD by registers); pass 0 holds
    the prefix, the queue and the wave tables in less than 26 KiB of static LDS (six workgroups per CU), pass 1 none."""
    import json
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_digest.py"), "--src", "fmd_pulses.hip"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    ks = {r["name"].split("(")[0]: r for r in map(json.loads, p.stdout.splitlines()) if "kernel" in r["name"]}
    assert sorted(ks) == ["fmd_pl::fmd_pulses_gather_kernel", "fmd_pl::fmd_pulses_tile_kernel"]
    for k in ks.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 64 and k.get("agpr", 0) == 0, k
    T = 4096
    assert 4 * (T + 72) + 2 * T <= ks["fmd_pl::fmd_pulses_tile_kernel"]["lds"] < 26 * 1024 and ks["fmd_pl::fmd_pulses_gather_kernel"]["lds"] == 0


# ---- the slicer -----------------------------------------------------------------------------------------------------------------------

def records_of(iq, W=1, lo=1000, hi=5000):
    return ref.Stream(W, lo, hi).run(iq)[1]


def both(modulation, short, long, tol, reset):
    import rtl_sdr_rs_amd as fmd
    return fmd.PulseSlicer(modulation, short, long, tol, reset), sref.Slicer(fmd.pulses._modulation(modulation), short, long, tol, reset)


@pytest.mark.parametrize("modulation", ["pwm", "ppm"])
def test_slicer_round_trip_of_the_sender(fmd, modulation):
    rng = np.random.default_rng(8)
    bits = rng.integers(0, 2, 41).tolist()
    iq = fmd.ook_encode(bits, modulation, 10, 30, 20, lead=50, trail=200)
    on = iq[0::2] == 188
    assert iq.dtype == np.uint8 and set(iq.tolist()) == {128, 188} and (iq[1::2] == 128).all() and not on[:50].any() and on[50]
    if modulation == "pwm":
        assert on.sum() == sum(10 if b else 30 for b in bits) and iq.size == 2 * (50 + on.sum() + 41 * 20 + 200)
    else:
        assert on.sum() == 42 * 20 and iq.size == 2 * (50 + 42 * 20 + sum(30 if b else 10 for b in bits) + 200)
    recs = records_of(iq)
    lib_s, ref_s = both(modulation, 10, 30, 2, 100)
    for s in (lib_s, ref_s):
        s.push(recs, 1000)
        assert s.take() == []                                # still open
        s.idle(1, 500)
        s.idle(0, 99)
        assert s.take() == []
        s.idle(0, 100)
    got = lib_s.take()
    assert got == ref_s.take() and len(got) == 1
    k = got[0]
    assert k["start"] == 1050 and k["n_bits"] == 41 and k["flags"] == 0 and k["n_pulses"] == (41 if modulation == "pwm" else 42)
    assert fmd.package_bits(k) == bits and k["bits"][6:] == bytes(26)
    with pytest.raises(ValueError):
        fmd.ook_encode(bits, "fsk", 10, 30, 20)


def test_slicer_tolerance_bad_and_the_order_of_the_windows(fmd):
    rec = lambda k, w, g: {"k_rel": k, "width": w, "gap": g, "level": 0}
    lib_s, ref_s = both("pwm", 10, 30, 3, 100)
    widths = [7, 13, 27, 33, 10, 30]                         # on both sides of tol, inside: 1 1 0 0 1 0
    for s in (lib_s, ref_s):
        s.push([rec(100 * i + 50, w, 20) for i, w in enumerate(widths)], 0)
        s.push([rec(1000, 14, 200)], 0)                      # closes it; 14 is outside: a bad package of its own
        s.push([rec(1100, 10, 20), rec(1200, 6, 20), rec(1300, 34, 20), rec(1400, 10, 500)], 0)
        s.idle(0, 100)
    got = lib_s.take()
    assert got == ref_s.take() and len(got) == 3
    assert (got[0]["n_bits"], got[0]["flags"], got[0]["n_pulses"], got[0]["start"]) == (6, 0, 6, 43) and fmd.package_bits(got[0]) == [1, 1, 0, 0, 1, 0]
    assert (got[1]["n_bits"], got[1]["flags"], got[1]["n_pulses"], got[1]["start"]) == (0, sref.BAD, 4, 986)      # skipped to its end
    assert (got[2]["n_bits"], got[2]["flags"], got[2]["n_pulses"]) == (1, 0, 1)
    lib_s, ref_s = both("ppm", 10, 30, 3, 100)
    for s in (lib_s, ref_s):
        s.push([rec(50, 5, 999), rec(100, 5, 13), rec(150, 5, 27), rec(200, 5, 14), rec(250, 5, 10)], 0)
        s.idle(0, 1000)
    got = lib_s.take()
    assert got == ref_s.take() and fmd.package_bits(got[0]) == [0, 1] and got[0]["flags"] == sref.BAD and got[0]["n_pulses"] == 5
    lib_s, ref_s = both("pwm", 10, 12, 5, 100)               # overlapping windows: short wins
    for s in (lib_s, ref_s):
        s.push([rec(50, 11, 0), rec(100, 16, 20)], 0)
        s.idle(0, 100)
    got = lib_s.take()
    assert got == ref_s.take() and fmd.package_bits(got[0]) == [1, 0]


def test_slicer_truncates_at_256_bits_and_spans_calls(fmd):
    bits = [i % 3 == 0 for i in range(300)]
    iq = fmd.ook_encode(bits, "pwm", 4, 9, 5, lead=3, trail=20)
    recs = records_of(iq)
    assert len(recs) == 300
    lib_s, ref_s = both("pwm", 4, 9, 1, 12)
    for s in (lib_s, ref_s):
        for a in range(0, 300, 7):                           # a package split across pushes
            s.push(recs[a:a + 7], 0)
            s.idle(0, 5)
        assert s.take() == []
        s.idle(0, 12)
    got = lib_s.take()
    assert got == ref_s.take() and len(got) == 1
    assert got[0]["n_bits"] == 256 and got[0]["flags"] == sref.TRUNCATED and got[0]["n_pulses"] == 300 and got[0]["start"] == 3
    assert fmd.package_bits(got[0]) == [int(b) for b in bits[:256]]
    lib_s, ref_s = both("pwm", 4, 9, 1, 12)                  # 64 wait; the 65th is dropped
    for s in (lib_s, ref_s):
        s.push([{"k_rel": 100 * i, "width": 4, "gap": 50, "level": 0} for i in range(1, 70)], 7)
    got = lib_s.take(10) + lib_s.take()
    assert got == ref_s.take(10) + ref_s.take() and len(got) == 64 and [k["start"] for k in got] == [7 + 100 * i - 4 for i in range(1, 65)]
    assert lib_s.take() == []


def test_slicer_matches_its_definition_on_random_records(fmd):
    rng = np.random.default_rng(12)
    for trial in range(40):
        modulation = ("pwm", "ppm")[trial % 2]
        short, long, tol, reset = int(rng.integers(1, 40)), int(rng.integers(1, 80)), int(rng.integers(0, 8)), int(rng.integers(1, 200))
        lib_s, ref_s = both(modulation, short, long, tol, reset)
        pos, got, want = 0, [], []
        for call in range(12):
            n = int(rng.integers(0, 40))
            pick = lambda: int(rng.choice([short, long, short + tol, long + tol + 1, max(0, short - tol), rng.integers(0, 300), 2 ** 32 - 1]))
            recs = [{"k_rel": int(k), "width": pick(), "gap": pick(), "level": 0} for k in np.sort(rng.integers(0, 5000, n))]
            state, run = int(rng.integers(0, 2)), int(rng.integers(0, 400))
            for s, out in ((lib_s, got), (ref_s, want)):
                s.push(recs, pos)
                s.idle(state, run)
                if call % 3 == 2:
                    out += s.take()
            pos += 5000
        assert got == want and got, trial


def test_slicer_refusals(fmd):
    lib, cfgs = fmd.lib(), fmd.pulses.PulseSlicerConfig
    h = C.c_void_p()
    for bad, text in ((cfgs(2, 1, 1, 0, 1), "modulation"), (cfgs(0, 0, 1, 0, 1), "short_w"), (cfgs(1, 1, 0, 0, 1), "long_w"), (cfgs(1, 1, 1, 0, 0), "reset")):
        assert lib.fmd_pulse_slicer_new(C.byref(bad), C.byref(h)) == UNSUPPORTED and not h
        assert text in lib.fmd_last_error().decode()
    assert lib.fmd_pulse_slicer_new(None, C.byref(h)) == INVALID_ARG and lib.fmd_pulse_slicer_new(C.byref(cfgs(0, 1, 2, 0, 5)), None) == INVALID_ARG
    n = C.c_size_t(0)
    assert lib.fmd_pulse_slicer_push(None, None, 0, 0) == INVALID_ARG and lib.fmd_pulse_slicer_idle(None, 0, 0) == INVALID_ARG
    assert lib.fmd_pulse_slicer_take(None, None, 0, C.byref(n)) == INVALID_ARG
    lib.fmd_pulse_slicer_free(None)
    s = fmd.PulseSlicer("pwm", 1, 2, 0, 5)
    assert lib.fmd_pulse_slicer_push(s._h, None, 3, 0) == INVALID_ARG and lib.fmd_pulse_slicer_take(s._h, None, 3, C.byref(n)) == INVALID_ARG
    assert lib.fmd_pulse_slicer_take(s._h, None, 0, None) == INVALID_ARG and lib.fmd_pulse_slicer_push(s._h, None, 0, 0) == 0


def test_thresholds_from_a_quiet_capture(fmd):
    iq = pc.noise(1, 20000, 5)[0]
    lo, hi = fmd.pulse_thresholds(iq, 8, 4.0)
    st = ref.Stream(8, lo, hi)
    e = st.box(iq)[0][8:]
    assert hi == round(4.0 * float(np.median(e))) and lo == hi // 2 and 8 * 300 < np.median(e) < 8 * 700
    assert ref.Stream(8, lo, hi).run(iq)[0] <= 2 and 8 * pc.M_STRONG >= hi      # quiet stays quiet; a strong pulse is seen
    assert fmd.pulse_thresholds(np.full(400, 255, np.uint8), 64, 100.0) == (64 * 65025 // 2, 64 * 65025)
    assert fmd.pulse_thresholds(np.full(400, 128, np.uint8), 1, 1.0) == (1, 2)
    with pytest.raises(ValueError):
        fmd.pulse_thresholds(iq[:8], 8)


def test_host_slicer_under_the_sanitizers(tmp_path):
    """tests/cpp/pulse_slice_fuzz.cpp with csrc/fmd_pulse_slice.cpp, a program of its own: random record lists through push, idle and
    take with buffers of exactly the size each call may touch.  It ends clean."""
    exe = str(tmp_path / "pulse_slice_fuzz")
    # (the sanitizers' runtimes are linked in statically: the program needs nothing preloaded and runs in any environment)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpp", "pulse_slice_fuzz.cpp"),
                    os.path.join(ROOT, "rtl-sdr-rs_amd", "csrc", "fmd_pulse_slice.cpp"), "-o", exe], check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", (p.returncode, p.stderr.decode()[-2000:])
    words = p.stdout.decode().split()
    assert words[0] == "ok" and int(words[2]) > 1000 and int(words[4]) > 100
