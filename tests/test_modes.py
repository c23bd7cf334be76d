"""The Mode S bank without a GPU: the definition (tests/modes_ref.py) against the published messages, the library's host table, syndrome
and field decoder against the definition and the published worked values, the sender, the host's de-duplication, every refusal that is
decided before a device is touched, and the case table of tests/test_gpu_modes.py checking itself."""
import ctypes as C
import os

import numpy as np
import pytest

import modes_cases as mc
import modes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_LENGTH, UNSUPPORTED, NO_DEVICE = -1, -2, -6, -8


def stream_of(fmd, placed, n, **kw):
    """(count, records) of the definition over one quiet stream of n samples with the messages `placed` [(p, msg)]."""
    iq = mc.quiet(1, n)
    for p, msg in placed:
        mc.place(iq, 0, p, msg)
    return ref.Stream(**kw).run(iq[0])


def test_symbols_are_declared_everywhere(fmd):
    from rtl_sdr_rs_amd import _ffi
    rust = open(os.path.join(ROOT, "rust", "fmd-gpu", "src", "lib.rs")).read()
    for name in ("new", "free", "reset", "run_batch", "run_device", "check", "counts", "msgs", "info", "kernel_name", "tile", "table",
                 "syndrome", "decode", "cpr_global"):
        name = "fmd_modes_" + name
        assert name in _ffi.PROTOTYPES and hasattr(fmd.lib(), name) and "pub fn %s(" % name in rust, name
    assert C.sizeof(fmd.modes.ModesMsg) == 32 and C.sizeof(fmd.modes.ModesTotals) == 32 and C.sizeof(fmd.modes.ModesConfig) == 16


def test_table_values_of_the_definition():
    assert ref.T112[0] == 0x3935EA and ref.T112[87] == 0xFFF409 and ref.T112[88] == 0x800000 and ref.T112[111] == 1
    assert ref.T56 == ref.T112[56:] and len(set(ref.T112)) == 112


def test_library_table_and_syndrome_match_the_definition(fmd):
    assert fmd.modes_table(112).tolist() == ref.T112 and fmd.modes_table(56).tolist() == ref.T56
    rng = np.random.default_rng(5)
    msgs = mc.LONG + [mc.flip(mc.LONG[0], 111)] + [bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist()) for n in (7, 14) * 8]
    for m in msgs:
        bits = np.unpackbits(np.frombuffer(m, np.uint8)).tolist()
        assert fmd.modes_syndrome(m) == ref.syndrome_bits(bits), m.hex()
    assert [fmd.modes_syndrome(m) for m in mc.LONG] == [0, 0, 0, 0] and fmd.modes_syndrome(mc.flip(mc.LONG[0], 111)) == 1
    lib = fmd.lib()
    syn, buf = C.c_uint32(0), (C.c_uint8 * 14)()
    assert lib.fmd_modes_syndrome(buf, 8, C.byref(syn)) == BAD_LENGTH and lib.fmd_modes_syndrome(None, 7, C.byref(syn)) == INVALID_ARG
    assert lib.fmd_modes_table(57, (C.c_uint32 * 112)()) == UNSUPPORTED and lib.fmd_modes_table(56, None) == INVALID_ARG


@pytest.mark.parametrize("k", range(4))
def test_definition_finds_the_published_messages(fmd, k):
    for p in (0, 1, 777):
        count, recs = stream_of(fmd, [(p, mc.LONG[k])], 1400)
        assert count == 1 and recs[0]["k_rel"] == p and recs[0]["bytes"] == mc.LONG[k] and recs[0]["n_bytes"] == 14
        assert recs[0]["df"] == 17 and recs[0]["fixed_bit"] == 0xFF and recs[0]["power"] == 4 * mc.M_PULSE


def test_the_fix_restores_any_single_bit_behind_the_df_field(fmd):
    msg = mc.LONG[3]
    for t in range(112):
        count, recs = stream_of(fmd, [(40, mc.flip(msg, t))], 400, fix_errors=1)
        if t < 5:
            assert count == 0, t
        else:
            assert count == 1 and recs[0]["fixed_bit"] == t and recs[0]["bytes"] == msg and recs[0]["k_rel"] == 40, t
        assert stream_of(fmd, [(40, mc.flip(msg, t))], 400, fix_errors=0)[0] == 0


def test_two_flips_are_not_accepted(fmd):
    fixable = set(ref.T112[5:])
    pairs = [(a, b) for a, b in ((5, 6), (20, 77), (8, 111), (33, 34), (60, 100)) if ref.T112[a] ^ ref.T112[b] not in fixable]
    assert len(pairs) >= 3                                   # (a pair whose syndrome is a single bit's would be "fixed" wrongly)
    for a, b in pairs:
        assert stream_of(fmd, [(40, mc.flip(mc.LONG[1], a, b))], 400, fix_errors=1)[0] == 0, (a, b)


def test_short_messages_need_df11(fmd):
    for address, iid in ((0x4840D6, 0), (0xABCDEF, 5), (0x000001, 127)):
        msg = fmd.modes_df11(address, iid)
        assert len(msg) == 7 and msg[0] >> 3 == 11 and int.from_bytes(msg[1:4], "big") == address and fmd.modes_syndrome(msg) == iid
        count, recs = stream_of(fmd, [(90, msg)], 500, df11=1)
        assert count == 1 and recs[0]["k_rel"] == 90 and recs[0]["n_bytes"] == 7 and recs[0]["df"] == 11
        assert recs[0]["bytes"] == msg + bytes(7)
        assert stream_of(fmd, [(90, msg)], 500, df11=0)[0] == 0
    bad = mc.flip(fmd.modes_df11(0x4840D6, 3), 40)           # a parity bit above the IID's seven
    assert stream_of(fmd, [(90, bad)], 500, df11=1)[0] == 0


def test_preamble_rule_rejects_a_constant_and_a_pulse_in_a_quiet_slot(fmd):
    for level in (0, 128, 255):
        ok, _ = ref.preamble(ref.magnitude(np.full(2000, level, np.uint8)), 0)
        assert not ok.any()
    good = mc.quiet(1, 400)
    mc.place(good, 0, 50, mc.LONG[0])
    ok, S = ref.preamble(ref.magnitude(good[0]), 0)
    assert ok[50] and S[50] == 4 * mc.M_PULSE
    for slot in (1, 3, 4, 5, 6, 8, 11, 12, 13, 14):
        bad = good.copy()
        bad[0, 2 * (50 + slot)] = 128 + mc.AMP
        assert not ref.preamble(ref.magnitude(bad[0]), 0)[0][50], slot
    assert not ref.preamble(ref.magnitude(good[0]), 4 * mc.M_PULSE + 1)[0][50]


def test_noise_candidate_rate():
    """Gaussian noise of sigma 12 passes the preamble rule at a few positions in a thousand: the kernel's candidate rate in the empty
    case (0.27 % over 2^20 samples)."""
    ok, _ = ref.preamble(ref.magnitude(mc.noise(1, 1 << 18, 1)[0]), 0)
    assert 0.0015 < ok.mean() < 0.004


def test_definition_does_not_depend_on_the_cuts():
    per_call, info = mc.check_case("cuts_one")
    for how in ("random", "four"):
        other, oinfo = mc.check_case("cuts_" + how)
        assert other == per_call and oinfo == info, how
    assert info[0]["messages"] >= 9 and info[0]["samples"] == 4 * mc.tile()


@pytest.mark.parametrize("name", [n for n in mc.CASE_NAMES if not n.startswith("cuts_")])
def test_case_table_checks_itself(name):
    assert name in mc.CASE_NAMES and mc.case(name).name == name
    mc.check_case(name)


def test_case_names_are_the_cases():
    assert [c.name for c in mc.all_cases()] == mc.CASE_NAMES


def test_field_decoder_gives_the_published_values(fmd):
    f = fmd.modes_fields(mc.VECTORS[0])
    assert (f["df"], f["icao"], f["type_code"], f["callsign"]) == (17, 0x4840D6, 4, "KLM1023")
    even, odd = fmd.modes_fields(mc.VECTORS[1]), fmd.modes_fields(mc.VECTORS[2])
    assert even["icao"] == odd["icao"] == 0x40621D and even["altitude_ft"] == odd["altitude_ft"] == 38000
    assert (even["cpr_odd"], even["cpr_lat"], even["cpr_lon"]) == (0, 93000, 51372)
    assert (odd["cpr_odd"], odd["cpr_lat"], odd["cpr_lon"]) == (1, 74158, 50194)
    lat, lon = fmd.cpr_global(mc.VECTORS[1], mc.VECTORS[2])
    assert abs(lat - 52.2572) < 1e-3 and abs(lon - 3.9194) < 1e-3
    lat_o, lon_o = fmd.cpr_global(even, odd, latest="odd")
    assert abs(lat_o - 52.2658) < 1e-3 and abs(lon_o - lon) < 0.05     # (the odd message's own position, nearby)
    v = fmd.modes_fields(mc.VECTORS[3])
    assert (v["type_code"], v["subtype"]) == (19, 1)
    assert (round(v["speed_kt"]), round(v["track_deg"]), v["vrate_fpm"]) == (159, 183, -832)
    with pytest.raises(fmd.FmdError) as ei:
        fmd.modes_fields(fmd.modes_df11(1))
    assert ei.value.status == UNSUPPORTED
    with pytest.raises(ValueError):
        fmd.cpr_global(odd, even)


def test_sender_and_dedupe(fmd):
    e = fmd.modes_encode(mc.LONG[0], 60, lead=3, trail=2)
    assert e.dtype == np.uint8 and e.size == 2 * (3 + 240 + 2) and set(e.tolist()) == {128, 188}
    on = np.nonzero(e[0::2] == 188)[0] - 3
    assert on[:4].tolist() == [0, 2, 7, 9] and on.size == 4 + 112 and (e[1::2] == 128).all()
    assert fmd.modes_encode(fmd.modes_df11(7)).size == 2 * (16 + 112)
    with pytest.raises(ValueError):
        fmd.modes_encode(b"123456")
    recs = [{"p": 100, "n_bytes": 14}, {"p": 101, "n_bytes": 7}, {"p": 339, "n_bytes": 7}, {"p": 340, "n_bytes": 7}, {"p": 400, "n_bytes": 14},
            {"p": 468, "n_bytes": 14}]
    assert [r["p"] for r in fmd.modes_dedupe(recs)] == [100, 340, 468]
    assert [r["k_rel"] for r in fmd.modes_dedupe([{"k_rel": -239, "n_bytes": 7}, {"k_rel": -112, "n_bytes": 7}, {"k_rel": -111, "n_bytes": 7}])] == [-239, -111]


def test_domain_errors_are_decided_before_a_device(fmd):
    lib, cfgs = fmd.lib(), fmd.modes.ModesConfig
    dev, h = fmd.DeviceConfig(2, -1, 0), C.c_void_p()
    for bad, text in ((cfgs(262145, 0, 0, 4), "min_power"), (cfgs(0, 2, 0, 4), "fix_errors"), (cfgs(0, 0, 2, 4), "df11"),
                      (cfgs(0, 0, 0, 0), "msg_cap"), (cfgs(0, 0, 0, 257), "msg_cap")):
        assert lib.fmd_modes_new(C.byref(bad), C.byref(dev), C.byref(h)) == UNSUPPORTED and not h
        assert text in lib.fmd_last_error().decode()
    good = cfgs(262144, 1, 1, 256)
    assert lib.fmd_modes_new(None, C.byref(dev), C.byref(h)) == INVALID_ARG
    assert lib.fmd_modes_new(C.byref(good), None, C.byref(h)) == INVALID_ARG
    assert lib.fmd_modes_new(C.byref(good), C.byref(dev), None) == INVALID_ARG
    assert lib.fmd_modes_new(C.byref(good), C.byref(fmd.DeviceConfig(0, -1, 0)), C.byref(h)) == INVALID_ARG
    buf = (C.c_uint8 * 16)()
    assert lib.fmd_modes_run_batch(None, buf, 8, 8) == INVALID_ARG and lib.fmd_modes_run_device(None, buf, 8, 8, None) == INVALID_ARG
    assert lib.fmd_modes_counts(None, buf) == INVALID_ARG and lib.fmd_modes_info(None, buf) == INVALID_ARG
    assert lib.fmd_modes_msgs(None, None, 0, None) == INVALID_ARG and lib.fmd_modes_check(None) == INVALID_ARG
    assert lib.fmd_modes_reset(None) == INVALID_ARG and lib.fmd_modes_kernel_name(None, 0, None, 0) == INVALID_ARG
    lib.fmd_modes_free(None)
    if fmd.device_count() == 0:
        assert lib.fmd_modes_new(C.byref(good), C.byref(dev), C.byref(h)) == NO_DEVICE and not h
        with pytest.raises(fmd.FmdError) as ei:
            fmd.ModeSBank(2)
        assert ei.value.status == NO_DEVICE
    assert fmd.modes_tile() % 8 == 0 and fmd.modes_tile() >= 512


def test_kernels_fit_their_budget():
    """both passes without scratch or spills, at most 64 VGPRs (eight waves per SIMD by registers); pass 0 holds the
    plane, the queue and the wave sums in 16896 bytes of static LDS, pass 1 none."""
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_digest.py"), "--src", "fmd_modes.hip"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    import json
    ks = {r["name"].split("(")[0]: r for r in map(json.loads, p.stdout.splitlines()) if "kernel" in r["name"]}
    assert sorted(ks) == ["fmd_ms::fmd_modes_gather_kernel", "fmd_ms::fmd_modes_tile_kernel"]
    for k in ks.values():
        assert k["scratch"] == 0 and k["vgpr"] <= 64 and k.get("agpr", 0) == 0, k
    assert ks["fmd_ms::fmd_modes_tile_kernel"]["lds"] == 16896 and ks["fmd_ms::fmd_modes_gather_kernel"]["lds"] == 0


def test_host_decoder_under_the_sanitizers(tmp_path):
    """tests/cpp/modes_fuzz.cpp with csrc/fmd_modes_decode.cpp, a program of its own: random, published and damaged messages of every
    length through the table, the syndrome, the field decoder and the CPR solve.  It ends clean."""
    import subprocess
    exe = str(tmp_path / "modes_fuzz")
    # (the sanitizers' runtimes are linked in statically: the program needs nothing preloaded and runs in any environment)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpp", "modes_fuzz.cpp"),
                    os.path.join(ROOT, "rtl-sdr-rs_amd", "csrc", "fmd_modes_decode.cpp"), "-o", exe], check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", (p.returncode, p.stderr.decode()[-2000:])
    words = p.stdout.decode().split()
    assert words[0] == "ok" and int(words[2]) > 1000 and int(words[4]) > 1000
