"""Station bank (include/fmd.h, fmd_stations_*) on the MI355X: bit for bit against the reference chain (inc = 0 on rotated
bytes) and against the test-side definition (tests/stations_ref.py), call splitting, the f64 sample's settle path, the
device entry point, and the physics of many stations in one synthesised capture."""
import os
import subprocess

import numpy as np
import pytest

import stations_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ragged(rng, total, parts, least=8 * 200):
    while True:
        cuts = np.sort(rng.choice(np.arange(1, total // 8), parts - 1, replace=False)) * 8
        sizes = np.diff(np.concatenate([[0], cuts, [total]]))
        if sizes.min() >= least:
            return sizes.tolist()


def test_anchor_inc0_ones_on_rotated_bytes_is_demodbank_is_the_oracle(fmd, oracle):
    D, S = 10, 3
    cfg = fmd.DemodConfig(240000, 240000, 32000, D, 1)
    dbank = fmd.DemodBank(cfg, S, device_id=0)
    bank = fmd.StationBank(np.ones(D, np.int16), D, [[0]] * S, 240000, 32000, n_streams=S, shift=0, device_id=0)
    assert bank.kernel_name().find("fmd_stations") >= 0
    ods = [oracle.new(oracle.config(D, 240000, 32000)) for _ in range(S)]
    rng = np.random.default_rng(11)
    sizes = [8 * 5 * D, 8 * 123, fmd.DEFAULT_BUF_LENGTH, 8 * 777, 4096]
    for n in sizes + ["full"]:
        if n == "full":
            B = np.tile(np.array([255, 0, 0, 255, 255, 255, 0, 0], np.uint8), (S, 600))
        else:
            B = rng.integers(0, 256, (S, n), dtype=np.uint8)
        R = np.stack([sr.rot90(B[s]) for s in range(S)])
        got = bank.demodulate_batch(R)
        exp = dbank.demodulate_batch(B)
        for s in range(S):
            o = oracle.demodulate(ods[s], B[s])
            assert np.array_equal(exp[s], o)
            assert np.array_equal(got[s, 0], o), (n, s)
    for s in range(S):
        st = bank.get_state(s, 0).as_dict()
        want = oracle.state_of(ods[s])
        assert st["demod_pre"] == want["demod_pre"] and st["now_lpr"] == want["now_lpr"]
        assert st["prev_lpr_index"] == want["prev_lpr_index"]


def _offsets(rng, K):
    fixed = [0, 1 << 30, (1 << 32) - (1 << 30), 1 << 31]
    return [fixed[k] if k < len(fixed) else int(rng.integers(0, 1 << 32)) for k in range(K)]


@pytest.mark.parametrize("K,digits", [(1, 2), (3, 2), (8, 1), (8, 2), (17, 2), (32, 1)])
def test_definition_parity_random_shapes(fmd, oracle, K, digits):
    rng = np.random.default_rng(1000 * K + digits)
    S = 2
    D = int(rng.choice([2, 4, 6, 10, 16, 24]))
    T = int(rng.integers(1, 97))
    hmax = 127 if digits == 1 else 2047
    h = rng.integers(-hmax, hmax + 1, T).astype(np.int16)
    if digits == 1:
        h = (h // 2).astype(np.int16)                        # every |W| <= 127 -> the one-digit form
    fast = int(rng.integers(80000, 400000)) // D * D
    slow = int(rng.integers(8000, fast // 2))
    incs = np.array([_offsets(rng, K) for _ in range(S)], dtype=np.uint32)
    g = sr.max_gain(h, incs)
    shift = 0
    while -(-256 * g >> shift) > (16384 if K % 2 else 2048):  # odd K: the integer discriminator, even K: the f32 one
        shift += 1
    bank = fmd.StationBank(h, D, incs, fast, slow, n_streams=S, shift=shift, device_id=0)
    refs = [sr.StationsRef(oracle, h, D, incs[s], fast, slow, shift) for s in range(S)]
    total = 8 * int(rng.integers(3000, 9000))
    data = rng.integers(0, 256, (S, total), dtype=np.uint8)
    data[:, : total // 4] = np.where(rng.random((S, total // 4)) < 0.5, 0, 255)      # full-scale stretch
    pos = 0
    for n in _ragged(rng, total, 5):
        chunk = data[:, pos:pos + n]
        pos += n
        try:
            exp = [r.feed(chunk[s]) for s, r in enumerate(refs)]
        except sr.TooShort:
            with pytest.raises(fmd.FmdError):
                bank.demodulate_batch(chunk)
            continue
        got = bank.demodulate_batch(chunk)
        for s in range(S):
            for k in range(K):
                assert np.array_equal(got[s, k], exp[s][k]), (s, k, n)
    for s in range(S):
        for k in range(K):
            st = bank.get_state(s, k).as_dict()
            want = refs[s].state(k)
            assert st["demod_pre"] == want["demod_pre"] and st["now_lpr"] == want["now_lpr"], (s, k)


def test_splitting_and_reset(fmd):
    rng = np.random.default_rng(21)
    h = rng.integers(-300, 301, 48).astype(np.int16)
    incs = [sr.phase_inc(o, 2400000) for o in (-600000, -100000, 250000, 900000)]
    data = rng.integers(0, 256, (2, 8 * 30000), dtype=np.uint8)
    one = fmd.StationBank(h, 10, incs, 240000, 32000, n_streams=2, device_id=0)
    whole = one.demodulate_batch(data)
    many = fmd.StationBank(h, 10, incs, 240000, 32000, n_streams=2, device_id=0)
    parts, pos = [], 0
    for n in _ragged(rng, data.shape[1], 7):
        parts.append(many.demodulate_batch(data[:, pos:pos + n]))
        pos += n
    # (the f64 sample at every call start (:359) makes split audio differ from whole-call audio where it and fast_atan2
    #  disagree -- test_split_calls_match_the_definition_cut_for_cut compares cut for cut); reset restarts the stream exactly
    one.reset()
    again = one.demodulate_batch(data)
    assert np.array_equal(again, whole)
    many.reset()
    first = many.demodulate_batch(data[:, :8 * 5000])
    fresh = fmd.StationBank(h, 10, incs, 240000, 32000, n_streams=2, device_id=0).demodulate_batch(data[:, :8 * 5000])
    assert np.array_equal(first, fresh)
    assert sum(p.shape[2] for p in parts) == whole.shape[2]


def test_split_calls_match_the_definition_cut_for_cut(fmd, oracle):
    rng = np.random.default_rng(22)
    h = rng.integers(-200, 201, 33).astype(np.int16)
    incs = [sr.phase_inc(o, 2400000) for o in (-700000, 0, 333333)]
    data = rng.integers(0, 256, 8 * 20000, dtype=np.uint8)
    bank = fmd.StationBank(h, 6, incs, 200000, 48000, device_id=0)
    ref = sr.StationsRef(oracle, h, 6, incs, 200000, 48000, bank.shift)
    pos = 0
    for n in _ragged(rng, data.size, 9):
        exp = ref.feed(data[pos:pos + n])
        got = bank.demodulate_batch(data[None, pos:pos + n])
        pos += n
        for k in range(3):
            assert np.array_equal(got[0, k], exp[k])


def test_f64_guard_patch_path_exp_build(fmd, oracle, request):
    """Experiment build, guard band 2^-2 wide and a skew of +3 on guarded samples: every guarded f64 sample is patched by the
    host libm and the audio is still the definition's, bit for bit."""
    from conftest import run_in_exp_child
    if run_in_exp_child(request, {"FMD_F64_GUARD_LOG2": "-2", "FMD_F64_SKEW": "3"}):
        return
    rng = np.random.default_rng(31)
    h = rng.integers(-500, 501, 40).astype(np.int16)
    incs = np.array([[sr.phase_inc(o, 2400000) for o in (-500000, 0, 700000)] for _ in range(4)], np.uint32)
    bank = fmd.StationBank(h, 8, incs, 300000, 32000, n_streams=4, device_id=0)
    refs = [sr.StationsRef(oracle, h, 8, incs[s], 300000, 32000, bank.shift) for s in range(4)]
    for n in (8 * 1000, 8 * 64, 8 * 4000, 8 * 333):
        data = rng.integers(0, 256, (4, n), dtype=np.uint8)
        got = bank.demodulate_batch(data)
        for s in range(4):
            exp = refs[s].feed(data[s])
            for k in range(3):
                assert np.array_equal(got[s, k], exp[k])
    g, p = bank.f64_stats()
    assert g > 0 and p == g, (g, p)


def _fm_capture(rng, fs, n, stations, amp=14.0, dev=75000.0):
    t = np.arange(n) / fs
    x = np.zeros(n, np.complex128)
    for off, tone in stations:
        phase = 2 * np.pi * off * t + (dev / tone) * np.sin(2 * np.pi * tone * t)
        x += amp * np.exp(1j * phase)
    x += rng.normal(0, 1.0, n) + 1j * rng.normal(0, 1.0, n)
    iq = np.empty(2 * n, np.uint8)
    iq[0::2] = np.clip(np.round(x.real + 127.5), 0, 255)
    iq[1::2] = np.clip(np.round(x.imag + 127.5), 0, 255)
    return iq


def _lowpass(T, cutoff):
    n = np.arange(T) - (T - 1) / 2
    h = np.sinc(2 * cutoff * n) * np.hamming(T)
    h = h / h.sum()
    return np.round(h * 2047 / np.abs(h).max()).astype(np.int16)


def test_physics_six_stations_each_hear_their_own_tone(fmd):
    fs, n = 2400000, 2400000 // 2
    stations = [(-1000000, 400.0), (-600000, 700.0), (-250000, 1100.0), (100000, 1700.0), (450000, 2300.0), (850000, 3100.0)]
    iq = _fm_capture(np.random.default_rng(41), fs, n, stations)
    h = _lowpass(64, 100000 / fs)
    incs = [fmd.phase_inc(off, fs) for off, _ in stations]
    bank = fmd.StationBank(h, 10, incs, 240000, 32000, shift=fmd.stations_auto_shift(h, incs, limit=16384), device_id=0)
    audio = bank.demodulate_batch(iq[None, :])[0].astype(np.float64)
    for k, (_, tone) in enumerate(stations):
        a = audio[k, 3200:]                                    # skip the start-up
        spec = np.abs(np.fft.rfft(a * np.hanning(a.size)))
        f = np.fft.rfftfreq(a.size, 1.0 / 32000)
        power = {tn: spec[np.abs(f - tn) < 15].max() for _, tn in stations}
        own = power[tone]
        for _, other in stations:
            if other != tone:
                assert 20 * np.log10(own / power[other]) >= 20.0, (k, tone, other, own, power[other])


def test_device_path_and_too_short(fmd, oracle):
    import torch
    rng = np.random.default_rng(51)
    S, K = 3, 5
    h = rng.integers(-900, 901, 30).astype(np.int16)
    incs = np.array([[int(x) for x in rng.integers(0, 1 << 32, K)] for _ in range(S)], np.uint32)
    bank = fmd.StationBank(h, 4, incs, 128000, 32000, n_streams=S, device_id=0)
    assert "fmd_stations" in bank.kernel_name()
    refs = [sr.StationsRef(oracle, h, 4, incs[s], 128000, 32000, bank.shift) for s in range(S)]
    dev = torch.device("cuda:0")
    for n in (8 * 2000, 8 * 3001):
        data = rng.integers(0, 256, (S, n), dtype=np.uint8)
        d_iq = torch.from_numpy(data).to(dev)
        cap = bank.out_cap(n)
        d_out = torch.zeros((S, K, cap), dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        got_n = bank.demodulate_device(d_iq.data_ptr(), n, d_out.data_ptr(), cap)
        bank.check()
        got = d_out.cpu().numpy()
        for s in range(S):
            exp = refs[s].feed(data[s])
            for k in range(K):
                assert got_n == exp[k].size and np.array_equal(got[s, k, :got_n], exp[k])
    before = [bank.get_state(s, k).as_dict() for s in range(S) for k in range(K)]
    tiny = torch.zeros((S, 8), dtype=torch.uint8, device=dev)
    out = torch.zeros((S, K, 4), dtype=torch.int16, device=dev)
    with pytest.raises(fmd.FmdError) as e:
        bank.demodulate_device(tiny.data_ptr(), 8, out.data_ptr(), 4)
    assert e.value.status == -3                               # FMD_ERR_TOO_SHORT
    assert [bank.get_state(s, k).as_dict() for s in range(S) for k in range(K)] == before
    data = rng.integers(0, 256, (S, 8 * 500), dtype=np.uint8)
    got = bank.demodulate_batch(data)
    for s in range(S):
        exp = refs[s].feed(data[s])
        for k in range(K):
            assert np.array_equal(got[s, k], exp[k])


def test_cli_station_mode_writes_one_file_per_station(fmd, tmp_path):
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "simple_fm_gpu")
    radio, cfg = fmd.optimal_settings(94_900_000, 170_000)
    capture, D = radio.capture_rate, cfg.downsample
    offs = [-300000, 0, 200000]
    iq = _fm_capture(np.random.default_rng(61), capture, 3 * fmd.DEFAULT_BUF_LENGTH // 2 + 500,
                     [(-300000, 500.0), (0, 900.0), (200000, 1300.0)], amp=30.0, dev=40000.0)
    (tmp_path / "cap.bin").write_bytes(iq.tobytes())
    p = subprocess.run([exe, "-S", ",".join(str(o) for o in offs), "-o", str(tmp_path / "st"), str(tmp_path / "cap.bin")],
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    shift = 0
    while -(-512 * D >> shift) > 16384:
        shift += 1
    bank = fmd.StationBank(np.ones(D, np.int16), D, [fmd.phase_inc(o, capture) for o in offs], cfg.rate_out, cfg.rate_resample,
                           shift=shift, device_id=0)
    n = fmd.DEFAULT_BUF_LENGTH
    exp = [[] for _ in offs]
    for b in range(iq.size // n):
        a = bank.demodulate_batch(iq[None, b * n:(b + 1) * n])
        for k in range(len(offs)):
            exp[k].append(a[0, k])
    for k in range(len(offs)):
        got = np.fromfile(str(tmp_path / ("st.%d.s16" % k)), dtype=np.int16)
        assert got.size > 0 and np.array_equal(got, np.concatenate(exp[k])), k
