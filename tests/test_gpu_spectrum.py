"""Power-spectrum scanner (include/fmd.h, fmd_spectrum_*) on the MI355X: bit for bit against the test-side definition
(tests/spectrum_ref.py) over every bin count, hop class and tap form, the extreme magnitudes, the device path with accumulation,
the refusals that need a handle, the physics of finding six FM stations and tuning a station bank to them, and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import spectrum_ref as spr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(rng, S, nbytes):
    b = rng.integers(0, 256, (S, nbytes), dtype=np.uint8)
    for s in range(S):                                           # runs of 0 and of 255
        for v in (0, 255):
            a = int(rng.integers(0, nbytes - nbytes // 8))
            b[s, a:a + nbytes // 8] = v
    return b


CASES = [(N, hop, d) for N in spr.BINS for hop in sorted({N, N // 2, 8}) for d in (1, 2)]


@pytest.mark.parametrize("N,hop,digits", CASES)
def test_definition_parity(fmd, N, hop, digits):
    rng = np.random.default_rng(1000 * N + 10 * hop + digits)
    S = int(rng.choice([1, 2, 5, 17, 64]))
    w = spr.hann(N, 127) if digits == 1 else rng.integers(-2047, 2048, N).astype(np.int16)
    if digits == 1:
        w[int(rng.integers(0, N))] = -127
    assert spr.digits(w) == digits
    shift = int(rng.integers(0, 24))
    sp = fmd.Spectrum(N, hop, window=w, shift=shift, n_streams=S, device_id=0)
    assert sp.tap_digits() == digits and "fmd_spectrum" in sp.kernel_name()
    F = int(rng.integers(1, 300))
    partial = int(rng.integers(0, hop))                          # samples that do not fill a frame
    nbytes = 2 * (N + hop * (F - 1) + partial)
    nbytes += (-nbytes) % 8
    data = _bytes(rng, S, nbytes)
    assert sp.frames(nbytes) == spr.frames(N, hop, nbytes) >= F
    got = sp.power_batch(data)
    assert np.array_equal(got, spr.power(w, hop, shift, data)), (N, hop, digits, S, nbytes)
    # a second call on the same handle carries nothing: one frame
    one = data[:, nbytes - 2 * N:]
    assert np.array_equal(sp.power_batch(one), spr.power(w, hop, shift, one))


def test_extreme_full_scale_under_a_2047_window(fmd):
    N = 256
    rng = np.random.default_rng(7)
    w = np.where(rng.random(N) < 0.5, -2047, 2047).astype(np.int16)
    S, nbytes = 3, 2 * (N + 8 * 40)
    data = np.where(rng.random((S, nbytes)) < 0.5, 0, 255).astype(np.uint8)
    data[1] = np.tile(np.array([255, 0], np.uint8), nbytes // 2)
    data[2] = 255
    for hop in (8, N):
        sp = fmd.Spectrum(N, hop, window=w, shift=0, n_streams=S, device_id=0)
        assert sp.tap_digits() == 2
        assert np.array_equal(sp.power_batch(data), spr.power(w, hop, 0, data)), hop


def test_device_path_accumulates_on_a_side_stream_and_too_short_writes_nothing(fmd):
    import torch
    N, hop, S = 128, 64, 4
    rng = np.random.default_rng(9)
    sp = fmd.Spectrum(N, hop, shift=3, n_streams=S, device_id=0)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    calls = [_bytes(rng, S, n) for n in (8 * 1000, 8 * 333, 16 * 1024)]
    d_power = torch.full((S, N), -1, dtype=torch.int64, device=dev)
    singles = []
    with torch.cuda.stream(side):
        d_iq = [torch.from_numpy(c).to(dev) for c in calls]
        for i, (c, t) in enumerate(zip(calls, d_iq)):
            sp.power_device(t.data_ptr(), c.shape[1], d_power.data_ptr(), accumulate=i > 0, stream=side.cuda_stream)
    sp.check()
    side.synchronize()
    total = d_power.cpu().numpy().view(np.uint64)
    for c in calls:
        singles.append(sp.power_batch(c))
        assert np.array_equal(singles[-1], spr.power(sp.window, hop, 3, c))
    assert np.array_equal(total, singles[0] + singles[1] + singles[2])
    # refusals with a handle: nothing is written
    before = d_power.clone()
    tiny = torch.zeros((S, 2 * N), dtype=torch.uint8, device=dev)
    with pytest.raises(fmd.FmdError) as e:
        sp.power_device(tiny.data_ptr(), 2 * N - 8, d_power.data_ptr(), accumulate=False, stream=side.cuda_stream)
    assert e.value.status == -3                                  # FMD_ERR_TOO_SHORT
    with pytest.raises(fmd.FmdError) as e:
        sp.power_device(tiny.data_ptr(), 2 * N - 4, d_power.data_ptr(), accumulate=False, stream=side.cuda_stream)
    assert e.value.status == -2                                  # FMD_ERR_BAD_LENGTH
    with pytest.raises(fmd.FmdError) as e:
        sp.power_batch(np.zeros((S, 2 * N - 8), np.uint8))
    assert e.value.status == -3
    sp.check()
    torch.cuda.synchronize()
    assert torch.equal(d_power, before)


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


def test_physics_scan_finds_six_stations_and_the_bank_hears_each(fmd):
    fs, n, N = 2400000, 2400000 // 2, 256
    stations = [(-1000000, 400.0), (-600000, 700.0), (-250000, 1100.0), (100000, 1700.0), (450000, 2300.0), (850000, 3100.0)]
    iq = _fm_capture(np.random.default_rng(41), fs, n, stations)
    sp = fmd.Spectrum(N, shift=16, device_id=0)
    power = sp.power_batch(iq[None, :])[0]
    offs, bins = fmd.find_stations(power, fs, count=8)
    truth = np.array([o for o, _ in stations], np.float64)
    assert offs.size == len(stations), offs
    assert np.all(np.abs(offs - truth) <= fs / N), (offs, truth)
    assert np.allclose(sp.bin_offsets_hz(fs)[bins], offs, atol=fs / N / 2)
    h = _lowpass(64, 100000 / fs)
    incs = [sp.bin_inc(b) for b in bins]
    bank = fmd.StationBank(h, 10, incs, 240000, 32000, shift=fmd.stations_auto_shift(h, incs, limit=16384), device_id=0)
    audio = bank.demodulate_batch(iq[None, :])[0].astype(np.float64)
    for k, (_, tone) in enumerate(stations):
        a = audio[k, 3200:]                                    # skip the start-up
        a = a - a.mean()                                       # (a bin centre is up to half a bin off the carrier: a DC offset)
        spec = np.abs(np.fft.rfft(a * np.hanning(a.size)))
        f = np.fft.rfftfreq(a.size, 1.0 / 32000)
        pw = {tn: spec[np.abs(f - tn) < 15].max() for _, tn in stations}
        for _, other in stations:
            if other != tone:
                assert 20 * np.log10(pw[tone] / pw[other]) >= 20.0, (k, tone, other)


def test_offset_tuned_station_peaks_at_three_quarters(fmd):
    """optimal_settings' offset tuning (simple_fm.rs:194-195) puts the wanted station at -capture_rate / 4: bin 3 N / 4."""
    radio, _ = fmd.optimal_settings(94_900_000, 170_000)
    fs = radio.capture_rate
    for N in (64, 256):
        iq = _fm_capture(np.random.default_rng(N), fs, 4 * fmd.DEFAULT_BUF_LENGTH // 2 // 2, [(-fs / 4, 1000.0)], amp=30.0, dev=5000.0)
        sp = fmd.Spectrum(N, shift=12, device_id=0)
        power = sp.power_batch(iq[None, :])[0]
        offs, bins = fmd.find_stations(power, fs, count=1)
        assert list(bins) == [3 * N // 4], (N, offs, bins)
        assert abs(offs[0] + fs / 4) < fs / N / 2


def test_cli_power_mode_prints_the_accumulated_spectrum(fmd, tmp_path):
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "simple_fm_gpu")
    fs, N, hop = 2400000, 128, 64
    n = fmd.DEFAULT_BUF_LENGTH
    iq = _fm_capture(np.random.default_rng(61), fs, (2 * n + 1000) // 2, [(-300000, 500.0), (200000, 1300.0)], amp=30.0)
    (tmp_path / "cap.bin").write_bytes(iq.tobytes())
    p = subprocess.run([exe, "-s", str(fs), "-P", str(N), "-H", str(hop), str(tmp_path / "cap.bin")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().split("\n")
    rows = [ln.split() for ln in lines if ln.strip()]
    assert len(rows) == N
    sp = fmd.Spectrum(N, hop, shift=16, device_id=0)
    exp = sp.power_batch(iq[None, :n])[0] + sp.power_batch(iq[None, n:2 * n])[0]
    order = np.fft.fftshift(np.arange(N))                       # frequency order
    assert [int(r[1]) for r in rows] == [int(v) for v in exp[order]]
    assert np.allclose([float(r[0]) for r in rows], sp.bin_offsets_hz(fs)[order], atol=1e-3)
