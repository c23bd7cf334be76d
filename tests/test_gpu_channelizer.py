"""Channelizer (include/fmd.h, fmd_channelizer_*) on the MI355X: bit for bit against the test-side definition
(tests/channelizer_ref.py) over the whole filter domain, against the reference's low_pass_complex (inc = 0 on rotated bytes), against
the station bank (its audio is the oracle's fm_demod + low_pass_real over the channelizer's output), call splitting and reset,
refused calls, the device entry point, production size, physics and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import channelizer_ref as cr
import stations_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_SHORT = -3


def _shift(h, incs, limit=16384):
    g, s = sr.max_gain(h, incs), 0
    while -(-256 * g >> s) > limit:
        s += 1
    return s


def _incs(rng, S, K):
    fixed = [0, 1 << 30, (1 << 32) - (1 << 30), 1 << 31]
    return np.array([[fixed[k] if k < len(fixed) and s == 0 else int(rng.integers(0, 1 << 32)) for k in range(K)] for s in range(S)],
                    dtype=np.uint32)


def _bytes(rng, S, n):
    b = rng.integers(0, 256, (S, n), dtype=np.uint8)
    b[:, : n // 3] = np.where(rng.random((S, n // 3)) < 0.5, 0, 255)          # full-scale stretch
    return b


def _check_call(fmd, ch, refs, data):
    """One call of every stream: the channelizer and the definition agree, or both refuse (and the channelizer changes nothing)."""
    S = data.shape[0]
    if refs[0].outputs_after(data.shape[1] // 2) - refs[0].m_next < 1:
        before = ch.outputs()
        with pytest.raises(fmd.FmdError) as e:
            ch.run_batch(data)
        assert e.value.status == TOO_SHORT and ch.outputs() == before
        return 0
    got = ch.run_batch(data)
    for s in range(S):
        exp = refs[s].feed(data[s])
        assert got.shape[2] == exp.shape[1] and np.array_equal(got[s], exp), (s, data.shape[1])
    assert ch.outputs() == refs[0].m_next
    return got.shape[2]


@pytest.mark.parametrize("K,digits", [(1, 2), (1, 1), (3, 2), (8, 1), (8, 2), (32, 1), (32, 2)])
def test_definition_parity_random_shapes(fmd, K, digits):
    rng = np.random.default_rng(2000 + 10 * K + digits)
    S = 2
    for case in range(3):
        D = int(rng.choice([2, 4, 6, 10, 16, 24, 38, 64]))
        T = [int(rng.integers(1, D + 1)), int(rng.integers(1, 257)), 256][case]
        if digits == 1:
            h = rng.integers(-127, 128, T).astype(np.int16) // 2   # every |W| <= 127 -> the one-digit form
        else:
            h = rng.integers(-2047, 2048, T).astype(np.int16)
        incs = _incs(rng, S, K)
        ch = fmd.Channelizer(h, D, incs, n_streams=S, device_id=0)
        assert ch.shift == _shift(h, incs) and "fmd_channelizer" in ch.kernel_name()
        refs = [cr.ChannelizerRef(h, D, incs[s], ch.shift, z=sr.z_corr) for s in range(S)]
        for n in (8 * (T // 4 + 1), 8 * int(rng.integers(1, 400)), 8 * int(rng.integers(2000, 9000)), 8 * 3, 8 * (64 * D + 5)):
            _check_call(fmd, ch, refs, _bytes(rng, S, n))


@pytest.mark.parametrize("D,T,hval", [(2, 128, 1024), (10, 64, 2047), (64, 256, -2047), (64, 3, 2047), (8, 8, 127)])
def test_full_scale_at_the_16384_edge(fmd, D, T, hval):
    """Full-scale bytes and taps, the shift at the smallest value the 16384 rule admits, every phase class."""
    rng = np.random.default_rng(D * 1000 + T)
    h = np.full(T, hval, np.int16)
    incs = np.array([0, 1 << 29, 3 << 29, 1 << 31, int(rng.integers(0, 1 << 32))], np.uint32)
    s = _shift(h, incs)
    assert s == 0 or -(-256 * sr.max_gain(h, incs) >> (s - 1)) > 16384
    ch = fmd.Channelizer(h, D, incs, shift=s, device_id=0)
    ref = cr.ChannelizerRef(h, D, incs, s, z=sr.z_corr)
    peak = 0
    for pattern in ([255, 255], [0, 0], [255, 0], [0, 255]):
        data = np.tile(np.array(pattern, np.uint8), 4 * (40 * D + T))[None, :]
        got = ch.run_batch(data)
        exp = ref.feed(data[0])
        assert np.array_equal(got[0], exp)
        peak = max(peak, int(np.abs(exp).max()))
    assert 2048 < peak <= 16384, peak                      # the inc = 0 station alone reaches 128 T |h| / 2^shift


def test_reference_anchor_is_low_pass_complex(fmd, oracle):
    """inc = 0, h = 1...1, T = D, shift = 0 fed rot(B): the oracle's low_pass_complex (simple_fm.rs:337-352) of B, call for call."""
    rng = np.random.default_rng(77)
    for D in (2, 6, 10, 64):
        S = 2
        ch = fmd.Channelizer(np.ones(D, np.int16), D, [[0]] * S, n_streams=S, shift=0, device_id=0)
        ods = [oracle.new(oracle.config(D, 240000, 32000)) for _ in range(S)]
        for n in (8 * 5 * D, 8 * 37, 8 * (5 * D + 3), 65536, fmd.DEFAULT_BUF_LENGTH, "full"):
            B = (np.tile(np.array([255, 0, 0, 255, 255, 255, 0, 0], np.uint8), (S, 40 * D)) if n == "full"
                 else rng.integers(0, 256, (S, n), dtype=np.uint8))
            R = np.stack([sr.rot90(B[s]) for s in range(S)])
            got = ch.run_batch(R)
            for s in range(S):
                o = B[s].copy()
                assert oracle.lib.fmo_rotate_90(o.ctypes.data_as(C.POINTER(C.c_uint8)), o.size) == 0
                exp = cr.oracle_low_pass_complex(oracle, ods[s], o)
                assert np.array_equal(got[s, 0], exp), (D, n, s)


def test_bank_anchor_station_bank_audio_is_oracle_demod_over_the_channelizer(fmd, oracle):
    rng = np.random.default_rng(88)
    S, D, fast, slow = 2, 10, 240000, 32000
    h = rng.integers(-1500, 1501, 64).astype(np.int16)
    incs = np.array([[fmd.phase_inc(o, 2400000) for o in (-700000, -100000, 0, 250000, 900000)] for _ in range(S)], np.uint32)
    shift = _shift(h, incs)
    bank = fmd.StationBank(h, D, incs, fast, slow, n_streams=S, shift=shift, device_id=0)
    ch = fmd.Channelizer(h, D, incs, n_streams=S, shift=shift, device_id=0)
    demods = [[oracle.new(oracle.config(D, fast, slow)) for _ in range(incs.shape[1])] for _ in range(S)]
    for n in (8 * 3000, 8 * 257, fmd.DEFAULT_BUF_LENGTH, 8 * 40, 8 * 1234):
        data = _bytes(rng, S, n)
        audio = bank.demodulate_batch(data)
        y = ch.run_batch(data)
        for s in range(S):
            exp = cr.oracle_chain(oracle, demods[s], y[s])
            for k in range(incs.shape[1]):
                assert np.array_equal(audio[s, k], exp[k]), (n, s, k)


def test_call_split_invariance_short_calls_and_reset(fmd):
    rng = np.random.default_rng(99)
    for D, T in ((4, 200), (10, 64), (64, 20), (2, 1)):
        h = rng.integers(-2047, 2048, T).astype(np.int16)
        incs = [fmd.phase_inc(o, 2400000) for o in (-500000, 123456, 800000)]
        data = rng.integers(0, 256, (2, 8 * (300 * D + T)), dtype=np.uint8)
        one = fmd.Channelizer(h, D, incs, n_streams=2, device_id=0)
        whole = one.run_batch(data)
        many = fmd.Channelizer(h, D, incs, n_streams=2, device_id=0)
        parts, pos, pending = [], 0, np.zeros((2, 0), np.uint8)
        while pos < data.shape[1]:
            n = min(8 * int(rng.integers(1, T // 4 + 2 * D + 2)) if rng.random() < 0.7 else 8 * int(rng.integers(1, 3000)),
                    data.shape[1] - pos)
            buf = np.concatenate([pending, data[:, pos:pos + n]], axis=1)
            pos += n
            try:
                parts.append(many.run_batch(buf))
                pending = np.zeros((2, 0), np.uint8)
            except fmd.FmdError as e:
                assert e.status == TOO_SHORT
                pending = buf
        assert np.array_equal(np.concatenate(parts, axis=2), whole), (D, T)
        assert many.outputs() == whole.shape[2] == one.outputs()
        one.reset()
        assert one.outputs() == 0
        assert np.array_equal(one.run_batch(data), whole)
        many.reset()
        first = many.run_batch(data[:, :8 * 100 * D])
        assert np.array_equal(first, whole[:, :, :first.shape[2]])


def test_too_short_changes_nothing(fmd):
    rng = np.random.default_rng(111)
    h = rng.integers(-2047, 2048, 64).astype(np.int16)
    incs = [fmd.phase_inc(o, 2400000) for o in (-300000, 0, 600000)]
    ch = fmd.Channelizer(h, 10, incs, device_id=0)
    ref = cr.ChannelizerRef(h, 10, incs, ch.shift)
    with pytest.raises(fmd.FmdError) as e:                   # the first output needs 64 samples
        ch.run_batch(np.zeros((1, 8 * 15), np.uint8))
    assert e.value.status == TOO_SHORT and ch.outputs() == 0
    with pytest.raises(fmd.FmdError) as e:
        ch.run_batch(np.zeros((1, 12), np.uint8))
    assert e.value.status == -2                              # FMD_ERR_BAD_LENGTH
    for n in (8 * 333, 8, 8 * 2, 8 * 5000, 8, 8 * 3):
        _check_call(fmd, ch, [ref], rng.integers(0, 256, (1, n), dtype=np.uint8))


def test_device_path_unaligned_and_padded(fmd):
    """d_iq 4 bytes past an aligned address (nbytes % 16 == 8: no row is 16-byte aligned), out_cap padded so that rows are not
    16-byte aligned (and, second handle, padded to a multiple of 4 so that they are); the padding keeps its sentinel."""
    import torch
    rng = np.random.default_rng(808)
    S, K, D = 3, 6, 6
    h = rng.integers(-2047, 2048, 59).astype(np.int16)
    incs = _incs(rng, S, K)
    dev = torch.device("cuda:0")
    SENT = -12345
    for pad in (37, 64):
        ch = fmd.Channelizer(h, D, incs, n_streams=S, device_id=0)
        refs = [cr.ChannelizerRef(h, D, incs[s], ch.shift) for s in range(S)]
        for n in (8 * 1001, 8 * 7, 8 * 2403, 8):
            data = _bytes(rng, S, n)
            buf = torch.zeros(S * n + 16, dtype=torch.uint8, device=dev)
            buf[4:4 + S * n] = torch.from_numpy(data.ravel()).to(dev)
            cap = ch.out_cap(n) + pad
            cap += (-cap) % 4 if pad == 64 else 0
            d_out = torch.full((S, K, cap, 2), SENT, dtype=torch.int16, device=dev)
            torch.cuda.synchronize()
            if refs[0].outputs_after(n // 2) - refs[0].m_next < 1:
                with pytest.raises(fmd.FmdError) as e:
                    ch.run_device(buf.data_ptr() + 4, n, d_out.data_ptr(), cap)
                assert e.value.status == TOO_SHORT
                continue
            got_n = ch.run_device(buf.data_ptr() + 4, n, d_out.data_ptr(), cap)
            ch.check()
            got = d_out.cpu().numpy()
            for s in range(S):
                exp = refs[s].feed(data[s])
                assert got_n == exp.shape[1] and np.array_equal(got[s, :, :got_n], exp), (pad, n, s)
                assert (got[s, :, got_n:] == SENT).all(), (pad, n, s)
        big = torch.zeros((S, 8 * 4000), dtype=torch.uint8, device=dev)
        with pytest.raises(fmd.FmdError) as e:                # out_cap too small
            ch.run_device(big.data_ptr(), 8 * 4000, d_out.data_ptr(), 10)
        assert e.value.status == -5                          # FMD_ERR_CAPACITY


def test_production_size_512_streams(fmd):
    """512 streams x 262144 B, two calls, on the device path; a sample of streams against the definition (z_corr)."""
    import torch
    S, n, D, T, K = 512, 262144, 10, 64, 8
    rng = np.random.default_rng(512)
    nn = np.arange(T) - (T - 1) / 2
    proto = np.sinc(2 * (100000 / 2400000) * nn) * np.hamming(T)
    h = np.round(proto / np.abs(proto).max() * 2047).astype(np.int16)
    incs = np.array([[fmd.phase_inc(int(o), 2400000) for o in np.linspace(-1000000, 1000000, K) + rng.integers(-5000, 5000)]
                     for _ in range(S)], np.uint32)
    ch = fmd.Channelizer(h, D, incs, n_streams=S, device_id=0)
    sample = [0, 1, 255, 300, 511]
    refs = {s: cr.ChannelizerRef(h, D, incs[s], ch.shift, z=sr.z_corr) for s in sample}
    cap = ch.out_cap(n)
    d_out = torch.empty((S, K, cap, 2), dtype=torch.int16, device="cuda")
    for call in range(2):
        data = rng.integers(0, 256, (S, n), dtype=np.uint8)
        d_iq = torch.from_numpy(data).cuda()
        got_n = ch.run_device(d_iq.data_ptr(), n, d_out.data_ptr(), cap)
        ch.check()
        got = d_out[sample].cpu().numpy()
        for i, s in enumerate(sample):
            exp = refs[s].feed(data[s])
            assert got_n == exp.shape[1] and np.array_equal(got[i, :, :got_n], exp), (call, s)


def test_physics_tone_lands_at_plus_5khz_in_each_baseband(fmd):
    fs, n, D = 2400000, 2400000 // 4, 10
    offs = [-900000, -250000, 0, 400000, 1000000]
    t = np.arange(n) / fs
    x = sum(20.0 * np.exp(2j * np.pi * (o + 5000.0) * t) for o in offs)
    x = x + np.random.default_rng(5).normal(0, 1.0, n) + 1j * np.random.default_rng(6).normal(0, 1.0, n)
    iq = np.empty(2 * n, np.uint8)
    iq[0::2] = np.clip(np.round(x.real + 127.5), 0, 255)
    iq[1::2] = np.clip(np.round(x.imag + 127.5), 0, 255)
    T = 64
    nn = np.arange(T) - (T - 1) / 2
    proto = np.sinc(2 * (60000 / fs) * nn) * np.hamming(T)
    h = np.round(proto / np.abs(proto).max() * 2047).astype(np.int16)
    ch = fmd.Channelizer(h, D, [fmd.phase_inc(o, fs) for o in offs], device_id=0)
    y = fmd.as_complex(ch.run_batch(iq[None, :])[0])
    f = np.fft.fftfreq(y.shape[1] - 100, D / fs)
    for k in range(len(offs)):
        spec = np.abs(np.fft.fft(y[k, 100:] * np.hanning(y.shape[1] - 100)))
        assert abs(f[np.argmax(spec)] - 5000.0) < 2 * fs / D / spec.size, (k, f[np.argmax(spec)])


def test_cli_iq_mode_writes_the_channelizer_output(fmd, tmp_path):
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "simple_fm_gpu")
    radio, cfg = fmd.optimal_settings(94_900_000, 170_000)
    capture, D = radio.capture_rate, cfg.downsample
    offs = [-300000, 0, 200000]
    rng = np.random.default_rng(61)
    iq = rng.integers(0, 256, 3 * fmd.DEFAULT_BUF_LENGTH // 2 + 504, dtype=np.uint8)
    (tmp_path / "cap.bin").write_bytes(iq.tobytes())
    p = subprocess.run([exe, "-S", ",".join(str(o) for o in offs), "-I", "-o", str(tmp_path / "st"), str(tmp_path / "cap.bin")],
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    shift = 0
    while -(-512 * D >> shift) > 16384:
        shift += 1
    ch = fmd.Channelizer(np.ones(D, np.int16), D, [fmd.phase_inc(o, capture) for o in offs], shift=shift, device_id=0)
    n = fmd.DEFAULT_BUF_LENGTH
    exp = [[] for _ in offs]
    for b in range(iq.size // n):
        a = ch.run_batch(iq[None, b * n:(b + 1) * n])
        for k in range(len(offs)):
            exp[k].append(a[0, k].ravel())
    for k in range(len(offs)):
        got = np.fromfile(str(tmp_path / ("st.%d.cs16" % k)), dtype=np.int16)
        assert got.size > 0 and np.array_equal(got, np.concatenate(exp[k])), k
        assert not (tmp_path / ("st.%d.s16" % k)).exists()
