"""Stereo station bank (include/fmd.h, fmd_stereo_*) on the MI355X: bit for bit against the test-side definition (tests/stereo_ref.py)
over the domain's corners, anchored to the channelizer (with pilot_min = 0 the output is the reference's discriminator and the FIR
over the channelizer's y), stereo separation at production shape, the pilot indicator, the device path on a caller's stream, refused
calls and the CLI.  Everything runs in this process."""
import os
import subprocess

import numpy as np
import pytest

import pyref
import stations_ref as sr
import stereo_ref as st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_SHORT = -3


def _bytes(rng, S, n):
    b = rng.integers(0, 256, (S, n), dtype=np.uint8)
    b[:, : n // 3] = np.where(rng.random((S, n // 3)) < 0.5, 0, 255)
    return b


def _refs(sb, incs, z=None):
    return [st.StereoRef(sb.taps, sb.decim, incs[s], sb.shift, sb.capture_rate, sb.audio_taps, sb.audio_decim, sb.block, sb.pilot_min,
                         sb.audio_shift, z=z) for s in range(sb.n_streams)]


def _check_call(fmd, sb, refs, data):
    """One call of every stream: bank and definition agree, or both refuse and the bank changes nothing."""
    if refs[0].completes(data.shape[1]) < 1:
        before = sb.outputs()
        with pytest.raises(fmd.FmdError) as e:
            sb.run_batch(data)
        assert e.value.status == TOO_SHORT and sb.outputs() == before
        return 0
    got = sb.run_batch(data)
    for s in range(data.shape[0]):
        exp = refs[s].feed(data[s])
        assert got.shape[2] == exp.shape[1] and np.array_equal(got[s], exp), (s, data.shape[1])
    assert sb.outputs() == refs[0].n_next
    return got.shape[2]


# (K, D, Ta, R, P, pilot_min): every corner value of K, D, Ta, R and P appears
CORNERS = [(1, 2, 1, 1, 1024, 1), (3, 10, 63, 5, 1024, None), (8, 64, 256, 32, 16384, 1), (32, 10, 256, 1, 1024, 1),
           (8, 2, 63, 32, 16384, 0), (1, 64, 1, 5, 1024, 16384), (32, 64, 63, 5, 16384, None)]


@pytest.mark.parametrize("K,D,Ta,R,P,pmin", CORNERS)
def test_definition_parity_corners(fmd, K, D, Ta, R, P, pmin):
    rng = np.random.default_rng(7000 + K * 100 + D + Ta + R)
    S = 2
    T = int(rng.integers(1, 129))
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    incs = np.array([[int(rng.integers(0, 1 << 32)) for _ in range(K)] for _ in range(S)], np.uint32)   # per-stream increments
    rate = 106000 * D + int(rng.integers(0, 50000)) * D
    g = rng.integers(-200, 201, Ta)
    g = (np.sign(g) * (np.abs(g) * 16383 // max(1, int(np.abs(g).sum())))).astype(np.int16)
    shift = fmd.stations_auto_shift(h, incs, limit=int(rng.choice([256, 2048, 16384])))
    sb = fmd.StereoBank(h, D, incs, rate, g, R, n_streams=S, block=P, pilot_min=pmin, audio_shift=int(rng.integers(0, 17)),
                        shift=shift, device_id=0)
    assert "fmd_stereo" in sb.kernel_name(0) and "fmd_stereo" in sb.kernel_name(1)
    refs = _refs(sb, incs, z=sr.z_corr)
    sizes = [8 * int(rng.integers(1, 40)), 8 * int(rng.integers(1, 600)), 8 * D * (Ta * R // 4 + 3), 8 * int(rng.integers(2000, 9000)),
             8 * 3, 8 * D * P // 2 + 8, 8 * int(rng.integers(100, 3000))]
    pending = np.zeros((S, 0), np.uint8)
    done = 0
    for n in sizes:
        data = np.concatenate([pending, _bytes(rng, S, n)], axis=1)
        got = _check_call(fmd, sb, refs, data)
        pending = data if got == 0 else np.zeros((S, 0), np.uint8)
        done += got
    assert done > 0
    for s in range(S):
        for k in range(K):
            assert sb.pilot(s, k) == refs[s].pilot(k), (s, k)
    sb.reset()
    assert sb.outputs() == 0
    refs = _refs(sb, incs)
    _check_call(fmd, sb, refs, _bytes(rng, S, 8 * D * (Ta * R // 4 + 40)))


def test_anchor_mono_is_the_channelizer_through_the_reference_discriminator(fmd):
    """pilot_min = 0: L == R == sat16(FIR(x) >> (audio_shift + 1)), x = pyref.polar_discriminant_fast over the channelizer's y."""
    rng = np.random.default_rng(31)
    D, T, R, fs = 10, 48, 5, 2400000
    h = st.lowpass(T, 120000 / fs)
    incs = [fmd.phase_inc(o, fs) for o in (-500000, 250000)]
    g = fmd.stereo_taps(fs // D, R, 31)
    sb = fmd.StereoBank(h, D, incs, fs, g, R, pilot_min=0, device_id=0)
    ch = fmd.Channelizer(h, D, incs, shift=sb.shift, device_id=0)
    ys, outs = [], []
    for n in (8 * 2000, 8 * 777, 8 * 3001):
        data = rng.integers(0, 256, (1, n), dtype=np.uint8)
        ys.append(ch.run_batch(data)[0].astype(np.int64))
        outs.append(sb.run_batch(data)[0])
    y = np.concatenate(ys, axis=1)
    got = np.concatenate(outs, axis=1)
    assert np.array_equal(got[..., 0], got[..., 1])
    for k in range(len(incs)):
        prev, x = (0, 0), []
        for m in range(y.shape[1]):
            cur = (int(y[k, m, 0]), int(y[k, m, 1]))
            x.append(pyref.wrap16(pyref.polar_discriminant_fast(cur, prev)))
            prev = cur
        M = np.correlate(np.array(x, np.int64), g.astype(np.int64), "valid")[::R]
        exp = np.clip(M >> (sb.audio_shift + 1), -32768, 32767)
        assert got.shape[1] == exp.size and np.array_equal(got[k, :, 0], exp), k


def _production(fmd, S):
    fs, D, T, R, Ta = 2400000, 10, 64, 5, 127
    h = st.lowpass(T, 130000 / fs)
    g = fmd.stereo_taps(fs // D, R, Ta)
    return fs, D, h, R, g


def test_physics_separation_64_streams_production_shape(fmd):
    """64 streams x 262144 B, two calls, two stations per stream, a 1 kHz tone on L only at four pilot phases: the tone on R is
    >= 25 dB down, the pilot is present with a level near 0.1 x 75 kHz in discriminator units; sampled streams bit-exact (z_corr)."""
    import torch
    S, n = 64, fmd.DEFAULT_BUF_LENGTH
    fs, D, h, R, g = _production(fmd, S)
    offs = [-400000, 300000]
    phis = [0, 90, 180, 271]
    tone = lambda t: 0.15 * np.sin(2 * np.pi * 1000 * t)
    zero = lambda t: 0 * t
    caps = [st.synth_iq(n, fs, [(o, tone, zero, np.deg2rad(p), True) for o in offs], seed=p) for p in phis]   # 2 calls each
    incs = [fmd.phase_inc(o, fs) for o in offs]
    sb = fmd.StereoBank(h, D, incs, fs, g, R, n_streams=S, device_id=0)
    sample = [0, 1, 2, 3, 37, 63]
    refs = {s: st.StereoRef(h, D, incs, sb.shift, fs, g, R, sb.block, sb.pilot_min, sb.audio_shift, z=sr.z_corr) for s in sample}
    cap = sb.out_cap(n)
    d_out = torch.empty((S, 2, cap, 2), dtype=torch.int16, device="cuda")
    audio = []
    for call in range(2):
        data = np.stack([caps[s % 4][call * n:(call + 1) * n] for s in range(S)])
        d_iq = torch.from_numpy(data).cuda()
        m = sb.run_device(d_iq.data_ptr(), n, d_out.data_ptr(), cap)
        sb.check()
        got = d_out[:, :, :m].cpu().numpy()
        for s in sample:
            assert np.array_equal(got[s], refs[s].feed(data[s])), (call, s)
        audio.append(got)
    a = np.concatenate(audio, axis=2)
    fa = fs / D / R
    skip = 2 * sb.block // R
    for s in range(4):
        for k in range(2):
            Ld, Rd = st.tone_db(a[s, k, :, 0], 1000, fa, skip), st.tone_db(a[s, k, :, 1], 1000, fa, skip)
            assert Ld - Rd >= 25, (phis[s], k, Ld, Rd)
            present, level = sb.pilot(s, k)
            assert present and 900 <= level <= 1600, (s, k, level)


def test_no_pilot_is_mono_and_pilot_reports_absent(fmd):
    fs, D, h, R, g = _production(fmd, 1)
    tone = lambda t: 0.15 * np.sin(2 * np.pi * 1000 * t)
    zero = lambda t: 0 * t
    iq = st.synth_iq(fmd.DEFAULT_BUF_LENGTH // 2, fs, [(200000, tone, zero, 0.3, False)], seed=5)
    sb = fmd.StereoBank(h, D, [fmd.phase_inc(200000, fs)], fs, g, R, device_id=0)
    a = sb.run_batch(iq[None, :])
    assert a.shape[2] > 0 and np.array_equal(a[..., 0], a[..., 1])
    assert sb.pilot(0, 0)[0] is False


def test_run_device_on_a_callers_stream_and_too_short(fmd):
    import torch
    rng = np.random.default_rng(55)
    fs, D, h, R, g = _production(fmd, 3)
    S = 3
    incs = np.array([[fmd.phase_inc(int(o), fs) for o in rng.integers(-900000, 900000, 4)] for _ in range(S)], np.uint32)
    sb = fmd.StereoBank(h, D, incs, fs, g, R, n_streams=S, block=1024, device_id=0)
    refs = _refs(sb, incs)
    with pytest.raises(fmd.FmdError) as e:                  # the first audio sample needs 64 + 10 * 126 samples
        sb.run_batch(np.zeros((S, 8 * 100), np.uint8))
    assert e.value.status == TOO_SHORT and sb.outputs() == 0
    with pytest.raises(fmd.FmdError) as e:
        sb.run_batch(np.zeros((S, 12), np.uint8))
    assert e.value.status == -2
    stream = torch.cuda.Stream()
    SENT = -4321
    for n in (8 * 1001, 8 * 7, 8 * 2403, 8 * 50, 8 * 9000):
        data = _bytes(rng, S, n)
        cap = sb.out_cap(n) + 3
        d_out = torch.full((S, 4, cap, 2), SENT, dtype=torch.int16, device="cuda")
        buf = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        if refs[0].completes(n) < 1:
            before = sb.outputs()
            with pytest.raises(fmd.FmdError) as e:
                sb.run_device(buf.data_ptr(), n, d_out.data_ptr(), cap, stream.cuda_stream)
            assert e.value.status == TOO_SHORT and sb.outputs() == before
            continue
        m = sb.run_device(buf.data_ptr(), n, d_out.data_ptr(), cap, stream.cuda_stream)
        sb.check()
        got = d_out.cpu().numpy()
        for s in range(S):
            assert np.array_equal(got[s, :, :m], refs[s].feed(data[s])), (n, s)
            assert (got[s, :, m:] == SENT).all()
    big = torch.zeros((S, 8 * 40000), dtype=torch.uint8, device="cuda")
    with pytest.raises(fmd.FmdError) as e:
        sb.run_device(big.data_ptr(), 8 * 40000, d_out.data_ptr(), 10, stream.cuda_stream)
    assert e.value.status == -5


def test_cli_stereo_mode_writes_interleaved_lr(fmd, tmp_path):
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "simple_fm_gpu")
    radio, cfg = fmd.optimal_settings(94_900_000, 170_000)
    capture, D = radio.capture_rate, cfg.downsample
    offs = [-300000, 0, 200000]
    rng = np.random.default_rng(62)
    iq = rng.integers(100, 156, 3 * fmd.DEFAULT_BUF_LENGTH // 2 + 504, dtype=np.uint8)
    (tmp_path / "cap.bin").write_bytes(iq.tobytes())
    p = subprocess.run([exe, "-S", ",".join(str(o) for o in offs), "-2", "-o", str(tmp_path / "st"), str(tmp_path / "cap.bin")],
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    f_m = capture // D
    R = max(1, f_m // 48000)
    assert ("%.3f Hz" % (capture / D / R)) in p.stderr.decode()
    shift = 0
    while -(-512 * D >> shift) > 256:
        shift += 1
    sb = fmd.StereoBank(np.ones(D, np.int16), D, [fmd.phase_inc(o, capture) for o in offs], capture, fmd.stereo_taps(f_m, R, 127), R,
                        shift=shift, device_id=0)
    n = fmd.DEFAULT_BUF_LENGTH
    exp = [[] for _ in offs]
    for b in range(iq.size // n):
        a = sb.run_batch(iq[None, b * n:(b + 1) * n])
        for k in range(len(offs)):
            exp[k].append(a[0, k].ravel())
    for k in range(len(offs)):
        got = np.fromfile(str(tmp_path / ("st.%d.s16" % k)), dtype=np.int16)
        assert got.size > 0 and np.array_equal(got, np.concatenate(exp[k])), k
