"""RDS bank (include/fmd.h, fmd_rds_*) on the MI355X: bit for bit against the test-side definition (tests/rds_ref.py) -- the issue's
shape, the same bytes re-cut, the domain's corners, a refused call, the device path on a caller's stream, the pilot report against
the stereo bank's -- and end to end through the host decoder, in Python and through the CLI."""
import os
import subprocess

import numpy as np
import pytest

import rds_ref as rr
import stations_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_SHORT = -3


def _taps(rng, Ta):
    g = rng.integers(-200, 201, Ta)
    g[g == 0] = 1
    return (np.sign(g) * np.maximum(1, np.abs(g) * 16000 // int(np.abs(g).sum()))).astype(np.int16) if Ta > 1 else np.array([16383], np.int16)


def _refs(rb, incs):
    return [rr.RdsRef(rb.taps, rb.decim, incs[s], rb.shift, rb.capture_rate, rb.rds_taps, rb.out_decim, rb.rds_shift, rb.block,
                      rb.pilot_min, z=sr.z_corr) for s in range(rb.n_streams)]


@pytest.fixture(scope="module")
def issue_case(fmd):
    """2 streams x 2 stations, D = 2, capture_rate 256000, R = 16, Ta = 255, 3 x 65536 B; station 1 of every stream has inc = 0 and
    stream 1 is all zero bytes.  (bank arguments, bytes, the definition's output)"""
    rng = np.random.default_rng(2024)
    h = rr.front_taps()
    incs = np.array([[sr.phase_inc(40000, rr.FS), 0], [sr.phase_inc(-70000, rr.FS), 0]], np.uint32)
    g, rs = fmd.rds_taps(rr.FS // rr.D, rr.R, 255)
    data = rng.integers(0, 256, (2, 3 * 65536), dtype=np.uint8)
    data[1] = 0
    shift = fmd.stations_auto_shift(h, incs, limit=2048)
    refs = [rr.RdsRef(h, rr.D, incs[s], shift, rr.FS, g, rr.R, rs, 4096, 1, z=sr.z_corr) for s in range(2)]
    exp = np.stack([refs[s].feed(data[s]) for s in range(2)])
    return dict(h=h, incs=incs, g=g, rs=rs, shift=shift), data, exp


def _bank(fmd, a):
    return fmd.RdsBank(a["h"], rr.D, a["incs"], rr.FS, a["g"], rr.R, n_streams=2, rds_shift=a["rs"], shift=a["shift"], pilot_min=1, device_id=0)


def test_parity_three_calls(fmd, issue_case):
    args, data, exp = issue_case
    rb = _bank(fmd, args)
    assert rb.kernel_name(0) == "fmd_sto::fmd_stereo_mpx_kernel" and "fmd_rds_baseband_kernel" in rb.kernel_name(1)
    got = np.concatenate([rb.run_batch(data[:, c * 65536:(c + 1) * 65536]) for c in range(3)], axis=2)
    assert got.dtype == np.int16 and got.shape == exp.shape and np.array_equal(got, exp)
    assert rb.outputs() == exp.shape[2]
    assert np.abs(exp[0, 0]).max() > 0


def test_parity_does_not_depend_on_the_cut(fmd, issue_case):
    args, data, exp = issue_case
    rb = _bank(fmd, args)
    # every cut lies inside an RDS filter window (255 taps); the shortest call, 72 B = 18 MPX samples, still completes an output
    # (one per R = 16 MPX samples), so none of the five is refused
    cuts = [8 * 5000, 8 * 37, 8 * 11111, 8 * 9, 3 * 65536 - 8 * (5000 + 37 + 11111 + 9)]
    pos, outs = 0, []
    for n in cuts:
        outs.append(rb.run_batch(data[:, pos:pos + n]))
        pos += n
    assert pos == data.shape[1] and len(outs) == 5
    assert np.array_equal(np.concatenate(outs, axis=2), exp)


# (K, D, Ta, R, P): R = 1 and 32, Ta = 1 and 256, P = 1024 and 16384, n_stations = 32, D = 64
CORNERS = [(1, 2, 1, 1, 1024), (32, 64, 256, 32, 16384), (3, 2, 256, 1, 16384), (2, 64, 1, 32, 1024), (32, 10, 63, 5, 4096)]


@pytest.mark.parametrize("K,D,Ta,R,P", CORNERS)
def test_definition_parity_corners(fmd, K, D, Ta, R, P):
    rng = np.random.default_rng(9000 + K * 100 + D + Ta + R)
    S = 2
    T = int(rng.integers(1, 129))
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    incs = np.array([[int(rng.integers(0, 1 << 32)) for _ in range(K)] for _ in range(S)], np.uint32)
    rate = 120000 * D + int(rng.integers(0, 50000)) * D
    g = _taps(rng, Ta)
    shift = fmd.stations_auto_shift(h, incs, limit=int(rng.choice([256, 2048, 16384])))
    rb = fmd.RdsBank(h, D, incs, rate, g, R, n_streams=S, block=P, pilot_min=1, shift=shift, device_id=0)
    refs = _refs(rb, incs)
    # the shortest call that completes one output: T + D (Ta - 1) samples, rounded up to 8 bytes
    n0 = -(-2 * (T + D * (Ta - 1)) // 8) * 8
    assert refs[0].completes(n0) >= 1 and refs[0].completes(n0 - 8) < 1
    for n in (n0, 8 * int(rng.integers(1, 40)) + 8 * D * R, 8 * int(rng.integers(300, 900)) + 2 * D * R * 60):
        data = rng.integers(0, 256, (S, n), dtype=np.uint8)
        data[:, : n // 3] = np.where(rng.random((S, n // 3)) < 0.5, 0, 255)
        got = rb.run_batch(data)
        for s in range(S):
            exp = refs[s].feed(data[s])
            assert got.shape[2] == exp.shape[1] and np.array_equal(got[s], exp), (s, n)
    assert rb.outputs() == refs[0].n_next
    for s in range(S):
        for k in (0, K - 1):
            assert rb.pilot(s, k) == refs[s].pilot(k), (s, k)
    rb.reset()
    assert rb.outputs() == 0
    refs = _refs(rb, incs)
    data = rng.integers(0, 256, (S, n0 + 8 * D * R), dtype=np.uint8)
    got = rb.run_batch(data)
    assert all(np.array_equal(got[s], refs[s].feed(data[s])) for s in range(S))


def test_a_call_one_sample_short_is_refused_and_changes_nothing(fmd):
    """T = 65, D = 2, Ta = 255: the first output needs 65 + 2 * 254 = 573 samples; 572 (1144 B, a multiple of 8) is one short."""
    rng = np.random.default_rng(77)
    h = rng.integers(-500, 501, 65).astype(np.int16)
    incs = [sr.phase_inc(30000, rr.FS), sr.phase_inc(-45000, rr.FS)]
    g, rs = fmd.rds_taps(rr.FS // 2, 16, 255)
    rb = fmd.RdsBank(h, 2, incs, rr.FS, g, 16, rds_shift=rs, device_id=0)
    ref = _refs(rb, [incs])[0]
    short = rng.integers(0, 256, (1, 1144), dtype=np.uint8)
    assert ref.completes(1144) == 0 and ref.completes(1152) == 1
    with pytest.raises(fmd.FmdError) as e:
        rb.run_batch(short)
    assert e.value.status == TOO_SHORT and rb.outputs() == 0
    with pytest.raises(fmd.FmdError) as e:
        rb.run_batch(np.zeros((1, 12), np.uint8))
    assert e.value.status == -2
    for n in (1152, 8 * 700):
        data = rng.integers(0, 256, (1, n), dtype=np.uint8)
        assert np.array_equal(rb.run_batch(data)[0], ref.feed(data[0])), n      # as if the refused call had never been made


def test_run_device_on_a_callers_stream_then_check(fmd, issue_case):
    import torch
    args, data, exp = issue_case
    rb = _bank(fmd, args)
    stream = torch.cuda.Stream()
    SENT = -4321
    pos = 0
    for n in (65536, 320, 2 * 65536 - 320):
        cap = rb.out_cap(n) + 3
        d_out = torch.full((2, 2, cap, 2), SENT, dtype=torch.int16, device="cuda")
        buf = torch.from_numpy(np.ascontiguousarray(data[:, pos:pos + n])).cuda()
        torch.cuda.synchronize()
        before = rb.outputs()
        m = rb.run_device(buf.data_ptr(), n, d_out.data_ptr(), cap, stream.cuda_stream)
        rb.check()
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:, :, :m], exp[:, :, before:before + m]) and (got[:, :, m:] == SENT).all(), n
        pos += n
    assert rb.outputs() == exp.shape[2]
    with pytest.raises(fmd.FmdError) as e:
        rb.run_device(buf.data_ptr(), n, d_out.data_ptr(), 10, stream.cuda_stream)
    assert e.value.status == -5


@pytest.fixture(scope="module")
def capture():
    """0.7 s of the test station at +40 kHz (nothing at -86 kHz), capture_rate 256000."""
    return rr.station_capture(0.7)[0]


def test_pilot_is_the_stereo_banks(fmd, capture):
    h = rr.front_taps()
    incs = [sr.phase_inc(40000, rr.FS), sr.phase_inc(-86000, rr.FS)]
    g, rs = fmd.rds_taps(rr.FS // rr.D, rr.R, 255)
    rb = fmd.RdsBank(h, rr.D, incs, rr.FS, g, rr.R, block=1024, device_id=0)
    sb = fmd.StereoBank(h, rr.D, incs, rr.FS, fmd.stereo_taps(rr.FS // rr.D, 4, 63), 4, block=1024, device_id=0)
    assert rb.pilot(0, 0) == (False, 0)
    for n in (8 * 1000, 65536, 8 * 333):
        rb.run_batch(capture[None, :n])
        sb.run_batch(capture[None, :n])
        for k in range(2):
            assert rb.pilot(0, k) == sb.pilot(0, k), (n, k)
    present, level = rb.pilot(0, 0)
    assert present and 1200 <= level <= 2200, level          # 32768 * 6750 / 128000 = 1728
    assert rb.pilot(0, 1)[0] is False


def _calls(iq, n):
    return [iq[None, p:p + n] for p in range(0, iq.size, n)]


def test_end_to_end_bank_and_decoder(fmd, capture):
    h = rr.front_taps()
    incs = [sr.phase_inc(40000, rr.FS), sr.phase_inc(-86000, rr.FS)]
    g, rs = fmd.rds_taps(rr.FS // rr.D, rr.R, 255)
    rb = fmd.RdsBank(h, rr.D, incs, rr.FS, g, rr.R, device_id=0)
    assert capture.size == 2 * 179200
    info = fmd.decode_stations(rb, _calls(capture, 65536))[0]
    print(info)
    st, empty = info
    assert st["pi"] == rr.PI and st["ps"] == rr.PS and st["rt"] == rr.RT
    assert st["synced"] and st["blocks_bad"] == 0 and st["groups_ok"] >= 7
    assert not empty["synced"] and empty["groups_ok"] == 0 and not empty["groups"] and empty["pi"] == 0
    assert fmd.as_complex(rb.run_batch(capture[None, :65536])).dtype == np.complex64


def test_end_to_end_cli(fmd, tmp_path):
    """simple_fm_gpu -S ... -R in a child process, on 0.7 s of the same station synthesized at the CLI's capture rate (-s 170000:
    1.02 Msps, downsample 6), one station at +150 kHz and nothing at -300 kHz."""
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "simple_fm_gpu")
    radio, cfg = fmd.optimal_settings(94_900_000, 170_000)
    assert radio.capture_rate == 1_020_000 and cfg.downsample == 6
    iq, _ = rr.station_capture(0.7, offsets=(150000,), fs=radio.capture_rate)
    (tmp_path / "cap.bin").write_bytes(iq.tobytes())
    p = subprocess.run([exe, "-S", "150000,-300000", "-R", "-I", "-o", str(tmp_path / "rds"), str(tmp_path / "cap.bin")],
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    print(lines)
    assert len(lines) == 2
    assert lines[0].startswith('150000 %04X %s "%s" ' % (rr.PI, rr.PS, rr.RT)), lines[0]
    ok, bad = (int(v) for v in lines[0].rsplit(" ", 2)[1:])
    assert ok >= 7 and bad == 0
    assert lines[1] == '-300000 0000          "" 0 0', lines[1]
    for k in range(2):
        u = np.fromfile(str(tmp_path / ("rds.%d.rds.cs16" % k)), dtype=np.int16)
        assert u.size > 2 * 5000 and u.size % 2 == 0
