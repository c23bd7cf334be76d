"""FM receiver bank (include/fmd.h, fmd_receiver_*) on the MI355X: both outputs bit for bit against the test-side definition
(tests/receiver_ref.py) and against what a StereoBank and an RdsBank return for the same bytes -- the issue's shape, the same bytes
re-cut, the refusal of a call that completes an output of one stage only, the domain's corners, the device path on a caller's stream,
reset, three handles interleaved -- and end to end: PS and RadioText through receive_stations, stereo separation, the CLI."""
import os
import subprocess

import numpy as np
import pytest

import rds_ref as rr
import receiver_ref as rxr
import stations_ref as sr
import stereo_ref as st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_SHORT = -3
FA, RA = 127, 5                                              # the issue case's audio stage: 127 taps at stride 5
SEPARATION_DB = 25                                           # tests/test_gpu_stereo.py, test_physics_separation_64_streams_production_shape


def _refs(rx, incs):
    return [rxr.ReceiverRef(rx.taps, rx.decim, incs[s], rx.shift, rx.capture_rate, rx.audio_taps, rx.audio_decim, rx.audio_shift, rx.rds_taps,
                            rx.rds_decim, rx.rds_shift, rx.block, rx.pilot_min, z=sr.z_corr) for s in range(rx.n_streams)]


def _feed(refs, data):
    out = [r.feed(d) for r, d in zip(refs, data)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.fixture(scope="module")
def issue_case(fmd):
    """2 streams x 2 stations, D = 2, capture_rate 256000, audio R = 5 with 127 taps, RDS R = 16 with 255 taps, 3 x 65536 B; station 1
    of every stream has inc = 0 and stream 1 is all zero bytes.  (bank arguments, bytes, the definition's outputs and pilots)"""
    rng = np.random.default_rng(2025)
    h = rr.front_taps()
    incs = np.array([[sr.phase_inc(40000, rr.FS), 0], [sr.phase_inc(-70000, rr.FS), 0]], np.uint32)
    ga = fmd.stereo_taps(rr.FS // rr.D, RA, FA)
    gr, rs = fmd.rds_taps(rr.FS // rr.D, rr.R, 255)
    data = rng.integers(0, 256, (2, 3 * 65536), dtype=np.uint8)
    data[1] = 0
    a = dict(h=h, incs=incs, ga=ga, gr=gr, rs=rs, ash=4, shift=fmd.stations_auto_shift(h, incs, limit=2048))
    refs = [rxr.ReceiverRef(h, rr.D, incs[s], a["shift"], rr.FS, ga, RA, a["ash"], gr, rr.R, rs, 4096, 1, z=sr.z_corr) for s in range(2)]
    audio, rds = _feed(refs, data)
    return a, data, audio, rds, [[refs[s].pilot(k) for k in range(2)] for s in range(2)]


def _bank(fmd, a):
    return fmd.ReceiverBank(a["h"], rr.D, a["incs"], rr.FS, a["ga"], RA, a["gr"], rr.R, n_streams=2, audio_shift=a["ash"], rds_shift=a["rs"],
                            shift=a["shift"], pilot_min=1, device_id=0)


def _stereo(fmd, a):
    return fmd.StereoBank(a["h"], rr.D, a["incs"], rr.FS, a["ga"], RA, n_streams=2, audio_shift=a["ash"], shift=a["shift"], pilot_min=1, device_id=0)


def _rds(fmd, a):
    return fmd.RdsBank(a["h"], rr.D, a["incs"], rr.FS, a["gr"], rr.R, n_streams=2, rds_shift=a["rs"], shift=a["shift"], pilot_min=1, device_id=0)


def test_issue_case_is_the_definition_and_the_two_banks(fmd, issue_case):
    args, data, audio, rds, pilots = issue_case
    rx, sb, rb = _bank(fmd, args), _stereo(fmd, args), _rds(fmd, args)
    assert rx.kernel_name(0) == sb.kernel_name(0) == rb.kernel_name(0) == "fmd_sto::fmd_stereo_mpx_kernel"
    assert rx.kernel_name(1) == "fmd_rx::fmd_receiver_second_kernel"
    assert rx.audio_rate == sb.audio_rate and (rx.rate_num, rx.rate_den) == (rb.rate_num, rb.rate_den)
    ga, gu, sa, su = [], [], [], []
    for c in range(3):
        call = data[:, c * 65536:(c + 1) * 65536]
        assert rx.out_caps(call.shape[1]) == (sb.out_cap(call.shape[1]), rb.out_cap(call.shape[1]))
        a, u = rx.run_batch(call)
        ga.append(a); gu.append(u)
        sa.append(sb.run_batch(call)); su.append(rb.run_batch(call))
        assert rx.outputs() == (sb.outputs(), rb.outputs())
        for s in range(2):
            for k in range(2):
                assert rx.pilot(s, k) == sb.pilot(s, k) == rb.pilot(s, k), (c, s, k)
    ga, gu = np.concatenate(ga, axis=2), np.concatenate(gu, axis=2)
    assert ga.dtype == np.int16 and ga.shape == audio.shape and np.array_equal(ga, audio)
    assert gu.dtype == np.int16 and gu.shape == rds.shape and np.array_equal(gu, rds)
    assert np.array_equal(ga, np.concatenate(sa, axis=2)) and np.array_equal(gu, np.concatenate(su, axis=2))
    assert rx.outputs() == (audio.shape[2], rds.shape[2])
    assert [[rx.pilot(s, k) for k in range(2)] for s in range(2)] == pilots
    assert np.abs(audio[0, 0]).max() > 0 and np.abs(rds[0, 0]).max() > 0


def test_parity_does_not_depend_on_the_cut(fmd, issue_case):
    args, data, audio, rds, _ = issue_case
    rx = _bank(fmd, args)
    # every cut lies inside both filter windows (127 and 255 taps); the shortest call, 72 B = 18 MPX samples, completes an output of
    # each stage (one per 5 and one per 16 MPX samples), so none of the five is refused
    cuts = [8 * 5000, 8 * 37, 8 * 11111, 8 * 9, 3 * 65536 - 8 * (5000 + 37 + 11111 + 9)]
    pos, aa, uu = 0, [], []
    for n in cuts:
        a, u = rx.run_batch(data[:, pos:pos + n])
        assert a.shape[2] >= 1 and u.shape[2] >= 1
        aa.append(a); uu.append(u)
        pos += n
    assert pos == data.shape[1] and len(aa) == 5
    assert np.array_equal(np.concatenate(aa, axis=2), audio) and np.array_equal(np.concatenate(uu, axis=2), rds)


def test_a_call_that_completes_audio_but_no_rds_output_is_refused_and_changes_nothing(fmd):
    """D = 2, audio R = 1 with one tap, RDS R = 32: after a first call, the longest call that still completes no RDS output."""
    rng = np.random.default_rng(78)
    h = rng.integers(-500, 501, 65).astype(np.int16)
    incs = np.array([[sr.phase_inc(30000, rr.FS), sr.phase_inc(-45000, rr.FS)]], np.uint32)
    gr, rs = fmd.rds_taps(rr.FS // 2, 32, 255)
    mk = lambda: fmd.ReceiverBank(h, 2, incs, rr.FS, np.array([16383], np.int16), 1, gr, 32, audio_shift=14, rds_shift=rs, device_id=0)  # noqa: E731
    rx = mk()
    ref, uncut = _refs(rx, incs)[0], _refs(rx, incs)[0]
    data = rng.integers(0, 256, (1, 8 * 1500), dtype=np.uint8)
    whole = uncut.feed(data[0])
    first = 8 * 700
    a0, u0 = rx.run_batch(data[:, :first])
    e0 = ref.feed(data[0, :first])
    assert np.array_equal(a0[0], e0[0]) and np.array_equal(u0[0], e0[1])
    short = max(n for n in range(8, 8 * 40, 8) if ref.completes(n)[1] == 0)      # from the definition's counts
    na, nr = ref.completes(short)
    print("short call: %d B completes %d audio and %d RDS outputs" % (short, na, nr))
    assert na >= 1 and nr == 0 and ref.completes(short + 8)[1] == 1
    before = rx.outputs()
    with pytest.raises(fmd.FmdError) as e:
        rx.run_batch(data[:, first:first + short])
    assert e.value.status == TOO_SHORT and rx.outputs() == before == ref.outputs()
    with pytest.raises(fmd.FmdError) as e:
        rx.run_batch(np.zeros((1, 12), np.uint8))
    assert e.value.status == -2
    a1, u1 = rx.run_batch(data[:, first:])                   # the same bytes again, as the head of a longer call
    assert np.array_equal(np.concatenate([a0, a1], axis=2)[0], whole[0]) and np.array_equal(np.concatenate([u0, u1], axis=2)[0], whole[1])
    # a first call that completes audio only is refused the same way
    rx2 = mk()
    with pytest.raises(fmd.FmdError) as e:
        rx2.run_batch(data[:, :8 * 50])
    assert e.value.status == TOO_SHORT and rx2.outputs() == (0, 0)
    a, u = rx2.run_batch(data)
    assert np.array_equal(a[0], whole[0]) and np.array_equal(u[0], whole[1])


# (K, D, audio Ta, audio R, RDS Ta, RDS R, P)
CORNERS = [(1, 2, 1, 1, 256, 32, 1024), (32, 64, 256, 32, 1, 1, 16384), (3, 2, 256, 1, 256, 1, 16384), (2, 64, 1, 32, 1, 32, 1024),
           (32, 10, 127, 5, 255, 32, 4096)]


def _taps(rng, Ta):
    g = rng.integers(-200, 201, Ta)
    g[g == 0] = 1
    return (np.sign(g) * np.maximum(1, np.abs(g) * 16000 // int(np.abs(g).sum()))).astype(np.int16) if Ta > 1 else np.array([16383], np.int16)


def _tiles(Ta_a, Ra, Ta_r, Rr, na, nr):
    """Second-pass tiles per row of a call with na audio and nr RDS outputs (the tile sizes of the two sides)."""
    ta, tr = min((2048 - 2 * Ta_a) // Ra, 256), min((1984 - Ta_r) // Rr, 256)
    return -(-na // ta), -(-nr // tr)


# Whether the longest call of each corner (about 1500 multiplex samples) has several tiles per row on the (audio, RDS) side: corner 0
# gives the RDS side a single tile while the audio side has several, corner 1 the reverse, corner 2 several on both over 6 rows of 3
# stations, so that the split of the block index falls off any round number.
SEVERAL = [(True, False), (False, True), (True, True), (False, False), (True, False)]
assert (True, False) in SEVERAL and (False, True) in SEVERAL and SEVERAL[2] == (True, True) and CORNERS[2][0] % 2 == 1


@pytest.mark.parametrize("K,D,Ta,Ra,Tr,Rr,P", CORNERS)
def test_definition_parity_corners(fmd, K, D, Ta, Ra, Tr, Rr, P):
    rng = np.random.default_rng(9100 + K * 100 + D + Ta + Ra + Tr + Rr)
    S = 2
    T = int(rng.integers(1, 129))
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    incs = np.array([[int(rng.integers(0, 1 << 32)) for _ in range(K)] for _ in range(S)], np.uint32)
    rate = 120000 * D + int(rng.integers(0, 50000)) * D
    ga, gr = _taps(rng, Ta), _taps(rng, Tr)
    shift = fmd.stations_auto_shift(h, incs, limit=int(rng.choice([256, 2048, 16384])))
    rx = fmd.ReceiverBank(h, D, incs, rate, ga, Ra, gr, Rr, n_streams=S, block=P, pilot_min=1, audio_shift=int(rng.integers(0, 17)),
                          shift=shift, device_id=0)
    refs = _refs(rx, incs)
    # the shortest accepted call: an output of each stage, T + D (max Ta - 1) samples, rounded up to 8 bytes
    n0 = -(-2 * (T + D * (max(Ta, Tr) - 1)) // 8) * 8
    assert min(refs[0].completes(n0)) >= 1 and min(refs[0].completes(n0 - 8)) < 1
    if n0 > 8:
        with pytest.raises(fmd.FmdError) as e:
            rx.run_batch(np.zeros((S, n0 - 8), np.uint8))
        assert e.value.status == TOO_SHORT and rx.outputs() == (0, 0)
    # ... then the shortest later one, and a call of a few tiles on the side with the smaller tiles
    for n in (n0, 8 * (-(-2 * D * max(Ra, Rr) // 8)), 8 * int(rng.integers(1, 40)) + 2 * D * 1500):
        data = rng.integers(0, 256, (S, n), dtype=np.uint8)
        data[:, : n // 3] = np.where(rng.random((S, n // 3)) < 0.5, 0, 255)
        a, u = rx.run_batch(data)
        ea, eu = _feed(refs, data)
        assert a.shape == ea.shape and np.array_equal(a, ea), n
        assert u.shape == eu.shape and np.array_equal(u, eu), n
    ta, tr = _tiles(Ta, Ra, Tr, Rr, a.shape[2], u.shape[2])
    print("tiles per row of the longest call: audio %d, RDS %d" % (ta, tr))
    assert (ta > 1, tr > 1) == SEVERAL[CORNERS.index((K, D, Ta, Ra, Tr, Rr, P))]
    assert rx.outputs() == refs[0].outputs()
    for s in range(S):
        for k in (0, K - 1):
            assert rx.pilot(s, k) == refs[s].pilot(k), (s, k)
    rx.reset()
    assert rx.outputs() == (0, 0)
    refs = _refs(rx, incs)
    data = rng.integers(0, 256, (S, n0 + 8 * D * max(Ra, Rr)), dtype=np.uint8)
    a, u = rx.run_batch(data)
    ea, eu = _feed(refs, data)
    assert np.array_equal(a, ea) and np.array_equal(u, eu)


def test_run_device_on_a_callers_stream_then_check(fmd, issue_case):
    import torch
    args, data, audio, rds, _ = issue_case
    rx = _bank(fmd, args)
    stream = torch.cuda.Stream()
    SENT = -4321
    pos = 0
    for n in (65536, 320, 2 * 65536 - 320):
        ca, cr = (c + 3 for c in rx.out_caps(n))
        d_a = torch.full((2, 2, ca, 2), SENT, dtype=torch.int16, device="cuda")
        d_u = torch.full((2, 2, cr, 2), SENT, dtype=torch.int16, device="cuda")
        buf = torch.from_numpy(np.ascontiguousarray(data[:, pos:pos + n])).cuda()
        torch.cuda.synchronize()
        ba, bu = rx.outputs()
        na, nr = rx.run_device(buf.data_ptr(), n, d_a.data_ptr(), ca, d_u.data_ptr(), cr, stream.cuda_stream)
        rx.check()
        ga, gu = d_a.cpu().numpy(), d_u.cpu().numpy()
        assert np.array_equal(ga[:, :, :na], audio[:, :, ba:ba + na]) and (ga[:, :, na:] == SENT).all(), n
        assert np.array_equal(gu[:, :, :nr], rds[:, :, bu:bu + nr]) and (gu[:, :, nr:] == SENT).all(), n
        pos += n
    assert rx.outputs() == (audio.shape[2], rds.shape[2])
    for ca, cr in ((10, cr), (ca, 10)):                      # either capacity too small
        with pytest.raises(fmd.FmdError) as e:
            rx.run_device(buf.data_ptr(), n, d_a.data_ptr(), ca, d_u.data_ptr(), cr, stream.cuda_stream)
        assert e.value.status == -5
    assert rx.outputs() == (audio.shape[2], rds.shape[2])


def test_reset_reproduces_the_first_call(fmd, issue_case):
    args, data, audio, rds, _ = issue_case
    rx = _bank(fmd, args)
    first = rx.run_batch(data[:, :65536])
    rx.run_batch(data[:, 65536:2 * 65536])
    rx.reset()
    assert rx.outputs() == (0, 0) and rx.pilot(0, 0) == (False, 0)
    again = rx.run_batch(data[:, :65536])
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert np.array_equal(again[0], audio[:, :, :again[0].shape[2]]) and np.array_equal(again[1], rds[:, :, :again[1].shape[2]])


def test_three_handles_interleaved_with_a_refusal_and_a_free_in_between(fmd, issue_case):
    args, data, audio, rds, _ = issue_case
    rx, sb, rb = _bank(fmd, args), _stereo(fmd, args), _rds(fmd, args)
    cuts = [8 * 3000, 8 * 41, 8 * 7000]
    cuts.append(data.shape[1] - sum(cuts))
    pos, ga, gu, sa, su = 0, [], [], [], []
    for i, n in enumerate(cuts):
        call = data[:, pos:pos + n]
        su.append(rb.run_batch(call))
        a, u = rx.run_batch(call)
        ga.append(a); gu.append(u)
        if sb is not None:
            sa.append(sb.run_batch(call))
        if i == 1:
            with pytest.raises(fmd.FmdError) as e:           # 8 B: no output of either stage; the receiver and the others go on
                rx.run_batch(data[:, :8])
            assert e.value.status == TOO_SHORT
            sb.close()                                       # freed between the calls of the other two
            sb = None
        pos += n
    ga, gu = np.concatenate(ga, axis=2), np.concatenate(gu, axis=2)
    assert np.array_equal(ga, audio) and np.array_equal(gu, rds)
    assert np.array_equal(np.concatenate(su, axis=2), rds)
    assert np.array_equal(np.concatenate(sa, axis=2), audio[:, :, :sum(x.shape[2] for x in sa)])


def test_end_to_end_ps_and_radiotext_through_receive_stations(fmd):
    capture = rr.station_capture(0.7)[0]
    h = rr.front_taps()
    incs = [sr.phase_inc(40000, rr.FS), sr.phase_inc(-86000, rr.FS)]
    gr, _ = fmd.rds_taps(rr.FS // rr.D, rr.R, 255)
    rx = fmd.ReceiverBank(h, rr.D, incs, rr.FS, fmd.stereo_taps(rr.FS // rr.D, 4, 63), 4, gr, rr.R, device_id=0)
    audio, info = fmd.receive_stations(rx, [capture[None, p:p + 65536] for p in range(0, capture.size, 65536)])
    got, empty = info[0]
    print(got["ps"], got["rt"], got["groups_ok"], got["blocks_bad"])
    assert got["pi"] == rr.PI and got["ps"] == rr.PS and got["rt"] == rr.RT
    assert got["synced"] and got["blocks_bad"] == 0 and got["groups_ok"] >= 7
    assert not empty["synced"] and empty["groups_ok"] == 0 and not empty["groups"] and empty["pi"] == 0
    assert audio.dtype == np.int16 and audio.shape[:2] == (1, 2) and audio.shape[2] == rx.outputs()[0] and audio.shape[3] == 2
    assert rx.pilot(0, 0)[0] and not rx.pilot(0, 1)[0]


def test_end_to_end_stereo_separation(fmd):
    """tests/test_gpu_stereo.py's signal (a 1 kHz tone on L only at four pilot phases, production shape) on four streams: the tone on
    R is down by what that test requires of the stereo bank."""
    S, n = 4, fmd.DEFAULT_BUF_LENGTH
    fs, D, T, R, Ta = 2400000, 10, 64, 5, 127
    h = st.lowpass(T, 130000 / fs)
    g = fmd.stereo_taps(fs // D, R, Ta)
    gr, _ = fmd.rds_taps(fs // D, 32, 255)
    offs, phis = [-400000, 300000], [0, 90, 180, 271]
    tone = lambda t: 0.15 * np.sin(2 * np.pi * 1000 * t)     # noqa: E731
    zero = lambda t: 0 * t                                   # noqa: E731
    caps = np.stack([st.synth_iq(n, fs, [(o, tone, zero, np.deg2rad(p), True) for o in offs], seed=p) for p in phis])   # 2 calls each
    rx = fmd.ReceiverBank(h, D, [fmd.phase_inc(o, fs) for o in offs], fs, g, R, gr, 32, n_streams=S, device_id=0)
    a = np.concatenate([rx.run_batch(caps[:, c * n:(c + 1) * n])[0] for c in range(2)], axis=2)
    fa, skip = fs / D / R, 2 * rx.block // R
    for s in range(S):
        for k in range(2):
            Ld, Rd = st.tone_db(a[s, k, :, 0], 1000, fa, skip), st.tone_db(a[s, k, :, 1], 1000, fa, skip)
            print("phase %d station %d: L %.1f dB, R %.1f dB" % (phis[s], k, Ld, Rd))
            assert Ld - Rd >= SEPARATION_DB, (phis[s], k, Ld, Rd)
            present, level = rx.pilot(s, k)
            assert present and 900 <= level <= 1600, (s, k, level)


def test_end_to_end_cli_writes_the_python_banks_bytes_and_station_line(fmd, tmp_path):
    """fm_receiver_gpu -S ... -I in a child process, on 0.7 s of tests/rds_ref.py's station synthesized at the CLI's capture rate
    (-s 170000: 1.02 Msps, downsample 6), one station at +150 kHz and nothing at -300 kHz, against a ReceiverBank built with the
    arguments the CLI documents, fed the same blocks."""
    from test_cpp_wrapper import rds_front
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "fm_receiver_gpu")
    radio, cfg = fmd.optimal_settings(94_900_000, 170_000)
    capture, D = radio.capture_rate, cfg.downsample
    assert (capture, D) == (1_020_000, 6)
    iq, _ = rr.station_capture(0.7, offsets=(150000,), fs=capture)
    (tmp_path / "cap.bin").write_bytes(iq.tobytes())
    offs = [150000, -300000]
    p = subprocess.run([exe, "-S", ",".join(str(o) for o in offs), "-I", "-o", str(tmp_path / "rx"), str(tmp_path / "cap.bin")],
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    f_m = capture // D
    Ra, Rr = max(1, f_m // 48000), max(1, f_m // 7500)
    assert ("stereo audio: %.3f Hz" % (capture / D / Ra)) in p.stderr.decode() and ("RDS baseband: %.3f Hz" % (capture / D / Rr)) in p.stderr.decode()
    h, shift = rds_front(capture)
    gr, rs = fmd.rds_taps(f_m, Rr, 255)
    rx = fmd.ReceiverBank(np.array(h, np.int16), D, [fmd.phase_inc(o, capture) for o in offs], capture, fmd.stereo_taps(f_m, Ra, 127), Ra, gr, Rr,
                          rds_shift=rs, shift=shift, device_id=0)
    n = fmd.DEFAULT_BUF_LENGTH
    calls = [iq[None, b:b + n] for b in range(0, iq.size // 8 * 8, n)]          # whole blocks and the tail's whole 8 bytes
    audio, info = fmd.receive_stations(rx, calls)
    lines = p.stdout.decode().splitlines()
    print(lines)
    assert len(lines) == 2
    for k, off in enumerate(offs):
        i = info[0][k]
        assert lines[k] == '%d %04X %s "%s" %d %d' % (off, i["pi"], i["ps"], i["rt"], i["groups_ok"], i["blocks_bad"]), lines[k]
        got = np.fromfile(str(tmp_path / ("rx.%d.s16" % k)), dtype=np.int16)
        assert got.size == audio[0, k].size and np.array_equal(got, audio[0, k].ravel()), k
    assert lines[0].startswith('150000 %04X %s "%s" ' % (rr.PI, rr.PS, rr.RT)) and info[0][0]["groups_ok"] >= 7
    assert lines[1] == '-300000 0000          "" 0 0'
    rx.reset()
    u = np.concatenate([rx.run_batch(c)[1] for c in calls], axis=2)
    for k in range(2):
        got = np.fromfile(str(tmp_path / ("rx.%d.rds.cs16" % k)), dtype=np.int16)
        assert got.size > 2 * 5000 and np.array_equal(got, u[0, k].ravel()), k
