"""Narrow-band bank (include/fmd.h, fmd_narrow_*) on the MI355X: bit for bit against the test-side definition (tests/narrow_ref.py)
through the C ABI -- every mode over the domain's corners, maximal taps with full-scale input, sequences of calls that straddle
blocks, refused calls, reset, the level read-out, the device path with an unaligned out_cap and pointer on a caller's stream, 512
streams, the IQ anchor against a Channelizer handle, and the CLI.  Everything runs in this process."""
import os
import subprocess

import numpy as np
import pytest

import narrow_ref as nr
import stations_ref as sr
import stereo_ref as st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_SHORT = -3


def _bytes(rng, S, n):
    """Loud and quiet stretches (the squelch sees both), a third of it at the rails."""
    b = rng.integers(0, 256, (S, n), dtype=np.uint8)
    b[:, : n // 3] = np.where(rng.random((S, n // 3)) < 0.5, 0, 255)
    q = slice(n // 2, n // 2 + n // 4)
    b[:, q] = rng.integers(120, 136, (S, b[:, q].shape[1]), dtype=np.uint8)
    return b


def _refs(nb, incs, z=None):
    return [nr.NarrowRef(nb.taps, nb.decim, incs[s], nb.shift, nb.gr, nb.gi, nb.mode, nb.chan_decim, nb.chan_shift, nb.block,
                         nb.squelch, nb.gain, z=z) for s in range(nb.n_streams)]


def _check_call(fmd, nb, refs, data):
    """One call of every stream: bank and definition agree, or both refuse and the bank changes nothing."""
    if refs[0].completes(data.shape[1]) < 1:
        before = nb.outputs()
        with pytest.raises(fmd.FmdError) as e:
            nb.run_batch(data)
        assert e.value.status == TOO_SHORT and nb.outputs() == before
        return 0
    got = nb.run_batch(data)
    for s in range(data.shape[0]):
        exp = refs[s].feed(data[s])
        assert got.shape[2] == exp.shape[1] and np.array_equal(got[s], exp), (s, data.shape[1])
    assert nb.outputs() == refs[0].n_next
    return got.shape[2]


def _chan_taps(rng, Ta, cplx, peak=300):
    """Random taps scaled to the rule: sum |gr| + |gi| <= 65535, every tap within 16383."""
    gr = rng.integers(-peak, peak + 1, Ta).astype(np.int64)
    gi = rng.integers(-peak, peak + 1, Ta).astype(np.int64) if cplx else np.zeros(Ta, np.int64)
    if cplx and not gi.any():
        gi[0] = 1
    tot = max(1, int(np.abs(gr).sum() + np.abs(gi).sum()))
    f = min(65535 / tot, 16383 / max(1, int(max(np.abs(gr).max(), np.abs(gi).max()))))
    gr, gi = np.trunc(gr * f).astype(np.int16), np.trunc(gi * f).astype(np.int16)
    if cplx and not gi.any():
        gi[0] = 1 if gr[0] < 16383 and int(np.abs(gr.astype(np.int64)).sum()) < 65535 else 0
    return gr, (gi if cplx and gi.any() else None)


# (K, D, Ta, R, P, mode, complex taps): every mode, R in {1, 2, 5, 20, 32}, Ta in {1, 2, 255, 256}, P in {16, 4096}, K in {1, 32},
# D in {2, 10, 64}, real and complex taps
CORNERS = [(1, 2, 1, 1, 16, nr.IQ, False), (3, 10, 255, 5, 16, nr.FM, True), (8, 64, 256, 32, 4096, nr.AM, True),
           (32, 10, 256, 1, 16, nr.SSB, True), (8, 2, 2, 32, 4096, nr.FM, False), (1, 64, 1, 5, 16, nr.AM, False),
           (32, 64, 255, 20, 4096, nr.IQ, True), (4, 10, 256, 20, 256, nr.AM, False), (2, 10, 2, 2, 16, nr.SSB, False),
           (5, 10, 64, 2, 64, nr.IQ, True), (2, 2, 255, 20, 16, nr.FM, False)]


@pytest.mark.parametrize("K,D,Ta,R,P,mode,cplx", CORNERS)
def test_definition_parity_corners(fmd, K, D, Ta, R, P, mode, cplx):
    rng = np.random.default_rng(9000 + K * 100 + D + Ta + R + mode)
    S = 2
    T = int(rng.integers(1, 129))
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    incs = np.array([[int(rng.integers(0, 1 << 32)) for _ in range(K)] for _ in range(S)], np.uint32)   # per-stream increments
    gr, gi = _chan_taps(rng, Ta, cplx)
    shift = fmd.stations_auto_shift(h, incs, limit=int(rng.choice([256, 2048, 16384])))
    lim = int(rng.choice([256, 4096, 16384]))
    cs = fmd.narrow_auto_shift(h, incs, shift, gr, gi, limit=lim)
    sizes = [8 * int(rng.integers(1, 40)), 8 * int(rng.integers(1, 600)), 8 * D * (Ta * R // 4 + 3), 8 * int(rng.integers(2000, 9000)),
             8 * 3, min(8 * D * R * P // 4 + 8, 8 * 70000), 8 * int(rng.integers(100, 3000))]
    datas = [_bytes(rng, S, n) for n in sizes]
    # a squelch that some blocks pass and some do not: the median block RMS of stream 0, station 0 with the squelch off
    probe = nr.NarrowRef(h, D, incs[0][:1], shift, gr, gi, nr.IQ, R, cs, P, 0, 256, z=sr.z_corr)
    u = probe.feed(np.concatenate([d[0] for d in datas]))[0]
    nblk = u.shape[0] // P
    squelch = 0
    if nblk >= 2 and rng.random() < 0.8:
        rms = np.sqrt((u[:nblk * P].astype(np.float64) ** 2).sum(axis=1).reshape(nblk, P).mean(axis=1))
        squelch = min(23170, int(np.median(rms)))
    nb = fmd.NarrowBank(h, D, incs, (gr, gi), R, mode=mode, n_streams=S, block=P, squelch=squelch, gain=int(rng.integers(1, 65536)),
                        chan_shift=cs, shift=shift, device_id=0)
    assert "fmd_narrow" in nb.kernel_name(0) and "fmd_narrow" in nb.kernel_name(1)
    assert nb.level(0, 0) == (False, 0)
    refs = _refs(nb, incs, z=sr.z_corr)
    pending = np.zeros((S, 0), np.uint8)
    done = 0
    for data in datas:
        data = np.concatenate([pending, data], axis=1)
        got = _check_call(fmd, nb, refs, data)
        pending = data if got == 0 else np.zeros((S, 0), np.uint8)
        done += got
        for s in range(S):
            assert nb.level(s, K - 1) == refs[s].level(K - 1), (s, done)
    assert done > 0
    for s in range(S):
        for k in range(K):
            assert nb.level(s, k) == refs[s].level(k), (s, k)
    nb.reset()
    assert nb.outputs() == 0 and nb.level(0, 0) == (False, 0)
    refs = _refs(nb, incs)
    _check_call(fmd, nb, refs, _bytes(rng, S, 8 * D * (Ta * R // 4 + 40)))


@pytest.mark.parametrize("mode", [nr.IQ, nr.FM, nr.AM, nr.SSB])
@pytest.mark.parametrize("cplx", [False, True])
def test_maximal_taps_full_scale_input_at_the_bound(fmd, mode, cplx):
    """Front-end taps of 2047 at offset 0 over bytes at the rails, channel taps of 16383 (G = 65532) and the smallest shifts the
    domain admits: |v| reaches B_y G, |u| the neighbourhood of 16384, the magnitude and the sums their largest values."""
    rng = np.random.default_rng(77 + mode)
    D, T, R, P = 2, 16, 1, 16
    h = np.full(T, 2047, np.int16)
    incs = np.zeros((1, 1), np.uint32)
    shift = fmd.stations_auto_shift(h, incs, limit=16384)
    gr = np.array([16383, 16383, 16383, 16383] if not cplx else [16383, 16383, 0, 0], np.int16)
    gi = np.array([0, 0, 16383, 16383], np.int16) if cplx else None
    cs = fmd.narrow_auto_shift(h, incs, shift, gr, gi, limit=16384)
    nb = fmd.NarrowBank(h, D, incs, (gr, gi), R, mode=mode, block=P, squelch=8000, gain=65535, chan_shift=cs, shift=shift, device_id=0)
    refs = _refs(nb, incs)
    n = 8 * 600
    b = np.empty((1, n), np.uint8)
    b[0, 0::2] = np.repeat(np.where(rng.random(n // 64 + 1) < 0.5, 0, 255), 32)[:n // 2]
    b[0, 1::2] = np.repeat(np.where(rng.random(n // 64 + 1) < 0.5, 0, 255), 32)[:n // 2]
    b[0, :400] = 255
    _check_call(fmd, nb, refs, b)
    assert refs[0].v_max > (1 << 28)                         # the input does reach the top quarter of the bound
    assert nb.level(0, 0) == refs[0].level(0)


def test_anchor_iq_is_the_channelizer_and_fm_its_discriminator(fmd):
    """R = 1, Ta = 1, gr = [1], chan_shift = 0: IQ mode is a Channelizer handle's y, FM mode the reference's discriminator of
    consecutive y wrapped to i16 (gain 256 = 1.0)."""
    rng = np.random.default_rng(31)
    D, T, fs = 10, 48, 2400000
    h = st.lowpass(T, 120000 / fs)
    incs = [fmd.phase_inc(o, fs) for o in (-500000, 250000)]
    shift = fmd.stations_auto_shift(h, incs, limit=256)
    one = np.array([1], np.int16)
    iq = fmd.NarrowBank(h, D, incs, one, 1, mode="iq", chan_shift=0, shift=shift, device_id=0)
    fm = fmd.NarrowBank(h, D, incs, one, 1, mode="fm", chan_shift=0, shift=shift, device_id=0)
    ch = fmd.Channelizer(h, D, incs, shift=shift, device_id=0)
    ys, a, b = [], [], []
    for n in (8 * 2000, 8 * 777, 8 * 3001):
        data = rng.integers(0, 256, (1, n), dtype=np.uint8)
        ys.append(ch.run_batch(data)[0])
        a.append(iq.run_batch(data)[0])
        b.append(fm.run_batch(data)[0])
    y, a, b = np.concatenate(ys, axis=1), np.concatenate(a, axis=1), np.concatenate(b, axis=1)
    assert np.array_equal(a, y)
    y = y.astype(np.int64)
    for k in range(len(incs)):
        yy = np.concatenate([np.zeros((1, 2), np.int64), y[k]])
        assert np.array_equal(b[k], st.wrap16(st.disc_fast(yy[1:, 0], yy[1:, 1], yy[:-1, 0], yy[:-1, 1]))), k


@pytest.mark.parametrize("mode", [nr.IQ, nr.AM])
def test_run_device_unaligned_on_a_callers_stream_and_refusals(fmd, mode):
    import torch
    rng = np.random.default_rng(55 + mode)
    fs, D, T, R, Ta, S, K = 2400000, 10, 64, 5, 127, 3, 4
    h = st.lowpass(T, 100000 / fs)
    incs = np.array([[fmd.phase_inc(int(o), fs) for o in rng.integers(-900000, 900000, K)] for _ in range(S)], np.uint32)
    g = fmd.narrow_taps(fs // D, Ta, -6000, 6000)
    nb = fmd.NarrowBank(h, D, incs, g, R, mode=mode, n_streams=S, block=64, squelch=40, device_id=0)
    refs = _refs(nb, incs)
    W = nb.width
    with pytest.raises(fmd.FmdError) as e:                  # the first audio sample needs 64 + 10 * 126 samples
        nb.run_batch(np.zeros((S, 8 * 100), np.uint8))
    assert e.value.status == TOO_SHORT and nb.outputs() == 0
    with pytest.raises(fmd.FmdError) as e:
        nb.run_batch(np.zeros((S, 12), np.uint8))
    assert e.value.status == -2
    stream = torch.cuda.Stream()
    SENT = -4321
    for n in (8 * 1001, 8 * 7, 8 * 2403, 8 * 50, 8 * 9000):
        data = _bytes(rng, S, n)
        cap = nb.out_cap(n) + 3                              # odd rows: 2-byte aligned only outside IQ mode
        flat = torch.full((S * K * cap * W + 8,), SENT, dtype=torch.int16, device="cuda")
        off = W                                              # the pointer one sample past the allocation's alignment
        d_out = flat[off:off + S * K * cap * W]
        buf = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        if refs[0].completes(n) < 1:
            before = nb.outputs()
            with pytest.raises(fmd.FmdError) as e:
                nb.run_device(buf.data_ptr(), n, d_out.data_ptr(), cap, stream.cuda_stream)
            assert e.value.status == TOO_SHORT and nb.outputs() == before
            continue
        m = nb.run_device(buf.data_ptr(), n, d_out.data_ptr(), cap, stream.cuda_stream)
        nb.check()
        whole = flat.cpu().numpy()
        assert (whole[:off] == SENT).all() and (whole[off + S * K * cap * W:] == SENT).all()
        got = whole[off:off + S * K * cap * W].reshape(S, K, cap, W)
        for s in range(S):
            exp = refs[s].feed(data[s])
            assert np.array_equal(got[s, :, :m] if mode == nr.IQ else got[s, :, :m, 0], exp), (n, s)
            assert (got[s, :, m:] == SENT).all()
    big = torch.zeros((S, 8 * 40000), dtype=torch.uint8, device="cuda")
    with pytest.raises(fmd.FmdError) as e:
        nb.run_device(big.data_ptr(), 8 * 40000, d_out.data_ptr(), 10, stream.cuda_stream)
    assert e.value.status == -5


def test_512_streams_production_shape(fmd):
    """512 streams x 262144 B, two calls, an AM and a quiet channel per stream; sampled streams bit-exact (z_corr), the level of
    the carrier read back."""
    import torch
    S, n = 512, fmd.DEFAULT_BUF_LENGTH
    fs, D, T, R, Ta, P = 2400000, 10, 64, 20, 256, 256
    h = st.lowpass(T, 100000 / fs)
    offs = [-400000, 300000]
    incs = [fmd.phase_inc(o, fs) for o in offs]
    g = fmd.narrow_taps(fs // D, Ta, -5000, 5000)
    caps = [nr.to_u8(nr.am(n, fs, offs[0], 20.0 + 5 * v, 1000.0), noise=1.0, seed=v) for v in range(4)]          # 2 calls each
    nb = fmd.NarrowBank(h, D, incs, g, R, mode="am", n_streams=S, block=P, squelch=200, device_id=0)
    sample = [0, 1, 2, 3, 255, 511]
    refs = {s: nr.NarrowRef(h, D, incs, nb.shift, nb.gr, nb.gi, nb.mode, R, nb.chan_shift, P, nb.squelch, nb.gain, z=sr.z_corr)
            for s in sample}
    cap = nb.out_cap(n)
    d_out = torch.empty((S, 2, cap), dtype=torch.int16, device="cuda")
    for call in range(2):
        data = np.stack([caps[s % 4][call * n:(call + 1) * n] for s in range(S)])
        d_iq = torch.from_numpy(data).cuda()
        m = nb.run_device(d_iq.data_ptr(), n, d_out.data_ptr(), cap)
        nb.check()
        got = d_out[:, :, :m].cpu().numpy()
        for s in sample:
            assert np.array_equal(got[s], refs[s].feed(data[s])), (call, s)
    for s in sample:
        assert nb.level(s, 0) == refs[s].level(0) and nb.level(s, 1) == refs[s].level(1)
        assert nb.level(s, 0)[0] and not nb.level(s, 1)[0]
    assert np.abs(got[0, 0]).max() > 0 and not got[0, 1].any()


def test_cli_narrow_mode_matches_the_python_handle(fmd, tmp_path):
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "simple_fm_gpu")
    radio, cfg = fmd.optimal_settings(94_900_000, 170_000)
    capture, D = radio.capture_rate, cfg.downsample
    f_m = capture // D
    offs = [-300000, 12500, 200000]
    rng = np.random.default_rng(62)
    n = fmd.DEFAULT_BUF_LENGTH
    iq = rng.integers(100, 156, 3 * n // 2 + 504, dtype=np.uint8)
    (tmp_path / "cap.bin").write_bytes(iq.tobytes())
    shift = 0
    while -(-512 * D >> shift) > 16384:
        shift += 1
    for spec, mode, R, lo, hi, sq in (("am:10:-4000:4000", "am", 10, -4000, 4000, 30), ("usb:14:300:3000", "usb", 14, 300, 3000, 0),
                                      ("lsb", "lsb", f_m // 12000, -3000, -300, 0), ("iq:5:-12000:12000", "iq", 5, -12000, 12000, 0),
                                      ("fm:10", "fm", 10, -6000, 6000, 0)):
        pre = str(tmp_path / ("nb_" + mode))
        p = subprocess.run([exe, "-S", ",".join(str(o) for o in offs), "-N", spec, "-q", str(sq), "-o", pre, str(tmp_path / "cap.bin")],
                           capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        assert ("%.3f Hz" % (capture / D / R)) in p.stderr.decode()
        gr, gi = fmd.narrow_taps(f_m, 256, lo, hi)
        peak = -(-512 * D >> shift) * fmd.narrow.narrow_gain_sum(gr, gi)
        cs = 0
        while -(-peak >> cs) > (256 if mode == "fm" else 16384):
            cs += 1
        nb = fmd.NarrowBank(np.ones(D, np.int16), D, [fmd.phase_inc(o, capture) for o in offs], (gr, gi), R, mode=mode, squelch=sq,
                            chan_shift=cs, shift=shift, device_id=0)
        exp = [[] for _ in offs]
        for b in range(iq.size // n):
            a = nb.run_batch(iq[None, b * n:(b + 1) * n])
            for k in range(len(offs)):
                exp[k].append(a[0, k].ravel())
        for k in range(len(offs)):
            got = np.fromfile(pre + (".%d.cs16" % k if mode == "iq" else ".%d.s16" % k), dtype=np.int16)
            assert got.size > 0 and np.array_equal(got, np.concatenate(exp[k])), (mode, k)
