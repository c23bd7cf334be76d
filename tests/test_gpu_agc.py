"""Automatic gain control (include/fmd.h, fmd_agc_*) on the MI355X: bit for bit against the test-side definition (tests/agc_ref.py)
at both widths and P in {16, 256, 4096}, unaligned rows and odd capacities, call cuts around block edges, calls that complete no
block, one call of more blocks than an LDS segment holds, full-scale values and zero runs over the configuration's corners, the gain
read-out, refused calls, reset, a caller's stream, two handles, and composed with the narrow-band bank, the stereo bank, the resampler
and the command-line tool; and, for the resampler as well, which check answers a call that two of them refuse.  Everything but the
tool runs in this process."""
import os
import subprocess

import numpy as np
import pytest

import agc_ref as ar
import narrow_ref as nr
import resample_ref as rr
from rows_gpu import SENT, call as _call, iq_bytes
import stations_ref as sr
import stereo_ref as st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = -5


def _agc(fmd, cfg, rows, width):
    cfg = ar.Cfg(*cfg)
    return fmd.Agc(n_rows=rows, width=width, target=cfg.target, block=cfg.block, hang=cfg.hang, decay=cfg.decay, gain_max=cfg.gain_max,
                   device_id=0)


def _odd(n):
    """an odd capacity above n: at width 1 every second row then starts at a 2-byte but not a 4-byte boundary"""
    return n + 1 + n % 2


def _feed(ag, ref, x, cuts, batch=False):
    """The stream x in pieces of `cuts` samples and then the rest, call by call against the definition: the outputs, the counters and
    every row's (G, h).  Returns the outputs."""
    out, lo = [], 0
    for n in list(cuts) + [x.shape[1]]:
        hi = min(x.shape[1], lo + n)
        piece = x[:, lo:hi]
        exp = ref.push(piece) if hi > lo else np.zeros((x.shape[0], 0, x.shape[2]), np.int16)
        got = ag.run_batch(piece) if batch else _call(ag, piece, _odd(hi - lo))
        assert got.shape == exp.shape and np.array_equal(got, exp), (lo, hi)
        assert ag.counts() == (ref.N, ar.outputs(ref.N, ref.P))
        assert all(ag.gain(r) == ref.gain(r) for r in range(x.shape[0])), (lo, hi)
        out.append(got)
        lo = hi
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("P", [16, 256, 4096])
def test_definition_parity_cut_and_uncut(fmd, P, width):
    """5 rows through the cuts 7 | 1000 | 333 | rest on device pointers (odd in_cap, odd out_cap), 3 rows in one call, 1 row through
    the host entry in the same cuts: all equal the definition over the whole stream, so the cuts equal one call."""
    rng = np.random.default_rng(100 * P + width)
    cfg = ar.Cfg(P, 12000, 262144, 3, 64)
    x = ar.envelope(rng, 5, 3000 // P + 5, P, width)
    whole = ar.agc_all(x, cfg)
    assert whole.shape[1] >= 4 * P
    ag = _agc(fmd, cfg, 5, width)
    assert ag.kernel_name() == "fmd_ag::fmd_agc_kernel<%d>" % width and ag.gain(4) == (262144, 0)
    assert np.array_equal(_feed(ag, ar.Agc(cfg), x, [7, 1000, 333]), whole)
    three = _agc(fmd, cfg, 3, width)
    assert np.array_equal(_call(three, x[1:4], _odd(x.shape[1])), whole[1:4])
    one = _agc(fmd, cfg, 1, width)
    assert np.array_equal(_feed(one, ar.Agc(cfg), x[4:], [7, 1000, 333], batch=True), whole[4:])
    if width == 1:                                           # [rows, n] in, [rows, n] out
        one.reset()
        assert np.array_equal(one.run_batch(x[4:, :, 0]), whole[4:, :, 0])


@pytest.mark.parametrize("width", [1, 2])
def test_calls_that_end_around_a_blocks_last_sample(fmd, width):
    """P = 64: a first call ending one sample before a block's last, exactly at it, and one after it, then the rest."""
    rng = np.random.default_rng(17 + width)
    P = 64
    cfg = ar.Cfg(P, 20000, 65536, 1, 256)
    x = ar.envelope(rng, 3, 12, P, width)
    whole = ar.agc_all(x, cfg)
    for k in (1, 2, 3, 7):
        for n in (k * P - 1, k * P, k * P + 1):
            ag = _agc(fmd, cfg, 3, width)
            first = _call(ag, x[:, :n], _odd(n))
            assert first.shape[1] == ar.outputs(n, P) == P * max(0, (k - 1 if n < k * P else k) - 1)
            rest = _call(ag, x[:, n:])
            assert np.array_equal(np.concatenate([first, rest], axis=1), whole), (k, n)


def test_calls_that_complete_no_block_are_taken(fmd):
    """P = 4096 and the narrow bank's 655 samples per call: twelve calls return FMD_OK with no output and go into the history, the
    thirteenth completes block 1 and emits block 0.  A call of no samples in between launches nothing and changes nothing."""
    import torch
    rng = np.random.default_rng(19)
    P = 4096
    cfg = ar.Cfg(P, 12000, 65536, 4, 32)
    x = ar.envelope(rng, 3, 4, P, 1, levels=(3, 900, 32767))
    ag, ref = _agc(fmd, cfg, 3, 1), ar.Agc(cfg)
    outs = []
    for i in range(12):
        got = _call(ag, x[:, 655 * i:655 * (i + 1)], 657)
        assert got.shape[1] == 0 and ref.push(x[:, 655 * i:655 * (i + 1)]).shape[1] == 0
        assert ag.counts() == (655 * (i + 1), 0) and ag.gain(1) == (65536, 0)
        if i == 5:
            d = torch.full((3, 9), SENT, dtype=torch.int16, device="cuda")
            assert ag.run_device(d.data_ptr(), 0, 9, d.data_ptr(), 9) == 0 and ag.counts() == (655 * 6, 0)
            ag.check()
            assert (d.cpu().numpy() == SENT).all() and ag.run_batch(np.zeros((3, 0, 1), np.int16)).shape == (3, 0, 1)
    outs.append(_call(ag, x[:, 7860:8515], 655))
    assert outs[0].shape[1] == P and np.array_equal(outs[0], ref.push(x[:, 7860:8515])) and ag.gain(2) == ref.gain(2)
    outs.append(_call(ag, x[:, 8515:]))
    assert np.array_equal(np.concatenate(outs, axis=1), ar.agc_all(x, cfg))


@pytest.mark.parametrize("width", [1, 2])
def test_one_call_of_more_blocks_than_a_segment_holds(fmd, width):
    """One row, P = 16, 40000 samples: 2499 blocks in one call, where an LDS segment holds 511 (width 1) or 255 (width 2); and the
    same stream cut in two inside a segment."""
    rng = np.random.default_rng(23 + width)
    cfg = ar.Cfg(16, 12000, 262144, 3, 64)
    x = ar.envelope(rng, 1, 2500, 16, width)[:, :40000]
    whole = ar.agc_all(x, cfg)
    assert whole.shape[1] == 16 * 2499
    ag = _agc(fmd, cfg, 1, width)
    assert np.array_equal(_call(ag, x, 40001), whole)
    assert ag.gain() == ar.agc_row(x[0], cfg)[1][-1]
    ag.reset()
    assert ag.counts() == (0, 0) and ag.gain() == (262144, 0)
    assert np.array_equal(_feed(ag, ar.Agc(cfg), x, [12345]), whole)


AMPS = [900, 0, 32768, 40, 0, 0, 32767, 3, 0, 0, 0, 0, 0, 32768, 32768, 900, 40, 3, 3, 3, 3, 40, 3, 3, 3, 3, 3, 3, 900, 0, 3, 3]


@pytest.mark.parametrize("target,gain_max", [(1, 1), (1, 262144), (32767, 1), (32767, 262144)])
def test_full_scale_values_zero_runs_and_the_configurations_corners(fmd, target, gain_max):
    """Zero runs of 1, 2 and 5 blocks, a full-scale block (-32768 included) directly behind each, then a long quiet stretch that lets
    the gain recover; hang 0 and 3, decay 1, 64 and 256, both widths; two rows, the second the first one's blocks in reverse."""
    rng = np.random.default_rng(29 + target + gain_max)
    P = 64
    for i, (hang, decay) in enumerate([(0, 1), (0, 64), (0, 256), (3, 1), (3, 64), (3, 256)]):
        width = 1 + i % 2
        cfg = ar.Cfg(P, target, gain_max, hang, decay)
        x = np.stack([ar.from_peaks(rng, AMPS, P, width, 5), ar.from_peaks(rng, AMPS[::-1], P, width, 5)])
        assert x.min() == -32768 and np.abs(x[:, :, 0].astype(np.int64)).max() >= 32767
        whole = ar.agc_all(x, cfg)
        assert np.abs(whole.astype(np.int64)).max() <= target
        ag = _agc(fmd, cfg, 2, width)
        assert np.array_equal(_feed(ag, ar.Agc(cfg), x, [3 * P + 1, 9 * P]), whole), cfg


def test_refused_calls_write_nothing_and_take_nothing(fmd):
    import torch
    rng = np.random.default_rng(31)
    P = 256
    cfg = ar.Cfg(P, 12000, 65536, 4, 32)
    x = ar.envelope(rng, 2, 12, P, 2)
    whole = ar.agc_all(x, cfg)
    ag = _agc(fmd, cfg, 2, 2)
    first = _call(ag, x[:, :700])
    rest = x[:, 700:]
    n = rest.shape[1]
    made = ar.outputs(x.shape[1], P) - ar.outputs(700, P)
    d_in = torch.from_numpy(np.ascontiguousarray(rest)).cuda()
    d_out = torch.full((2, made + 8, 2), SENT, dtype=torch.int16, device="cuda")
    before, gain = ag.counts(), ag.gain(1)
    for n_in, in_cap, out_cap in ((n, n - 1, made + 8), (n, n, made - 1), (n, n, 0)):   # n_in > in_cap; out_cap below the outputs
        with pytest.raises(fmd.FmdError) as e:
            ag.run_device(d_in.data_ptr(), n_in, in_cap, d_out.data_ptr(), out_cap)
        assert e.value.status == CAPACITY and ag.counts() == before
    with pytest.raises(fmd.FmdError) as e:                  # a width-2 row at a 2-byte offset
        ag.run_device(d_in.data_ptr() + 2, n - 1, n - 1, d_out.data_ptr(), made + 8)
    assert e.value.status == -1 and ag.counts() == before and ag.gain(1) == gain
    ag.check()
    assert (d_out.cpu().numpy() == SENT).all()
    assert np.array_equal(np.concatenate([first, _call(ag, rest)], axis=1), whole)   # the next call equals the uncut one


def test_reset_a_callers_stream_and_two_handles(fmd):
    import torch
    rng = np.random.default_rng(37)
    ca, cb = ar.Cfg(256, 12000, 65536, 4, 32), ar.Cfg(16, 3000, 262144, 0, 256)
    xa, xb = ar.envelope(rng, 7, 8, 256, 2), ar.envelope(rng, 2, 200, 16, 1)
    a, b = _agc(fmd, ca, 7, 2), _agc(fmd, cb, 2, 1)
    ra, rb = ar.Agc(ca), ar.Agc(cb)
    stream = torch.cuda.Stream()
    first = None
    for lo, hi in ((0, 600), (600, 601), (601, 2048)):      # the two handles interleaved, a on the caller's stream, b on the default one
        ya = _call(a, xa[:, lo:hi], stream=stream.cuda_stream)
        yb = _call(b, xb[:, lo:hi], _odd(hi - lo))
        assert np.array_equal(ya, ra.push(xa[:, lo:hi])) and np.array_equal(yb, rb.push(xb[:, lo:hi]))
        assert a.gain(6) == ra.gain(6) and b.gain(1) == rb.gain(1)
        first = ya if first is None else first
    a.reset()
    assert a.counts() == (0, 0) and a.gain(3) == (65536, 0)
    assert np.array_equal(_call(a, xa[:, :600]), first)      # reset reproduces the first call
    assert b.counts() == (2048, ar.outputs(2048, 16))


def test_narrow_bank_am_into_leveled_on_device_buffers(fmd):
    """The narrow-band bank in AM mode at gain = 256 (w as it is): its d_out, as it stands and with its out_cap as in_cap, through
    leveled(bank) equals the definition over narrow_ref, call by call."""
    import torch
    rng = np.random.default_rng(41)
    fs, D, T, R, Ta, S, K = 2400000, 10, 64, 5, 127, 2, 3
    h = st.lowpass(T, 100000 / fs)
    incs = np.array([[fmd.phase_inc(int(o), fs) for o in rng.integers(-900000, 900000, K)] for _ in range(S)], np.uint32)
    g = fmd.narrow_taps(fs // D, Ta, -6000, 6000)
    nb = fmd.NarrowBank(h, D, incs, g, R, mode=nr.AM, n_streams=S, block=64, squelch=0, gain=256, device_id=0)
    refs = [nr.NarrowRef(nb.taps, nb.decim, incs[s], nb.shift, nb.gr, nb.gi, nb.mode, nb.chan_decim, nb.chan_shift, nb.block, nb.squelch,
                         nb.gain) for s in range(S)]
    ag = fmd.leveled(nb, target=10000, block=64, hang=2, decay=64, gain_max=262144, device_id=0)
    assert (ag.n_rows, ag.width) == (S * K, 1)
    ref = ar.Agc(ar.Cfg(64, 10000, 262144, 2, 64))
    total = 0
    for n in (8 * 2403, 8 * 1001, 8 * 9000):
        data = iq_bytes(rng, S, n, quiet=True)
        cap = nb.out_cap(n) + 3
        d_audio = torch.full((S, K, cap), SENT, dtype=torch.int16, device="cuda")
        out_cap = ag.out_cap(cap) | 1
        d_out = torch.full((S * K, out_cap), SENT, dtype=torch.int16, device="cuda")
        d_iq = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        m = nb.run_device(d_iq.data_ptr(), n, d_audio.data_ptr(), cap)
        n_out = ag.run_device(d_audio.data_ptr(), m, cap, d_out.data_ptr(), out_cap)      # the bank's out_cap is the in_cap
        ag.check()
        audio = np.stack([refs[s].feed(data[s]) for s in range(S)]).reshape(S * K, m, 1).astype(np.int16)
        exp = ref.push(audio)
        got = d_out.cpu().numpy()
        assert n_out == exp.shape[1] and np.array_equal(got[:, :n_out], exp[:, :, 0]) and (got[:, n_out:] == SENT).all()
        total += n_out
    assert total > 0 and ag.gain(S * K - 1) == ref.gain(S * K - 1)


def test_stereo_bank_into_agc_into_resampler_on_device_buffers(fmd):
    """The stereo bank's smallest corner at 256 kHz: its (L, R) rows through a width-2 Agc and on through a 15 / 16 resampler, each
    taking the buffer before it as it stands, equal the three definitions composed."""
    import torch
    rng = np.random.default_rng(43)
    S, K, D, R, P, rate = 2, 1, 2, 1, 1024, 256000
    h = rng.integers(-2047, 2048, 17).astype(np.int16)
    incs = np.array([[int(rng.integers(0, 1 << 32)) for _ in range(K)] for _ in range(S)], np.uint32)
    g = np.array([16383], np.int16)
    sb = fmd.StereoBank(h, D, incs, rate, g, R, n_streams=S, block=P, pilot_min=1, audio_shift=3,
                        shift=fmd.stations_auto_shift(h, incs, limit=256), device_id=0)
    refs = [st.StereoRef(sb.taps, D, incs[s], sb.shift, rate, g, R, P, 1, 3, z=sr.z_corr) for s in range(S)]
    ag = fmd.leveled(sb, target=12000, block=256, hang=4, decay=32, gain_max=65536, device_id=0)
    assert (ag.n_rows, ag.width) == (S * K, 2)
    aref = ar.Agc(ar.Cfg(256, 12000, 65536, 4, 32))
    taps, shift = fmd.resample_taps(15, 16, 32)
    rs = fmd.Resampler(taps, 15, 16, shift, n_rows=S * K, width=2, device_id=0)
    rref = rr.Resampler(taps, 15, 16, shift)
    for n in (8 * 1500, 8 * 701):
        data = iq_bytes(rng, S, n, quiet=True)
        cap = sb.out_cap(n) + 1
        d_audio = torch.full((S, K, cap, 2), SENT, dtype=torch.int16, device="cuda")
        lev_cap = ag.out_cap(cap) | 1
        d_lev = torch.full((S * K, lev_cap, 2), SENT, dtype=torch.int16, device="cuda")
        out_cap = rs.out_cap(lev_cap) | 1
        d_out = torch.full((S * K, out_cap, 2), SENT, dtype=torch.int16, device="cuda")
        d_iq = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        m = sb.run_device(d_iq.data_ptr(), n, d_audio.data_ptr(), cap)
        k = ag.run_device(d_audio.data_ptr(), m, cap, d_lev.data_ptr(), lev_cap)
        n_out = rs.run_device(d_lev.data_ptr(), k, lev_cap, d_out.data_ptr(), out_cap)
        rs.check()
        audio = np.stack([refs[s].feed(data[s]) for s in range(S)]).reshape(S * K, m, 2)
        lev = aref.push(audio)
        exp = rref.push(lev)
        assert k == lev.shape[1] > 256 and np.array_equal(d_lev.cpu().numpy()[:, :k], lev)
        got = d_out.cpu().numpy()
        assert n_out == exp.shape[1] and np.array_equal(got[:, :n_out], exp) and (got[:, n_out:] == SENT).all()


@pytest.mark.parametrize("width", [1, 2])
def test_the_tool_levels_a_file_to_its_own_length(fmd, width, tmp_path):
    """agc_gpu over a file equals the definition over the input with 2 P zero samples behind it, cut to the input's length; from a
    pipe to a pipe as well."""
    rng = np.random.default_rng(47 + width)
    P = 64
    x = ar.envelope(rng, 1, 2100, P, width, levels=(0, 40, 900, 32767, 32768))     # more than two reads of 65536 samples
    n = x.shape[1]
    padded = np.concatenate([x, np.zeros((1, 2 * P, width), np.int16)], axis=1)
    exp = ar.agc_all(padded, ar.Cfg(P, 9000, 131072, 2, 128))[0, :n]
    assert exp.shape[0] == n > 2 * 65536
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "agc_gpu")
    args = [exe, "-c", str(width), "-t", "9000", "-b", "64", "-H", "2", "-d", "128", "-g", "131072"]
    (tmp_path / "in.s16").write_bytes(x.tobytes())
    p = subprocess.run(args + [str(tmp_path / "in.s16"), str(tmp_path / "out.s16")], capture_output=True, timeout=300)
    assert (p.returncode, p.stdout) == (0, b""), p.stderr.decode()
    assert (tmp_path / "out.s16").read_bytes() == exp.tobytes()
    p = subprocess.run(args, input=x[:, :1000].tobytes(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    short = np.concatenate([x[:, :1000], np.zeros((1, 2 * P, width), np.int16)], axis=1)
    assert p.stdout == ar.agc_all(short, ar.Cfg(P, 9000, 131072, 2, 128))[0, :1000].tobytes()


INVALID_ARG, TOO_SHORT, UNSUPPORTED = -1, -3, -6
BIG = (1 << 28) + 1
# (handle, byte offset of d_in, n_in, in_cap, out_cap, status, text): calls over buffers of 2 x 80 samples that two checks refuse, or
# that lie at the edge of one
REFUSALS = [(k,) + c for k in ("resample", "agc") for c in [
    (2, 81, 80, 80, INVALID_ARG, "misaligned device buffer"),
    (0, 81, 80, 0, CAPACITY, "n_in > in_cap"),
    (0, BIG, BIG, 0, UNSUPPORTED, "n_in out of range"),      # (out_cap 0: whatever the order of the checks, nothing is launched)
]] + [
    ("resample", 0, 63, 62, 80, CAPACITY, "n_in > in_cap"),  # not too-short
    ("resample", 0, 63, 63, 0, TOO_SHORT, "completes no output"),
    ("resample", None, 0, 0, 0, TOO_SHORT, ""),              # run_batch of zero samples
    ("agc", 0, 0, 80, 0, 0, ""),                             # nothing to take: accepted, returns 0
]


@pytest.mark.parametrize("kind,off,n_in,in_cap,out_cap,status,text", REFUSALS,
                         ids=["%s-%s-%d-%d-%d" % (c[0], c[1], c[2] if c[2] < BIG else -1, c[3] if c[3] < BIG else -1, c[4]) for c in REFUSALS])
def test_the_order_of_refusals_and_what_they_leave(fmd, kind, off, n_in, in_cap, out_cap, status, text):
    """3 / 16 at T = 64 and an AGC of P = 16, 2 rows of width 2, fresh: where two checks refuse a call the first one answers -- the
    alignment, then n_in > in_cap, then the range of n_in, then what the call completes and out_cap -- and a refused call takes
    nothing and writes nothing."""
    import torch
    if kind == "resample":
        g = np.zeros((3, 64), np.int16)
        g[:, 0] = 16384
        h = fmd.Resampler(g, 3, 16, 14, n_rows=2, width=2, device_id=0)
    else:
        h = _agc(fmd, (16, 12000, 65536, 4, 32), 2, 2)
    d_in = torch.full((2, 80, 2), SENT, dtype=torch.int16, device="cuda")
    d_out = torch.full((2, 80, 2), SENT, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    before = h.counts()

    def run():
        if off is None:
            return h.run_batch(np.zeros((2, 0, 2), np.int16)).shape[1]
        return h.run_device(d_in.data_ptr() + off, n_in, in_cap, d_out.data_ptr(), out_cap)
    if status == 0:
        assert run() == 0
    else:
        with pytest.raises(fmd.FmdError) as e:
            run()
        assert e.value.status == status and text in str(e.value), str(e.value)
    assert h.counts() == before == (0, 0)
    h.check()
    assert (d_out.cpu().numpy() == SENT).all() and (d_in.cpu().numpy() == SENT).all()
