"""Rational resampler (include/fmd.h, fmd_resample_*) on the MI355X: bit for bit against the test-side definition
(tests/resample_ref.py) over the issue's ratios at both widths, unaligned rows and odd capacities, tile edges, call cuts, the
skip-ahead path, refused calls, saturation, reset, a caller's stream, two handles, and composed with the stereo bank, the
channelizer and the command-line tool.  Everything but the tool runs in this process."""
import functools
import os
import subprocess

import numpy as np
import pytest

import channelizer_ref as cr
import resample_ref as rr
from rows_cases import taps as _taps
from rows_gpu import SENT, TOO_SHORT, call, iq_bytes
import stations_ref as sr
import stereo_ref as st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = -5
_call = functools.partial(call, out_pad=3)

# (L, M, T, samples per row): the issue's shapes; the sample counts give more than one tile of 256 outputs wherever 6000 inputs can
SHAPES = [(1, 1, 1, 1500), (1, 1, 256, 2000), (15, 16, 32, 3000), (3, 16, 64, 6000), (441, 512, 24, 3000), (160, 147, 48, 2500),
          (6, 1, 8, 1400), (1, 32, 256, 6000), (1024, 1023, 16, 2500)]


def _feed(fmd, rs, ref, x, cuts, odd_caps=True):
    """The stream x in pieces of `cuts` samples and then the rest, call by call against the definition; a piece that completes no
    output is refused by both, changes nothing, and is handed over again in front of the next one.  Returns the outputs."""
    out, lo, pos, calls = [], 0, 0, 0
    for n in list(cuts) + [x.shape[1]]:
        pos = min(x.shape[1], pos + n)
        if pos == lo:
            continue
        piece = x[:, lo:pos]
        in_cap = piece.shape[1] + (0 if not odd_caps or calls % 2 == 0 else 2 + piece.shape[1] % 2)   # n_in, or odd and larger
        try:
            exp = ref.push(piece)
        except rr.TooShort:
            before = rs.counts()
            with pytest.raises(fmd.FmdError) as e:
                _call(rs, piece, in_cap)
            assert e.value.status == TOO_SHORT and rs.counts() == before
            continue
        got = _call(rs, piece, in_cap)
        assert got.shape == exp.shape and np.array_equal(got, exp), (lo, pos)
        assert rs.counts() == (ref.N, rr.outputs(ref.N, ref.L, ref.M, ref.T))
        out.append(got)
        lo = pos
        calls += 1
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("L,M,T,N", SHAPES, ids=["%d/%d-T%d" % s[:3] for s in SHAPES])
def test_definition_parity_cut_and_uncut(fmd, L, M, T, N, width):
    """5 rows through the cuts 7 | 1000 | 333 | rest (odd in_cap on every second call, odd out_cap), then row 0 alone in one call:
    both equal the definition over the whole stream, so the cuts equal one call."""
    rng = np.random.default_rng(100 * L + M + T + width)
    g, shift = _taps(rng, L, T), int(rng.integers(12, 17))
    x = rng.integers(-32768, 32768, (5, N, width)).astype(np.int16)
    whole = rr.resample_all(x, g, L, M, shift)
    rs = fmd.Resampler(g, L, M, shift, n_rows=5, width=width, device_id=0)
    assert rs.kernel_name() == "fmd_rs::fmd_resample_kernel<%d>" % width
    got = _feed(fmd, rs, rr.Resampler(g, L, M, shift), x, [7, 1000, 333])
    assert np.array_equal(got, whole)
    one = fmd.Resampler(g, L, M, shift, n_rows=1, width=width, device_id=0)
    assert np.array_equal(_call(one, x[:1], in_cap=N + 1), whole[:1])


@pytest.mark.parametrize("width", [1, 2])
def test_identity_and_designed_taps_through_the_host_path(fmd, width):
    rng = np.random.default_rng(3 + width)
    x = rng.integers(-32768, 32768, (2, 1000, width)).astype(np.int16)
    ident = fmd.Resampler(np.array([[1]], np.int16), 1, 1, 0, n_rows=2, width=width, device_id=0)
    assert np.array_equal(ident.run_batch(x), x)
    g, shift = fmd.resample_taps(15, 16, 32)
    rs = fmd.Resampler(g, 15, 16, shift, n_rows=2, width=width, device_id=0)
    ref = rr.Resampler(g, 15, 16, shift)
    for lo, hi in ((0, 400), (400, 1000)):
        assert np.array_equal(rs.run_batch(x[:, lo:hi]), ref.push(x[:, lo:hi]))
    if width == 1:                                           # [rows, n] in, [rows, n] out
        rs.reset()
        assert np.array_equal(rs.run_batch(x[:, :400, 0]), rr.resample_all(x[:, :400], g, 15, 16, shift)[:, :, 0])


@pytest.mark.parametrize("width", [1, 2])
def test_calls_that_end_at_a_tiles_last_input(fmd, width):
    """15/16 at T = 32: output 255, the last of the first tile, reads x[272 ... 303].  303 samples stop one short of it, 304 end
    exactly at it, 305 start the second tile; the same once more around the second tile's last input (575), after a first call."""
    rng = np.random.default_rng(17)
    L, M, T = 15, 16, 32
    g, shift = _taps(rng, L, T), 14
    x = rng.integers(-32768, 32768, (1, 1200, width)).astype(np.int16)
    whole = rr.resample_all(x, g, L, M, shift)
    assert 255 * M // L + T == 304 and 511 * M // L + T == 577
    assert [rr.outputs(n, L, M, T) for n in (303, 304, 305, 576, 577)] == [255, 256, 257, 511, 512]
    for rows in (1, 5):
        xs = np.repeat(x, rows, axis=0)
        for n in (303, 304, 305, 576, 577, 578):
            outs = rr.outputs(n, L, M, T)
            rs = fmd.Resampler(g, L, M, shift, n_rows=rows, width=width, device_id=0)
            got = _call(rs, xs[:, :n], in_cap=n + 1 + n % 2)
            assert got.shape[1] == outs and all(np.array_equal(got[r], whole[0, :outs]) for r in range(rows)), (rows, n)
            got = _call(rs, xs[:, n:1200])                  # the rest, with the history of a call that ended there
            assert all(np.array_equal(got[r], whole[0, outs:]) for r in range(rows)), (rows, n)


@pytest.mark.parametrize("width", [1, 2])
def test_skip_ahead_where_the_stride_exceeds_the_taps(fmd, width):
    """1/32 at T = 8: after 10 samples output 0 is done and output 1 starts at x[32], beyond what has arrived: no history, and the
    next accepted call skips inputs.  Pieces of 5 samples: most complete nothing and are handed over again."""
    rng = np.random.default_rng(23)
    g = _taps(rng, 1, 8)
    x = rng.integers(-32768, 32768, (3, 700, width)).astype(np.int16)
    rs = fmd.Resampler(g, 1, 32, 15, n_rows=3, width=width, device_id=0)
    ref = rr.Resampler(g, 1, 32, 15)
    got = _feed(fmd, rs, ref, x, [5] * 139)
    assert np.array_equal(got, rr.resample_all(x, g, 1, 32, 15)) and got.shape[1] == rr.outputs(700, 1, 32, 8) == 22
    ref.reset()
    ref.push(x[:, :10])
    assert ref.history() == 0                                # (the state the pieces went through)


def test_refused_calls_change_nothing_and_write_nothing(fmd):
    import torch
    rng = np.random.default_rng(29)
    L, M, T = 3, 16, 64
    g = _taps(rng, L, T)
    x = rng.integers(-32768, 32768, (2, 2000, 2)).astype(np.int16)
    whole = rr.resample_all(x, g, L, M, 15)
    rs = fmd.Resampler(g, L, M, 15, n_rows=2, width=2, device_id=0)
    with pytest.raises(fmd.FmdError) as e:                  # 63 samples complete nothing
        _call(rs, x[:, :63])
    assert e.value.status == TOO_SHORT and rs.counts() == (0, 0)
    first = _call(rs, x[:, :700])
    with pytest.raises(fmd.FmdError) as e:                  # nor do 2 more
        _call(rs, x[:, 700:702])
    assert e.value.status == TOO_SHORT and rs.counts() == (700, first.shape[1])
    d_in = torch.from_numpy(x[:, 700:]).cuda()
    d_out = torch.full((2, 400, 2), SENT, dtype=torch.int16, device="cuda")
    before = rs.counts()
    for n_in, in_cap, out_cap in ((1300, 1299, 400), (1300, 1300, 243), (1300, 1300, 0)):   # n_in > in_cap; out_cap below the 244 outputs
        with pytest.raises(fmd.FmdError) as e:
            rs.run_device(d_in.data_ptr(), n_in, in_cap, d_out.data_ptr(), out_cap)
        assert e.value.status == CAPACITY and rs.counts() == before
    with pytest.raises(fmd.FmdError) as e:                  # a width-2 row at a 2-byte offset
        rs.run_device(d_in.data_ptr() + 2, 1200, 1300, d_out.data_ptr(), 400)
    assert e.value.status == -1 and rs.counts() == before
    rs.check()
    assert (d_out.cpu().numpy() == SENT).all()
    rest = _call(rs, x[:, 700:])                        # the next call equals the uncut one
    assert np.array_equal(np.concatenate([first, rest], axis=1), whole)


@pytest.mark.parametrize("shift", [0, 14])
def test_full_scale_input_saturates(fmd, shift):
    """Full-scale input of both signs through phases with sum |g| = 32767: |v| reaches 32767 * 32768 < 2^30, and the store clamps."""
    rng = np.random.default_rng(31 + shift)
    g = np.array([[32767, 0, 0, 0], [16384, -16383, 0, 0], [-8192, 8192, -8192, 8191]], np.int16)
    x = rng.choice(np.array([-32768, 32767, -32768, 32767, 5, -1], np.int16), (2, 1500, 2))
    x[0, :40] = -32768
    x[0, 40:80:2] = 32767
    exp = rr.resample_all(x, g, 3, 2, shift)
    assert (exp == 32767).any() and (exp == -32768).any() and ((exp > -32768) & (exp < 32767)).any()
    rs = fmd.Resampler(g, 3, 2, shift, n_rows=2, width=2, device_id=0)
    assert np.array_equal(_call(rs, x), exp)
    mono = fmd.Resampler(g, 3, 2, shift, n_rows=2, width=1, device_id=0)
    assert np.array_equal(_call(mono, x[:, :, :1], in_cap=1501), exp[:, :, :1])


def test_reset_a_callers_stream_and_two_handles(fmd):
    import torch
    rng = np.random.default_rng(37)
    ga, gb = _taps(rng, 160, 48), _taps(rng, 3, 64)
    xa = rng.integers(-32768, 32768, (7, 1500, 2)).astype(np.int16)
    xb = rng.integers(-32768, 32768, (2, 3000, 1)).astype(np.int16)
    a = fmd.Resampler(ga, 160, 147, 15, n_rows=7, width=2, device_id=0)
    b = fmd.Resampler(gb, 3, 16, 14, n_rows=2, width=1, device_id=0)
    ra, rb = rr.Resampler(ga, 160, 147, 15), rr.Resampler(gb, 3, 16, 14)
    stream = torch.cuda.Stream()
    first = None
    for lo, hi in ((0, 500), (500, 501), (501, 1500)):      # the two handles interleaved, a on the caller's stream, b on the default one
        ya = _call(a, xa[:, lo:hi], stream=stream.cuda_stream)
        yb = _call(b, xb[:, 2 * lo:2 * hi], in_cap=2 * (hi - lo) + 1)
        assert np.array_equal(ya, ra.push(xa[:, lo:hi])) and np.array_equal(yb, rb.push(xb[:, 2 * lo:2 * hi]))
        first = ya if first is None else first
    a.reset()
    assert a.counts() == (0, 0)
    assert np.array_equal(_call(a, xa[:, :500]), first)   # reset reproduces the first call
    assert b.counts() == (3000, rr.outputs(3000, 3, 16, 64))


def test_stereo_bank_into_fixed_rate_on_device_buffers(fmd):
    """The stereo bank's smallest corner (one station, decimate 2, one audio tap at stride 1, blocks of 1024) at 256 kHz: its d_out,
    as it stands, through fixed_rate(bank, 48000) -- 128 kHz to 48 kHz, L / M = 3 / 8 -- equals the definition over stereo_ref."""
    import torch
    rng = np.random.default_rng(41)
    S, K, D, R, P, rate = 2, 1, 2, 1, 1024, 256000
    h = rng.integers(-2047, 2048, 17).astype(np.int16)
    incs = np.array([[int(rng.integers(0, 1 << 32)) for _ in range(K)] for _ in range(S)], np.uint32)
    g = np.array([16383], np.int16)
    sb = fmd.StereoBank(h, D, incs, rate, g, R, n_streams=S, block=P, pilot_min=1, audio_shift=3,
                        shift=fmd.stations_auto_shift(h, incs, limit=256), device_id=0)
    refs = [st.StereoRef(sb.taps, D, incs[s], sb.shift, rate, g, R, P, 1, 3, z=sr.z_corr) for s in range(S)]
    rs = fmd.fixed_rate(sb, 48000)
    assert (rs.L, rs.M, rs.T, rs.n_rows, rs.width) == (3, 8, 32, S * K, 2) and fmd.bank_rate(sb) == 128000
    ref = rr.Resampler(rs.taps, rs.L, rs.M, rs.shift)
    for n in (8 * 1500, 8 * 701):
        data = iq_bytes(rng, S, n)
        cap = sb.out_cap(n) + 1
        d_audio = torch.full((S, K, cap, 2), SENT, dtype=torch.int16, device="cuda")
        out_cap = rs.out_cap(cap) | 1
        d_out = torch.full((S * K, out_cap, 2), SENT, dtype=torch.int16, device="cuda")
        d_iq = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        m = sb.run_device(d_iq.data_ptr(), n, d_audio.data_ptr(), cap)
        n_out = rs.run_device(d_audio.data_ptr(), m, cap, d_out.data_ptr(), out_cap)      # the bank's out_cap is the in_cap
        rs.check()
        audio = np.stack([refs[s].feed(data[s]) for s in range(S)]).reshape(S * K, m, 2)
        exp = ref.push(audio)
        got = d_out.cpu().numpy()
        assert n_out == exp.shape[1] and np.array_equal(got[:, :n_out], exp) and (got[:, n_out:] == SENT).all()


def test_channelizer_into_a_width_2_resampler_and_the_tool(fmd, tmp_path):
    """The channelizer's (yr, yi) rows at capture / 10 through 15 / 16 equal the definition over channelizer_ref, and resample_gpu over
    a file of row 0's bytes writes the same bytes."""
    import torch
    rng = np.random.default_rng(43)
    S, K, D = 2, 3, 10
    h = rng.integers(-2047, 2048, 40).astype(np.int16)
    incs = np.array([[int(rng.integers(0, 1 << 32)) for _ in range(K)] for _ in range(S)], np.uint32)
    ch = fmd.Channelizer(h, D, incs, n_streams=S, device_id=0)
    refs = [cr.ChannelizerRef(h, D, incs[s], ch.shift, z=sr.z_corr) for s in range(S)]
    g, shift = fmd.resample_taps(15, 16, 32)
    rs = fmd.Resampler(g, 15, 16, shift, n_rows=S * K, width=2, device_id=0)
    ref = rr.Resampler(g, 15, 16, shift)
    rows, outs = [], []
    for n in (8 * 2500, 8 * 1203):
        data = iq_bytes(rng, S, n)
        cap = ch.out_cap(n) + 3
        d_y = torch.full((S, K, cap, 2), SENT, dtype=torch.int16, device="cuda")
        out_cap = rs.out_cap(cap)
        d_out = torch.full((S * K, out_cap, 2), SENT, dtype=torch.int16, device="cuda")
        d_iq = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        m = ch.run_device(d_iq.data_ptr(), n, d_y.data_ptr(), cap)
        n_out = rs.run_device(d_y.data_ptr(), m, cap, d_out.data_ptr(), out_cap)
        rs.check()
        y = np.stack([refs[s].feed(data[s]) for s in range(S)]).reshape(S * K, m, 2).astype(np.int16)
        exp = ref.push(y)
        got = d_out.cpu().numpy()
        assert n_out == exp.shape[1] and np.array_equal(got[:, :n_out], exp) and (got[:, n_out:] == SENT).all()
        rows.append(y[0])
        outs.append(exp[0])
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "resample_gpu")
    (tmp_path / "row0.cs16").write_bytes(np.concatenate(rows).tobytes())
    p = subprocess.run([exe, "-i", "51200", "-r", "48000", "-c", "2", str(tmp_path / "row0.cs16")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert "L / M = 15 / 16" in p.stderr.decode()
    assert p.stdout == np.concatenate(outs).tobytes()
