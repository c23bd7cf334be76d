"""Tone-pair demodulator (include/fmd.h, fmd_afsk_*) on the MI355X: bit for bit against the test-side definition (tests/afsk_ref.py)
over windows and strides at the domain's ends, row counts, unaligned rows and odd capacities, call cuts, tile edges, refused calls,
the i32 bound, both rails, the shifts' ends, reset, a caller's stream, two handles, both entries, and composed with the narrow-band
bank, the host's AX.25 decoder and the command-line tool.  Everything but the tool runs in this process."""
import functools
import os
import subprocess

import numpy as np
import pytest

import afsk_ref as ar
import ax25_ref as xr
import narrow_ref as nr
from rows_gpu import SENT, TOO_SHORT, call, call_at
import stations_ref as sr
import stereo_ref as st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = -5
_call = functools.partial(call, out_pad=3)


def _table(rng, T):
    t = rng.integers(-1023, 1024, (4, T)).astype(np.int16)
    t[0, 0], t[3, -1] = 1023, -1023
    return t


def _x(rng, rows, n):
    x = rng.integers(-32768, 32768, (rows, n, 1)).astype(np.int16)
    x[:, n // 3] = -32768
    return x


def _feed(fmd, h, ref, x, cuts, odd_caps=True):
    """The stream x [rows, n, 1] in pieces of `cuts` samples and then the rest, call by call against the definition; a piece that
    completes no output is refused by both, changes nothing, and is handed over again in front of the next one."""
    out, lo, pos, calls = [], 0, 0, 0
    for n in list(cuts) + [x.shape[1]]:
        pos = min(x.shape[1], pos + n)
        if pos == lo:
            continue
        piece = x[:, lo:pos]
        in_cap = piece.shape[1] + (0 if not odd_caps or calls % 2 == 0 else 2 + piece.shape[1] % 2)   # n_in, or odd and larger
        exp = ref.push(piece[:, :, 0])
        if exp is None:
            before = h.counts()
            with pytest.raises(fmd.FmdError) as e:
                _call(h, piece, in_cap)
            assert e.value.status == TOO_SHORT and h.counts() == before
            continue
        got = _call(h, piece, in_cap)[:, :, 0]
        assert got.shape == exp.shape and np.array_equal(got, exp), (lo, pos)
        assert h.counts() == (ref.pos, ar.outputs(ref.T, ref.D, ref.pos))
        out.append(got)
        lo = pos
        calls += 1
    return np.concatenate(out, axis=1)


SHAPES = [(T, D) for T in (2, 3, 9, 10, 63, 64) for D in sorted({1, 2, min(T, 32)})]


@pytest.mark.parametrize("T,D", SHAPES, ids=["T%d-D%d" % s for s in SHAPES])
def test_definition_parity_cut_and_uncut(fmd, T, D):
    """Random tables; 3 rows through the cuts 7 | 1000 | 333 | rest (odd in_cap on every second call, odd out_cap; more than one tile
    of 256 outputs wherever 2600 samples give one), then row 0 alone in one call: both equal the definition over the whole stream."""
    rng = np.random.default_rng(100 * T + D)
    tab, pre, x = _table(rng, T), int(rng.integers(4, 10)), _x(rng, 3, 2600)
    out = next(s for s in range(49) if (np.abs(ar.demod(x[:, :, 0], tab, D, pre, s).astype(np.int64)) >= 32767).mean() < 0.25)
    whole = ar.demod(x[:, :, 0], tab, D, pre, out)          # (a quarter of the outputs at the rails at most, the rest in between)
    assert (np.abs(whole.astype(np.int64)) < 32767).any() and (np.abs(whole.astype(np.int64)) > 100).any()
    h = fmd.AfskDemod(tab, D, pre, out, n_rows=3, device_id=0)
    assert h.kernel_name() == "fmd_af::fmd_afsk_kernel"
    assert np.array_equal(_feed(fmd, h, ar.AfskDemod(tab, D, pre, out, rows=3), x, [7, 1000, 333]), whole)
    one = fmd.AfskDemod(tab, D, pre, out, n_rows=1, device_id=0)
    assert np.array_equal(_call(one, x[:1], in_cap=2601)[:, :, 0], whole[:1])


@pytest.mark.parametrize("rows", [1, 3, 70])
def test_row_counts_with_the_designed_table_through_both_entries(fmd, rows):
    """The designed table at 12 kHz (T 10, D 2): the host entry and the device entry give the definition, call by call."""
    rng = np.random.default_rng(rows)
    tab, pre, out = fmd.afsk_table(12000)
    x = _x(rng, rows, 1500)
    ref = ar.AfskDemod(tab, 2, pre, out, rows=rows)
    host, dev = fmd.AfskDemod(tab, 2, pre, out, n_rows=rows, device_id=0), fmd.AfskDemod(tab, 2, pre, out, n_rows=rows, device_id=0)
    for lo, hi in ((0, 655), (655, 1500)):
        exp = ref.push(x[:, lo:hi, 0])
        assert np.array_equal(host.run_batch(x[:, lo:hi, 0]), exp)                          # [rows, n] in, [rows, n] out
        assert np.array_equal(_call(dev, x[:, lo:hi], in_cap=hi - lo + 1)[:, :, 0], exp)
    assert host.counts() == dev.counts() == (1500, ar.outputs(10, 2, 1500))
    with pytest.raises(fmd.FmdError) as e:                  # the host entry refuses a short call like the device entry
        host.run_batch(x[:, :1, 0])
    assert e.value.status == TOO_SHORT and host.counts()[0] == 1500


@pytest.mark.parametrize("off_in,off_out", [(1, 0), (3, 5), (7, 1), (0, 7)])
def test_rows_at_odd_two_byte_offsets(fmd, off_in, off_out):
    """Input and output rows that start 2, 6, 14 bytes behind a 16-byte boundary: the 16-byte loads keep to whole chunks inside the
    row, the rest comes by elements; nothing outside the outputs is written."""
    rng = np.random.default_rng(10 * off_in + off_out)
    for T, D, n in ((10, 2, 700), (9, 1, 300), (64, 32, 9000)):
        tab = _table(rng, T)
        x = _x(rng, 3, n)
        h = fmd.AfskDemod(tab, D, 8, 14, n_rows=3, device_id=0)
        got = call_at(h, x, off_in=off_in, off_out=off_out)
        assert np.array_equal(got[:, :, 0], ar.demod(x[:, :, 0], tab, D, 8, 14)), (T, D)
        more = _x(rng, 3, 41)                                # a short second call: history in front, an odd offset again
        assert np.array_equal(call_at(h, more, off_in=off_out, off_out=off_in)[:, :, 0],
                              ar.demod(np.concatenate([x, more], axis=1)[:, :, 0], tab, D, 8, 14, first=ar.outputs(T, D, n)))


def test_calls_of_exactly_the_window_then_the_stride(fmd):
    """T samples give output 0; every further D samples give one more; D - 1 give none and are refused."""
    rng = np.random.default_rng(11)
    for T, D in ((10, 2), (9, 9), (64, 32), (3, 1)):
        tab = _table(rng, T)
        x = _x(rng, 2, T + 6 * D)
        whole = ar.demod(x[:, :, 0], tab, D, 8, 14)
        h = fmd.AfskDemod(tab, D, 8, 14, n_rows=2, device_id=0)
        if T > 1:
            with pytest.raises(fmd.FmdError) as e:
                _call(h, x[:, :T - 1])
            assert e.value.status == TOO_SHORT and h.counts() == (0, 0)
        assert np.array_equal(_call(h, x[:, :T])[:, :, 0], whole[:, :1])
        for k in range(6):
            lo = T + k * D
            if D > 1:
                with pytest.raises(fmd.FmdError) as e:
                    _call(h, x[:, lo:lo + D - 1])
                assert e.value.status == TOO_SHORT and h.counts() == (lo, k + 1)
            assert np.array_equal(_call(h, x[:, lo:lo + D])[:, :, 0], whole[:, k + 1:k + 2])
        assert h.counts() == (T + 6 * D, 7)


def test_calls_that_end_at_a_tiles_last_input(fmd):
    """T 10, D 2: output 255, the last of the first tile, reads x[510 ... 519].  519 samples stop one short of it, 520 end exactly at
    it, 521 lie behind it and 522 start the second tile; the same around the second tile's last input (1031), after a first call."""
    rng = np.random.default_rng(17)
    T, D = 10, 2
    tab = _table(rng, T)
    x = _x(rng, 1, 1400)
    whole = ar.demod(x[:, :, 0], tab, D, 8, 14)
    assert [ar.outputs(T, D, n) for n in (519, 520, 521, 522, 1031, 1032, 1034)] == [255, 256, 256, 257, 511, 512, 513]
    for rows in (1, 5):
        xs = np.repeat(x, rows, axis=0)
        for n in (519, 520, 521, 522, 1031, 1032, 1033, 1034):
            outs = ar.outputs(T, D, n)
            h = fmd.AfskDemod(tab, D, 8, 14, n_rows=rows, device_id=0)
            got = _call(h, xs[:, :n], in_cap=n + 1 + n % 2)[:, :, 0]
            assert got.shape[1] == outs and all(np.array_equal(got[r], whole[0, :outs]) for r in range(rows)), (rows, n)
            got = _call(h, xs[:, n:1400])[:, :, 0]          # the rest, with the history of a call that ended there
            assert all(np.array_equal(got[r], whole[0, outs:]) for r in range(rows)), (rows, n)


def test_refused_calls_change_nothing_and_write_nothing(fmd):
    import torch
    rng = np.random.default_rng(29)
    T, D = 21, 4
    tab = _table(rng, T)
    x = _x(rng, 2, 2000)
    whole = ar.demod(x[:, :, 0], tab, D, 8, 14)
    h = fmd.AfskDemod(tab, D, 8, 14, n_rows=2, device_id=0)
    with pytest.raises(fmd.FmdError) as e:                  # 20 samples complete nothing
        _call(h, x[:, :20])
    assert e.value.status == TOO_SHORT and h.counts() == (0, 0)
    first = _call(h, x[:, :701])[:, :, 0]                   # the same samples handed over again, with more behind them
    with pytest.raises(fmd.FmdError) as e:                  # nor do 3 more: 701 = 21 + 4 * 170
        _call(h, x[:, 701:704])
    assert e.value.status == TOO_SHORT and h.counts() == (701, first.shape[1]) and first.shape[1] == 171
    d_in = torch.from_numpy(x[:, 701:, 0].copy()).cuda()
    d_out = torch.full((2, 400), SENT, dtype=torch.int16, device="cuda")
    before = h.counts()
    outs = ar.outputs(T, D, 2000) - ar.outputs(T, D, 701)
    for n_in, in_cap, out_cap in ((1299, 1298, 400), (1299, 1299, outs - 1), (1299, 1299, 0)):    # n_in > in_cap; out_cap below the outputs
        with pytest.raises(fmd.FmdError) as e:
            h.run_device(d_in.data_ptr(), n_in, in_cap, d_out.data_ptr(), out_cap)
        assert e.value.status == CAPACITY and h.counts() == before
    with pytest.raises(fmd.FmdError) as e:                  # a row at a 1-byte offset
        h.run_device(d_in.data_ptr() + 1, 1200, 1299, d_out.data_ptr(), 400)
    assert e.value.status == -1 and h.counts() == before
    h.check()
    assert (d_out.cpu().numpy() == SENT).all()
    n = h.run_device(d_in.data_ptr(), 1299, 1299, d_out.data_ptr(), outs)                    # out_cap exactly the outputs
    h.check()
    flat = d_out.cpu().numpy().reshape(-1)                  # (rows of out_cap = outs samples in the buffer of 2 x 400)
    assert n == outs and np.array_equal(np.concatenate([first, flat[:2 * outs].reshape(2, outs)], axis=1), whole)
    assert (flat[2 * outs:] == SENT).all()


def test_the_i32_bound_and_both_rails(fmd):
    """All samples -32768 against rows of +1023 and -1023 at T = 64: |S| = 2 145 386 496, the largest an i32 sum can be asked for.
    At pre_shift 0 the squares reach 2^61.9 and their difference both signs; out_shift 0 saturates at both rails, 48 does not."""
    T = 64
    S = 64 * 32768 * 1023
    tab = np.zeros((4, T), np.int16)
    tab[0], tab[1] = 1023, -1023                             # mark: S_0 = -S, S_1 = +S; space silent
    x = np.full((2, 300, 1), -32768, np.int16)
    x[1, 100:] = 32767
    x[1, 150::2] = -32768
    for tb in (tab, tab[::-1].copy()):                       # and the same energy on the space side
        for D in (1, 32):
            for pre, out in ((0, 0), (0, 48), (16, 0), (16, 48), (0, 31), (8, 12)):
                exp = ar.demod(x[:, :, 0], tb, D, pre, out)
                h = fmd.AfskDemod(tb, D, pre, out, n_rows=2, device_id=0)
                assert np.array_equal(_call(h, x)[:, :, 0], exp), (D, pre, out)
    assert ar.demod(x[:1, :64, 0], tab, 1, 0, 0).tolist() == [[32767]] and ar.demod(x[:1, :64, 0], tab[::-1].copy(), 1, 0, 0).tolist() == [[-32768]]
    assert ar.demod(x[:1, :64, 0], tab, 1, 0, 48).tolist() == [[(2 * S * S) >> 48]]
    both = np.zeros((4, T), np.int16)                        # mark on the first half of the window, space on the second
    both[0, :32], both[2, 32:] = 1023, 1023
    y = np.zeros((1, 400, 1), np.int16)
    y[0, :200], y[0, 200:] = 32767, -32768
    y[0, 100:110], y[0, 300:340] = 0, 0
    exp = ar.demod(y[:, :, 0], both, 1, 8, 12)
    assert (exp == 32767).any() and (exp == -32768).any() and ((exp > -32768) & (exp < 32767)).any()
    assert np.array_equal(_call(fmd.AfskDemod(both, 1, 8, 12, device_id=0), y)[:, :, 0], exp)


def test_reset_inside_a_window_a_callers_stream_and_two_handles(fmd):
    import torch
    rng = np.random.default_rng(37)
    ta, tb = _table(rng, 40), _table(rng, 9)
    xa, xb = _x(rng, 7, 1500), _x(rng, 2, 3000)
    a = fmd.AfskDemod(ta, 8, 8, 18, n_rows=7, device_id=0)
    b = fmd.AfskDemod(tb, 2, 6, 10, n_rows=2, device_id=0)
    ra, rb = ar.AfskDemod(ta, 8, 8, 18, rows=7), ar.AfskDemod(tb, 2, 6, 10, rows=2)
    stream = torch.cuda.Stream()
    first = None
    for lo, hi in ((0, 500), (500, 511), (511, 1500)):      # the two handles interleaved, a on the caller's stream, b on the default one
        ya = _call(a, xa[:, lo:hi], stream=stream.cuda_stream)[:, :, 0]
        yb = _call(b, xb[:, 2 * lo:2 * hi], in_cap=2 * (hi - lo) + 1)[:, :, 0]
        assert np.array_equal(ya, ra.push(xa[:, lo:hi, 0])) and np.array_equal(yb, rb.push(xb[:, 2 * lo:2 * hi, 0]))
        first = ya if first is None else first
    assert a.counts() == (1500, ar.outputs(40, 8, 1500)) and (1500 - ar.outputs(40, 8, 1500) * 8) > 0      # samples are carried
    a.reset()
    assert a.counts() == (0, 0)
    assert np.array_equal(_call(a, xa[:, :500])[:, :, 0], first)   # reset inside a window: the carried samples are forgotten
    assert b.counts() == (3000, ar.outputs(9, 2, 3000))


# ---- composed --------------------------------------------------------------------------------------------------------------------------
def test_narrow_bank_nfm_into_packets_into_frames_and_the_tool(fmd, tmp_path):
    """Two AX.25 frames as 1200 baud AFSK, FM-modulated at 3 kHz deviation onto station 0 of a 240 kHz capture (station 1 is a bare
    carrier): the narrow-band bank in NFM mode at 12 kHz, its d_out as it stands through packets(bank, 12000), the soft decisions
    through one Ax25Decoder per row.  Bit for bit narrow_ref -> afsk_ref, call by call; both frames are delivered, and afsk_gpu over
    row 0's audio prints them.  (Deviation and rates chosen on the CPU with the two definitions: 3 kHz at 12 kHz gives an audio peak
    of about 8500.)"""
    import torch
    fs, D, T, R, Ta, S, K = 240000, 10, 40, 2, 31, 1, 2
    rate = fs // D // R
    h = st.lowpass(T, 12000 / fs)
    offs = np.array([[-40000, 55000]])
    incs = np.array([[fmd.phase_inc(int(o), fs) for o in offs[0]]], np.uint32)
    nb = fmd.NarrowBank(h, D, incs, fmd.narrow_taps(fs // D, Ta, -6000, 6000), R, mode=nr.FM, n_streams=S, block=64, squelch=0, gain=256,
                        device_id=0)
    ref = nr.NarrowRef(nb.taps, nb.decim, incs[0], nb.shift, nb.gr, nb.gi, nb.mode, nb.chan_decim, nb.chan_shift, nb.block, nb.squelch,
                       nb.gain, z=sr.z_corr)
    frames = [xr.ui_frame(("APRS", 0), ("N0CALL", 7), b"!4903.50N/07201.75W-packet one", digis=[("WIDE1", 1)]),
              xr.ui_frame(("APDR16", 0), ("DL1ABC", 0), b">second frame")]
    levels, level = [], 1
    for f in frames:
        lv = xr.nrzi(xr.frame_bits(f, flags=8, closing=2), level)
        level = lv[-1]
        levels += lv
    audio = np.concatenate([np.zeros(2000), xr.afsk_audio(levels, fs, amp=1.0)[0], np.zeros(4000)])
    n = audio.size // 4 * 4
    t = np.arange(n) / fs
    z = 60.0 * np.exp(1j * (2 * np.pi * offs[0, 0] * t + 2 * np.pi * 3000.0 * np.cumsum(audio[:n]) / fs)) + nr.carrier(n, fs, float(offs[0, 1]), 40.0)
    data_all = nr.to_u8(z, noise=2.0, seed=1)[None]

    pk = fmd.packets(nb, rate, device_id=0)
    assert (pk.n_rows, pk.width, pk.taps, pk.stride, pk.pre_shift, pk.rate) == (S * K, 1, 10, 2, 8, rate)
    aref = ar.AfskDemod(pk.table, pk.stride, pk.pre_shift, pk.out_shift, rows=S * K)
    decs = [fmd.Ax25Decoder(rate, pk.stride) for _ in range(S * K)]
    got_frames, rows, lo = [[] for _ in range(S * K)], [], 0
    for nbytes in (8 * 9001, 8 * 13000, data_all.shape[1] - 8 * 22001):
        data = np.ascontiguousarray(data_all[:, lo:lo + nbytes])
        lo += nbytes
        cap = nb.out_cap(nbytes) + 3
        d_audio = torch.full((S, K, cap), SENT, dtype=torch.int16, device="cuda")
        out_cap = pk.out_cap(cap) | 1
        d_soft = torch.full((S * K, out_cap), SENT, dtype=torch.int16, device="cuda")
        d_iq = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        m = nb.run_device(d_iq.data_ptr(), nbytes, d_audio.data_ptr(), cap)
        k = pk.run_device(d_audio.data_ptr(), m, cap, d_soft.data_ptr(), out_cap)            # the bank's out_cap is the in_cap
        pk.check()
        a = ref.feed(data[0]).reshape(S * K, m).astype(np.int16)
        exp = aref.push(a)
        got = d_soft.cpu().numpy()
        assert k == exp.shape[1] and np.array_equal(got[:, :k], exp) and (got[:, k:] == SENT).all()
        rows.append(a[0])
        for r in range(S * K):
            got_frames[r] += decs[r].push(got[r, :k])
    assert [f["data"] for f in got_frames[0]] == frames and got_frames[1] == []
    assert decs[0].info()["frames_ok"] == 2
    assert [fmd.ax25_text(f) for f in got_frames[0]] == ["N0CALL-7>APRS,WIDE1-1:!4903.50N/07201.75W-packet one", "DL1ABC>APDR16:>second frame"]
    # decode_rows: the same through the host entry, from the definition's audio
    res = fmd.decode_rows(fmd.packets(nb, rate, device_id=0), [np.stack([rows[i], rows[i]]) for i in range(3)])
    assert [[f["data"] for f in r["frames"]] for r in res] == [frames, frames] and res[0]["frames_ok"] == 2
    # the tool over row 0's audio
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "afsk_gpu")
    (tmp_path / "row0.s16").write_bytes(np.concatenate(rows).tobytes())
    p = subprocess.run([exe, "-r", str(rate), str(tmp_path / "row0.s16")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode().splitlines() == [fmd.ax25_text(f) for f in frames]
    i = decs[0].info()
    assert p.stderr.decode() == "frames_ok 2 bad_fcs %d aborts %d\n" % (i["bad_fcs"], i["aborts"])
