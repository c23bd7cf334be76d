"""The frame bank (include/fmd.h, fmd_hdlc_*) on the MI355X: after every call the counts, the frame records of all rows and the
counters bit for bit against the test-side definition (tests/hdlc_ref.py: an ax25_ref.Decoder per row), over the lane, wave and
workgroup edges, rates, cuts, the chunk edge, closings on chosen samples, the sign edge, unaligned rows, both frame capacities, lanes
that close together, noise, refusals, reset, streams, rows 2 GiB apart, and composed with the narrow-band bank, the packet
demodulator and the command-line tool."""
import os
import subprocess

import numpy as np
import pytest

import ax25_ref as xr
import big_cases as bc
import hdlc_ref as hr
import narrow_ref as nr
import stereo_ref as st
from big_gpu import Pitched

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, CAPACITY = -1, -5
CUTS = (1, 7, 1000, 333)


def _framer(fmd, num, den=1, cap=4, rows=1):
    return fmd.Ax25Framer(num, den, 1200, cap, n_rows=rows, device_id=0)


def _records(fmd, fr, rows):
    rows = np.ascontiguousarray(rows, np.uint32)
    rec = np.full((len(rows), fr.frame_cap), 0x5A, np.uint8).repeat(hr.FRAME_DTYPE.itemsize, axis=1).view(hr.FRAME_DTYPE)
    fmd.check(fmd.lib().fmd_hdlc_frames(fr._h, rows.ctypes.data, len(rows), rec.ctypes.data))
    return rec


def _same(fmd, fr, ref, what=None):
    """counts, the records of all rows (every byte) and the counters are the definition's after its last call"""
    counts, rec, every = ref.last
    got = _records(fmd, fr, np.arange(fr.n_rows))
    assert np.array_equal(fr.counts(), counts), (what, fr.counts().tolist(), counts.tolist())
    bad = [r for r in range(fr.n_rows) if got[r].tobytes() != rec[r].tobytes()]
    assert not bad, (what, bad)
    assert fr.info() == ref.info(), what
    assert fr.inputs() == ref.pos
    assert fr.frames(list(range(fr.n_rows))) == [e[:fr.frame_cap] for e in every]


def _device(soft, in_cap=None, off=0):
    """soft [rows, n] in a device buffer whose rows lie in_cap apart and start `off` samples behind a 16-byte boundary"""
    import torch
    rows, n = soft.shape
    in_cap = max(1, n) if in_cap is None else in_cap
    host = np.full(rows * in_cap + off + 16, 12321, np.int16)
    host[off:off + rows * in_cap].reshape(rows, in_cap)[:, :n] = soft
    d = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return d, d.data_ptr() + 2 * off, in_cap, host


def _feed(fmd, fr, ref, soft, cuts, batch=False, stream=None, off=0, odd=False):
    """soft [rows, n] through handle and definition in calls of `cuts` and then the rest, compared after every call; the frames"""
    lo, total = 0, 0
    for m in list(cuts) + [soft.shape[1]]:
        part = np.ascontiguousarray(soft[:, lo:lo + m])
        if part.shape[1] == 0 and m:
            break
        ref.run(part)
        if batch:
            fr.run_batch(part)
        else:
            d, ptr, in_cap, host = _device(part, (part.shape[1] + 2) | 1 if odd else None, off)
            fr.run_device(ptr, part.shape[1], in_cap, stream)
            fr.check()
            assert np.array_equal(d.cpu().numpy(), host)
        _same(fmd, fr, ref, (lo, m))
        lo += part.shape[1]
        total += int(ref.last[0].sum()) if part.shape[1] else 0
    assert lo == soft.shape[1]
    return total


def _body(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist())


def _row_bits(rng, r, frames=2, lo=15, hi=60):
    """flags and frames of row r's own: its own lengths, contents and gaps"""
    bits = xr.FLAG * (1 + r % 5)
    for k in range(frames):
        bits += xr.frame_bits(_body(rng, int(rng.integers(lo, hi))), flags=1 + (r + k) % 3, closing=1)
        bits += [1] * int(rng.integers(0, 12))               # idle or an abort between frames
    return bits + xr.FLAG * 2


def _signal(rng, rows, num, den=1, frames=2, n=None, amp=9000, lo=15, hi=60):
    """int16 [rows, n]: every row its own frames, held num / den samples per bit, from its own start sample"""
    per = []
    for r in range(rows):
        s = hr.levels_to_soft(xr.nrzi(_row_bits(rng, r, frames, lo, hi)), num, den, amp)
        per.append(np.concatenate([np.full(int(rng.integers(0, 40)), amp, np.int16), s]))
    n = max(len(s) for s in per) + 8 if n is None else n
    x = np.full((rows, n), amp, np.int16)
    for r, s in enumerate(per):
        x[r, :min(n, len(s))] = s[:n]
    return x


# ---- rows, rates, cuts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 63, 64, 65, 70, 257])
def test_every_row_count_cut_and_uncut_through_both_entries(fmd, rows):
    rng = np.random.default_rng(rows)
    x = _signal(rng, rows, 5, frames=1, lo=15, hi=25)
    x[rows // 2] = rng.integers(-32768, 32768, x.shape[1])   # a noise row between them
    fr = _framer(fmd, 6000, rows=rows)
    assert fr.kernel_name() == "fmd_hd::fmd_hdlc_kernel" and fr.inputs() == 0 and not fr.counts().any()
    total = _feed(fmd, fr, hr.Framer(6000, rows=rows), x, [])
    assert total >= rows - 1
    fr.reset()
    assert _feed(fmd, fr, hr.Framer(6000, rows=rows), x, CUTS, batch=rows % 2 == 0, odd=True) == total


U32 = (1 << 32) - 1
# (rate_num, rate_den, the samples a bit is held as a fraction); the last two at the top of the domain, where ph + step needs 33 bits
RATES = [(4800, 1, 4, 1), (6000, 1, 5, 1), (76800, 1, 64, 1), (11025, 2, 11025, 2400), (U32, 894784, U32, 1200 * 894784),
         (U32, 55925, U32, 1200 * 55925)]


@pytest.mark.parametrize("num,den,hold_num,hold_den", RATES, ids=["4", "5", "64", "11025-2", "wide-4", "wide-64"])
def test_rates_cut_and_uncut(fmd, num, den, hold_num, hold_den):
    rng = np.random.default_rng(num % 100000 + den)
    rows = 5
    slow = hold_num // hold_den >= 60
    frames = 1 if slow else 3
    x = _signal(rng, rows, hold_num, hold_den, frames=frames, lo=15, hi=18 if slow else 30)
    fr = _framer(fmd, num, den, rows=rows)
    total = _feed(fmd, fr, hr.Framer(num, den, rows=rows), x, [])
    assert total == frames * rows
    fr.reset()
    assert _feed(fmd, fr, hr.Framer(num, den, rows=rows), x, CUTS) == total


def test_calls_of_one_sample_and_the_chunk_edge(fmd):
    rng = np.random.default_rng(11)
    rows = 4
    x = _signal(rng, rows, 5, frames=2, lo=15, hi=20)
    fr = _framer(fmd, 6000, rows=rows)
    want = _feed(fmd, fr, hr.Framer(6000, rows=rows), x, [])
    for cuts in ([63, 64, 65, 1, 63, 1, 64, 128, 127, 129, 65], [1] * 150 + [64, 1, 64, 63, 1, 65]):
        fr.reset()
        assert _feed(fmd, fr, hr.Framer(6000, rows=rows), x, cuts, odd=True) == want == 2 * rows


# ---- where a frame closes ----------------------------------------------------------------------------------------------------------------
def _padded(rng, want_mod, frames=1):
    """one row whose first frame closes on a sample that is `want_mod` mod 64: (soft, the closing sample)"""
    bits = xr.FLAG * 3
    for _ in range(frames):
        bits += xr.stuffed_bits(xr.with_fcs(_body(rng, 20))) + xr.FLAG
    s = hr.levels_to_soft(xr.nrzi(bits + xr.FLAG), 5)
    for pad in range(0, 200):
        x = np.concatenate([np.full(pad, 9000, np.int16), s])
        f = xr.Decoder(6000).push(x)
        if len(f) == frames and f[0]["end_sample"] % 64 == want_mod:
            return x, [g["end_sample"] for g in f]
    raise AssertionError("no pad closes the frame there")


def test_frames_closing_on_a_chunks_last_and_first_sample_and_a_calls_last(fmd):
    rng = np.random.default_rng(12)
    last, e_last = _padded(rng, 63)
    first, e_first = _padded(rng, 0)
    both, e_both = _padded(rng, 63, frames=2)
    n = max(len(last), len(first), len(both))
    x = np.stack([np.concatenate([s, np.full(n - len(s), 9000, np.int16)]) for s in (last, first, both)])
    fr, ref = _framer(fmd, 6000, rows=3), hr.Framer(6000, rows=3)
    assert _feed(fmd, fr, ref, x, []) == 4
    got = fr.frames([0, 1, 2])
    assert got[0][0]["end_sample"] == e_last[0] and got[1][0]["end_sample"] == e_first[0] and e_last[0] % 64 == 63 and e_first[0] % 64 == 0
    # the call ends with the closing sample; the next begins behind it
    fr.reset()
    ref = hr.Framer(6000, rows=3)
    assert _feed(fmd, fr, ref, x, [e_last[0] + 1, 1]) == 4
    fr.reset()
    ref = hr.Framer(6000, rows=3)
    ref.run(x[:, :e_both[0] + 1])
    fr.run_batch(x[:, :e_both[0] + 1])
    _same(fmd, fr, ref)
    assert fr.counts()[2] == 1 and fr.info()[2]["in_frame"] == 1
    # a frame open across three calls: cut twice inside it
    fr.reset()
    ref = hr.Framer(6000, rows=3)
    a = e_both[0] + 100
    assert _feed(fmd, fr, ref, x, [a, 200, e_both[1] - a - 200 + 1]) == 4
    assert e_both[1] - e_both[0] > 700


def test_two_lanes_closing_on_the_same_and_on_adjacent_samples(fmd):
    rng = np.random.default_rng(13)

    def row(data, pad):
        s = hr.levels_to_soft(xr.nrzi(xr.frame_bits(data, flags=4, closing=2)), 5)
        return np.concatenate([np.full(pad, 9000, np.int16), s, np.full(n, s[-1], np.int16)])[:n]
    bodies = []
    while len(bodies) < 4:                                   # four frames of one length on the line: no stuffed bit in any
        d = _body(rng, 30)
        if len(xr.stuffed_bits(xr.with_fcs(d))) == 256:
            bodies.append(d)
    n = 5 * (256 + 48) + 40
    x = np.stack([row(bodies[0], 20), row(bodies[1], 20), row(bodies[2], 21), row(bodies[3], 20)])
    x = np.concatenate([x, np.full((60, n), -9000, np.int16)])      # (rows 0, 1, 3 close together, row 2 a sample later, row 63 too)
    x[63] = row(bodies[0], 21)
    fr, ref = _framer(fmd, 6000, rows=64), hr.Framer(6000, rows=64)
    assert _feed(fmd, fr, ref, x, []) == 5
    ends = [e[0]["end_sample"] for e in (ref.last[2][r] for r in (0, 1, 2, 3, 63))]
    assert ends[0] == ends[1] == ends[3] and ends[2] == ends[4] == ends[0] + 1
    assert [f[0]["data"] for f in fr.frames([0, 1, 2, 3, 63])] == [bodies[0], bodies[1], bodies[2], bodies[3], bodies[0]]


# ---- the values, the addresses, the capacities ------------------------------------------------------------------------------------------
def test_sign_edge_and_both_rails(fmd):
    """0 is mark and -1 is space (cur = v >= 0): a line that shows its levels as 0 / -1, as the rails, and as a mix."""
    rng = np.random.default_rng(14)
    rows = 6
    lv = _signal(rng, rows, 5, frames=2, lo=15, hi=40) > 0
    x = np.where(lv, 0, -1).astype(np.int16)
    x[1] = np.where(lv[1], 32767, -32768)
    x[2] = np.where(lv[2], rng.choice([0, 1, 32767], lv.shape[1]), rng.choice([-1, -2, -32768], lv.shape[1]))
    x[3] = 0                                                 # all mark: the idle line, seven 1s and no frame
    x[4] = -1
    fr, ref = _framer(fmd, 6000, rows=rows), hr.Framer(6000, rows=rows)
    assert _feed(fmd, fr, ref, x, [501]) == 2 * (rows - 2)
    assert [i["frames_ok"] for i in ref.info()] == [2, 2, 2, 0, 0, 2]


@pytest.mark.parametrize("off", [1, 3, 7])
def test_rows_at_odd_offsets_with_an_odd_in_cap(fmd, off):
    rng = np.random.default_rng(15 + off)
    rows = 9
    x = _signal(rng, rows, 5, frames=2, lo=15, hi=30)
    fr, ref = _framer(fmd, 6000, rows=rows), hr.Framer(6000, rows=rows)
    assert _feed(fmd, fr, ref, x, [257, 64, 1001], off=off, odd=True) == 2 * rows


@pytest.mark.parametrize("cap,frames", [(1, 2), (1, 17), (16, 2), (16, 17)])
def test_frame_cap_1_and_16_under_two_and_seventeen_frames_in_one_call(fmd, cap, frames):
    rng = np.random.default_rng(16)
    bits = xr.FLAG * 2
    datas = [_body(rng, 15) for _ in range(frames)]          # 17 bytes with the FCS
    for d in datas:
        bits += xr.stuffed_bits(xr.with_fcs(d)) + xr.FLAG    # one flag between two
    one = hr.levels_to_soft(xr.nrzi(bits + xr.FLAG), 5)
    x = np.stack([one, -one, np.full(one.shape, 9000, np.int16)])
    fr, ref = _framer(fmd, 6000, cap=cap, rows=3), hr.Framer(6000, frame_cap=cap, rows=3)
    assert _feed(fmd, fr, ref, x, []) == 2 * frames
    assert fr.counts().tolist() == [frames, frames, 0] and [i["frames_ok"] for i in fr.info()] == [frames, frames, 0]
    got = fr.frames([0])[0]
    assert [f["data"] for f in got] == datas[:cap] and fr.max_frames(x.shape[1]) >= frames


def test_a_noise_row_beside_a_frame_row(fmd):
    rng = np.random.default_rng(17)
    rows = 8
    x = _signal(rng, rows, 4, frames=6, lo=15, hi=30)
    n = x.shape[1]
    x[1::2] = np.repeat(rng.integers(0, 2, (rows // 2, n // 4 + 1)) * 2 - 1, 4, axis=1)[:, :n] * rng.integers(1, 30000, (rows // 2, n))
    x[7] = rng.integers(-32768, 32768, n)
    fr, ref = _framer(fmd, 4800, rows=rows), hr.Framer(4800, rows=rows)
    assert _feed(fmd, fr, ref, x, [700, 64]) == 6 * (rows // 2)
    info = ref.info()
    assert sum(i["bad_fcs"] for i in info[1::2]) > 0 and sum(i["aborts"] for i in info[1::2]) > 0


# ---- refusals and the handle's state ---------------------------------------------------------------------------------------------------
def test_refused_calls_and_calls_of_no_samples_leave_the_last_results(fmd):
    rng = np.random.default_rng(18)
    rows = 5
    x = _signal(rng, rows, 5, frames=2, lo=15, hi=30)
    half = x.shape[1] // 2
    fr, ref = _framer(fmd, 6000, rows=rows), hr.Framer(6000, rows=rows)
    _feed(fmd, fr, ref, x[:, :half], [])
    d, ptr, in_cap, host = _device(x[:, half:])
    m = x.shape[1] - half
    for args, status in (((ptr, m, m - 1), CAPACITY), ((ptr + 1, m, m), INVALID_ARG), ((0, m, m), INVALID_ARG)):
        with pytest.raises(fmd.FmdError) as e:
            fr.run_device(*args)
        assert e.value.status == status
        _same(fmd, fr, ref)
    assert fmd.lib().fmd_hdlc_run_batch(fr._h, x.ctypes.data, 5, 4) == CAPACITY
    _same(fmd, fr, ref)
    # a row index at or beyond n_rows: nothing is written
    sel = np.array([0, rows], np.uint32)
    rec = np.full((2, fr.frame_cap), 0x5A, np.uint8).repeat(528, axis=1)
    assert fmd.lib().fmd_hdlc_frames(fr._h, sel.ctypes.data, 2, rec.ctypes.data) == INVALID_ARG and (rec == 0x5A).all()
    # no samples: no launch, the last call's counts and frames stay
    before = fr.counts().copy()
    fr.run_device(ptr, 0, m)
    fr.run_batch(x[:, :0])
    ref.run(x[:, :0])
    _same(fmd, fr, ref)
    assert np.array_equal(fr.counts(), before)
    # and the refused samples are taken when handed over again
    fr.run_device(ptr, m, in_cap)
    fr.check()
    ref.run(x[:, half:])
    _same(fmd, fr, ref)
    assert sum(i["frames_ok"] for i in fr.info()) == 2 * rows


def test_a_selection_out_of_order_with_a_repeat_and_a_selection_of_no_rows(fmd):
    rng = np.random.default_rng(20)
    rows = 5
    x = _signal(rng, rows, 5, frames=1, lo=25, hi=40)        # (about 2000 soft decisions, a frame in every row)
    fr, ref = _framer(fmd, 6000, rows=rows), hr.Framer(6000, rows=rows)
    assert _feed(fmd, fr, ref, x, [], batch=True) == rows
    every = _records(fmd, fr, np.arange(rows))
    assert every[0].tobytes() != every[4].tobytes()
    # each listed row's records in the order listed, byte for byte the identity selection's
    got = _records(fmd, fr, [4, 0, 0])
    assert [g.tobytes() for g in got] == [every[r].tobytes() for r in (4, 0, 0)]
    assert fr.frames([4, 0, 0]) == [ref.last[2][r][:fr.frame_cap] for r in (4, 0, 0)]
    # no rows: null pointers pass, and nothing is written where there is a buffer
    assert fmd.lib().fmd_hdlc_frames(fr._h, None, 0, None) == 0
    rec = np.full(fr.frame_cap * hr.FRAME_DTYPE.itemsize, 0x5A, np.uint8)
    assert fmd.lib().fmd_hdlc_frames(fr._h, None, 0, rec.ctypes.data) == 0 and (rec == 0x5A).all()
    assert fr.frame_records([]) == [] and fr.frames([]) == []
    _same(fmd, fr, ref)


def test_reset_inside_a_frame_a_callers_stream_and_two_handles(fmd):
    import torch
    rng = np.random.default_rng(19)
    xa, xb = _signal(rng, 70, 5, frames=2, lo=15, hi=30), _signal(rng, 2, 11025, 2400, frames=2)
    a, b = _framer(fmd, 6000, rows=70), _framer(fmd, 11025, 2, cap=1, rows=2)
    ra, rb = hr.Framer(6000, rows=70), hr.Framer(11025, 2, frame_cap=1, rows=2)
    stream = torch.cuda.Stream()
    n = min(xa.shape[1], xb.shape[1])
    for lo, hi in ((0, 400), (400, 401), (401, n)):          # the two handles interleaved, a on the caller's stream, b on the default one
        _feed(fmd, a, ra, xa[:, lo:hi], [], stream=stream.cuda_stream)
        _feed(fmd, b, rb, xb[:, lo:hi], [])
    first = hr.Framer(6000, rows=70)
    first.run(xa[:, :400])
    assert max(i["in_frame"] for i in first.info()) == 1     # sample 400 lies inside frames
    a.run_batch(xa[:, :400])
    a.reset()
    assert a.inputs() == 0 and not a.counts().any() and a.info() == hr.Framer(6000, rows=70).info()
    assert _feed(fmd, a, hr.Framer(6000, rows=70), xa, []) == 2 * 70
    assert b.inputs() == n and b.info() == rb.info()


def test_rows_2_gib_apart(fmd):
    """Five rows 2^31 - 6 bytes apart in the input: rows 1, 2 and 4 start just below byte 2^31, 2^32 and 2^33, and the pitch is no
    multiple of 16 bytes.  Two calls; the wide buffer is allocated and never filled, only its windows hold data (decoy samples around
    the rows), and they are unchanged behind the calls."""
    rng = np.random.default_rng(20)
    rows = 5
    x = _signal(rng, rows, 5, frames=3, lo=15, hi=30)
    cut = x.shape[1] // 2
    ns = (cut, x.shape[1] - cut)
    geo = bc.Geo(rows, 2, (1 << 31) - 6, ns, (1, 2), 6)
    big = Pitched(geo, geo.size + bc.SLACK, "decoy", 20)
    fr, ref = _framer(fmd, 6000, rows=rows), hr.Framer(6000, rows=rows)
    try:
        lo = 0
        for n in ns:
            part = np.ascontiguousarray(x[:, lo:lo + n])
            for r in range(rows):
                big.put(r, part[r])
            import torch
            torch.cuda.synchronize()
            fr.run_device(big.ptr, n, geo.cap)
            fr.check()
            ref.run(part)
            _same(fmd, fr, ref, lo)
            big.check("the input after the call at %d" % lo)
            lo += n
        assert [i["frames_ok"] for i in fr.info()] == [3] * rows
    finally:
        big.release()
        fr.close()


# ---- composed --------------------------------------------------------------------------------------------------------------------------
def test_narrow_bank_nfm_into_packets_into_the_frame_bank_and_the_tool(fmd, tmp_path):
    """The two AX.25 frames of test_gpu_afsk.py's chain, FM-modulated onto station 0 of a 240 kHz capture: NarrowBank (NFM, 12 kHz) ->
    packets(bank) -> framed(demod), each taking the one before's device buffer as it stands.  Both payloads are delivered, row 1 (a
    bare carrier) has none; the frame bank equals the host decoders over the same soft decisions and the definition; decode_rows_gpu
    equals decode_rows over the same calls; afsk_gpu -G prints what afsk_gpu prints."""
    import torch
    fs, D, T, R, Ta, S, K = 240000, 10, 40, 2, 31, 1, 2
    rate = fs // D // R
    h = st.lowpass(T, 12000 / fs)
    offs = np.array([[-40000, 55000]])
    incs = np.array([[fmd.phase_inc(int(o), fs) for o in offs[0]]], np.uint32)
    nb = fmd.NarrowBank(h, D, incs, fmd.narrow_taps(fs // D, Ta, -6000, 6000), R, mode=nr.FM, n_streams=S, block=64, squelch=0, gain=256,
                        device_id=0)
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
    fb = fmd.framed(pk, device_id=0)
    assert (fb.n_rows, fb.rate_num, fb.rate_den, fb.baud, fb.frame_cap) == (S * K, rate, pk.stride, 1200, 4)
    ref = hr.Framer(rate, pk.stride, 1200, 4, rows=S * K)
    decs = [fmd.Ax25Decoder(rate, pk.stride) for _ in range(S * K)]
    got, host, audio_rows, lo = [[] for _ in range(S * K)], [[] for _ in range(S * K)], [], 0
    for nbytes in (8 * 9001, 8 * 13000, data_all.shape[1] - 8 * 22001):
        data = np.ascontiguousarray(data_all[:, lo:lo + nbytes])
        lo += nbytes
        cap = nb.out_cap(nbytes) + 3
        d_audio = torch.full((S, K, cap), -12345, dtype=torch.int16, device="cuda")
        out_cap = pk.out_cap(cap) | 1
        d_soft = torch.full((S * K, out_cap), -12345, dtype=torch.int16, device="cuda")
        d_iq = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        m = nb.run_device(d_iq.data_ptr(), nbytes, d_audio.data_ptr(), cap)
        k = pk.run_device(d_audio.data_ptr(), m, cap, d_soft.data_ptr(), out_cap)            # the bank's out_cap is the in_cap
        fb.run_device(d_soft.data_ptr(), k, out_cap)                                         # the demodulator's out_cap is the in_cap
        fb.check()
        soft = d_soft.cpu().numpy()
        assert (soft[:, k:] == -12345).all()
        ref.run(soft[:, :k])
        _same(fmd, fb, ref, lo)
        audio_rows.append(d_audio.cpu().numpy().reshape(S * K, cap)[:, :m])
        for r, fs_ in enumerate(fb.frames(list(range(S * K)))):
            got[r] += fs_
            host[r] += decs[r].push(soft[r, :k])
    assert [f["data"] for f in got[0]] == frames and got[1] == [] and got == host
    assert fb.info() == [d.info() for d in decs] and fb.info()[0]["frames_ok"] == 2
    # the same calls through both row decoders
    a = fmd.decode_rows(fmd.packets(nb, rate, device_id=0), audio_rows)
    b = fmd.decode_rows_gpu(fmd.packets(nb, rate, device_id=0), audio_rows)
    assert a == b and [f["data"] for f in b[0]["frames"]] == frames and b[0]["frames"] == got[0]
    # the tool over row 0's audio, with and without -G
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "afsk_gpu")
    (tmp_path / "row0.s16").write_bytes(np.concatenate([r[0] for r in audio_rows]).tobytes())
    p = subprocess.run([exe, "-r", str(rate), str(tmp_path / "row0.s16")], capture_output=True, timeout=300)
    g = subprocess.run([exe, "-r", str(rate), "-G", str(tmp_path / "row0.s16")], capture_output=True, timeout=300)
    assert p.returncode == 0 and g.returncode == 0, (p.stderr.decode(), g.stderr.decode())
    assert g.stdout == p.stdout and g.stderr == p.stderr
    assert g.stdout.decode().splitlines() == [fmd.ax25_text(f) for f in frames] and g.stderr.decode().startswith("frames_ok 2 ")
