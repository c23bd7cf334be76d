"""Tone squelch (include/fmd.h, fmd_tonesq_*) on the MI355X: every output and every status bit for bit against the test-side
definition (tests/tonesq_ref.py) at both widths, P in {64, 256, 4096} and F in {1, 2, 38, 64} with random tables, 1, 3, 33 and 70 rows
(a workgroup owns a tile of 32 rows: 33 is one full tile and a tile of one row, 70 two full tiles and a tile of six), unaligned rows
and odd capacities, call cuts around block ends, calls of one sample, one call over five block ends, full-scale values, the corners
of the decision and of the configuration, in place, refused calls, reset, a caller's stream, two handles, and composed with the
narrow-band bank, the AGC and the command-line tool.  Everything but the tool runs in this process."""
import os
import subprocess

import numpy as np
import pytest

import agc_ref as ar
import narrow_ref as nr
from rows_gpu import SENT, call as _call
import stereo_ref as st
import tonesq_ref as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = -5
ALL = (1 << 64) - 1


def _sq(fmd, tab, cfg, rows, width):
    cfg = tr.Cfg(*cfg)
    return fmd.ToneSquelch(tab, n_rows=rows, width=width, accept=cfg.accept, guard=cfg.guard, dom_shift=cfg.dom_shift,
                           min_power=cfg.min_power, confirm=cfg.confirm, hang=cfg.hang, ramp=cfg.ramp, device_id=0)


def _odd(n):
    """an odd capacity above n: at width 1 every second row then starts at a 2-byte but not a 4-byte boundary"""
    return n + 1 + n % 2


def _status_equal(sq, ref):
    tone, power, gate = sq.status()
    rt, rp, rg = ref.status()
    return tone.tolist() == rt and [int(p) for p in power] == rp and gate.tolist() == rg


def _feed(sq, ref, x, cuts, batch=False):
    """The stream x in pieces of `cuts` samples and then the rest, call by call against the definition: the outputs, the counters and
    every row's status.  Returns the outputs."""
    out, lo = [], 0
    for n in list(cuts) + [x.shape[1]]:
        hi = min(x.shape[1], lo + n)
        piece = x[:, lo:hi]
        exp = ref.push(piece)
        got = sq.run_batch(piece) if batch else _call(sq, piece, _odd(hi - lo))
        assert got.shape == exp.shape and np.array_equal(got, exp), (lo, hi)
        assert sq.counts() == (ref.N, ref.N) and _status_equal(sq, ref), (lo, hi)
        out.append(got)
        lo = hi
    return np.concatenate(out, axis=1)


def _table(rng, F, P):
    t = rng.integers(-1023, 1024, (F, P, 2)).astype(np.int16)
    t[0, :2] = [[1023, -1023], [-1023, 1023]]
    return t


def _audio(rng, rows, n, width):
    """Rows at different levels, full scale among them, with -32768 and a silent stretch."""
    x = rng.integers(-32768, 32768, (rows, n, width)).astype(np.int64)
    x = (x * rng.choice([1, 64, 4096, 32768], (rows, 1, 1))) >> 15
    x[:, n // 3] = -32768
    x[rows // 2, n // 2:n // 2 + n // 5] = 0
    return x.astype(np.int16)


def _loose(P, F, rng):
    """A configuration under which noise opens and closes the gate: any strongest tone is a hit, about half of the tones open."""
    return tr.Cfg(P, 0, 0, 1, int(rng.integers(0, 2)), min(P, 64), 1, int(rng.integers(1, 1 << 62)) | 1)


SHAPES = [(w, P, F) for w in (1, 2) for P in (64, 256, 4096) for F in (1, 2, 38, 64)]
ROWS = [1, 3, 33, 70]


@pytest.mark.parametrize("width,P,F", SHAPES, ids=["w%d-P%d-F%d" % s for s in SHAPES])
def test_definition_parity_cut_and_uncut(fmd, width, P, F):
    """Random table entries in [-1023, 1023].  The rows through the cuts 7 | 1000 | 333 | rest on device pointers (odd in_cap, odd
    out_cap), a tile-straddling subset of them in one call, one row through the host entry in the same cuts: all equal the
    definition over the whole stream, so the cuts equal one call."""
    rng = np.random.default_rng(1000 * P + 10 * F + width)
    rows = ROWS[((64, 256, 4096).index(P) + (1, 2, 38, 64).index(F) + width) % 4]
    tab, cfg = _table(rng, F, P), _loose(P, F, rng)
    n = max(1500, 4 * P) + P + int(rng.integers(1, P))
    x = _audio(rng, rows, n, width)
    whole = tr.tonesq_all(x, tab, cfg)
    sq = _sq(fmd, tab, cfg, rows, width)
    assert sq.kernel_name() == "fmd_tq::fmd_tonesq_kernel<%d>" % width and sq.status()[0].tolist() == [-1] * rows
    ref = tr.ToneSquelch(tab, cfg)
    assert np.array_equal(_feed(sq, ref, x, [7, 1000, 333]), whole)
    assert len({h for _, _, h in ref.hits}) > (1 if F > 2 else 0)
    sub = slice(rows // 2, rows)
    part = _sq(fmd, tab, cfg, rows - rows // 2, width)
    assert np.array_equal(_call(part, x[sub], _odd(n)), whole[sub])
    one = _sq(fmd, tab, cfg, 1, width)
    assert np.array_equal(_feed(one, tr.ToneSquelch(tab, cfg), x[-1:], [7, 1000, 333], batch=True), whole[-1:])
    if width == 1:                                           # [rows, n] in, [rows, n] out
        one.reset()
        assert np.array_equal(one.run_batch(x[-1:, :, 0]), whole[-1:, :, 0])


@pytest.mark.parametrize("rows", ROWS)
def test_every_row_count_with_the_ctcss_table(fmd, rows):
    """1, 3, 33 and 70 rows at both widths over the designed 38-tone table at P = 256: a partial last tile and more than one tile."""
    rng = np.random.default_rng(rows)
    tab = fmd.tone_table(12000, fmd.CTCSS_TONES, 256)
    for width in (1, 2):
        cfg = tr.Cfg(256, 1, 0, 1, 1, 16, 1000, ALL >> 27)
        x = _audio(rng, rows, 5 * 256 + 31, width)
        sq, ref = _sq(fmd, tab, cfg, rows, width), tr.ToneSquelch(tab, cfg)
        y = _feed(sq, ref, x, [300, 1])
        assert y.any() and not y[:, :256].any()


@pytest.mark.parametrize("width", [1, 2])
def test_calls_of_one_sample_and_around_a_block_end(fmd, width):
    """P = 64: 130 calls of one sample; then a first call ending one sample before a block's end, at it, and one behind it."""
    rng = np.random.default_rng(17 + width)
    P, F = 64, 3
    tab, cfg = _table(rng, F, P), tr.Cfg(P, 0, 0, 1, 0, 8, 1, 0b101)
    x = _audio(rng, 3, 9 * P + 5, width)
    whole = tr.tonesq_all(x, tab, cfg)
    sq, ref = _sq(fmd, tab, cfg, 3, width), tr.ToneSquelch(tab, cfg)
    assert np.array_equal(_feed(sq, ref, x, [1] * 130), whole)
    for k in (1, 2, 5):
        for n in (k * P - 1, k * P, k * P + 1):
            sq, ref = _sq(fmd, tab, cfg, 3, width), tr.ToneSquelch(tab, cfg)
            assert np.array_equal(_feed(sq, ref, x, [n]), whole), (k, n)


@pytest.mark.parametrize("width", [1, 2])
def test_one_call_over_five_block_ends_changes_the_gate_inside_the_call(fmd, width):
    """One tone row of all +1023, 35 rows: every second row carries a positive signal in blocks 0 and 1 and a zero-mean one behind
    them.  In ONE call of 5 P + 9 samples those rows come out closed, ramping up, open, ramping down and closed."""
    P, Q = 256, 32
    tab = np.zeros((1, P, 2), np.int16)
    tab[0, :, 0] = 1023
    cfg = tr.Cfg(P, 0, 0, 1, 0, Q, 1, 1)
    rng = np.random.default_rng(23 + width)
    n = 5 * P + 9
    x = np.zeros((35, n, width), np.int16)
    sig = rng.integers(1, 32768, (18, n, width)).astype(np.int16)
    sig[:, 2 * P:] = 0
    sig[:, 2 * P:, 0] = np.where(np.arange(n - 2 * P) % 2 == 0, 12345, -12345)      # the sums of a block cancel
    if width == 2:
        sig[:, 2 * P:, 1] = sig[:, 2 * P:, 0]
    x[0::2] = sig
    sq, ref = _sq(fmd, tab, cfg, 35, width), tr.ToneSquelch(tab, cfg)
    y = _feed(sq, ref, x, [])
    assert not y[:, :P].any() and np.array_equal(y[0::2, P + Q:3 * P], x[0::2, P + Q:3 * P]) and y[0, P + Q:3 * P].all()
    assert np.abs(y[0, 3 * P:3 * P + Q, 0].astype(int)).tolist() == sorted(np.abs(y[0, 3 * P:3 * P + Q, 0].astype(int)).tolist(), reverse=True)
    assert not y[:, 3 * P + Q:].any() and not y[1::2].any()
    assert sq.status()[0].tolist() == [-1] * 35 and ref.hits[0] == (0, 0, 0) and ref.hits[1] == (0, 1, tr.NONE)


def test_a_call_of_no_samples_changes_nothing(fmd):
    import torch
    rng = np.random.default_rng(29)
    tab, cfg = _table(rng, 2, 64), tr.Cfg(64, 0, 0, 1, 0, 1, 1, 3)
    x = _audio(rng, 3, 200, 1)
    sq, ref = _sq(fmd, tab, cfg, 3, 1), tr.ToneSquelch(tab, cfg)
    a = _call(sq, x[:, :100])
    d = torch.full((3, 9), SENT, dtype=torch.int16, device="cuda")
    assert sq.run_device(d.data_ptr(), 0, 9, d.data_ptr(), 9) == 0 and sq.counts() == (100, 100)
    sq.check()
    assert (d.cpu().numpy() == SENT).all() and sq.run_batch(np.zeros((3, 0, 1), np.int16)).shape == (3, 0, 1)
    b = _call(sq, x[:, 100:])
    assert np.array_equal(np.concatenate([a, b], axis=1), ref.push(x))
    assert _status_equal(sq, ref)


@pytest.mark.parametrize("width", [1, 2])
def test_full_scale_at_the_grouping_bound(fmd, width):
    """All samples -32768 against a table row of all +1023 and one of all -1023 over two whole blocks at P = 8192, F = 2: every run
    of 64 products sums to -+2 145 386 496, the i32 grouping bound, and |Re| = |Im| = 2^15 1023 8192, the top of their range."""
    P = 8192
    tab = np.empty((2, P, 2), np.int16)
    tab[0], tab[1] = 1023, -1023
    cfg = tr.Cfg(P, 0, 0, 1, 0, P, 1, 0b01)
    x = np.full((33, 2 * P, width), -32768, np.int16)
    sq, ref = _sq(fmd, tab, cfg, 33, width), tr.ToneSquelch(tab, cfg)
    y = _feed(sq, ref, x, [P - 1, 2])
    a = (32768 * 1023 * P) >> 14
    assert a << 14 == 32768 * 1023 * P > 1 << 37
    tone, power, gate = sq.status()
    # tone 0: Re = Im = -2^15 1023 P, floor-shifted; tone 1 the same with the other sign: a tie, which goes to tone 0
    assert tone.tolist() == [0] * 33 and int(power[0]) == 2 * a * a and gate.all()
    assert not y[:, :P].any() and y[0, 2 * P - 1, 0] == -32768 and y[0, P, 0] == (-32768 * ((256 * 1) >> 13)) >> 8


def test_decision_corners(fmd):
    rng = np.random.default_rng(31)
    P = 64
    x = rng.integers(-20000, 20001, (4, 6 * P, 1)).astype(np.int16)
    x[3] = 0                                                 # a silent row
    # two identical table rows: the tie goes to the smaller index
    tab = _table(rng, 3, P)
    tab[2] = tab[1]
    tab[0] = 0
    cfg = tr.Cfg(P, 0, 0, 1, 0, 1, 1, ALL)
    sq, ref = _sq(fmd, tab, cfg, 4, 1), tr.ToneSquelch(tab, cfg)
    _feed(sq, ref, x, [100])
    assert sq.status()[0].tolist() == [1, 1, 1, -1] and sq.status()[2].tolist() == [True, True, True, False]     # silence never opens
    # a guard so large that `rest` is 0: every block with W >= min_power is a hit, whatever dom_shift
    tab = _table(rng, 38, P)
    for guard, dom in ((63, 0), (37, 32), (0, 32), (0, 0)):
        cfg = tr.Cfg(P, guard, dom, 1, 0, 1, 1, ALL)
        sq, ref = _sq(fmd, tab, cfg, 4, 1), tr.ToneSquelch(tab, cfg)
        _feed(sq, ref, x, [65])
        hit = [h != tr.NONE for _, row, h in ref.hits if row < 3]
        assert all(hit) if guard >= 37 or dom == 0 else not any(hit), (guard, dom)
    # accept of zero never opens while status still reports the tone
    cfg = tr.Cfg(P, 63, 0, 1, 0, 1, 1, 0)
    sq, ref = _sq(fmd, tab, cfg, 4, 1), tr.ToneSquelch(tab, cfg)
    assert not _feed(sq, ref, x, []).any()
    tone, power, gate = sq.status()
    assert (tone[:3] >= 0).all() and (power[:3] > 0).all() and not gate.any()
    # accept with only bit 63 set at F = 64
    tab = np.zeros((64, P, 2), np.int16)
    tab[63, :, 0] = 1023
    tab[62, :, 0] = 1022
    cfg = tr.Cfg(P, 0, 0, 1, 0, 1, 1, 1 << 63)
    pos = np.abs(x[:3].astype(np.int64)).clip(1, 32767).astype(np.int16)
    sq, ref = _sq(fmd, tab, cfg, 3, 1), tr.ToneSquelch(tab, cfg)
    y = _feed(sq, ref, pos, [P])
    assert sq.status()[0].tolist() == [63] * 3 and np.array_equal(y[:, P:], pos[:, P:]) and not y[:, :P].any()
    cfg = tr.Cfg(P, 0, 0, 1, 0, 1, 1, (1 << 63) - 1)
    sq, ref = _sq(fmd, tab, cfg, 3, 1), tr.ToneSquelch(tab, cfg)
    assert not _feed(sq, ref, pos, []).any() and sq.status()[0].tolist() == [63] * 3


CORNERS = [(1, 0, 1), (1, 65535, 64), (3, 2, 1), (255, 0, 64), (2, 1, 8)]


@pytest.mark.parametrize("confirm,hang,ramp", CORNERS)
def test_the_configurations_corners(fmd, confirm, hang, ramp):
    """confirm 1 and 255, hang 0 and 65535, ramp 1 and P, at width 2 over 33 rows whose signal comes and goes block by block."""
    rng = np.random.default_rng(37 + confirm + hang + ramp)
    P, F = 64, 4
    tab = np.zeros((F, P, 2), np.int16)
    tab[1, :, 0] = 1000
    tab[2, :, 1] = -400
    cfg = tr.Cfg(P, 0, 1, confirm, hang, ramp, 100_000_000, 0b0110)   # (a block with the bias gives W of about 6e9, one without 1e6)
    n = 14 * P + 3
    x = _audio(rng, 33, n, 2)
    on = rng.random((33, 15)) < 0.6
    on[:, :4] = True
    bias = np.repeat(on, P, axis=1)[:, :n, None] * 20000
    x = ((x.astype(np.int64) >> 3) + bias).clip(-32768, 32767).astype(np.int16)
    sq, ref = _sq(fmd, tab, cfg, 33, 2), tr.ToneSquelch(tab, cfg)
    y = _feed(sq, ref, x, [5 * P + 1])
    assert y.any() == (confirm < 255)
    if hang == 65535:
        assert sq.status()[2].all()                          # once open, held


def test_in_place_and_refused_calls(fmd):
    import torch
    rng = np.random.default_rng(41)
    P, F = 256, 38
    tab, cfg = _table(rng, F, P), _loose(P, F, rng)
    x = _audio(rng, 35, 3 * P + 50, 2)
    whole = tr.tonesq_all(x, tab, cfg)
    sq = _sq(fmd, tab, cfg, 35, 2)
    first = _call(sq, x[:, :700])
    rest = x[:, 700:]
    n = rest.shape[1]
    d_in = torch.from_numpy(np.ascontiguousarray(rest)).cuda()
    d_out = torch.full((35, n + 8, 2), SENT, dtype=torch.int16, device="cuda")
    before, status = sq.counts(), sq.status()
    for n_in, in_cap, out_cap in ((n, n - 1, n + 8), (n, n, n - 1), (n, n, 0)):        # n_in > in_cap; out_cap below n_in
        with pytest.raises(fmd.FmdError) as e:
            sq.run_device(d_in.data_ptr(), n_in, in_cap, d_out.data_ptr(), out_cap)
        assert e.value.status == CAPACITY and sq.counts() == before
    with pytest.raises(fmd.FmdError) as e:                  # a width-2 row at a 2-byte offset
        sq.run_device(d_in.data_ptr() + 2, n - 1, n - 1, d_out.data_ptr(), n + 8)
    assert e.value.status == -1 and sq.counts() == before
    sq.check()
    assert all(np.array_equal(a, b) for a, b in zip(sq.status(), status))
    assert (d_out.cpu().numpy() == SENT).all() and np.array_equal(d_in.cpu().numpy(), rest)
    # in place: d_out == d_in with out_cap == in_cap; the next call equals the uncut one
    assert sq.run_device(d_in.data_ptr(), n, n, d_in.data_ptr(), n) == n
    sq.check()
    assert np.array_equal(np.concatenate([first, d_in.cpu().numpy()], axis=1), whole)


def test_reset_mid_block_a_callers_stream_and_two_handles(fmd):
    import torch
    rng = np.random.default_rng(43)
    ta, tb = _table(rng, 38, 256), _table(rng, 2, 64)
    ca, cb = _loose(256, 38, rng), _loose(64, 2, rng)
    xa, xb = _audio(rng, 7, 2048, 2), _audio(rng, 2, 2048, 1)
    a, b = _sq(fmd, ta, ca, 7, 2), _sq(fmd, tb, cb, 2, 1)
    ra, rb = tr.ToneSquelch(ta, ca), tr.ToneSquelch(tb, cb)
    stream = torch.cuda.Stream()
    first = None
    for lo, hi in ((0, 600), (600, 601), (601, 2048)):      # the two handles interleaved, a on the caller's stream, b on the default one
        ya = _call(a, xa[:, lo:hi], stream=stream.cuda_stream)
        yb = _call(b, xb[:, lo:hi], _odd(hi - lo))
        assert np.array_equal(ya, ra.push(xa[:, lo:hi])) and np.array_equal(yb, rb.push(xb[:, lo:hi]))
        assert _status_equal(a, ra) and _status_equal(b, rb)
        first = ya if first is None else first
    _call(a, xa[:, :100])                                    # 2148 samples: inside a block, sums carried
    a.reset()
    assert a.counts() == (0, 0) and a.status()[0].tolist() == [-1] * 7 and not a.status()[1].any() and not a.status()[2].any()
    assert np.array_equal(_call(a, xa[:, :600]), first)      # reset reproduces the first call
    ra.reset()
    ra.push(xa[:, :600])
    assert np.array_equal(_call(a, xa[:, 600:]), ra.push(xa[:, 600:])) and _status_equal(a, ra)
    assert b.counts() == (2048, 2048)


def test_narrow_bank_nfm_into_tone_squelch_into_agc_on_device_buffers(fmd):
    """The narrow-band bank in NFM mode on synthetic IQ whose first station carries a 100 Hz sub-tone: its d_out, as it stands and
    with its out_cap as in_cap, through tone_squelched(bank) and on through an Agc equals the three definitions composed, call by
    call; the gate of the station with the tone opens."""
    import torch
    rng = np.random.default_rng(47)
    fs, D, T, R, Ta, S, K, P = 2400000, 10, 64, 5, 127, 2, 3, 256
    rate = fs // D // R
    h = st.lowpass(T, 100000 / fs)
    offs = rng.integers(-900000, 900000, (S, K))
    incs = np.array([[fmd.phase_inc(int(o), fs) for o in offs[s]] for s in range(S)], np.uint32)
    g = fmd.narrow_taps(fs // D, Ta, -6000, 6000)
    nb = fmd.NarrowBank(h, D, incs, g, R, mode=nr.FM, n_streams=S, block=64, squelch=0, gain=256, device_id=0)
    refs = [nr.NarrowRef(nb.taps, nb.decim, incs[s], nb.shift, nb.gr, nb.gi, nb.mode, nb.chan_decim, nb.chan_shift, nb.block, nb.squelch,
                         nb.gain) for s in range(S)]
    tones = (100.0, 250.3)
    sq = fmd.tone_squelched(nb, rate, accept=(100.0,), tones=tones, block=P, guard=1, dom_shift=1, min_power=200, confirm=1, hang=1,
                            ramp=32, device_id=0)
    assert (sq.n_rows, sq.width, sq.accept) == (S * K, 1, 1)
    sref = tr.ToneSquelch(fmd.tone_table(rate, tones, P), tr.Cfg(P, 1, 1, 1, 1, 32, 200, 1))
    ag = fmd.leveled(nb, target=10000, block=64, hang=2, decay=64, gain_max=262144, device_id=0)
    aref = ar.Agc(ar.Cfg(64, 10000, 262144, 2, 64))
    lens = (8 * 2403, 8 * 1001, 8 * 9000)
    total = sum(lens) // 2
    z = np.zeros((S, total), np.complex128)
    z[0] = nr.nfm(total, fs, float(offs[0, 0]), 60.0, 100.0, 500.0)
    z[1] = nr.carrier(total, fs, float(offs[1, 1]), 60.0)
    data_all = np.stack([nr.to_u8(z[s], noise=2.0, seed=s) for s in range(S)])
    lo, opened = 0, np.zeros(S * K, bool)
    for n in lens:
        data = np.ascontiguousarray(data_all[:, lo:lo + n])
        lo += n
        cap = nb.out_cap(n) + 3
        d_audio = torch.full((S, K, cap), SENT, dtype=torch.int16, device="cuda")
        sq_cap = cap | 1
        d_sq = torch.full((S * K, sq_cap), SENT, dtype=torch.int16, device="cuda")
        out_cap = ag.out_cap(sq_cap) | 1
        d_out = torch.full((S * K, out_cap), SENT, dtype=torch.int16, device="cuda")
        d_iq = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        m = nb.run_device(d_iq.data_ptr(), n, d_audio.data_ptr(), cap)
        k = sq.run_device(d_audio.data_ptr(), m, cap, d_sq.data_ptr(), sq_cap)            # the bank's out_cap is the in_cap
        n_out = ag.run_device(d_sq.data_ptr(), k, sq_cap, d_out.data_ptr(), out_cap)
        ag.check()
        audio = np.stack([refs[s].feed(data[s]) for s in range(S)]).reshape(S * K, m, 1).astype(np.int16)
        gated = sref.push(audio)
        exp = aref.push(gated)
        got_sq = d_sq.cpu().numpy()
        assert k == m and np.array_equal(got_sq[:, :k], gated[:, :, 0]) and (got_sq[:, k:] == SENT).all()
        got = d_out.cpu().numpy()
        assert n_out == exp.shape[1] and np.array_equal(got[:, :n_out], exp[:, :, 0]) and (got[:, n_out:] == SENT).all()
        assert _status_equal(sq, sref)
        opened |= sq.status()[2]
    assert opened[0] and not opened.all() and sq.status()[0][0] == 0


@pytest.mark.parametrize("width", [1, 2])
def test_the_tool_gates_a_file_like_the_handle(fmd, width, tmp_path):
    """tonesq_gpu over a file of more than two reads equals the handle over the same samples (and so the definition), and reports
    every change of the selected tone or the gate on stderr as `block tone_hz power open`."""
    rng = np.random.default_rng(53 + width)
    rate, P = 12000, 4096
    n = 2 * 65536 + 4 * P + 77
    t = np.arange(n)
    x = rng.normal(0, 200, (n, width))
    x[5 * P:18 * P] += 1500 * np.cos(2 * np.pi * 123.0 * t[5 * P:18 * P] / rate)[:, None]
    x[24 * P:] += 1500 * np.cos(2 * np.pi * 203.5 * t[24 * P:] / rate)[:, None]
    x = np.rint(x).astype(np.int16)[None]
    tones = fmd.CTCSS_TONES
    accept = (1 << tones.index(123.0)) | (1 << tones.index(67.0))
    cfg = tr.Cfg(P, 1, 3, 2, 2, 64, 20_000_000, accept)
    ref = tr.ToneSquelch(fmd.tone_table(rate, tones, P), cfg)
    exp = ref.push(x)
    sq = _sq(fmd, fmd.tone_table(rate, tones, P), cfg, 1, width)
    assert np.array_equal(_call(sq, x), exp) and exp[0, 8 * P:17 * P].any() and not exp[0, 27 * P:].any()
    lines, last = [], (-1, False)
    per_block = {b: h for b, _, h in ref.hits}
    chk = tr.ToneSquelch(fmd.tone_table(rate, tones, P), cfg)
    for b in range(n // P):
        chk.push(x[:, b * P:(b + 1) * P])
        tone, power, gate = chk.status()
        if (tone[0], gate[0]) != last:
            lines.append("%d %s %d %d" % (b, "%.1f" % tones[tone[0]] if tone[0] >= 0 else "-", power[0], gate[0]))
        last = (tone[0], gate[0])
    assert len(lines) >= 3 and per_block[10] == tones.index(123.0)
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "tonesq_gpu")
    args = [exe, "-r", str(rate), "-c", str(width), "-b", str(P), "-a", "123.0,67.0"]
    (tmp_path / "in.s16").write_bytes(x.tobytes())
    p = subprocess.run(args + [str(tmp_path / "in.s16"), str(tmp_path / "out.s16")], capture_output=True, timeout=300)
    assert (p.returncode, p.stdout) == (0, b""), p.stderr.decode()
    assert (tmp_path / "out.s16").read_bytes() == exp.tobytes() and p.stderr.decode().splitlines() == lines
    p = subprocess.run(args, input=x[:, :3000].tobytes(), capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stdout == exp[:, :3000].tobytes()
