"""Code squelch (include/fmd.h, fmd_dcs_*) on the MI355X: every output and every status bit for bit against the test-side definition
(tests/dcs_ref.py) at both widths, B in {1, 8, 64}, T in {1, 2, 33, 64}, F in {1, 2, 65, 128}, P in {64, 192, 4160}, tap[22] in {0, 22,
511} with repeated offsets, tol in {0, 3, 23}, random lp and words, 1, 3, 33 and 70 rows (a workgroup owns a tile of 16 rows), odd
capacities, call cuts around box and block ends, calls of one sample, one call over five block ends, both rails of soft, the corners of
the decision and of the configuration, in place, refused calls, reset, a caller's stream, two handles, and composed with the
narrow-band bank, the AGC and the command-line tool.  Everything but the tool runs in this process."""
import os
import subprocess

import numpy as np
import pytest

import agc_ref as ar
import dcs_ref as dr
import narrow_ref as nr
from rows_gpu import SENT, call as _call
import stereo_ref as st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = -5
ALL = (1 << 128) - 1


def _sq(fmd, words, cfg, rows, width):
    cfg = dr.Cfg(*cfg)
    return fmd.CodeSquelch(words, cfg.block, cfg.box, cfg.lp, cfg.lshift, cfg.tap, n_rows=rows, width=width, accept=cfg.accept,
                           tol=cfg.tol, min_hits=cfg.min_hits, confirm=cfg.confirm, hang=cfg.hang, ramp=cfg.ramp, device_id=0)


def _odd(n):
    """an odd capacity above n: at width 1 every second row then starts at a 2-byte but not a 4-byte boundary"""
    return n + 1 + n % 2


def _status_equal(sq, ref):
    code, hits, gate = sq.status()
    rc, rh, rg = ref.status()
    return code.tolist() == rc and [int(h) for h in hits] == rh and gate.tolist() == rg


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


def _audio(rng, rows, n, width):
    """Rows at different levels, full scale among them, with -32768 and a silent stretch."""
    x = rng.integers(-32768, 32768, (rows, n, width)).astype(np.int64)
    x = (x * rng.choice([1, 64, 4096, 32768], (rows, 1, 1))) >> 15
    x[:, n // 3] = -32768
    x[rows // 2, n // 2:n // 2 + n // 5] = 0
    return x.astype(np.int16)


def _taps(rng, last):
    """23 non-decreasing offsets from 0 to `last`, with repeats"""
    if last == 0:
        return [0] * 23
    t = np.sort(rng.integers(0, last + 1, 21)).tolist()
    return [0] + t[:10] + [t[10]] + t[10:20] + [last]


def _lp(rng, T):
    lp = rng.integers(-1023, 1024, T).tolist()
    lp[0], lp[-1] = (1023, -1023) if T > 1 else (lp[0], 1023)
    return lp


def _words(rng, F):
    w = rng.integers(0, 1 << 23, F).astype(np.uint32)
    if F > 1:
        w[-1] = w[0]                                         # a repeated word: the first of the two is the match
    return w


def _lshift(lp, B):
    """a shift that leaves soft a few thousand on full-scale noise boxed by B"""
    return max(0, int(np.abs(np.array(lp)).sum()).bit_length() - 2 - (B.bit_length() - 1) // 2)


def _loose(rng, P, B, T, F, tol, last):
    """A configuration under which noise opens and closes the gate: a block is a hit from its first matching k on (from a quarter
    of its k at tol 23, where every k matches), about half of the words open."""
    lp = _lp(rng, T)
    min_hits = max(1, P // B // 4) if tol == 23 else 1
    return dr.Cfg(P, B, lp, _lshift(lp, B), _taps(rng, last), tol, min_hits, 1, int(rng.integers(0, 2)), min(64, P),
                  int(rng.integers(1, 1 << 62)) | (int(rng.integers(0, 1 << 62)) << 64) | 1)


BS, TS, FS, PS, TOLS, LASTS, ROWS = (1, 8, 64), (1, 2, 33, 64), (1, 2, 65, 128), (64, 192, 4160), (0, 3, 23), (0, 22, 511), (1, 3, 33, 70)
SHAPES = [(w, B, T, F) for w in (1, 2) for B in BS for T in TS for F in FS]


@pytest.mark.parametrize("width,B,T,F", SHAPES, ids=["w%d-B%d-T%d-F%d" % s for s in SHAPES])
def test_definition_parity_cut_and_uncut(fmd, width, B, T, F):
    """Random lp and words.  P, tol, tap[22] and the row count go round their values with the case's index, so that every value of
    each meets every value of B, T and F at one width or the other.  The rows through the cuts 7 | 1000 | 333 | rest on device
    pointers (odd in_cap, odd out_cap), a tile-straddling subset of them in one call, one row through the host entry in the same
    cuts: all equal the definition over the whole stream, so the cuts equal one call."""
    i = BS.index(B) * 16 + TS.index(T) * 4 + FS.index(F) + 5 * (width - 1)
    P, tol, last, rows = PS[i % 3], TOLS[(i // 3 + i) % 3], LASTS[(i // 9 + i) % 3], ROWS[(i + i // 4) % 4]
    rng = np.random.default_rng(100000 * B + 1000 * T + 10 * F + width)
    words, cfg = _words(rng, F), _loose(rng, P, B, T, F, tol, last)
    n = max(1500, 2 * P) + P + int(rng.integers(1, P))
    x = _audio(rng, rows, n, width)
    whole = dr.dcs_all(x, words, cfg)
    sq = _sq(fmd, words, cfg, rows, width)
    assert sq.kernel_name() == "fmd_dc::fmd_dcs_kernel<%d>" % width and sq.status()[0].tolist() == [-1] * rows
    ref = dr.CodeSquelch(words, cfg)
    assert np.array_equal(_feed(sq, ref, x, [7, 1000, 333]), whole)
    if tol == 23:
        assert any(h[2] != dr.NONE for h in ref.hits)
    sub = slice(rows // 2, rows)
    part = _sq(fmd, words, cfg, rows - rows // 2, width)
    assert np.array_equal(_call(part, x[sub], _odd(n)), whole[sub])
    one = _sq(fmd, words, cfg, 1, width)
    assert np.array_equal(_feed(one, dr.CodeSquelch(words, cfg), x[-1:], [7, 1000, 333], batch=True), whole[-1:])
    if width == 1:                                           # [rows, n] in, [rows, n] out
        one.reset()
        assert np.array_equal(one.run_batch(x[-1:, :, 0]), whole[-1:, :, 0])


def _tight(fmd, rate=12000, **kw):
    accept = kw.pop("accept", (1 << 104) - 1)
    d = fmd.dcs_design(rate)._replace(**kw)
    return dr.Cfg(d.block, d.box, d.lp, d.lshift, d.tap, d.tol, d.min_hits, d.confirm, d.hang, d.ramp, accept)


def _coded(fmd, rng, rate, n, codes, on=None, amp=1500.0):
    """Rows of noise of 200 rms, row r with the code codes[r] (None: no code) NRZ at amplitude `amp` while `on`[r] (a bool per
    sample; None: always)."""
    x = rng.normal(0.0, 200.0, (len(codes), n))
    for r, code in enumerate(codes):
        if code is None:
            continue
        c = fmd.dcs_codeword(code)
        bit = np.floor(np.arange(n) * 134.4 / rate + rng.uniform(0, 23)).astype(np.int64) % 23
        s = amp * (2.0 * ((c >> bit) & 1) - 1.0)
        x[r] += s if on is None else s * on[r]
    return np.rint(x).astype(np.int16)[:, :, None]


@pytest.mark.parametrize("rows", ROWS)
def test_every_row_count_with_the_designed_detector(fmd, rows):
    """1, 3, 33 and 70 rows at both widths over dcs_design(12000) and the 104 words: a partial last tile and more than one tile;
    every second row carries a code and opens."""
    rng = np.random.default_rng(rows)
    codes = fmd.DCS_CODES
    words = [fmd.dcs_word(c) for c in codes]
    cfg = _tight(fmd)
    for width in (1, 2):
        sent = [codes[(7 * r) % 104] if r % 2 == 0 else None for r in range(rows)]
        x = np.repeat(_coded(fmd, rng, 12000, 3 * cfg.block + 31, sent), width, axis=2)
        sq, ref = _sq(fmd, words, cfg, rows, width), dr.CodeSquelch(words, cfg)
        y = _feed(sq, ref, x, [300, 1])
        assert y[0::2].any() and not y[:, :cfg.block].any() and not y[1::2].any()
        assert sq.status()[0].tolist() == [(7 * r) % 104 if r % 2 == 0 else -1 for r in range(rows)]


@pytest.mark.parametrize("width", [1, 2])
def test_calls_of_one_sample_and_around_box_and_block_ends(fmd, width):
    """P = 64, B = 8: 130 calls of one sample; then a first call ending one sample before, at and behind a box end and a block end."""
    rng = np.random.default_rng(17 + width)
    P, B, F = 64, 8, 3
    words = _words(rng, F)
    cfg = _loose(rng, P, B, 5, F, 23, 22)._replace(min_hits=1, accept=0b101)
    x = _audio(rng, 3, 9 * P + 5, width)
    whole = dr.dcs_all(x, words, cfg)
    sq, ref = _sq(fmd, words, cfg, 3, width), dr.CodeSquelch(words, cfg)
    assert np.array_equal(_feed(sq, ref, x, [1] * 130), whole)
    for end in (B, 3 * B, P, 2 * P, 5 * P, 5 * P + 2 * B):
        for n in (end - 1, end, end + 1):
            sq, ref = _sq(fmd, words, cfg, 3, width), dr.CodeSquelch(words, cfg)
            assert np.array_equal(_feed(sq, ref, x, [n]), whole), n


@pytest.mark.parametrize("width", [1, 2])
def test_one_call_over_five_block_ends_changes_the_gate_inside_the_call(fmd, width):
    """dcs_design(12000) with a ramp of 32 and min_hits 4, 35 rows: every second row carries a code from the start to 2400 samples
    before the end of block 1 (a word looks back 246 decimated samples of 8, so no word of block 2 lies in the code) and noise alone
    behind that.  In ONE call of 5 P + 9 samples those rows come out closed, ramping up, open, held (hang 1), ramping down and closed."""
    rng = np.random.default_rng(23 + width)
    codes = fmd.DCS_CODES
    words = [fmd.dcs_word(c) for c in codes]
    cfg = _tight(fmd, ramp=32, min_hits=4)
    P, Q = cfg.block, 32
    n = 5 * P + 9
    on = np.zeros((35, n))
    on[:, :2 * P - 2400] = 1
    x = np.repeat(_coded(fmd, rng, 12000, n, [codes[r] if r % 2 == 0 else None for r in range(35)], on), width, axis=2)
    sq, ref = _sq(fmd, words, cfg, 35, width), dr.CodeSquelch(words, cfg)
    y = _feed(sq, ref, x, [])
    hit = {(b, row): h for b, row, h, _, _ in ref.hits}
    assert [hit[(b, 0)] for b in range(5)] == [0, 0, dr.NONE, dr.NONE, dr.NONE] and hit[(0, 1)] == dr.NONE
    # block 1 ramps up, 2 and 3 are open (the decision of block 2 is held one block), 4 ramps down
    assert not y[:, :P].any() and np.array_equal(y[0::2, P + Q:4 * P], x[0::2, P + Q:4 * P]) and not y[:, 4 * P + Q:].any()
    assert not y[1::2].any() and sq.status()[0].tolist() == [-1] * 35


def test_a_call_of_no_samples_changes_nothing(fmd):
    import torch
    rng = np.random.default_rng(29)
    words = _words(rng, 2)
    cfg = _loose(rng, 64, 8, 3, 2, 23, 5)._replace(min_hits=1, accept=3)
    x = _audio(rng, 3, 200, 1)
    sq, ref = _sq(fmd, words, cfg, 3, 1), dr.CodeSquelch(words, cfg)
    a = _call(sq, x[:, :100])
    d = torch.full((3, 9), SENT, dtype=torch.int16, device="cuda")
    assert sq.run_device(d.data_ptr(), 0, 9, d.data_ptr(), 9) == 0 and sq.counts() == (100, 100)
    sq.check()
    assert (d.cpu().numpy() == SENT).all() and sq.run_batch(np.zeros((3, 0, 1), np.int16)).shape == (3, 0, 1)
    b = _call(sq, x[:, 100:])
    assert np.array_equal(np.concatenate([a, b], axis=1), ref.push(x))
    assert _status_equal(sq, ref)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("lshift,sign", [(0, 1), (0, -1), (31, 1), (31, -1)])
def test_both_rails_of_soft(fmd, width, lshift, sign):
    """All samples -32768 against lp of all +1023 or all -1023 at T = 64: the sum is -+64 * 32768 * 1023, the i32 bound, so soft is
    -32768 or +32767 at lshift 0 and -1 or 0 at lshift 31.  A constant soft slices to the word 0, which word 1 of the table is."""
    P, B = 256, 1
    cfg = dr.Cfg(P, B, [sign * 1023] * 64, lshift, list(range(0, 44, 2)) + [44], 0, P - 100, 1, 0, P, 0b10)
    words = [0x7FFFFF, 0, 0]
    x = np.full((17, 2 * P + 3, width), -32768, np.int16)
    soft = dr.dcs_row(x[0], words, cfg)[2]
    assert soft[100] == {(0, 1): -32768, (0, -1): 32767, (31, 1): -1, (31, -1): 0}[(lshift, sign)]
    sq, ref = _sq(fmd, words, cfg, 17, width), dr.CodeSquelch(words, cfg)
    y = _feed(sq, ref, x, [P - 1, 2])
    code, hits, gate = sq.status()
    assert code.tolist() == [1] * 17 and gate.all() and int(hits[0]) == P
    assert not y[:, :P].any() and y[0, 2 * P - 1, 0] == -32768 and y[0, P, 0] == (-32768 * ((256 * 1) // P)) >> 8


def test_decision_corners(fmd):
    rng = np.random.default_rng(31)
    codes = fmd.DCS_CODES
    P, rate = 4160, 12000
    x = _coded(fmd, rng, rate, 3 * P, [codes[0], codes[103], codes[50], None])
    # accept of zero never opens while status still reports the code
    words = [fmd.dcs_word(c) for c in codes]
    cfg = _tight(fmd, accept=0)
    sq, ref = _sq(fmd, words, cfg, 4, 1), dr.CodeSquelch(words, cfg)
    assert not _feed(sq, ref, x, [100]).any()
    code, hits, gate = sq.status()
    assert code.tolist() == [0, 103, 50, -1] and (hits[:3] >= 8).all() and not gate.any()
    # accept of bit 0 alone, and of bit 127 alone at F = 128 (the 104 words, then 23 zeros, then code 754 once more as word 127:
    # the first of two equal words is the match, so word 127 is one that only its own entry can reach -- the inverse of 023)
    for accept, opens in ((1, [True, False, False, False]), (1 << 127, [False, False, False, True])):
        w128 = words + [0] * 23 + [fmd.dcs_word(codes[0], True)]
        xi = _coded(fmd, rng, rate, 3 * P, [codes[0], codes[103], codes[50], codes[0]])
        xi[3] = -xi[3]                                       # the other polarity
        cfg = _tight(fmd, accept=accept)
        sq, ref = _sq(fmd, w128, cfg, 4, 1), dr.CodeSquelch(w128, cfg)
        _feed(sq, ref, xi, [P])
        assert sq.status()[2].tolist() == opens, accept
    # hits == min_hits - 1 and hits == min_hits: the measured count of a block decides both ways
    cfg = _tight(fmd)
    ref = dr.CodeSquelch(words, cfg)
    ref.push(x[:1])
    n1 = [h[4] for h in ref.hits][1]
    for min_hits, hit in ((n1, 0), (n1 + 1, dr.NONE)):
        cfg = _tight(fmd, min_hits=min_hits)
        sq, ref = _sq(fmd, words, cfg, 1, 1), dr.CodeSquelch(words, cfg)
        _feed(sq, ref, x[:1, :2 * P], [])
        assert ref.hits[1][2] == hit and int(sq.status()[1][0]) == n1
    # a tie inside the match: of two equal words the first takes every hit
    wt = [words[3], words[3], words[9]]
    cfg = _tight(fmd, accept=0b010)
    xt = _coded(fmd, rng, rate, 3 * P, [codes[3], codes[9]])
    sq, ref = _sq(fmd, wt, cfg, 2, 1), dr.CodeSquelch(wt, cfg)
    assert not _feed(sq, ref, xt, []).any() and sq.status()[0].tolist() == [0, 2]
    # a tie between two counters: with tap = 0 ... 0, 1 a sample above the one before it slices to 0x3FFFFF and one below it to
    # 0x400000; 10, 20, 10, 20, ... gives block 1 (P = 64, B = 1) 32 hits on each, and the first of the two indices is f*,
    # whichever word stands there; min_hits 32 is met exactly, 33 is missed by one
    up, down = 0x3FFFFF, 0x400000
    c = np.tile(np.array([10, 20], np.int16), 64)[None, :, None]
    for wt, min_hits, code in (([5, up, down], 32, 1), ([5, down, up], 32, 1), ([5, up, down], 33, -1)):
        cfg = dr.Cfg(64, 1, [1], 0, [0] * 22 + [1], 0, min_hits, 1, 0, 1, 0b110)
        sq, ref = _sq(fmd, wt, cfg, 1, 1), dr.CodeSquelch(wt, cfg)
        _feed(sq, ref, c, [64])
        assert ref.hits[1][3:] == (1, 32) and sq.status()[0].tolist() == [code] and sq.status()[1].tolist() == [32]


CORNERS = [(1, 0, 1), (1, 65535, 64), (3, 2, 1), (255, 0, 64), (2, 1, 8)]


@pytest.mark.parametrize("confirm,hang,ramp", CORNERS)
def test_the_configurations_corners(fmd, confirm, hang, ramp):
    """confirm 1 and 255, hang 0 and 65535, ramp 1 and 64, at width 2 over 33 rows whose matching input comes and goes block by
    block: P = 64, B = 1, a constant block slices to the word 0 (a hit on word 1), a block of noise to nothing in the table."""
    rng = np.random.default_rng(37 + confirm + hang + ramp)
    P = 64
    cfg = dr.Cfg(P, 1, [1], 0, list(range(23)), 0, P - 23, confirm, hang, ramp, 0b10)
    words = [0x2AAAAA, 0]
    n = 14 * P + 3
    x = _audio(rng, 33, n, 2)
    on = rng.random((33, 15)) < 0.6
    on[:, :4] = True
    flat = np.repeat(on, P, axis=1)[:, :n, None]
    x = np.where(flat, np.int16(1234), x)
    sq, ref = _sq(fmd, words, cfg, 33, 2), dr.CodeSquelch(words, cfg)
    y = _feed(sq, ref, x, [5 * P + 1])
    assert y.any() == (confirm < 255)
    if hang == 65535:
        assert sq.status()[2].all()                          # once open, held


def test_in_place_and_refused_calls(fmd):
    import torch
    rng = np.random.default_rng(41)
    P, F = 192, 65
    words, cfg = _words(rng, F), _loose(rng, P, 8, 33, F, 23, 22)
    x = _audio(rng, 35, 4 * P + 50, 2)
    whole = dr.dcs_all(x, words, cfg)
    sq = _sq(fmd, words, cfg, 35, 2)
    first = _call(sq, x[:, :300])
    rest = x[:, 300:]
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
    # the refused call handed over again, in place: d_out == d_in with out_cap == in_cap; it equals the uncut stream
    assert sq.run_device(d_in.data_ptr(), n, n, d_in.data_ptr(), n) == n
    sq.check()
    assert np.array_equal(np.concatenate([first, d_in.cpu().numpy()], axis=1), whole) and whole.any()


def test_reset_inside_a_block_a_callers_stream_and_two_handles(fmd):
    import torch
    rng = np.random.default_rng(43)
    wa, wb = _words(rng, 65), _words(rng, 2)
    ca, cb = _loose(rng, 192, 8, 33, 65, 23, 22), _loose(rng, 64, 1, 2, 2, 23, 511)
    xa, xb = _audio(rng, 7, 2048, 2), _audio(rng, 2, 2048, 1)
    a, b = _sq(fmd, wa, ca, 7, 2), _sq(fmd, wb, cb, 2, 1)
    ra, rb = dr.CodeSquelch(wa, ca), dr.CodeSquelch(wb, cb)
    stream = torch.cuda.Stream()
    first = None
    for lo, hi in ((0, 600), (600, 601), (601, 2048)):      # the two handles interleaved, a on the caller's stream, b on the default one
        ya = _call(a, xa[:, lo:hi], stream=stream.cuda_stream)
        yb = _call(b, xb[:, lo:hi], _odd(hi - lo))
        assert np.array_equal(ya, ra.push(xa[:, lo:hi])) and np.array_equal(yb, rb.push(xb[:, lo:hi]))
        assert _status_equal(a, ra) and _status_equal(b, rb)
        first = ya if first is None else first
    _call(a, xa[:, :101])                                    # 2149 samples: inside a block and inside a box, everything carried
    a.reset()
    assert a.counts() == (0, 0) and a.status()[0].tolist() == [-1] * 7 and not a.status()[1].any() and not a.status()[2].any()
    assert np.array_equal(_call(a, xa[:, :600]), first)      # reset reproduces the first call
    ra.reset()
    ra.push(xa[:, :600])
    assert np.array_equal(_call(a, xa[:, 600:]), ra.push(xa[:, 600:])) and _status_equal(a, ra)
    assert b.counts() == (2048, 2048)


def _fm(n, fs, off, amp, msg_hz):
    """A carrier at `off` whose frequency moves by msg_hz[i] Hz"""
    ph = 2 * np.pi * np.cumsum(msg_hz) / fs
    return amp * np.exp(1j * (2 * np.pi * off * np.arange(n) / fs + ph))


def test_narrow_bank_nfm_into_code_squelch_into_agc_on_device_buffers(fmd):
    """The narrow-band bank in NFM mode on a synthetic 240 kHz capture whose first station carries code 023 (500 Hz deviation) under a
    1 kHz voice tone: its d_out at 12 kHz, as it stands and with its out_cap as in_cap, through code_squelched(bank) and on through an
    Agc equals the three definitions composed, call by call; the gate of the station with the code opens.  (Which sign the bank's
    discriminator gives the code is the bank's own: the table of all 104 reports it as 023 or as its inverse partner 047.)"""
    import torch
    rng = np.random.default_rng(47)
    fs, D, T, R, Ta, S, K = 240000, 4, 64, 5, 127, 1, 3
    rate = fs // D // R
    h = st.lowpass(T, 20000 / fs)
    offs = np.array([[-70000, 20000, 85000]])
    incs = np.array([[fmd.phase_inc(int(o), fs) for o in offs[s]] for s in range(S)], np.uint32)
    g = fmd.narrow_taps(fs // D, Ta, -6000, 6000)
    nb = fmd.NarrowBank(h, D, incs, g, R, mode=nr.FM, n_streams=S, block=64, squelch=0, gain=256, device_id=0)
    refs = [nr.NarrowRef(nb.taps, nb.decim, incs[s], nb.shift, nb.gr, nb.gi, nb.mode, nb.chan_decim, nb.chan_shift, nb.block, nb.squelch,
                         nb.gain) for s in range(S)]
    codes = fmd.DCS_CODES
    P = 2112                                                 # one word period: the capture is short
    sq = fmd.code_squelched(nb, rate, accept=(0o023, 0o047), block=P, min_hits=3, device_id=0)
    assert (sq.n_rows, sq.width, sq.accept) == (S * K, 1, (1 << codes.index(0o023)) | (1 << codes.index(0o047)))
    d = fmd.dcs_design(rate)
    sref = dr.CodeSquelch([fmd.dcs_word(c) for c in codes], dr.Cfg(P, d.box, d.lp, d.lshift, d.tap, d.tol, 3, d.confirm, d.hang, d.ramp, sq.accept))
    ag = fmd.leveled(nb, target=10000, block=64, hang=2, decay=64, gain_max=262144, device_id=0)
    aref = ar.Agc(ar.Cfg(64, 10000, 262144, 2, 64))
    lens = (8 * 24003, 8 * 10001, 8 * 90000)
    total = sum(lens) // 2
    c = fmd.dcs_codeword(0o023)
    t = np.arange(total)
    msg = 500.0 * (2.0 * ((c >> (np.floor(t * 134.4 / fs + 3.3).astype(np.int64) % 23)) & 1) - 1.0) + 1500.0 * np.sin(2 * np.pi * 1000.0 * t / fs)
    z = np.zeros((S, total), np.complex128)
    z[0] = _fm(total, fs, float(offs[0, 0]), 40.0, msg) + nr.carrier(total, fs, float(offs[0, 1]), 40.0)
    data_all = np.stack([nr.to_u8(z[s], noise=1.0, seed=s) for s in range(S)])
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
    assert opened.tolist() == [True, False, False] and codes[sq.status()[0][0]] in (0o023, 0o047)


@pytest.mark.parametrize("width", [1, 2])
def test_the_tool_gates_a_file_like_the_handle(fmd, width, tmp_path):
    """dcs_gpu over a file of more than two reads equals the handle over the same samples (and so the definition), and reports
    every change of the selected code or the gate on stderr as `block code hits open`."""
    rng = np.random.default_rng(53 + width)
    rate = 12000
    codes = fmd.DCS_CODES
    cfg = _tight(fmd, accept=(1 << codes.index(0o114)) | (1 << codes.index(0o023)))
    P = cfg.block
    n = 2 * 65536 + 4 * P + 77
    on = np.zeros((2, n))
    on[0, 5 * P:18 * P] = 1
    on[1, 24 * P:] = 1
    x = (_coded(fmd, rng, rate, n, [0o114, 0o754], on).sum(axis=0, dtype=np.int64)[None] >> 1).astype(np.int16)
    x = np.ascontiguousarray(np.repeat(x, width, axis=2))
    words = [fmd.dcs_word(c) for c in codes]
    ref = dr.CodeSquelch(words, cfg)
    exp = ref.push(x)
    sq = _sq(fmd, words, cfg, 1, width)
    assert np.array_equal(_call(sq, x), exp) and exp[0, 8 * P:17 * P].any() and not exp[0, 27 * P:].any()
    lines, last = [], (-1, False)
    chk = dr.CodeSquelch(words, cfg)
    for b in range(n // P):
        chk.push(x[:, b * P:(b + 1) * P])
        code, hits, gate = chk.status()
        if (code[0], gate[0]) != last:
            lines.append("%d %s %d %d" % (b, "%03o" % codes[code[0]] if code[0] >= 0 else "-", hits[0], gate[0]))
        last = (code[0], gate[0])
    assert len(lines) >= 3 and {h[0]: h[2] for h in ref.hits}[10] == codes.index(0o114)
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "dcs_gpu")
    args = [exe, "-r", str(rate), "-c", str(width), "-a", "114,023"]
    (tmp_path / "in.s16").write_bytes(x.tobytes())
    p = subprocess.run(args + [str(tmp_path / "in.s16"), str(tmp_path / "out.s16")], capture_output=True, timeout=300)
    assert (p.returncode, p.stdout) == (0, b""), p.stderr.decode()
    assert (tmp_path / "out.s16").read_bytes() == exp.tobytes() and p.stderr.decode().splitlines() == lines
    p = subprocess.run(args, input=x[:, :3000].tobytes(), capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stdout == exp[:, :3000].tobytes()
