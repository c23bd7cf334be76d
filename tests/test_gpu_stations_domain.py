"""Station bank (include/fmd.h, fmd_stations_*) on the MI355X across the whole documented domain: audio and get_state against
the test-side definition (tests/stations_ref.py), bit for bit, after every call.  Decims 2 ... 64 and n_taps 1 ... 256 with
station counts on both sides of every row-tile edge, every tap value of both digit forms, |y| at its bounds on each side of the
f32 discriminator, the call shapes that mix history with new bytes or carry a group sum through a call without audio, the rate
ratios up to the largest accepted one (the heaviest tile), the benchmark's 512 streams and the grid's 65535, and the device
path at a 4-byte offset with a padded out_cap.  FMD_FUZZ_CASES / FMD_FUZZ_SEED scale and reseed the shape sweep."""
import os

import numpy as np
import pytest

import stations_ref as sr

pytestmark = pytest.mark.gpu

TOO_SHORT = -3


def _shift(h, incs, limit):
    """The smallest shift with ceil(256 max_gain / 2^shift) <= limit."""
    g = sr.max_gain(h, np.unique(np.asarray(incs, dtype=np.uint64)))
    s = 0
    while -(-256 * g >> s) > limit:
        s += 1
    return s


def _incs(rng, S, K):
    """[S, K] phase_incs, every (stream, station) its own: an index slip between streams or stations cannot pass."""
    while True:
        v = rng.integers(0, 1 << 32, S * K, dtype=np.uint64)
        if np.unique(v).size == v.size:
            return v.reshape(S, K).astype(np.uint32)


class Run:
    """One bank and the definition of the streams in `check`; call() feeds both and compares audio and state."""

    def __init__(self, fmd, oracle, h, D, incs, fast, slow, shift, check=None, z=sr.z_direct):
        self.fmd = fmd
        incs = np.asarray(incs, dtype=np.uint32)
        self.S, self.K = incs.shape
        self.bank = fmd.StationBank(h, D, incs, fast, slow, n_streams=self.S, shift=shift, device_id=0)
        self.check = list(range(self.S)) if check is None else sorted(set(check))
        self.refs = {s: sr.StationsRef(oracle, h, D, incs[s], fast, slow, shift, z=z) for s in self.check}

    def states(self):
        return [self.bank.get_state(s, k).as_dict() for s in self.check for k in range(self.K)]

    def compare_states(self):
        for s in self.check:
            for k in range(self.K):
                st, want = self.bank.get_state(s, k).as_dict(), self.refs[s].state(k)
                assert [st[x] for x in ("demod_pre", "now_lpr", "prev_lpr_index")] == \
                       [want[x] for x in ("demod_pre", "now_lpr", "prev_lpr_index")], (s, k, st, want)

    def call(self, data):
        """Returns False when the call is too short (and checks that it changed nothing)."""
        try:
            exp = {s: r.feed(data[s]) for s, r in self.refs.items()}
        except sr.TooShort:
            before = self.states()
            with pytest.raises(self.fmd.FmdError) as e:
                self.bank.demodulate_batch(data)
            assert e.value.status == TOO_SHORT
            assert self.states() == before
            return False
        got = self.bank.demodulate_batch(data)
        self.last = got.shape[2]
        for s in self.check:
            for k in range(self.K):
                assert got.shape[2] == exp[s][k].size and np.array_equal(got[s, k], exp[s][k]), (s, k, data.shape[1])
        self.compare_states()
        return True


def _bytes(rng, S, n):
    b = rng.integers(0, 256, (S, n), dtype=np.uint8)
    if n >= 64:                                                    # a full-scale stretch
        a = int(rng.integers(0, n - n // 4)) & ~1
        b[:, a:a + n // 4] = np.where(rng.random((S, n // 4)) < 0.5, 0, 255)
    return b


DECIMS = (2, 4, 6, 30, 62, 64)
TAPS = (1, 2, 26, 27, 58, 59, 250, 256)
K_TWO = (4, 5, 8, 9, 28, 29, 32)                                   # row tiles of 4 stations
K_ONE = (8, 9, 16, 17, 24, 25, 32)                                 # row tiles of 8


def test_shape_sweep(fmd, oracle):
    n_cases = max(16, int(os.environ.get("FMD_FUZZ_CASES", "16")))
    rng = np.random.default_rng(int(os.environ.get("FMD_FUZZ_SEED", "20260101")) + 101)
    for i in range(n_cases):
        D, T = DECIMS[i % len(DECIMS)], TAPS[(3 * i) % len(TAPS)]
        if i % 8 == 5:
            T = int(rng.integers(1, D))                            # n_taps < decim
        digits = 2 if i % 2 == 0 else 1
        K = (K_TWO if digits == 2 else K_ONE)[(i // 2) % 7]
        S = int(rng.integers(1, 4))
        if digits == 2:
            h = rng.integers(-2047, 2048, T).astype(np.int16)
            h[int(rng.integers(0, T))] = 2047 * int(rng.choice([-1, 1]))
        else:
            h = rng.integers(-127, 128, T).astype(np.int16)
        incs = _incs(rng, S, K)
        incs[0, 0] = 0                                             # W = h: the digit form is the taps'
        w = [sr.complex_taps(h, int(x)) for x in incs.ravel()]
        assert (max(max(np.abs(a).max(), np.abs(b).max()) for a, b in w) <= 127) == (digits == 1)
        shift = _shift(h, incs, 16384 if i % 3 else 2048)
        slow = int(rng.choice([8000, 16000, 22050, 32000, 44100, 48000]))
        fast = int(slow * rng.uniform(1.0, 12.0))
        run = Run(fmd, oracle, h, D, incs, fast, slow, shift)
        sizes = [8 * int(rng.integers(1, (T + 2 * D) // 4 + 3)), 8 * int(rng.integers(1, 40)),
                 8 * int(rng.integers(200, 3000)), 8 * int(rng.integers(1, 3 * D + T // 4 + 2)), 8 * int(rng.integers(500, 4000))]
        fed = [run.call(_bytes(rng, S, n)) for n in sizes]
        assert any(fed), (D, T, K, sizes)


def test_every_tap_value_of_both_digit_forms(fmd, oracle):
    """inc = 0 makes the taps exactly h (one station per handle does so); 16 handles of 256 taps hold every value -2047 ... 2047,
    one holds -127 ... 127 (the one-digit form), and one forces the two-digit form with values around the split W = 128 hi + lo."""
    rng = np.random.default_rng(202)
    vals = rng.permutation(np.arange(-2047, 2048))
    handles = [vals[i:i + 256] for i in range(0, vals.size, 256)]
    handles[-1] = np.concatenate([handles[-1], rng.integers(-2047, 2048, 256 - handles[-1].size)])
    one = np.concatenate([np.arange(-127, 128), [127]])
    split = np.array([128, -128, 64, -64, 63, -63, 65, -65, 191, 192, -191, -192, 127, -127, 1, -1] * 16)
    handles += [rng.permutation(one), rng.permutation(split)]
    seen = set()
    for j, h in enumerate(handles):
        h = h.astype(np.int16)
        seen.update(int(x) for x in h)
        D = (2, 4, 10, 64)[j % 4]
        incs = np.array([[0, int(rng.integers(1, 1 << 32)), 1 << 30]], np.uint32)
        run = Run(fmd, oracle, h, D, incs, 240000, 32000, _shift(h, incs, 16384 if j % 2 else 2048))
        for n in (8 * (300 + 4 * D), 8 * 777):
            run.call(_bytes(rng, 1, n))
    assert seen >= set(range(-2047, 2048))


def _maximise(w, comp, sign):
    """Bytes of one window (2 T) that drive component `comp` (0: zr, 1: zi) of z = sum W c to its extreme of `sign`."""
    wr, wi = w
    a, b = (wr, -wi) if comp == 0 else (wi, wr)                    # weights of cI, cQ
    cI = np.where(sign * a > 0, 255, 0)                            # c = b - 127: 128 or -127
    cQ = np.where(sign * b > 0, 255, 0)
    out = np.empty(2 * wr.size, np.uint8)
    out[0::2], out[1::2] = cI, cQ
    return out


@pytest.mark.parametrize("limit,shift,gain", [(16384, 6, 4096), (2048, 8, 2048), (2049, 8, 2049)])
def test_y_at_its_bounds(fmd, oracle, limit, shift, gain):
    """Quarter-turn phase_incs keep sum |Wr| + |Wi| = sum |h| for every station, so lp_bound = ceil(256 G / 2^shift) is `limit`
    exactly at the minimal shift: 16384 (the integer discriminator's bound), 2048 (the f32 one) and 2049 (just past it).  Windows
    of chosen outputs are set to drive zr or zi of one station to either extreme."""
    rng = np.random.default_rng(303 + limit)
    T, D = 48, 6
    mag = rng.multinomial(gain - T, np.ones(T) / T) + 1
    h = (mag * rng.choice([-1, 1], T)).astype(np.int16)
    incs = np.array([[0, 1 << 30, 1 << 31, 3 << 30]], np.uint32)
    assert sr.max_gain(h, incs[0]) == gain and _shift(h, incs, limit) == shift
    assert -(-256 * gain >> shift) == limit
    if limit == 16384:
        with pytest.raises(fmd.FmdError):                          # the bound is tight: one shift less is refused
            fmd.StationBank(h, D, incs, 240000, 32000, shift=shift - 1, device_id=0)
    run = Run(fmd, oracle, h, D, incs, 240000, 32000, shift)
    W = [sr.complex_taps(h, int(x)) for x in incs[0]]
    for n in (8 * 3000, 8 * 1001):
        data = _bytes(rng, 1, n)
        first = -run.refs[0].pos % D                               # the first window that starts in this call
        for i, m in enumerate(range(first, n // 2 - T, D * (T // D + 1))):
            k, comp, sign = i % 4, (i // 4) % 2, 1 if (i // 8) % 2 == 0 else -1
            data[0, 2 * m:2 * (m + T)] = _maximise(W[k], comp, sign)
        run.call(data)


def test_call_shapes(fmd, oracle):
    rng = np.random.default_rng(404)
    # the smallest call with 2 outputs as the stream's first call, after a TOO_SHORT one; then the stream continues exactly
    for D, T in ((2, 1), (6, 27), (64, 256)):
        h = rng.integers(-2047, 2048, T).astype(np.int16)
        incs = _incs(rng, 2, 5)
        run = Run(fmd, oracle, h, D, incs, 48000 * (2 if D < 64 else 1), 48000, _shift(h, incs, 16384))
        need = 8 * -(-(2 * (T + D)) // 8)                           # 2 outputs: T + D samples
        if need > 8:
            assert not run.call(_bytes(rng, 2, need - 8))
        assert run.call(_bytes(rng, 2, need))
        if D > 2:                                                  # at most one output
            assert not run.call(_bytes(rng, 2, 8 if D < 64 else 128))
        assert run.call(_bytes(rng, 2, 8 * 900))
    # 256 taps, decim 2, c = 100: a run of calls shorter than the history (HB = 512 bytes), most without audio, so the history
    # is rebuilt from old history plus new bytes and the group sum is carried through calls that produce nothing
    h = rng.integers(-2047, 2048, 256).astype(np.int16)
    incs = _incs(rng, 3, 4)
    run = Run(fmd, oracle, h, 2, incs, 1000000, 10000, _shift(h, incs, 2048))
    assert run.call(_bytes(rng, 3, 8 * 600))
    quiet = 0
    for n in (16, 24, 8 * 63, 32, 8 * 17, 496, 40, 8 * 5, 504, 16, 8 * 33, 48, 8 * 61, 16, 24, 8 * 200, 8 * 9, 16):
        assert run.call(_bytes(rng, 3, n))
        quiet += run.last == 0
    assert quiet >= 8
    # nbytes % 16 == 8 on many streams
    h = rng.integers(-900, 901, 33).astype(np.int16)
    incs = _incs(rng, 40, 3)
    run = Run(fmd, oracle, h, 4, incs, 128000, 32000, _shift(h, incs, 2048))
    for n in (8 * 501, 8 * 37, 8 * 1999, 8 * 3):
        run.call(_bytes(rng, 40, n))


@pytest.mark.parametrize("D,T,K,fast,slow", [
    (10, 64, 8, 48000, 48000),                      # rate_out == rate_resample
    (4, 27, 5, 16777213, 999983),                   # reduced terms near 2^24 and 2^20, c = 17
    (2, 8, 3, 5592406, 5592405),                    # 3 sr = 2^24 - 1: the largest accepted reduced resample rate, kt = 1
    (2, 8, 1, 1260000, 10000),                      # c = 126: the largest ratio at a small shape
    (64, 256, 32, 1160000, 10000),                  # c = 116 at the largest shape: the heaviest tile (kt = 1, LDS > 40 KiB)
])
def test_rates(fmd, oracle, D, T, K, fast, slow):
    rng = np.random.default_rng(505 + D + T)
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    incs = _incs(rng, 2, K)
    run = Run(fmd, oracle, h, D, incs, fast, slow, _shift(h, incs, 16384 if K % 2 else 2048), z=sr.z_corr)
    c = -(-fast // slow)
    unit = 2 * D * c                                                # bytes per audio sample
    if fast == 5592406:
        sizes = (8 * 50, 8 * 120, 8 * 33)                           # fmd_ranges_fit32 keeps calls short at these terms
    else:
        sizes = (8 * -(-unit * 9 // 8), 8 * -(-unit * 2 // 8) + 8, 8 * -(-unit * 5 // 8))
    for n in sizes:
        assert run.call(_bytes(rng, 2, n))


def test_benchmark_shape_512_streams(fmd, oracle):
    """bench.py's station shape: 512 streams x 262144 B, decim 10, 64 taps, 8 stations, two calls; streams on both sides of the
    middle and at both ends are checked."""
    rng = np.random.default_rng(606)
    S, n = 512, 262144
    h = rng.integers(-2047, 2048, 64).astype(np.int16)
    incs = _incs(rng, S, 8)
    run = Run(fmd, oracle, h, 10, incs, 240000, 32000, _shift(h, incs, 2048), check=(0, 1, 255, 256, 510, 511), z=sr.z_corr)
    for _ in range(2):
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8))


def test_65535_streams(fmd, oracle):
    """The grid-y limit: 65535 streams of small calls, one station of 8 taps (the host plan holds 4 KiB per stream)."""
    rng = np.random.default_rng(707)
    S = 65535
    h = rng.integers(-2047, 2048, 8).astype(np.int16)
    incs = rng.integers(0, 1 << 32, (S, 1), dtype=np.uint64).astype(np.uint32)
    check = [0, 1, 2, 4095, 4096, 32767, 32768, 65533, 65534] + [int(x) for x in rng.integers(0, S, 7)]
    run = Run(fmd, oracle, h, 4, incs, 96000, 32000, _shift(h, incs, 2048), check=check)
    for n in (8 * 40, 8 * 13):
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8))


def test_device_path_unaligned_and_padded(fmd, oracle):
    """d_iq 4 bytes past an aligned address (nbytes % 16 == 8, so no row is 16-byte aligned), out_cap larger than needed and the
    padding filled with a sentinel that must survive."""
    import torch
    rng = np.random.default_rng(808)
    S, K, D = 3, 6, 6
    h = rng.integers(-2047, 2048, 59).astype(np.int16)
    incs = _incs(rng, S, K)
    shift = _shift(h, incs, 16384)
    bank = fmd.StationBank(h, D, incs, 192000, 48000, n_streams=S, shift=shift, device_id=0)
    refs = [sr.StationsRef(oracle, h, D, incs[s], 192000, 48000, shift) for s in range(S)]
    dev = torch.device("cuda:0")
    SENT = -12345
    for n in (8 * 1001, 8 * 7, 8 * 2403):
        data = _bytes(rng, S, n)
        buf = torch.zeros(S * n + 16, dtype=torch.uint8, device=dev)
        buf[4:4 + S * n] = torch.from_numpy(data.ravel()).to(dev)
        cap = bank.out_cap(n) + 37
        d_out = torch.full((S, K, cap), SENT, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        try:
            exp = [refs[s].feed(data[s]) for s in range(S)]
        except sr.TooShort:
            with pytest.raises(fmd.FmdError) as e:
                bank.demodulate_device(buf.data_ptr() + 4, n, d_out.data_ptr(), cap)
            assert e.value.status == TOO_SHORT
            continue
        got_n = bank.demodulate_device(buf.data_ptr() + 4, n, d_out.data_ptr(), cap)
        bank.check()
        got = d_out.cpu().numpy()
        for s in range(S):
            for k in range(K):
                assert got_n == exp[s][k].size and np.array_equal(got[s, k, :got_n], exp[s][k]), (n, s, k)
                assert (got[s, k, got_n:] == SENT).all(), (n, s, k)
                st, want = bank.get_state(s, k).as_dict(), refs[s].state(k)
                assert st["demod_pre"] == want["demod_pre"] and st["now_lpr"] == want["now_lpr"], (n, s, k)
