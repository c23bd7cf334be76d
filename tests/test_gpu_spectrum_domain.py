"""Power-spectrum scanner (include/fmd.h, fmd_spectrum_*) on the MI355X across its whole domain, bit for bit against the
test-side definition (tests/spectrum_ref.py): hops other than 8, N / 2 and N, streams split over many blocks with a partial last
batch, the mod-2^64 wrap across blocks, every window value, the unaligned device path with accumulation over calls of
different lengths, and 65535 streams."""
import numpy as np
import pytest

import spectrum_ref as spr

pytestmark = pytest.mark.gpu


def _bytes(rng, S, nbytes):
    b = rng.integers(0, 256, (S, nbytes), dtype=np.uint8)
    for s in range(S):                                           # runs of 0 and of 255
        for v in (0, 255):
            a = int(rng.integers(0, nbytes - nbytes // 8))
            b[s, a:a + nbytes // 8] = v
    return b


def _nbytes(N, hop, F, partial=0):
    n = 2 * (N + hop * (F - 1) + partial)
    return n + (-n) % 8


def _window(rng, N, digits):
    if digits == 1:
        w = rng.integers(-127, 128, N).astype(np.int16)
        w[0] = 127
    else:
        w = rng.integers(-2047, 2048, N).astype(np.int16)
        w[0] = -2047
    assert spr.digits(w) == digits
    return w


@pytest.mark.parametrize("N,hop", [(32, 24), (64, 40), (64, 56), (128, 120), (128, 72), (256, 248), (256, 136)])
def test_hops_that_are_not_8_half_or_whole(fmd, N, hop):
    rng = np.random.default_rng(10 * N + hop)
    for digits in (1, 2):
        S = 2
        w = _window(rng, N, digits)
        shift = int(rng.integers(0, 20))
        sp = fmd.Spectrum(N, hop, window=w, shift=shift, n_streams=S, device_id=0)
        assert sp.tap_digits() == digits
        F = int(rng.integers(2000, 3000))
        nbytes = _nbytes(N, hop, F, int(rng.integers(0, hop)))
        data = _bytes(rng, S, nbytes)
        assert sp.frames(nbytes) == spr.frames(N, hop, nbytes)
        assert np.array_equal(sp.power_batch(data), spr.power_chunked(w, hop, shift, data)), (N, hop, digits)


@pytest.mark.parametrize("N,hop,S,F", [
    (16, 8, 1, 2048 * 512 + 77),     # one stream over ~2048 blocks, a partial last block and batch
    (64, 40, 3, 683 * 512 - 5),      # three streams of ~683 blocks
    (256, 248, 1, 64 * 256 + 3),     # 64-frame batches at N = 256
])
def test_many_blocks_per_stream(fmd, N, hop, S, F):
    rng = np.random.default_rng(N + S)
    w = _window(rng, N, 2)
    sp = fmd.Spectrum(N, hop, window=w, shift=9, n_streams=S, device_id=0)
    nbytes = _nbytes(N, hop, F)
    data = rng.integers(0, 256, (S, nbytes), dtype=np.uint8)
    assert sp.frames(nbytes) == F
    assert np.array_equal(sp.power_batch(data), spr.power_chunked(w, hop, 9, data))


def test_sum_wraps_mod_2_64_across_blocks(fmd):
    """shift 0 under a full-scale +-2047 window: stream 0 holds full-scale bytes whose signs follow the window's (period 8 samples,
    the hop), so bin 0 adds ~2^53 per frame and wraps modulo 2^64 several times, split over the blocks' 64-bit atomics; stream 1
    holds random full-scale bytes."""
    rng = np.random.default_rng(11)
    N, hop, S, F = 256, 8, 2, 12000
    sign = rng.choice([-1, 1], 8)
    w = (2047 * np.tile(sign, N // 8)).astype(np.int16)
    sp = fmd.Spectrum(N, hop, window=w, shift=0, n_streams=S, device_id=0)
    nbytes = _nbytes(N, hop, F)
    data = np.where(rng.random((S, nbytes)) < 0.5, 0, 255).astype(np.uint8)
    data[0] = np.tile(np.repeat(np.where(sign > 0, 255, 0), 2), nbytes // 16).astype(np.uint8)
    exp = spr.power_chunked(w, hop, 0, data)
    wide = spr.power_chunked(w, hop, 40, data).astype(object) << 40      # a lower bound on the true sum, without the wrap
    assert wide[0, 0] >= 4 << 64
    assert np.array_equal(sp.power_batch(data), exp)


def test_every_window_value(fmd):
    """Bin 0 has the taps w itself (inc_0 = 0): 16 handles of N = 256 hold every value -2047 ... 2047, one every value of the
    one-digit form -127 ... 127."""
    rng = np.random.default_rng(12)
    vals = rng.permutation(np.arange(-2047, 2048))
    wins = [vals[i:i + 256] for i in range(0, vals.size, 256)]
    wins[-1] = np.concatenate([wins[-1], [2047]])
    wins.append(rng.permutation(np.concatenate([np.arange(-127, 128), [-127]])))
    seen = set()
    for j, w in enumerate(wins):
        w = w.astype(np.int16)
        seen.update(int(x) for x in w)
        hop = (8, 64, 128, 200, 256)[j % 5]
        sp = fmd.Spectrum(256, hop, window=w, shift=j % 24, n_streams=2, device_id=0)
        assert sp.tap_digits() == (1 if j == len(wins) - 1 else 2)
        data = _bytes(rng, 2, _nbytes(256, hop, 300, j % 7))
        assert np.array_equal(sp.power_batch(data), spr.power(w, hop, j % 24, data)), j
    assert seen >= set(range(-2047, 2048))


def test_device_path_unaligned_accumulates_over_calls_of_different_lengths(fmd):
    """d_iq 4 bytes past an aligned address with nbytes % 16 == 0: the unaligned load path.  Calls of different lengths accumulate
    into one d_power (mod 2^64), and the first call without accumulate overwrites what was there."""
    import torch
    rng = np.random.default_rng(13)
    N, hop, S = 64, 24, 3
    w = _window(rng, N, 2)
    sp = fmd.Spectrum(N, hop, window=w, shift=2, n_streams=S, device_id=0)
    dev = torch.device("cuda:0")
    d_power = torch.full((S, N), -1, dtype=torch.int64, device=dev)
    want = np.zeros((S, N), np.uint64)
    bufs = []
    for i, n in enumerate((16 * 4001, 16 * 37, 16 * 10000, 16 * 9)):
        assert n % 16 == 0
        data = _bytes(rng, S, n)
        buf = torch.zeros(S * n + 16, dtype=torch.uint8, device=dev)
        buf[4:4 + S * n] = torch.from_numpy(data.ravel()).to(dev)
        bufs.append(buf)
        torch.cuda.synchronize()
        sp.power_device(buf.data_ptr() + 4, n, d_power.data_ptr(), accumulate=i > 0)
        want += spr.power(w, hop, 2, data)
    sp.check()
    assert np.array_equal(d_power.cpu().numpy().view(np.uint64), want)


def test_65535_streams(fmd):
    rng = np.random.default_rng(14)
    S, N, hop = 65535, 16, 8
    w = _window(rng, N, 2)
    sp = fmd.Spectrum(N, hop, window=w, shift=5, n_streams=S, device_id=0)
    nbytes = _nbytes(N, hop, 11, 3)
    data = rng.integers(0, 256, (S, nbytes), dtype=np.uint8)
    got = sp.power_batch(data)
    pick = [0, 1, 2, 4095, 4096, 32767, 32768, 65533, 65534] + [int(x) for x in rng.integers(0, S, 7)]
    assert np.array_equal(got[pick], spr.power(w, hop, 5, data[pick]))
