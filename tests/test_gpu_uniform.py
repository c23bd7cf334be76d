"""Uniform channelizer (include/fmd.h, fmd_uniform_*) on the MI355X: bit for bit against the test-side definition
(tests/uniform_ref.py) -- anchored handle against handle to the channelizer where both are defined, over the smallest shapes at
which each part of the kernel can go wrong, at the 16384 edge, and through the call mechanics (refusals, splitting, tiles,
streams, reset, the device entry point)."""
import numpy as np
import pytest

import stations_ref as sr
import uniform_ref as ur

pytestmark = pytest.mark.gpu

BAD_LENGTH, TOO_SHORT = -2, -3


def _bytes(rng, S, n):
    b = rng.integers(0, 256, (S, n), dtype=np.uint8)
    b[:, : n // 3] = np.where(rng.random((S, n // 3)) < 0.5, 0, 255)          # full-scale stretch
    return b


def _one_digit_taps(rng, T):
    return rng.integers(-127, 128, T).astype(np.int16) // 2   # every |W| <= 127 -> the one-digit form


def _make(fmd, h, N, hop, channels=None, S=1, z=sr.z_corr, shift=None):
    u = fmd.UniformChannelizer(h, N, hop, channels=channels, n_streams=S, shift=shift, device_id=0)
    incs = ur.channel_incs(N, channels)
    assert u.shift == (ur.min_shift(h, incs) if shift is None else shift)
    assert u.tap_digits() == ur.digits(h, incs)
    assert u.kernel_name().startswith("fmd_uv::")
    refs = [ur.UniformRef(h, N, hop, u.shift, channels=channels, z=z) for _ in range(S)]
    return u, refs


def _call(fmd, u, refs, data, other=None):
    """One call of every stream: the handle and the definition agree (and `other`, a Channelizer, returns the same), or both
    refuse and the handle changes nothing."""
    if refs[0].outputs_after(data.shape[1] // 2) - refs[0].m_next < 1:
        before = u.outputs()
        with pytest.raises(fmd.FmdError) as e:
            u.run_batch(data)
        assert e.value.status == TOO_SHORT and u.outputs() == before
        return None
    got = u.run_batch(data)
    for s, ref in enumerate(refs):
        exp = ref.feed(data[s])
        assert got.shape[1:3] == exp.shape[:2], (got.shape, exp.shape)
        assert np.array_equal(got[s], exp), (s, data.shape[1])
    assert u.outputs() == refs[0].m_next
    if other is not None:
        assert np.array_equal(other.run_batch(data), got)
        assert other.outputs() == u.outputs()
    return got


@pytest.mark.parametrize("N,hop,T,digits", [(16, 8, 64, 2), (32, 16, 256, 1)])
def test_anchor_equals_the_channelizer_call_by_call(fmd, N, hop, T, digits):
    rng = np.random.default_rng(100 * N + T)
    h = _one_digit_taps(rng, T) if digits == 1 else rng.integers(-2047, 2048, T).astype(np.int16)
    S = 2
    u, refs = _make(fmd, h, N, hop, S=S)
    assert u.tap_digits() == digits
    ch = fmd.Channelizer(h, hop, [fmd.uniform_channel_inc(k, N) for k in range(N)], n_streams=S, shift=u.shift, device_id=0)
    for hops in (T // hop + 3, 1, 37, 700, 2):
        assert _call(fmd, u, refs, _bytes(rng, S, 2 * hop * hops), other=ch) is not None


SHAPES = {
    # N, hop, T, selection, digits, z, hops per call
    "1-n96-rounded-incs-24-chunks": (96, 48, 768, None, 2, sr.z_corr, (300, 17, 1)),
    "2-n12-partial-row-tile": (12, 8, 72, [0, 5, 11], 2, sr.z_corr, (150, 1, 400)),
    "3-no-history-odd-T": (16, 64, 5, None, 2, sr.z_corr, (1, 37, 200)),
    "4-history-of-one-hop": (64, 128, 129, None, 2, sr.z_corr, (2, 1, 140)),
    "5-n256-most-row-tiles": (256, 128, 256, None, 1, sr.z_direct, (131, 1, 40)),
    "6-largest-T-and-hop": (256, 256, 2048, [0, 1, 127, 128, 255], 2, sr.z_corr, (100, 1, 37)),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_cases(fmd, name):
    N, hop, T, sel, digits, z, calls = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("1"):
        h = ur.taps(96, 8).astype(np.int16)
    elif digits == 1:
        h = _one_digit_taps(rng, T)
    else:
        h = rng.integers(-2047, 2048, T).astype(np.int16)
    S = 2
    u, refs = _make(fmd, h, N, hop, channels=sel, S=S, z=z)
    assert u.tap_digits() == digits
    done = 0
    for hops in calls:
        assert 2 * hop * hops <= 65536
        done += _call(fmd, u, refs, _bytes(rng, S, 2 * hop * hops)) is not None
    assert done >= 2


@pytest.mark.parametrize("hval,N,hop", [(2047, 4, 64), (-2047, 6, 256)])
def test_full_scale_at_the_16384_edge(fmd, hval, N, hop):
    """h constant at full scale over T = 2048, full-scale byte patterns, the smallest admissible shift: the 16384 edge of y and the
    i32 range of z."""
    T = 2048
    h = np.full(T, hval, np.int16)
    incs = ur.channel_incs(N)
    s = ur.min_shift(h, incs)
    assert s > 0 and -(-256 * sr.max_gain(h, incs) >> (s - 1)) > 16384
    u, refs = _make(fmd, h, N, hop, shift=s)
    peak = 0
    for pattern in ([255, 255], [0, 0], [255, 0], [0, 255]):
        u.reset()
        refs[0].reset()
        data = np.tile(np.array(pattern, np.uint8), T + 12 * hop)[None, :]
        got = _call(fmd, u, refs, data)
        peak = max(peak, int(np.abs(got.astype(np.int64)).max()))
    assert 2048 < peak <= 16384, peak                      # channel 0 alone reaches 128 T |h| / 2^shift


def test_refused_calls_change_nothing(fmd):
    rng = np.random.default_rng(5)
    N, hop, T = 16, 8, 64
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    u, refs = _make(fmd, h, N, hop)
    assert _call(fmd, u, refs, _bytes(rng, 1, 2 * hop * (T // hop - 1))) is None     # shorter than T: TOO_SHORT
    assert u.outputs() == 0
    for n in (2 * hop * 20 + 8, 2 * hop * 20 - 2, 8):
        with pytest.raises(fmd.FmdError) as e:
            u.run_batch(np.zeros((1, n), np.uint8))
        assert e.value.status == BAD_LENGTH and u.outputs() == 0
    assert _call(fmd, u, refs, _bytes(rng, 1, 2 * hop * 50)) is not None             # ... and the next call is the stream's first


@pytest.mark.parametrize("N,hop,T,cuts", [(16, 8, 64, (37, 1)), (16, 64, 5, (1, 37)), (64, 128, 129, (37, 1))])
def test_one_long_call_equals_the_same_bytes_in_pieces(fmd, N, hop, T, cuts):
    """Calls of one hop, 37 hops and the rest (the longer piece first where one hop alone completes no output)."""
    rng = np.random.default_rng(N + hop + T)
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    S, total = 2, 230
    data = _bytes(rng, S, 2 * hop * total)
    u, refs = _make(fmd, h, N, hop, S=S)
    whole = _call(fmd, u, refs, data)
    v, refs2 = _make(fmd, h, N, hop, S=S)
    parts, at = [], 0
    for hops in cuts + (total - sum(cuts),):
        parts.append(_call(fmd, v, refs2, data[:, 2 * hop * at:2 * hop * (at + hops)]))
        at += hops
    assert all(p is not None for p in parts)
    assert np.array_equal(np.concatenate(parts, axis=2), whole)


def test_tiles_streams_and_reset(fmd):
    """Several tiles per stream plus a short tail tile, three streams with different data (each has its own history), and reset
    gives the first call's output again."""
    rng = np.random.default_rng(9)
    N, hop, T, S = 16, 8, 64, 3
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    u, refs = _make(fmd, h, N, hop, S=S)
    first = _bytes(rng, S, 2 * hop * (T // hop - 1 + 3 * 128 + 5))      # 3 tiles of 128 outputs (or 6 of 64) and 5 more
    a = _call(fmd, u, refs, first)
    assert a.shape[2] == 3 * 128 + 5
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
    for hops in (2 * 128 + 1, 1, 128):
        assert _call(fmd, u, refs, _bytes(rng, S, 2 * hop * hops)) is not None
    u.reset()
    assert u.outputs() == 0
    assert np.array_equal(u.run_batch(first), a)


def test_device_path_unaligned_input_and_odd_out_cap(fmd):
    """d_iq 4 bytes past an aligned address (no LDS-DMA piece is possible), an odd out_cap; rows beyond the call's outputs keep
    their sentinel."""
    import torch
    rng = np.random.default_rng(11)
    N, hop, T, S = 12, 8, 72, 3
    sel = [0, 5, 11]
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    u, refs = _make(fmd, h, N, hop, channels=sel, S=S)
    dev = torch.device("cuda:0")
    SENT = -12345
    for hops in (300, 1, 131):
        n = 2 * hop * hops
        data = _bytes(rng, S, n)
        buf = torch.zeros(S * n + 16, dtype=torch.uint8, device=dev)
        buf[4:4 + S * n] = torch.from_numpy(data.ravel()).to(dev)
        cap = u.out_cap(n) + 7 + (u.out_cap(n) % 2)
        assert cap % 2 == 1
        d_out = torch.full((S, len(sel), cap, 2), SENT, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        got_n = u.run_device(buf.data_ptr() + 4, n, d_out.data_ptr(), cap)
        u.check()
        got = d_out.cpu().numpy()
        for s in range(S):
            exp = refs[s].feed(data[s])
            assert got_n == exp.shape[1] and np.array_equal(got[s, :, :got_n], exp), (hops, s)
            assert (got[s, :, got_n:] == SENT).all(), (hops, s)
    with pytest.raises(fmd.FmdError) as e:                    # out_cap too small
        u.run_device(buf.data_ptr() + 4, n, d_out.data_ptr(), 10)
    assert e.value.status == -5                               # FMD_ERR_CAPACITY
