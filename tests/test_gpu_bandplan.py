"""Band-plan bank (include/fmd.h, fmd_bandplan_*) on the MI355X: bit for bit against the test-side definition
(tests/bandplan_ref.py) -- anchored handle against handle to the narrow-band bank where both are defined, over the smallest shapes
at which each part of the second pass can go wrong (every R path of the polyphase staging, tap counts below R and at 64, real and
complex taps at the |g| and gain-sum edges, both block lengths, squelch on and off), and through the call mechanics (refusals that
change nothing, splitting, the tile edge, reset, the device entry point with rows that are only 2-byte aligned, the activity map)."""
import numpy as np
import pytest

import bandplan_ref as br
import domain_cases as dc
import uniform_ref as ur

pytestmark = pytest.mark.gpu

BAD_LENGTH, TOO_SHORT, CAPACITY = -2, -3, -5
K_TILE = 256                                                 # fmd_bp::kTile: audio samples per second-pass tile


def _bytes(rng, S, n, quiet=True):
    """Random bytes with a full-scale stretch and, so that blocks fall on both sides of a squelch, a quiet last third."""
    b = rng.integers(0, 256, (S, n), dtype=np.uint8)
    b[:, : n // 3] = np.where(rng.random((S, n // 3)) < 0.5, 0, 255)
    if quiet:
        q = n - n // 3 & ~1
        b[:, q:] = rng.integers(124, 132, (S, n - q), dtype=np.uint8)
    return b


_edge_taps = dc.edge_taps                                   # shared with the band-plan domain cases


class Run:
    """One bank and the definition of every stream; call() feeds both and compares the output, outputs() and levels()."""

    def __init__(self, fmd, h, N, hop, gr, gi, mode, R, P, squelch=0, gain=300, channels=None, S=1, chan_shift=None):
        self.fmd, self.S = fmd, S
        self.bank = fmd.BandPlanBank(h, N, hop, (gr, gi) if gi is not None else gr, R, mode=mode, channels=channels, n_streams=S,
                                     block=P, squelch=squelch, gain=gain, chan_shift=chan_shift, device_id=0)
        b = self.bank
        assert b.shift == ur.min_shift(h, ur.channel_incs(N, channels))
        if chan_shift is None:
            assert b.chan_shift == br.min_chan_shift(h, N, b.shift, gr, gi, channels, limit=256 if mode == br.FM else 16384)
        assert b.kernel_name(0).startswith("fmd_uv::")
        assert b.kernel_name(1) == "fmd_bp::fmd_bandplan_chan_kernel<%s>" % ("true" if gi is not None and np.any(gi) else "false")
        self.refs = [br.BandPlanRef(h, N, hop, b.shift, gr, gi, mode, R, b.chan_shift, P, squelch, gain, channels=channels)
                     for _ in range(S)]

    def snapshot(self):
        o, r = self.bank.levels()
        return self.bank.outputs(), o.tolist(), r.tolist()

    def compare_state(self):
        assert self.bank.outputs() == self.refs[0].n_next
        o, r = self.bank.levels()
        assert o.dtype == np.bool_ and r.dtype == np.uint32 and o.shape == r.shape == (self.S, self.bank.n_selected)
        for s, ref in enumerate(self.refs):
            want = [ref.level(k) for k in range(ref.K)]
            assert list(zip(o[s].tolist(), r[s].tolist())) == want, s

    def call(self, data, other=None):
        """The output [S, rows, n(, 2)], or None when the call is refused (and then it changed nothing)."""
        if self.refs[0].completes(data.shape[1]) < 1:
            before = self.snapshot()
            with pytest.raises(self.fmd.FmdError) as e:
                self.bank.run_batch(data)
            assert e.value.status == TOO_SHORT and self.snapshot() == before
            if other is not None:
                with pytest.raises(self.fmd.FmdError) as e:
                    other.run_batch(data)
                assert e.value.status == TOO_SHORT
            return None
        got = self.bank.run_batch(data)
        for s, ref in enumerate(self.refs):
            exp = ref.feed(data[s])
            assert got.shape[2] == exp.shape[1] and np.array_equal(got[s], exp), (s, data.shape[1])
        self.compare_state()
        if other is not None:
            assert np.array_equal(other.run_batch(data), got) and other.outputs() == self.bank.outputs()
        return got


def _probe_squelch(h, N, hop, gr, gi, mode, R, P, channels, data, chan_shift=None):
    """The median block RMS of an always-open run of the definition over `data` (one stream): blocks fall on both sides of it."""
    shift = ur.min_shift(h, ur.channel_incs(N, channels))
    cs = br.min_chan_shift(h, N, shift, gr, gi, channels, limit=256 if mode == br.FM else 16384) if chan_shift is None else chan_shift
    ref = br.BandPlanRef(h, N, hop, shift, gr, gi, mode, R, cs, P, 0, 256, channels=channels)
    ref.feed(data)
    rms = [np.sqrt(ref.block(k, j)[0] / P) for k in range(ref.K) for j in range(ref.n_next // P)]
    assert len(rms) >= 2
    return max(1, min(23170, int(np.median(rms))))


@pytest.mark.parametrize("mode", [br.IQ, br.FM, br.AM, br.SSB])
@pytest.mark.parametrize("N,hop,T,digits", [(16, 8, 64, 2), (32, 16, 256, 1)])
def test_anchor_equals_the_narrow_bank_call_by_call(fmd, N, hop, T, digits, mode):
    rng = np.random.default_rng(1000 * N + 10 * T + mode)
    h = rng.integers(-127, 128, T).astype(np.int16) // 2 if digits == 1 else rng.integers(-2047, 2048, T).astype(np.int16)
    assert ur.digits(h, ur.channel_incs(N)) == digits
    S, R, Ta, P = 2, 3, 20, 16
    gr, gi = _edge_taps(rng, Ta, mode in (br.IQ, br.SSB))
    calls = [_bytes(rng, S, 2 * hop * hops) for hops in (T // hop + 61, 1, 37, 300, 2)]
    sq = _probe_squelch(h, N, hop, gr, gi, mode, R, P, None, np.concatenate([c[0] for c in calls]))
    run = Run(fmd, h, N, hop, gr, gi, mode, R, P, squelch=sq, S=S)
    incs = [fmd.uniform_channel_inc(k, N) for k in range(N)]
    nb = fmd.NarrowBank(h, hop, incs, (gr, gi) if gi is not None else gr, R, mode=mode, n_streams=S, block=P, squelch=sq, gain=300,
                        chan_shift=run.bank.chan_shift, shift=run.bank.shift, device_id=0)
    fed = [run.call(c, other=nb) is not None for c in calls]
    assert fed[0] and fed[2] and fed[3] and not fed[1]       # one hop is a third of an audio sample
    for s in range(S):
        for k in range(N):
            assert nb.level(s, k) == run.refs[s].level(k)


# R, Ta, complex, P, squelch on, mode: every R path of the staging, Ta below R, the tap-chunk edges (4 complex / 8 real taps)
COMBOS = [(1, 1, False, 16, False, br.AM), (2, 7, True, 64, True, br.IQ), (3, 32, False, 16, True, br.FM), (5, 64, True, 64, False, br.SSB),
          (8, 7, True, 16, True, br.AM), (8, 64, False, 64, True, br.FM), (5, 1, False, 16, True, br.IQ), (1, 64, True, 64, True, br.SSB)]
SHAPES = {"n16-all": (16, 8, 128, None), "n16-selected": (16, 8, 128, [1, 5, 6, 15]), "n12": (12, 8, 72, None), "hop128": (4, 128, 512, None)}


@pytest.mark.parametrize("combo", range(len(COMBOS)))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes(fmd, shape, combo):
    N, hop, T, sel = SHAPES[shape]
    R, Ta, cplx, P, use_sq, mode = COMBOS[combo]
    rng = np.random.default_rng(sum(map(ord, shape)) + 97 * combo)
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    gr, gi = _edge_taps(rng, Ta, cplx)
    S = 3
    first = -(-T // hop) + R * (2 * P + 3) + Ta                   # hops: two blocks and a few samples
    calls = [_bytes(rng, S, 2 * hop * hops) for hops in (first, R + 1, R * (P + 5))]
    sq = _probe_squelch(h, N, hop, gr, gi, mode, R, P, sel, np.concatenate([c[0] for c in calls])) if use_sq else 0
    run = Run(fmd, h, N, hop, gr, gi, mode, R, P, squelch=sq, channels=sel, S=S)
    outs = [run.call(c) for c in calls]
    assert all(o is not None for o in outs)
    got = np.concatenate(outs, axis=2)
    assert not np.array_equal(got[0], got[1]) and got.any()
    if use_sq:
        assert (got == 0).all(axis=tuple(range(3, got.ndim)))[:, :, P:].any()   # ... and some block after the first is muted
    assert max(r.v_max for r in run.refs) < 1 << 30


def test_extremes_v_near_2_to_the_30_and_both_rails(fmd):
    """A full-scale prototype over full-scale constant bytes puts channel 0's y at half of B_y in both components (bytes lie within
    128 of the centre, so the other half is out of reach).  At the smallest shifts B_y lies in (8192, 16384] and so does the bound
    on |u|: four taps of +16383 take v = 65532 y past 2^27 and every component of u past 2048, a = isqrt(ur^2 + ui^2) past 2896.  In
    AM mode at gain 65535 the loud blocks hit the upper rail and, once the input falls silent, a - dc the lower one."""
    N, hop, T, R, P = 16, 8, 64, 1, 16
    h = np.full(T, 2047, np.int16)
    gr = np.full(4, 16383, np.int16)
    run = Run(fmd, h, N, hop, gr, None, br.AM, R, P, squelch=0, gain=65535, channels=[0, 3])
    loud = np.full((1, 2 * hop * (T // hop + 3 * P)), 255, np.uint8)
    quiet = np.full((1, 2 * hop * 3 * P), 127, np.uint8)
    out = np.concatenate([run.call(loud), run.call(quiet)], axis=2)
    assert out.max() == 32767 and out.min() == -32768
    assert run.refs[0].v_max > 1 << 27 and run.refs[0].a_max > 2896


def test_call_sizes_and_refusals_at_r8(fmd):
    """Calls of T / hop + 3, 1, 37, 3000 and 2 hops at R = 8: the one-hop call completes a stage-one output but no audio sample --
    FMD_ERR_TOO_SHORT, and outputs(), levels() and the next call's result are what they would have been without it."""
    rng = np.random.default_rng(77)
    N, hop, T, S = 16, 8, 128, 2
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    gr, gi = _edge_taps(rng, 3, True)
    run = Run(fmd, h, N, hop, gr, gi, br.AM, 8, 64, squelch=0, S=S)
    fed = []
    for hops in (T // hop + 3, 1, 37, 3000, 2):
        data = _bytes(rng, S, 2 * hop * hops)
        m_before = run.refs[0].ch.m_next
        assert run.refs[0].ch.outputs_after(data.shape[1] // 2) > m_before     # every call completes stage-one outputs
        fed.append(run.call(data) is not None)
    assert fed[:4] == [True, False, True, True]
    for n in (2 * hop * 20 + 8, 2 * hop * 20 - 2, 8):
        before = run.snapshot()
        with pytest.raises(fmd.FmdError) as e:
            run.bank.run_batch(np.zeros((S, n), np.uint8))
        assert e.value.status == BAD_LENGTH and run.snapshot() == before
    assert run.call(_bytes(rng, S, 2 * hop * 50)) is not None


@pytest.mark.parametrize("mode,R", [(br.AM, 1), (br.FM, 3), (br.IQ, 8)])
def test_the_same_bytes_cut_differently_and_reset(fmd, mode, R):
    rng = np.random.default_rng(31 + R)
    N, hop, T, S, P = 16, 8, 128, 2, 16
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    gr, gi = _edge_taps(rng, 32, mode == br.IQ)
    total = 700
    data = _bytes(rng, S, 2 * hop * total)
    sq = _probe_squelch(h, N, hop, gr, gi, mode, R, P, None, data[0])
    run = Run(fmd, h, N, hop, gr, gi, mode, R, P, squelch=sq, S=S)
    whole = run.call(data)
    run.bank.reset()
    for r in run.refs:
        r.reset()
    assert run.snapshot() == (0, [[False] * N] * S, [[0] * N] * S)
    parts, at = [], 0
    for hops in (T // hop + 8 * R + 40, 1, 37, 2, 3 * R, total):
        hops = min(hops, total - at)
        p = run.call(data[:, 2 * hop * at:2 * hop * (at + hops)])
        at += hops
        if p is None:                                        # refused: its bytes never reached the handle, so the cut is void
            at -= hops
            continue
        parts.append(p)
    assert at == total and len(parts) >= 4
    assert np.array_equal(np.concatenate(parts, axis=2), whole)


@pytest.mark.parametrize("R,cplx", [(1, False), (4, True)])
def test_calls_that_end_one_before_on_and_one_after_the_tile(fmd, R, cplx):
    """Audio counts per row of kTile - 1, kTile and kTile + 1 (fmd_bp::kTile = 256), then again from wherever that left the blocks:
    blocks of 64 straddle calls and tiles."""
    rng = np.random.default_rng(500 + R)
    N, hop, T, S, P, Ta = 12, 8, 72, 2, 64, 9
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    gr, gi = _edge_taps(rng, Ta, cplx)
    probe = _bytes(rng, 1, 2 * hop * (T // hop + R * 800))[0]
    sq = _probe_squelch(h, N, hop, gr, gi, br.AM, R, P, [0, 5, 11], probe)
    run = Run(fmd, h, N, hop, gr, gi, br.AM, R, P, squelch=sq, channels=[0, 5, 11], S=S)
    for want in (K_TILE - 1, K_TILE, K_TILE + 1, 2 * K_TILE + 1, K_TILE - 1):
        hops = next(k for k in range(1, 4000) if run.refs[0].completes(2 * hop * k) == want)
        out = run.call(_bytes(rng, S, 2 * hop * hops))
        assert out is not None and out.shape[2] == want


@pytest.mark.parametrize("mode", [br.AM, br.IQ])
def test_device_path_odd_out_cap_and_two_byte_aligned_rows(fmd, mode):
    """run_device with an odd out_cap: in the int16 modes every other row starts 2 bytes off a dword, and d_out itself is given
    2 bytes off too; the sentinel beyond each row's outputs survives; a caller's stream."""
    import torch
    rng = np.random.default_rng(600 + mode)
    N, hop, T, S, R, P = 12, 8, 72, 3, 2, 16
    sel = [0, 5, 11]
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    gr, gi = _edge_taps(rng, 7, True)
    run = Run(fmd, h, N, hop, gr, gi, mode, R, P, squelch=0, channels=sel, S=S)
    bank, W = run.bank, run.bank.width
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    SENT = -12345
    off = 0 if mode == br.IQ else 1                          # int16 elements d_out is shifted by
    for hops in (700, 1, 131, 2 * K_TILE * R + 3):
        n = 2 * hop * hops
        data = _bytes(rng, S, n)
        buf = torch.zeros(S * n + 16, dtype=torch.uint8, device=dev)
        buf[4:4 + S * n] = torch.from_numpy(data.ravel()).to(dev)
        cap = bank.out_cap(n) + 7 - (bank.out_cap(n) % 2)
        assert cap % 2 == 1
        flat = torch.full((S * len(sel) * cap * W + 8,), SENT, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        before = run.snapshot()
        if run.refs[0].completes(n) < 1:
            with pytest.raises(fmd.FmdError) as e:
                bank.run_device(buf.data_ptr() + 4, n, flat.data_ptr() + 2 * off, cap, stream.cuda_stream)
            assert e.value.status == TOO_SHORT and run.snapshot() == before
            continue
        m = bank.run_device(buf.data_ptr() + 4, n, flat.data_ptr() + 2 * off, cap, stream.cuda_stream)
        bank.check()
        whole = flat.cpu().numpy()
        assert (whole[:off] == SENT).all() and (whole[off + S * len(sel) * cap * W:] == SENT).all()
        got = whole[off:off + S * len(sel) * cap * W].reshape(S, len(sel), cap, W)
        for s in range(S):
            exp = run.refs[s].feed(data[s])
            assert m == exp.shape[1] and np.array_equal(got[s, :, :m] if mode == br.IQ else got[s, :, :m, 0], exp), (hops, s)
            assert (got[s, :, m:] == SENT).all(), (hops, s)
        run.compare_state()
    with pytest.raises(fmd.FmdError) as e:                    # out_cap too small
        bank.run_device(buf.data_ptr() + 4, n, flat.data_ptr() + 2 * off, 10, stream.cuda_stream)
    assert e.value.status == CAPACITY
    torch.cuda.synchronize()


def test_levels_before_and_after_the_first_block(fmd):
    rng = np.random.default_rng(9)
    N, hop, T, S, R, P, Ta = 16, 8, 128, 2, 2, 64, 7
    h = rng.integers(-2047, 2048, T).astype(np.int16)
    gr, gi = _edge_taps(rng, Ta, False)
    run = Run(fmd, h, N, hop, gr, gi, br.FM, R, P, squelch=3, S=S)
    o, r = run.bank.levels()
    assert not o.any() and not r.any()
    hops = next(k for k in range(1, 4000) if run.refs[0].completes(2 * hop * k) == P - 1)
    assert run.call(_bytes(rng, S, 2 * hop * hops, quiet=False)) is not None
    o, r = run.bank.levels()
    assert not o.any() and not r.any()                       # 63 samples: no block yet
    assert run.call(_bytes(rng, S, 2 * hop * R, quiet=False)) is not None    # the sample that completes block 0
    o, r = run.bank.levels()
    assert run.refs[0].n_next == P and r.any() and np.array_equal(o, r >= 3)   # open_j: E_j >= 3^2 P, rms = isqrt(E_j / P)
    assert run.call(_bytes(rng, S, 2 * hop * R * (P + 9), quiet=False)) is not None
