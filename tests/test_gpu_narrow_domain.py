"""Narrow-band bank (include/fmd.h, fmd_narrow_*) on the MI355X across the whole documented domain: the output, outputs() and
level(s, k) against the test-side definition (tests/narrow_ref.py), bit for bit, after every call.  The cases come from
tests/domain_cases.py (tests/test_domain_cases.py asserts without a GPU what each one reaches): every chan_decim 1 ... 32 with tap
counts that give ceil(Ta / R) mod 4 = 0, 1, 2, 3, below R and 256, all modes with real and complex taps, station counts on both
sides of every row-tile edge in both digit forms, first-pass tiles of 256, 192 and 128 outputs, second-pass tiles below 256
samples; audio ends one sample before, on and after a block edge with the squelch toggling inside a tile and across calls and the
AM dc carried over a call boundary; calls of 1 ... Ta inputs; the squelch threshold at exact equality; gain and magnitude at their
limits; 65535 streams and 131072 rows; the device path at a 4-byte offset.  FMD_FUZZ_SEED reseeds the shape sweep."""
import copy

import numpy as np
import pytest

import domain_cases as dc
import narrow_ref as nr

pytestmark = pytest.mark.gpu

INVALID_ARG, TOO_SHORT = -1, -3


class Run:
    """One bank and the definition of the streams in `check`; call() feeds both and compares the output, outputs() and level()."""

    def __init__(self, fmd, c, check=None, squelch=None):
        if squelch is not None:
            c = copy.copy(c)
            c.squelch = squelch
        self.fmd, self.c = fmd, c
        self.bank = dc.narrow_handle(c, fmd)
        self.refs = dc.narrow_refs(c, nr, check)
        self.first = next(iter(self.refs.values()))

    def snapshot(self):
        return self.bank.outputs(), [self.bank.level(s, k) for s in self.refs for k in range(self.c.K)]

    def compare_state(self):
        assert self.bank.outputs() == self.first.n_next
        for s, r in self.refs.items():
            for k in range(self.c.K):
                assert self.bank.level(s, k) == r.level(k), (s, k)

    def call(self, data):
        """Returns the output [S, K, n(, 2)], or None when the call is refused (and checks that it changed nothing)."""
        if self.first.completes(data.shape[1]) < 1:
            before = self.snapshot()
            with pytest.raises(self.fmd.FmdError) as e:
                self.bank.run_batch(data)
            assert e.value.status == TOO_SHORT and self.snapshot() == before
            return None
        got = self.bank.run_batch(data)
        for s, r in self.refs.items():
            exp = r.feed(data[s])
            assert got.shape[2] == exp.shape[1] and np.array_equal(got[s], exp), (s, data.shape[1])
        self.compare_state()
        return got


def test_shape_sweep(fmd):
    seen, residues = set(), set()
    for c in dc.narrow_sweep():
        datas = dc.calls(c)
        if c.use_squelch:
            c.squelch = dc.probe_squelch(c, nr, np.concatenate([d[0] for d in datas[1:]]))
        run = Run(fmd, c)
        fed = [run.call(d) is not None for d in datas]
        assert any(fed), (c.i, c.sizes)
        seen.add((c.G, c.na < 256, c.mode, c.cplx))
        residues.add((c.R, -(-c.Ta // c.R) % 4))
    assert residues == {(r, q) for r in range(1, 33) for q in range(4)}
    assert {g for g, _, _, _ in seen} == {2, 3, 4} and any(n for _, n, _, _ in seen)


@pytest.mark.parametrize("P,mode", [(16, nr.AM), (16, nr.FM), (4096, nr.AM), (4096, nr.IQ)])
def test_block_edges(fmd, P, mode):
    """Audio ends on j P - 1, j P, j P + 1; block 16 puts 17 blocks into a tile, block 4096 keeps one block open over many calls;
    the squelch sits between the loud and the quiet block energy, so `open` changes inside tiles and between calls; in AM mode the
    dc of the block before is applied to a call that starts on an edge."""
    c = dc.narrow_edges(P, mode)
    c.squelch = dc.probe_squelch(c, nr, c.data[0])
    run = Run(fmd, c)
    levels = set()
    for d, n in zip(dc.calls(c), c.ends):
        assert run.call(d) is not None and run.first.n_next == n
        levels.add(run.first.level(0)[0])
    assert levels == {True, False}


@pytest.mark.parametrize("R", [1, 5])
def test_short_calls(fmd, R):
    c = dc.narrow_short(R)
    run = Run(fmd, c)
    for d, m in zip(dc.calls(c), c.ends):
        assert run.call(d) is not None and run.first.y[0].shape[0] == m


@pytest.mark.parametrize("mode", [nr.IQ, nr.AM])
def test_squelch_threshold_at_exact_equality(fmd, mode):
    """Blocks with E = squelch^2 P exactly (|u|^2 = 25 per sample, squelch 5, block 16), E - 1 and E + 1: equality opens.  The same
    bytes at squelch 4 (all three open) and 6 (none does)."""
    c = dc.narrow_threshold(mode)
    for sq, want in ((5, c.want_open), (4, [True] * len(c.kinds)), (6, [False] * len(c.kinds))):
        run = Run(fmd, c, squelch=sq)
        for d in dc.calls(c):
            assert run.call(d) is not None
        E = [run.first.block(0, j)[0] for j in range(len(c.kinds))]
        assert E == [400 + kd for kd in c.kinds]
        assert [run.first.estimate(0, j)[0] for j in range(len(c.kinds))] == want


def test_extremes_fm_gain_and_am_magnitude(fmd):
    """FM at gain 65535 over |u| up to the bound's half, where the discriminator's products wrap: the output reaches both rails.
    AM with both components of u at their largest together: a = isqrt(ur^2 + ui^2) reaches sqrt 2 * 8187 (bytes lie within 128 of
    the centre, so a component of y reaches half of the bound that the shifts are sized for, and 23170 itself is out of reach)."""
    for mode in (nr.FM, nr.AM):
        c = dc.narrow_extreme(mode)
        run = Run(fmd, c)
        out = np.concatenate([run.call(d) for d in dc.calls(c)], axis=2)
        assert out.min() == -32768 and out.max() == 32767
        assert run.first.v_max > (1 << 28) and (mode == nr.FM or run.first.a_max >= 11500)


def test_65535_streams(fmd):
    rng = np.random.default_rng(2707)
    S = 65535
    h = np.array([2047, -1000], np.int16)
    ii = rng.integers(0, 1 << 32, (S, 1), dtype=np.uint64).astype(np.uint32)
    gr = np.array([300, -200], np.int16)
    shift = dc.shift_for(h, ii, 16384)
    c = dc.NS(K=1, D=2, T=2, Ta=2, R=3, S=S, h=h, incs=ii, P=16, mode=nr.AM, gr=gr, gi=None, shift=shift,
              chan_shift=dc.chan_shift_for(h, ii, shift, gr, None, 16384), gain=700, squelch=0)
    check = [0, 1, 2, 4095, 4096, 32767, 32768, 65533, 65534] + [int(x) for x in rng.integers(0, S, 7)]
    run = Run(fmd, c, check=check)
    for n in (8 * 40, 8 * 13, 8 * 300):
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8)) is not None


def test_131072_rows_in_the_second_pass(fmd):
    rng = np.random.default_rng(2808)
    S, K = 4096, 32
    h = np.array([100, -127, 90], np.int16)
    ii = dc.incs(rng, S, K)
    gr, gi = np.array([900, -700, 30], np.int16), np.array([-5, 400, 800], np.int16)
    shift = dc.shift_for(h, ii, 16384)
    c = dc.NS(K=K, D=2, T=3, Ta=3, R=2, S=S, h=h, incs=ii, P=16, mode=nr.IQ, gr=gr, gi=gi, shift=shift,
              chan_shift=dc.chan_shift_for(h, ii, shift, gr, gi, 16384), gain=256, squelch=0)
    run = Run(fmd, c, check=(0, 1, 2047, 2048, 4094, 4095))
    for n in (8 * 16, 8 * 9, 8 * 300):
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8)) is not None


@pytest.mark.parametrize("mode", [nr.IQ, nr.SSB])
def test_device_path_unaligned_padded_on_a_callers_stream(fmd, mode):
    """d_iq 4 bytes past an aligned address with nbytes % 16 == 8 (the register staging path), out_cap padded with a sentinel that
    must survive, on a caller's stream; in IQ mode d_out 2 bytes off is refused and changes nothing."""
    import torch
    rng = np.random.default_rng(2909 + mode)
    S, K, D, T = 3, 6, 6, 59
    h, ii = dc.front(rng, T, S, K, 2)
    gr, gi = dc.chan_taps(rng, 63, True)
    shift = dc.shift_for(h, ii, 16384)
    c = dc.NS(K=K, D=D, T=T, Ta=63, R=5, S=S, h=h, incs=ii, P=64, mode=mode, gr=gr, gi=gi, shift=shift,
              chan_shift=dc.chan_shift_for(h, ii, shift, gr, gi, 16384), gain=500, squelch=0)
    run = Run(fmd, c)
    bank, refs, W = run.bank, run.refs, run.bank.width
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    SENT = -12345
    for n in (8 * 1001, 8 * 7, 8 * 2403, 8 * 3, 8 * 1501):
        data = dc.bytes_(rng, S, n)
        buf = torch.zeros(S * n + 16, dtype=torch.uint8, device=dev)
        buf[4:4 + S * n] = torch.from_numpy(data.ravel()).to(dev)
        cap = bank.out_cap(n) + 37
        flat = torch.full((S * K * cap * W + 8,), SENT, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        before = run.snapshot()
        if mode == nr.IQ:                                          # (re, im) pairs are stored as dwords
            with pytest.raises(fmd.FmdError) as e:
                bank.run_device(buf.data_ptr() + 4, n, flat.data_ptr() + 2, cap, stream.cuda_stream)
            assert e.value.status == INVALID_ARG and run.snapshot() == before
        if refs[0].completes(n) < 1:
            with pytest.raises(fmd.FmdError) as e:
                bank.run_device(buf.data_ptr() + 4, n, flat.data_ptr(), cap, stream.cuda_stream)
            assert e.value.status == TOO_SHORT and run.snapshot() == before
            continue
        m = bank.run_device(buf.data_ptr() + 4, n, flat.data_ptr(), cap, stream.cuda_stream)
        bank.check()
        whole = flat.cpu().numpy()
        assert (whole[S * K * cap * W:] == SENT).all()
        got = whole[:S * K * cap * W].reshape(S, K, cap, W)
        for s in range(S):
            exp = refs[s].feed(data[s])
            assert m == exp.shape[1] and np.array_equal(got[s, :, :m] if mode == nr.IQ else got[s, :, :m, 0], exp), (n, s)
            assert (got[s, :, m:] == SENT).all(), (n, s)
        run.compare_state()
