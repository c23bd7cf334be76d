"""RDS bank (include/fmd.h, fmd_rds_*) on the MI355X across the whole documented domain: (ur, ui), outputs() and pilot(s, k)
against the test-side definition (tests/rds_ref.py), bit for bit, after every call.  The cases come from tests/domain_cases.py
(tests/test_domain_cases.py asserts without a GPU what each one reaches, and that each family tells a wrong variant of the
definition from the right one): every out_decim 1 ... 32 with tap counts on both sides of it, station counts on both sides of
every row-tile edge in both digit forms, baseband tiles down to 54 outputs and more than three of them in a call; tiles that stage
the most pairs the kernel can hold; calls of 1 ... Ta MPX samples; calls that end one sample before, on and after a pilot block edge,
a block open over several calls, several whole blocks in one call; taps, shifts and input at their limits; 512 streams and 131072
rows; the device path at a 4-byte offset on a caller's stream.  FMD_FUZZ_CASES / FMD_FUZZ_SEED scale and reseed the shape sweep.

Run time on one MI355X: a plain `pytest tests/test_gpu_rds_domain.py` with nothing else on the GPU took 5.5 s (17 tests); the
shape sweep is 2.4 s of that, no other test more than 0.4 s."""
import numpy as np
import pytest

import domain_cases as dc
import rds_ref as rr
import stereo_ref as st

pytestmark = pytest.mark.gpu

INVALID_ARG, TOO_SHORT, CAPACITY = -1, -3, -5


class Run:
    """One bank and the definition of the streams in `check`; call() feeds both and compares u, outputs() and pilot()."""

    def __init__(self, fmd, c, check=None):
        self.fmd, self.c = fmd, c
        self.bank = dc.rds_handle(c, fmd)
        self.refs = dc.rds_refs(c, rr, check)
        self.first = next(iter(self.refs.values()))

    def snapshot(self):
        return self.bank.outputs(), [self.bank.pilot(s, k) for s in self.refs for k in range(self.c.K)]

    def compare_state(self):
        assert self.bank.outputs() == self.first.n_next
        for s, r in self.refs.items():
            for k in range(self.c.K):
                assert self.bank.pilot(s, k) == r.pilot(k), (s, k)

    def call(self, data):
        """Returns u [S, K, n, 2], or None when the call is refused (and checks that it changed nothing)."""
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
    seen = set()
    for c in dc.rds_sweep():
        run = Run(fmd, c)
        fed = [run.call(d) is not None for d in dc.calls(c)]
        assert any(fed) and run.first.x[0].size > c.P, (c.i, c.sizes)
        seen.add((c.R, c.G, c.na < 256))
    assert {r for r, _, _ in seen} == set(range(1, 33)) and {g for _, g, _ in seen} == {2, 3, 4} and any(n for _, _, n in seen)


@pytest.mark.parametrize("R", [8, 16, 32])
def test_full_tiles(fmd, R):
    """R na + Ta == 1984: two calls of two tiles each whose last tile stages 1983 pairs, up to LDS slot 2043; the second reads the
    whole history the first one wrote."""
    c = dc.rds_full_tiles(R)
    run = Run(fmd, c)
    for d, m in zip(dc.calls(c), c.ends):
        assert run.call(d) is not None and run.first.x[0].size == m


@pytest.mark.parametrize("R", [1, 3, 32])
def test_short_calls(fmd, R):
    c = dc.rds_short(R)
    run = Run(fmd, c)
    for d, m in zip(dc.calls(c), c.ends):
        assert run.call(d) is not None and run.first.x[0].size == m


@pytest.mark.parametrize("P", [1024, 4096])
def test_block_edges(fmd, P):
    """MPX ends on j P - 1, j P, j P + 1; block 1 open over four calls, four whole blocks in one call, a call that starts on an
    edge; stations whose pilot comes and goes, so the report differs from call to call."""
    c = dc.rds_edges(P)
    run = Run(fmd, c)
    seen = set()
    for d, m in zip(dc.calls(c), c.ends):
        assert run.call(d) is not None and run.first.x[0].size == m
        seen.add(run.bank.pilot(0, 0))
    assert len(seen) >= 3 and {p for p, _ in seen} == {False, True}


def test_reset_in_the_middle_of_a_block(fmd):
    """After four calls of an edges case -- block 1 half filled, a carry and a filter history on the device -- reset() gives
    outputs() == 0 and no pilot report, and the case's bytes from the start give what a fresh handle gives."""
    c = dc.rds_edges(1024)
    run = Run(fmd, c)
    data = dc.calls(c)
    for d in data[:4]:
        assert run.call(d) is not None
    assert run.first.x[0].size % c.P and run.bank.pilot(0, 0)[1] > 0
    run.bank.reset()
    assert run.bank.outputs() == 0
    assert all(run.bank.pilot(s, k) == (False, 0) for s in range(c.S) for k in range(c.K))
    fresh = Run(fmd, c)
    for d in data[:7]:
        a, b = run.bank.run_batch(d), fresh.call(d)
        assert np.array_equal(a, b)
        assert run.snapshot() == fresh.snapshot()


@pytest.mark.parametrize("g,rds_shift", dc.RDS_EXTREMES)
def test_extremes(fmd, g, rds_shift):
    """sum |g| = 16383 in one tap of either sign (|v| reaches 16384 * 16383, the device output spans +-16383) and in 256 taps, at
    the smallest rds_shift and at 24 (u = -1 for every small negative v)."""
    c = dc.rds_extreme(g, rds_shift)
    run = Run(fmd, c)
    out = np.concatenate([run.call(d) for d in dc.calls(c)], axis=2)
    if c.Ta == 1:
        assert run.first.v_max == 16384 * 16383 and out.min() == -16383 and out.max() == 16383
    if rds_shift == 24:
        assert set(np.unique(out).tolist()) == {-1, 0}


def test_512_streams(fmd):
    rng = np.random.default_rng(4606)
    S, n, K = 512, 262144, 2
    h = st.lowpass(64, 130000 / 2400000)
    g = dc.audio_taps(rng, 127, 16000)
    c = dc.NS(K=K, D=10, T=64, Ta=127, R=5, S=S, h=h, incs=dc.incs(rng, S, K), P=4096, rate=2400000, pilot_min=1, g=g,
              rds_shift=dc.rds_shift_for(g))
    c.shift = dc.shift_for(h, c.incs, 256)
    run = Run(fmd, c, check=(0, 1, 255, 256, 510, 511))
    for _ in range(2):
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8)) is not None


def test_131072_rows(fmd):
    """4096 streams x 32 stations, small calls: the baseband kernel's grid is nt2 * S * K workgroups in x."""
    rng = np.random.default_rng(4707)
    S, K = 4096, 32
    h = np.array([100, -127, 90], np.int16)
    ii = dc.incs(rng, S, K)
    g = np.array([9000, -7383], np.int16)
    c = dc.NS(K=K, D=2, T=3, Ta=2, R=1, S=S, h=h, incs=ii, P=1024, rate=250000, pilot_min=1, g=g, rds_shift=dc.rds_shift_for(g),
              shift=dc.shift_for(h, ii[:8], 16384) + 1)
    run = Run(fmd, c, check=(0, 1, 2047, 2048, 4094, 4095))
    for n in (8 * 16, 8 * 9, 8 * 300):                             # 600 outputs: three tiles per row
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8)) is not None


def test_device_path_unaligned_padded_on_a_callers_stream(fmd):
    """d_iq 4 bytes past an aligned address with nbytes % 16 == 8 (no row is 16-byte aligned), out_cap padded with a sentinel that
    must survive in every row's padding and after the whole buffer, on a caller's stream; d_out 2 bytes off and an out_cap one
    below the call's outputs are refused and change nothing."""
    import torch
    rng = np.random.default_rng(4808)
    S, K, D, T = 3, 6, 6, 59
    h, ii = dc.front(rng, T, S, K, 2)
    g = dc.audio_taps(rng, 63)
    c = dc.NS(K=K, D=D, T=T, Ta=63, R=5, S=S, h=h, incs=ii, P=1024, rate=125000 * D, pilot_min=1, g=g, rds_shift=dc.rds_shift_for(g),
              shift=dc.shift_for(h, ii, 2048))
    run = Run(fmd, c)
    bank, refs = run.bank, run.refs
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    SENT = -12345
    accepted = 0
    for n in (8 * 1001, 8 * 7, 8 * 2403, 8 * 3, 8 * 1501):
        assert n % 16 == 8
        data = dc.bytes_(rng, S, n)
        buf = torch.zeros(S * n + 16, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        buf[4:4 + S * n] = torch.from_numpy(data.ravel()).to(dev)
        cap = bank.out_cap(n) + 37
        flat = torch.full((S * K * cap * 2 + 8,), SENT, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        before = run.snapshot()
        with pytest.raises(fmd.FmdError) as e:                     # (ur, ui) pairs are stored as dwords
            bank.run_device(buf.data_ptr() + 4, n, flat.data_ptr() + 2, cap, stream.cuda_stream)
        assert e.value.status == INVALID_ARG and run.snapshot() == before
        want = refs[0].completes(n)
        if want < 1:
            with pytest.raises(fmd.FmdError) as e:
                bank.run_device(buf.data_ptr() + 4, n, flat.data_ptr(), cap, stream.cuda_stream)
            assert e.value.status == TOO_SHORT and run.snapshot() == before
            continue
        with pytest.raises(fmd.FmdError) as e:
            bank.run_device(buf.data_ptr() + 4, n, flat.data_ptr(), want - 1, stream.cuda_stream)
        assert e.value.status == CAPACITY and run.snapshot() == before
        torch.cuda.synchronize()
        assert (flat == SENT).all()                                # no refused call wrote anything
        m = bank.run_device(buf.data_ptr() + 4, n, flat.data_ptr(), cap, stream.cuda_stream)
        bank.check()
        whole = flat.cpu().numpy()
        assert (whole[S * K * cap * 2:] == SENT).all()
        got = whole[:S * K * cap * 2].reshape(S, K, cap, 2)
        for s in range(S):
            exp = refs[s].feed(data[s])
            assert m == want == exp.shape[1] and np.array_equal(got[s, :, :m], exp), (n, s)
            assert (got[s, :, m:] == SENT).all(), (n, s)
        run.compare_state()
        accepted += 1
    assert accepted >= 3
