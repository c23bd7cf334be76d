"""FM receiver bank (include/fmd.h, fmd_receiver_*) on the MI355X across the whole documented domain: (L, R), (ur, ui), outputs()
and pilot(s, k) against the test-side definition (tests/receiver_ref.py), bit for bit, after every call; a call that the definition
refuses must be refused with FMD_ERR_TOO_SHORT and change nothing.  The cases come from tests/domain_cases.py
(tests/test_domain_cases.py asserts without a GPU what each one reaches) and aim at what the receiver adds to the two banks it
combines -- one grid that holds the tiles of both second stages, the block carry written by the audio side alone, a call plan over two
stages, two outputs in one staging buffer: every audio stride 1 ... 32 against a different RDS stride 1 ... 32, with several tiles on
one side, on the other and on both (different counts, odd row counts); full tiles on both sides at once; calls of 1 ... Ta multiplex
samples behind refused calls that complete audio only, RDS only or neither; calls that end one sample before, on and after a pilot
block edge, a block open over several calls, pilots that come and go; the pilot threshold at exact equality; taps, shifts and input
at their limits; a staging buffer that grows, with the audio part no multiple of 256 bytes; 65535 streams and 131072 rows; the
device path at a 4-byte offset on a caller's stream.  FMD_FUZZ_CASES / FMD_FUZZ_SEED scale and reseed the shape sweep.

Run time on one MI355X: `pytest -m gpu` took 391 s (713 tests) with this file and 386 s (697 tests) without it; the file's 16 tests
are 4.8 s of that, the shape sweep 3.3 s, no other test more than 0.4 s.  In the same run tests/test_gpu_stereo_domain.py took 3.3 s
and tests/test_gpu_rds_domain.py 3.1 s, 6.4 s together."""
import copy

import numpy as np
import pytest

import domain_cases as dc
import receiver_ref as rxr

pytestmark = pytest.mark.gpu

INVALID_ARG, TOO_SHORT, CAPACITY = -1, -3, -5


class Run:
    """One bank and the definition of the streams in `check`; call() feeds both and compares audio, baseband, outputs() and
    pilot()."""

    def __init__(self, fmd, c, check=None, pilot_min=None):
        if pilot_min is not None:
            c = copy.copy(c)
            c.pilot_min = pilot_min
        self.fmd, self.c = fmd, c
        self.bank = dc.receiver_handle(c, fmd)
        self.refs = dc.receiver_refs(c, rxr, check)
        self.first = next(iter(self.refs.values()))

    def mpx(self):
        """Multiplex samples since creation, by the definition."""
        return self.first.stereo.x[0].size

    def snapshot(self):
        return self.bank.outputs(), [self.bank.pilot(s, k) for s in self.refs for k in range(self.c.K)]

    def compare_state(self):
        assert self.bank.outputs() == self.first.outputs()
        for s, r in self.refs.items():
            for k in range(self.c.K):
                assert self.bank.pilot(s, k) == r.pilot(k), (s, k)

    def refused(self, fn):
        before = self.snapshot()
        with pytest.raises(self.fmd.FmdError) as e:
            fn()
        assert self.snapshot() == before
        return e.value.status

    def call(self, data):
        """Returns (audio [S, K, na, 2], rds [S, K, nr, 2]), or None when the call is refused (and checks that it changed nothing)."""
        n = data.shape[1]
        if min(self.first.completes(n)) < 1:
            assert self.refused(lambda: self.bank.run_batch(data)) == TOO_SHORT
            return None
        a, u = self.bank.run_batch(data)
        assert a.dtype == np.int16 and u.dtype == np.int16
        for s, r in self.refs.items():
            ea, eu = r.feed(data[s])
            assert a.shape[1:] == (self.c.K, ea.shape[1], 2) and np.array_equal(a[s], ea), (s, n, "audio")
            assert u.shape[1:] == (self.c.K, eu.shape[1], 2) and np.array_equal(u[s], eu), (s, n, "rds")
        caps = self.bank.out_caps(n)
        assert a.shape[2] <= caps[0] and u.shape[2] <= caps[1], (n, caps)
        self.compare_state()
        return a, u


def test_shape_sweep(fmd):
    seen, tiles = set(), set()
    for c in dc.receiver_sweep():
        run = Run(fmd, c)
        fed = [run.call(d) for d in dc.calls(c)]
        assert any(f is None for f in fed) and any(f is not None for f in fed) and run.mpx() > c.P, (c.i, c.sizes)
        seen.add((c.Ra, c.Rr, c.G, c.na_a < 256, c.na_r < 256))
        tiles |= {(-(-a.shape[2] // c.na_a) > 1, -(-u.shape[2] // c.na_r) > 1) for a, u in (f for f in fed if f is not None)}
    assert {x[0] for x in seen} == set(range(1, 33)) == {x[1] for x in seen} and {x[2] for x in seen} == {2, 3, 4}
    assert any(x[3] for x in seen) and any(x[4] for x in seen) and len(tiles) == 4


def test_full_tiles(fmd):
    """R na + 2 Ta == 2048 on the audio side and R na + Ta == 1984 on the RDS side in one grid: two calls of 9 and 8 full tiles per
    row whose last tiles stage the most pairs either side can hold; the second reads the whole history the first one wrote."""
    c = dc.receiver_full_tiles()
    run = Run(fmd, c)
    for d, m in zip(dc.calls(c), c.ends):
        assert run.call(d) is not None and run.mpx() == m


@pytest.mark.parametrize("Ra,Rr", dc.RX_SHORT)
def test_short_calls(fmd, Ra, Rr):
    """Accepted calls of 1, 2 and Ta - 2 ... Ta multiplex samples; before them refused calls that complete an output of one stage
    only, or of neither, whose bytes come again as the head of the next call."""
    c = dc.receiver_short(Ra, Rr)
    run = Run(fmd, c)
    fed = [run.call(d) is not None for d in dc.calls(c)]
    assert [i for i, f in enumerate(fed) if not f] == [i for i, _ in c.refused] and fed[-1]
    assert run.mpx() == c.mcalls[-1][1]


@pytest.mark.parametrize("P", [1024, 4096])
def test_block_edges(fmd, P):
    """Multiplex ends on j P - 1, j P, j P + 1; block 1 open over four calls, four whole blocks in one call, a call that starts on
    an edge; stations whose pilot comes and goes, so that the block carry -- written by the audio side of the grid alone -- and
    the report differ from call to call."""
    c = dc.receiver_edges(P)
    run = Run(fmd, c)
    seen = set()
    for d, m in zip(dc.calls(c), c.ends):
        assert run.call(d) is not None and run.mpx() == m
        seen.add(run.bank.pilot(0, 0))
    assert len(seen) >= 3 and {p for p, _ in seen} == {False, True} and run.first.stereo.kc_max > 0


def test_pilot_threshold_at_exact_equality(fmd):
    """dc.stereo_threshold's bytes: block 0 has I = 2^26, Q = 0, the threshold of pilot_min 8 exactly.  Block 0 is present at
    pilot_min 7 and 8 and absent at 9, the audio over block 1 is stereo or mono accordingly, and the baseband is the same in the
    three runs: presence does not reach the RDS side."""
    c = dc.receiver_threshold()
    mono, base = {}, {}
    for pm in (8, 7, 9):
        run = Run(fmd, c, pilot_min=pm)
        outs = [run.call(d) for d in dc.calls(c)]
        I, Q = run.first.stereo.block_iq(0, 0)
        assert I * I + Q * Q == (8 * c.P * 8192) ** 2
        a = np.concatenate([o[0] for o in outs], axis=2)[0, 0, :2 * c.P - c.Ta_a + 1]
        mono[pm] = bool(np.array_equal(a[:, 0], a[:, 1]))
        base[pm] = np.concatenate([o[1] for o in outs], axis=2)
    assert mono == {7: False, 8: False, 9: True}
    assert np.array_equal(base[7], base[8]) and np.array_equal(base[8], base[9]) and base[8].any()


@pytest.mark.parametrize("which", dc.RX_EXTREMES)
def test_extremes(fmd, which):
    """Taps with sum |g| = 16383 on both sides, audio_shift 0, the smallest rds_shift and 24, the front-end shift at its limit,
    bytes at the rails: L and R reach both rails; the one-tap baseband spans +-16383; at rds_shift 24 only the sign is left."""
    c = dc.receiver_extreme(which)
    run = Run(fmd, c)
    outs = [run.call(d) for d in dc.calls(c)]
    a, u = (np.concatenate([o[j] for o in outs], axis=2) for j in (0, 1))
    for ch in (0, 1):
        assert a[..., ch].min() == -32768 and a[..., ch].max() == 32767
    if which == "stereo":
        assert run.first.stereo.kc_max >= 32000 and run.first.stereo.corr_max > (1 << 23)
    if which == "rds-plus":
        assert run.first.rds.v_max == 16384 * 16383 and u.min() == -16383 and u.max() == 16383
    if which == "rds-256":
        assert set(np.unique(u).tolist()) == {-1, 0}


@pytest.mark.parametrize("K", [1, 3])
def test_staging_layout(fmd, K):
    """run_batch lays both outputs in one staging buffer, the baseband behind the audio at the next 256-byte boundary.  One stream
    and an odd station count, so that the audio part -- 4 rows out_caps(n)[0] bytes -- is no multiple of 256 in any call; every call
    is larger than the one before, so the buffer grows each time, and a smaller one follows.  The audio stage runs at stride 1 from
    whole output counts, so the last audio row is full to its capacity or one short of it: a baseband that started below the
    boundary would overlap audio that is compared."""
    rng = np.random.default_rng(7707 + K)
    D = 2
    h, ii = dc.front(rng, 3, 1, K, 2)
    gr = dc.audio_taps(rng, 3)
    c = dc.NS(K=K, D=D, T=3, S=1, h=h, incs=ii, P=1024, rate=125000 * D, pilot_min=1, ga=dc.audio_taps(rng, 2), Ra=1, Ta_a=2, gr=gr, Rr=2,
              Ta_r=3, audio_shift=5, rds_shift=dc.rds_shift_for(gr), shift=dc.shift_for(h, ii, 2048))
    run = Run(fmd, c)
    pads, exposed = set(), 0
    sizes = [8 * 21, 8 * 37, 8 * 75, 8 * 139, 8 * 301, 8 * 11]
    assert all(b > a for a, b in zip(sizes[:-2], sizes[1:-1])) and sizes[-1] < sizes[0]
    for n in sizes:
        cap = run.bank.out_caps(n)[0]
        a_bytes = 4 * c.S * K * cap
        a, u = run.call(dc.bytes_(rng, 1, n))
        pads.add(a_bytes % 256)
        exposed += a_bytes % 256 > 4 * (cap - a.shape[2])           # the boundary rounded DOWN lies inside the last row's outputs
    assert 0 not in pads and len(pads) >= 3 and exposed >= 3, (pads, exposed)


def test_65535_streams(fmd):
    """The grid-y limit of the first pass: 65535 streams of small calls, one station, the smallest tap counts, both sides in the
    second pass's grid.  Compares the listed streams only: the ends, the powers of two inside and seven random ones."""
    rng = np.random.default_rng(7808)
    S = 65535
    h = np.array([2047, -1000], np.int16)
    ii = rng.integers(0, 1 << 32, (S, 1), dtype=np.uint64).astype(np.uint32)
    gr = np.array([9000, -7383], np.int16)
    c = dc.NS(K=1, D=2, T=2, S=S, h=h, incs=ii, P=1024, rate=250000, pilot_min=1, ga=np.array([16383], np.int16), Ra=1, Ta_a=1, gr=gr, Rr=2,
              Ta_r=2, audio_shift=3, rds_shift=dc.rds_shift_for(gr), shift=dc.shift_for(h, ii[:64], 16384) + 1)
    check = [0, 1, 2, 4095, 4096, 32767, 32768, 65533, 65534] + [int(x) for x in rng.integers(0, S, 7)]
    run = Run(fmd, c, check=check)
    for n in (8 * 40, 8 * 13, 8 * 300):
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8)) is not None


def test_131072_rows_in_the_second_pass(fmd):
    """4096 streams x 32 stations, small calls, both stages at stride 1 with 2 taps: the last call has three tiles per row on each
    side, so the one grid holds 6 * 131072 workgroups and splits at 3 * 131072.  Compares streams 0, 1, 2047, 2048, 4094 and 4095
    only."""
    rng = np.random.default_rng(7909)
    S, K = 4096, 32
    h = np.array([100, -127, 90], np.int16)
    ii = dc.incs(rng, S, K)
    gr = np.array([-8000, 8383], np.int16)
    c = dc.NS(K=K, D=2, T=3, S=S, h=h, incs=ii, P=1024, rate=250000, pilot_min=1, ga=np.array([9000, -7383], np.int16), Ra=1, Ta_a=2,
              gr=gr, Rr=1, Ta_r=2, audio_shift=2, rds_shift=dc.rds_shift_for(gr), shift=dc.shift_for(h, ii[:8], 16384) + 1)
    run = Run(fmd, c, check=(0, 1, 2047, 2048, 4094, 4095))
    for n in (8 * 16, 8 * 9, 8 * 300):                             # 600 outputs of each stage: three tiles per row on each side
        a, u = run.call(rng.integers(0, 256, (S, n), dtype=np.uint8))
    assert -(-a.shape[2] // 256) == 3 == -(-u.shape[2] // 256)


def test_device_path_unaligned_padded_on_a_callers_stream(fmd):
    """d_iq 4 bytes past an aligned address with nbytes % 16 == 8 (no row is 16-byte aligned), both capacities padded with a sentinel
    that must survive in every row's padding and after either buffer, on a caller's stream; d_audio 2 bytes off, d_rds 2 bytes off
    and a capacity one below the call's outputs on either side are refused and change nothing, and so is a call that completes an
    output of one stage only."""
    import torch
    rng = np.random.default_rng(8010)
    S, K, D, T = 3, 6, 6, 59
    h, ii = dc.front(rng, T, S, K, 2)
    gr = dc.audio_taps(rng, 63)
    c = dc.NS(K=K, D=D, T=T, S=S, h=h, incs=ii, P=1024, rate=125000 * D, pilot_min=1, ga=dc.audio_taps(rng, 63), Ra=5, Ta_a=63, gr=gr, Rr=7,
              Ta_r=63, audio_shift=8, rds_shift=dc.rds_shift_for(gr), shift=dc.shift_for(h, ii, 2048))
    run = Run(fmd, c)
    bank, refs = run.bank, run.refs
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    SENT = -12345
    accepted, short = 0, set()
    for n in (8 * 1001, 8 * 7, 8 * 2403, 8 * 3, 8 * 1501, 8 * 13):
        assert n % 16 == 8
        data = dc.bytes_(rng, S, n)
        buf = torch.zeros(S * n + 16, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        buf[4:4 + S * n] = torch.from_numpy(data.ravel()).to(dev)
        ca, cr = (x + 37 for x in bank.out_caps(n))
        fa = torch.full((S * K * ca * 2 + 8,), SENT, dtype=torch.int16, device=dev)
        fr = torch.full((S * K * cr * 2 + 8,), SENT, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        iq, pa, pr, st = buf.data_ptr() + 4, fa.data_ptr(), fr.data_ptr(), stream.cuda_stream
        # (L, R) and (ur, ui) pairs are stored as dwords
        assert run.refused(lambda: bank.run_device(iq, n, pa + 2, ca, pr, cr, st)) == INVALID_ARG
        assert run.refused(lambda: bank.run_device(iq, n, pa, ca, pr + 2, cr, st)) == INVALID_ARG
        wa, wr = refs[0].completes(n)
        if min(wa, wr) < 1:
            assert run.refused(lambda: bank.run_device(iq, n, pa, ca, pr, cr, st)) == TOO_SHORT
            short.add((wa >= 1, wr >= 1))
            continue
        assert run.refused(lambda: bank.run_device(iq, n, pa, wa - 1, pr, cr, st)) == CAPACITY
        assert run.refused(lambda: bank.run_device(iq, n, pa, ca, pr, wr - 1, st)) == CAPACITY
        torch.cuda.synchronize()
        assert (fa == SENT).all() and (fr == SENT).all()           # no refused call wrote anything
        na, nr = bank.run_device(iq, n, pa, ca, pr, cr, st)
        bank.check()
        assert (na, nr) == (wa, wr)
        exp = [refs[s].feed(data[s]) for s in range(S)]
        for j, (flat, cap, m) in enumerate(((fa, ca, na), (fr, cr, nr))):
            whole = flat.cpu().numpy()
            assert (whole[S * K * cap * 2:] == SENT).all()
            got = whole[:S * K * cap * 2].reshape(S, K, cap, 2)
            for s in range(S):
                assert m == exp[s][j].shape[1] and np.array_equal(got[s, :, :m], exp[s][j]), (n, s, j)
                assert (got[s, :, m:] == SENT).all(), (n, s, j)
        run.compare_state()
        accepted += 1
    assert accepted >= 3 and (True, False) in short and len(short) >= 2, short
