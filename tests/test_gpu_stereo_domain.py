"""Stereo station bank (include/fmd.h, fmd_stereo_*) on the MI355X across the whole documented domain: (L, R), outputs() and
pilot(s, k) against the test-side definition (tests/stereo_ref.py), bit for bit, after every call.  The cases come from
tests/domain_cases.py (tests/test_domain_cases.py asserts without a GPU what each one reaches): every audio_decim 1 ... 32 with
audio tap counts on both sides of it, station counts on both sides of every row-tile edge in both digit forms, first-pass tiles of
255, 191 and 127 outputs, audio tiles down to 48 samples; calls that end one sample before, on and after a block edge, a block
open over several calls, several whole blocks in one call; calls of 1 ... Ta MPX samples; the pilot threshold at exact equality;
taps, shifts and input at their limits; 512 and 65535 streams and 131072 rows; the device path at a 4-byte offset on a caller's
stream.  FMD_FUZZ_CASES / FMD_FUZZ_SEED scale and reseed the shape sweep.

Run time on one MI355X: `pytest -m gpu` took 354 s (399 tests) without the three *_domain files of the stereo bank, the
narrow-band bank and the channelizer; those three add 18 s (29 tests), 372 s in all."""
import copy

import numpy as np
import pytest

import domain_cases as dc
import stations_ref as sr
import stereo_ref as st

pytestmark = pytest.mark.gpu

INVALID_ARG, TOO_SHORT = -1, -3


class Run:
    """One bank and the definition of the streams in `check`; call() feeds both and compares audio, outputs() and pilot()."""

    def __init__(self, fmd, c, check=None, pilot_min=None):
        if pilot_min is not None:
            c = copy.copy(c)
            c.pilot_min = pilot_min
        self.fmd, self.c = fmd, c
        self.bank = dc.stereo_handle(c, fmd)
        self.refs = dc.stereo_refs(c, st, check)
        self.first = next(iter(self.refs.values()))

    def snapshot(self):
        return self.bank.outputs(), [self.bank.pilot(s, k) for s in self.refs for k in range(self.c.K)]

    def compare_state(self):
        assert self.bank.outputs() == self.first.n_next
        for s, r in self.refs.items():
            for k in range(self.c.K):
                assert self.bank.pilot(s, k) == r.pilot(k), (s, k)

    def call(self, data):
        """Returns the audio [S, K, n, 2], or None when the call is refused (and checks that it changed nothing)."""
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
    for c in dc.stereo_sweep():
        run = Run(fmd, c)
        fed = [run.call(d) is not None for d in dc.calls(c)]
        assert any(fed) and run.first.x[0].size > c.P, (c.i, c.sizes)
        seen.add((c.R, c.G, c.na < 256))
    assert {r for r, _, _ in seen} == set(range(1, 33)) and {g for _, g, _ in seen} == {2, 3, 4} and any(n for _, _, n in seen)


@pytest.mark.parametrize("P", [1024, 4096])
def test_block_edges(fmd, P):
    """MPX ends on j P - 1, j P, j P + 1 (byte counts from st_mpx: m outputs exist after T + (m - 1) D samples); block 1 open over
    four calls, four whole blocks in one call, a call that starts on an edge, first-pass tiles with an edge after their first and
    before their last column."""
    c = dc.stereo_edges(P)
    run = Run(fmd, c)
    for d, m in zip(dc.calls(c), c.ends):
        assert run.call(d) is not None and run.first.x[0].size == m
    assert dc.straddles(c) == (True, True) and run.first.kc_max > 0


@pytest.mark.parametrize("R", [1, 3])
def test_short_calls(fmd, R):
    c = dc.stereo_short(R)
    run = Run(fmd, c)
    for d, m in zip(dc.calls(c), c.ends):
        assert run.call(d) is not None and run.first.x[0].size == m


def test_pilot_threshold_at_exact_equality(fmd):
    """Exact equality is reachable through bytes (dc.stereo_threshold: one 45-degree turn where theta = 0 gives I = 2^26, Q = 0,
    and pilot_min 8 with block 1024 has threshold 2^26; the ratio is 1).  Block 0 is present at pilot_min 7 and 8 and absent at 9;
    the audio over block 1 is stereo or mono accordingly."""
    c = dc.stereo_threshold()
    mono = {}
    for pm in (8, 7, 9):
        run = Run(fmd, c, pilot_min=pm)
        outs = [run.call(d) for d in dc.calls(c)]
        I, Q = run.first.block_iq(0, 0)
        assert I * I + Q * Q == (8 * c.P * 8192) ** 2
        a = np.concatenate(outs, axis=2)[0, 0, :2 * c.P - c.Ta + 1]
        mono[pm] = bool(np.array_equal(a[:, 0], a[:, 1]))
    assert mono == {7: False, 8: False, 9: True}


@pytest.mark.parametrize("limit,sign", [(16384, 1), (256, -1), (256, 0)])
def test_extremes(fmd, limit, sign):
    """sum |g| = 16383, audio_shift 0, the front-end shift at `limit`, a strong station with pilot and then bytes at the rails: kc
    reaches its peak, the correlations pass 2^23 (e > 0), L and R reach both rails."""
    c = dc.stereo_extreme(limit, sign)
    run = Run(fmd, c)
    out = np.concatenate([run.call(d) for d in dc.calls(c)], axis=2)
    assert run.first.kc_max >= 32000 and run.first.corr_max > (1 << 23)
    for ch in (0, 1):
        assert out[..., ch].min() == -32768 and out[..., ch].max() == 32767


def test_512_streams_production_size(fmd):
    rng = np.random.default_rng(1606)
    S, n, K = 512, 262144, 2
    h = st.lowpass(64, 130000 / 2400000)
    c = dc.NS(K=K, D=10, T=64, Ta=127, R=5, S=S, h=h, incs=dc.incs(rng, S, K), P=4096, rate=2400000, pilot_min=1,
              g=dc.audio_taps(rng, 127, 16000), audio_shift=7)
    c.shift = dc.shift_for(h, c.incs, 256)
    run = Run(fmd, c, check=(0, 1, 255, 256, 510, 511))
    for _ in range(2):
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8)) is not None


def test_65535_streams(fmd):
    """The grid-y limit of the first pass: 65535 streams of small calls, one station, the smallest tap counts."""
    rng = np.random.default_rng(1707)
    S = 65535
    h = np.array([2047, -1000], np.int16)
    ii = rng.integers(0, 1 << 32, (S, 1), dtype=np.uint64).astype(np.uint32)
    c = dc.NS(K=1, D=2, T=2, Ta=1, R=1, S=S, h=h, incs=ii, P=1024, rate=250000, pilot_min=1, g=np.array([16383], np.int16),
              audio_shift=3, shift=dc.shift_for(h, ii[:64], 16384) + 1)
    check = [0, 1, 2, 4095, 4096, 32767, 32768, 65533, 65534] + [int(x) for x in rng.integers(0, S, 7)]
    run = Run(fmd, c, check=check)
    for n in (8 * 40, 8 * 13, 8 * 300):
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8)) is not None


def test_131072_rows_in_the_second_pass(fmd):
    """4096 streams x 32 stations, small calls: the audio kernel's grid is nt2 * S * K workgroups in x."""
    rng = np.random.default_rng(1808)
    S, K = 4096, 32
    h = np.array([100, -127, 90], np.int16)
    ii = dc.incs(rng, S, K)
    c = dc.NS(K=K, D=2, T=3, Ta=2, R=1, S=S, h=h, incs=ii, P=1024, rate=230000, pilot_min=1, g=np.array([9000, -7383], np.int16),
              audio_shift=2, shift=dc.shift_for(h, ii[:8], 16384) + 1)
    run = Run(fmd, c, check=(0, 1, 2047, 2048, 4094, 4095))
    for n in (8 * 16, 8 * 9, 8 * 300):                             # 600 audio samples: three tiles per row
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8)) is not None


def test_device_path_unaligned_padded_on_a_callers_stream(fmd):
    """d_iq 4 bytes past an aligned address with nbytes % 16 == 8 (no row is 16-byte aligned: the register staging path), out_cap
    padded with a sentinel that must survive, on a caller's stream; d_out 2 bytes off is refused and changes nothing."""
    import torch
    rng = np.random.default_rng(1909)
    S, K, D, T = 3, 6, 6, 59
    h, ii = dc.front(rng, T, S, K, 2)
    c = dc.NS(K=K, D=D, T=T, Ta=63, R=5, S=S, h=h, incs=ii, P=1024, rate=120000 * D, pilot_min=1, g=dc.audio_taps(rng, 63),
              audio_shift=8, shift=dc.shift_for(h, ii, 2048))
    run = Run(fmd, c)
    bank, refs = run.bank, run.refs
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    SENT = -12345
    for n in (8 * 1001, 8 * 7, 8 * 2403, 8 * 3, 8 * 1501):
        data = dc.bytes_(rng, S, n)
        buf = torch.zeros(S * n + 16, dtype=torch.uint8, device=dev)
        buf[4:4 + S * n] = torch.from_numpy(data.ravel()).to(dev)
        cap = bank.out_cap(n) + 37
        flat = torch.full((S * K * cap * 2 + 8,), SENT, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        before = run.snapshot()
        with pytest.raises(fmd.FmdError) as e:                     # (L, R) pairs are stored as dwords
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
        assert (whole[S * K * cap * 2:] == SENT).all()
        got = whole[:S * K * cap * 2].reshape(S, K, cap, 2)
        for s in range(S):
            exp = refs[s].feed(data[s])
            assert m == exp.shape[1] and np.array_equal(got[s, :, :m], exp), (n, s)
            assert (got[s, :, m:] == SENT).all(), (n, s)
        run.compare_state()
