"""Band-plan bank (include/fmd.h, fmd_bandplan_*) on the MI355X across its whole documented domain: the output, outputs() and
levels() of every stream against the test-side definition (tests/bandplan_ref.py), bit for bit, after every call.  The cases come
from tests/domain_cases.py (tests/test_domain_cases.py asserts without a GPU what each one reaches): every chan_decim 1 ... 8 with
complex and real tap counts on both sides of the tap-chunk edges, below R and 64, taps that fill the rule and taps at its edges,
the four modes with both tap kinds, all nine block lengths, squelch on and off, a random gain, chan_shift and shift at and above
their minimum, all six instantiations of the first pass under it -- the launched kernels are read back through kernel_name() --
with a refused call, a call of more than three tiles and one that rebuilds the y history from old history plus new samples;
audio ends one sample before, on and after a block edge at P = 16, 256 (block = tile, aligned and one sample off) and 4096; the
squelch threshold at exact equality; FM and AM at the largest |u| bytes can produce; 65535 streams.  FMD_FUZZ_SEED reseeds the
sweep."""
import copy

import numpy as np
import pytest

import bandplan_ref as br
import domain_cases as dc
import uniform_ref as ur

pytestmark = pytest.mark.gpu

TOO_SHORT = -3
seen = set()                                                 # (kernel_name(0), kernel_name(1)) of every sweep case run so far


class Run:
    """One bank and the definition of the streams in `check`; call() feeds both and compares the output, outputs() and levels()."""

    def __init__(self, fmd, c, check=None, squelch=None):
        if squelch is not None:
            c = copy.copy(c)
            c.squelch = squelch
        self.fmd, self.c = fmd, c
        self.bank = dc.bandplan_handle(c, fmd)
        self.refs = dc.bandplan_refs(c, br, check)
        self.first = next(iter(self.refs.values()))

    def snapshot(self):
        o, r = self.bank.levels()
        return self.bank.outputs(), o[list(self.refs)].tolist(), r[list(self.refs)].tolist()

    def compare_state(self):
        assert self.bank.outputs() == self.first.n_next
        o, r = self.bank.levels()
        assert o.dtype == np.bool_ and r.dtype == np.uint32 and o.shape == r.shape == (self.c.S, self.bank.n_selected)
        for s, ref in self.refs.items():
            want = [ref.level(k) for k in range(ref.K)]
            assert list(zip(o[s].tolist(), r[s].tolist())) == want, (getattr(self.c, "i", None), s)

    def call(self, data):
        """The output [S, rows, n(, 2)], or None when the call is refused (and then it changed nothing)."""
        if self.first.completes(data.shape[1]) < 1:
            before = self.snapshot()
            with pytest.raises(self.fmd.FmdError) as e:
                self.bank.run_batch(data)
            assert e.value.status == TOO_SHORT and self.snapshot() == before
            return None
        got = self.bank.run_batch(data)
        for s, ref in self.refs.items():
            exp = ref.feed(data[s])
            assert got.shape[2] == exp.shape[1], (got.shape, exp.shape)
            bad = np.argwhere(got[s] != exp)
            assert bad.size == 0, (getattr(self.c, "i", None), s, data.shape[1], len(bad), bad[:4].tolist())
        self.compare_state()
        return got


def _names(c):
    return ("fmd_uv::fmd_uniform_kernel<%d, %d>" % c.uv[:2], "fmd_bp::fmd_bandplan_chan_kernel<%s>" % ("true" if c.cplx else "false"))


def _run_case(fmd, c):
    datas = dc.calls(c)
    assert all(not np.array_equal(d[0], d[1]) for d in datas)
    if c.use_squelch:
        c.squelch = dc.bandplan_probe_squelch(c, br, np.concatenate([d[0] for d in datas[1:]]))
        assert c.squelch > 0
    run = Run(fmd, c)
    b = run.bank
    assert (b.shift, b.chan_shift) == (c.shift, c.chan_shift), c.i
    assert not c.auto_shift or b.shift == ur.min_shift(c.h, ur.channel_incs(c.N, c.sel))
    assert not c.auto_chan_shift or b.chan_shift == br.min_chan_shift(c.h, c.N, b.shift, c.gr, c.gi, c.sel,
                                                                      limit=256 if c.mode == br.FM else 16384)
    names = (b.kernel_name(0), b.kernel_name(1))
    assert names == _names(c), (c.i, names)
    outs = [run.call(d) for d in datas]
    assert [o is not None for o in outs] == [False, True, True, True, True], c.i
    assert outs[2].shape[2] > 3 * dc.BP_TILE and outs[3].shape[2] == 1
    got = np.concatenate(outs[1:], axis=2)
    assert got.any() or c.use_squelch, c.i                   # (a squelched case whose first block never completes stays mute)
    assert not got.any() or not np.array_equal(got[0], got[1]), c.i
    assert max(r.v_max for r in run.refs.values()) <= 1 << 30
    seen.add(names)


@pytest.mark.parametrize("R", range(1, 9))
def test_shape_sweep(fmd, R):
    mine = [c for c in dc.bandplan_sweep() if c.R == R]
    assert {c.uv[:2] for c in mine} == set(dc.UV_CELLS)
    for c in mine:
        _run_case(fmd, c)


def test_every_instantiation_was_launched(fmd):
    """The names read back from the banks that ran are all six first passes and both second passes.  After the sweep (file order)
    nothing is left to run; alone, the test runs one case of every first pass and of both second passes itself."""
    for c in dc.bandplan_sweep():
        if _names(c)[0] not in {a for a, _ in seen} or _names(c)[1] not in {b for _, b in seen}:
            _run_case(fmd, c)
    assert {a for a, _ in seen} == {"fmd_uv::fmd_uniform_kernel<%d, %d>" % x for x in dc.UV_CELLS}, sorted(seen)
    assert {b for _, b in seen} == {"fmd_bp::fmd_bandplan_chan_kernel<true>", "fmd_bp::fmd_bandplan_chan_kernel<false>"}


@pytest.mark.parametrize("P,mode,off", [(16, br.AM, 0), (16, br.FM, 0), (256, br.AM, 0), (256, br.FM, 1), (256, br.IQ, 1), (4096, br.AM, 0),
                                        (4096, br.SSB, 0)])
def test_block_edges(fmd, P, mode, off):
    """Audio ends on j P - 1, j P, j P + 1: 17 blocks in a tile (P = 16), block = tile with the two aligned and one sample apart
    (P = 256), one block open over many calls (P = 4096); the squelch sits between the loud and the quiet block energy."""
    c = dc.bandplan_edges(P, mode, off)
    c.squelch = dc.bandplan_probe_squelch(c, br, c.data[0])
    run = Run(fmd, c)
    for d, n in zip(dc.calls(c), c.ends):
        assert run.call(d) is not None and run.first.n_next == n
    assert {run.first.estimate(0, j)[0] for j in range(run.first.n_next // P)} == {True, False}


@pytest.mark.parametrize("mode", [br.IQ, br.FM, br.AM, br.SSB])
def test_squelch_threshold_at_exact_equality(fmd, mode):
    """Blocks with E = squelch^2 P exactly (|u|^2 = 25 per sample, squelch 5, block 16), E - 1 and E + 1 in both channels: equality
    opens.  The same bytes at squelch 4 (all open) and 6 (none does)."""
    c = dc.bandplan_threshold(mode)
    for sq, want in ((5, c.want_open), (4, [True] * len(c.kinds)), (6, [False] * len(c.kinds))):
        run = Run(fmd, c, squelch=sq)
        out = np.concatenate([run.call(d) for d in dc.calls(c)], axis=2)
        for k in (0, 1):
            assert [run.first.block(k, j)[0] for j in range(len(c.kinds))] == [400 + kd for kd in c.kinds]
            assert [run.first.estimate(k, j)[0] for j in range(len(c.kinds))] == want
            if mode != br.AM:
                loud = [bool(out[0, k, j * c.P:(j + 1) * c.P].any()) for j in range(len(c.kinds))]
                assert loud == [False] + want[:-1], (sq, k)


@pytest.mark.parametrize("mode", [br.FM, br.AM])
def test_extremes(fmd, mode):
    """FM at gain 65535 over the largest |u| bytes can produce, where the discriminator's i32 products wrap: both rails, -32768
    among them.  AM with both components of u at their largest together: a = 11578."""
    c = dc.bandplan_extreme(mode)
    run = Run(fmd, c)
    out = np.concatenate([run.call(d) for d in dc.calls(c)], axis=2)
    assert out.min() == -32768 and out.max() == 32767
    assert run.first.v_max > (1 << 28) and int(np.abs(run.first.u[0]).max()) == 8187 and (mode == br.FM or run.first.a_max == 11578)


def test_65535_streams(fmd):
    """The grid limits: 65535 streams in the first pass, 131070 rows in the second, each stream its own bytes."""
    rng = np.random.default_rng(6707)
    S = 65535
    h = dc.uniform_taps(rng, 8, 2)
    gr, gi = dc.chan_taps(rng, 3, True)
    shift = ur.min_shift(h, ur.channel_incs(2))
    c = dc.NS(N=2, hop=8, T=8, Ta=3, R=2, S=S, h=h, sel=None, P=16, mode=br.AM, gr=gr, gi=gi, shift=shift,
              chan_shift=br.min_chan_shift(h, 2, shift, gr, gi), gain=700, squelch=0, z=dc.sr.z_direct)
    check = [0, 1, 2, 4095, 4096, 32767, 32768, 65533, 65534] + [int(x) for x in rng.integers(0, S, 7)]
    run = Run(fmd, c, check=check)
    for n in (16 * 40, 16 * 13, 16 * 150):
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8)) is not None
