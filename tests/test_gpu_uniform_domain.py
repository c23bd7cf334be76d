"""Uniform channelizer (include/fmd.h, fmd_uniform_*) on the MI355X across its whole documented domain: y and outputs() against the
test-side definition (tests/uniform_ref.py), bit for bit, after every call.  The cases come from tests/domain_cases.py
(tests/test_domain_cases.py asserts without a GPU what each one reaches): all six instantiations fmd_uniform_kernel<R, G> in both
digit forms -- the launched one is read back through kernel_name() and must be the one the case claims -- with channel counts on
both sides of every R edge, last batches of fewer than R row tiles, a wave that takes two batches, 64 row tiles; both sides of
the two G edges (hop 240 at 1248 | 1249 taps, hop 248 at 224 | 225), the G = 8 side with exactly 64 KiB of LDS; all 32 hops; tap
counts at the K-chunk edges and around hop; the smallest admissible shift and larger ones; per case a refused call, one of three
tiles and a part, one of a single hop and one of a tile and a part, each stream with its own bytes; half of the cases through the
device entry point with d_iq 4 bytes past an aligned address (every piece staged through registers) and an odd out_cap; 65535
streams.  FMD_FUZZ_SEED reseeds the sweep."""
import numpy as np
import pytest

import domain_cases as dc
import uniform_ref as ur

pytestmark = pytest.mark.gpu

TOO_SHORT = -3
SENT = -12345
seen = set()                                                 # kernel_name() of every sweep case run so far


class Run:
    """One handle and the definition of the streams in `check`; call() feeds both and compares the output and outputs()."""

    def __init__(self, fmd, c, check=None):
        self.fmd, self.c = fmd, c
        self.u = dc.uniform_handle(c, fmd)
        self.refs = dc.uniform_refs(c, ur, check)
        self.first = next(iter(self.refs.values()))
        self.rows = c.N if c.sel is None else len(c.sel)

    def refused(self, data):
        if self.first.outputs_after(data.shape[1] // 2) - self.first.m_next >= 1:
            return False
        before = self.u.outputs()
        with pytest.raises(self.fmd.FmdError) as e:
            self.feed(data)
        assert e.value.status == TOO_SHORT and self.u.outputs() == before
        return True

    def feed(self, data):
        """[S, rows, n, 2] of one call, through run_batch or -- cases marked dev -- through run_device with the input 4 bytes past
        an aligned address and an odd out_cap; the sentinel beyond each row's outputs must survive."""
        if not self.c.dev:
            return self.u.run_batch(data)
        import torch
        S, n = data.shape
        dev = torch.device("cuda:0")
        buf = torch.zeros(S * n + 16, dtype=torch.uint8, device=dev)
        buf[4:4 + S * n] = torch.from_numpy(data.ravel()).to(dev)
        cap = self.u.out_cap(n) + 7 + (self.u.out_cap(n) % 2)
        assert cap % 2 == 1 and (buf.data_ptr() + 4) % 16 == 4
        d_out = torch.full((S, self.rows, cap, 2), SENT, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        try:
            m = self.u.run_device(buf.data_ptr() + 4, n, d_out.data_ptr(), cap)
            self.u.check()
        finally:
            torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[:, :, m:] == SENT).all(), (self.c.i, n)
        return got[:, :, :m]

    def call(self, data):
        """True when the call was accepted (and equal to the definition), False when refused (and nothing changed)."""
        if self.refused(data):
            return False
        got = self.feed(data)
        for s, r in self.refs.items():
            exp = r.feed(data[s])
            assert got.shape[1:3] == exp.shape[:2], (self.c.i, got.shape, exp.shape)
            bad = np.argwhere(got[s] != exp)
            assert bad.size == 0, (getattr(self.c, "i", None), s, data.shape[1], len(bad), bad[:4].tolist())
        assert self.u.outputs() == self.first.m_next
        return True


def _run_case(fmd, c):
    run = Run(fmd, c)
    incs = ur.channel_incs(c.N, c.sel)
    assert run.u.shift == c.shift and (c.limit != 16384 or c.shift == ur.min_shift(c.h, incs))
    assert run.u.tap_digits() == c.digits == ur.digits(c.h, incs), c.i
    assert run.u.kernel_name() == "fmd_uv::fmd_uniform_kernel<%d, %d>" % (c.R, c.G), (c.i, run.u.kernel_name())
    datas = dc.calls(c)
    assert all(not np.array_equal(d[0], d[s]) for d in datas for s in range(1, c.S))
    fed = [run.call(d) for d in datas]
    assert fed == ([False] if c.refuses else []) + [True] * 3, (c.i, fed)
    assert run.first.m_next > 4 * 16 * c.G, c.i
    seen.add(run.u.kernel_name())


@pytest.mark.parametrize("cell", dc.UV_CELLS, ids=lambda x: "R%d-G%d" % x)
def test_shape_sweep(fmd, cell):
    mine = [c for c in dc.uniform_sweep() if (c.R, c.G) == cell]
    assert {c.digits for c in mine} == {1, 2}
    for c in mine:
        _run_case(fmd, c)


def test_every_instantiation_was_launched(fmd):
    """The names read back from the handles that ran are all six.  After the sweep (file order) nothing is left to run; alone,
    the test runs one case of every instantiation itself."""
    names = {"fmd_uv::fmd_uniform_kernel<%d, %d>" % x for x in dc.UV_CELLS}
    for c in dc.uniform_sweep():
        if "fmd_uv::fmd_uniform_kernel<%d, %d>" % (c.R, c.G) not in seen:
            _run_case(fmd, c)
    assert seen == names, sorted(seen)


def test_65535_streams(fmd):
    """The grid-y limit: 65535 streams of small calls, both channels of N = 2, each stream its own bytes."""
    rng = np.random.default_rng(5707)
    S = 65535
    h = dc.uniform_taps(rng, 8, 2)
    c = dc.NS(N=2, hop=8, T=8, sel=None, S=S, h=h, limit=16384, shift=ur.min_shift(h, ur.channel_incs(2)), dev=False, z=dc.sr.z_direct)
    check = [0, 1, 2, 4095, 4096, 32767, 32768, 65533, 65534] + [int(x) for x in rng.integers(0, S, 7)]
    run = Run(fmd, c, check=check)
    assert run.u.kernel_name() == "fmd_uv::fmd_uniform_kernel<1, 8>"
    for n in (16 * 40, 16 * 13, 16 * 150):
        assert run.call(rng.integers(0, 256, (S, n), dtype=np.uint8))
