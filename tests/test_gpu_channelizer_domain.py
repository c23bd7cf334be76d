"""Channelizer (include/fmd.h, fmd_channelizer_*) on the MI355X where tests/test_gpu_channelizer.py does not reach: station counts
on both sides of every row-tile edge in both digit forms, across the decims and tap counts of the station bank's domain test, with
tiles of 256, 192 and 128 outputs and calls of several tiles, and the grid's 65535 streams -- y and outputs() against the
test-side definition (tests/channelizer_ref.py), bit for bit, after every call.  The cases come from tests/domain_cases.py."""
import numpy as np
import pytest

import channelizer_ref as cr
import domain_cases as dc
import stations_ref as sr

pytestmark = pytest.mark.gpu

TOO_SHORT = -3


def _call(fmd, ch, refs, data):
    first = next(iter(refs.values()))
    if first.outputs_after(data.shape[1] // 2) - first.m_next < 1:
        before = ch.outputs()
        with pytest.raises(fmd.FmdError) as e:
            ch.run_batch(data)
        assert e.value.status == TOO_SHORT and ch.outputs() == before
        return False
    got = ch.run_batch(data)
    for s, r in refs.items():
        exp = r.feed(data[s])
        assert got.shape[2] == exp.shape[1] and np.array_equal(got[s], exp), (s, data.shape[1])
    assert ch.outputs() == first.m_next
    return True


def test_shape_sweep(fmd):
    seen = set()
    for c in dc.channelizer_sweep():
        ch = fmd.Channelizer(c.h, c.D, c.incs, n_streams=c.S, shift=c.shift, device_id=0)
        refs = {s: cr.ChannelizerRef(c.h, c.D, c.incs[s], c.shift, z=sr.z_corr) for s in range(c.S)}
        fed = [_call(fmd, ch, refs, d) for d in dc.calls(c)]
        assert fed[1] and refs[0].m_next > 3 * 64 * c.G, c.i
        seen.add((c.K, c.digits, c.G))
    assert {(k, d) for k, d, _ in seen} >= set(dc.K_EDGES) and {g for _, _, g in seen} == {2, 3, 4}


def test_65535_streams(fmd):
    """The grid-y limit: 65535 streams of small calls, one station of 8 taps."""
    rng = np.random.default_rng(3707)
    S = 65535
    h = rng.integers(-2047, 2048, 8).astype(np.int16)
    ii = rng.integers(0, 1 << 32, (S, 1), dtype=np.uint64).astype(np.uint32)
    shift = dc.shift_for(h, ii, 16384)
    ch = fmd.Channelizer(h, 4, ii, n_streams=S, shift=shift, device_id=0)
    check = [0, 1, 2, 4095, 4096, 32767, 32768, 65533, 65534] + [int(x) for x in rng.integers(0, S, 7)]
    refs = {s: cr.ChannelizerRef(h, 4, ii[s], shift) for s in check}
    for n in (8 * 40, 8 * 13, 8 * 300):
        assert _call(fmd, ch, refs, rng.integers(0, 256, (S, n), dtype=np.uint8))
