"""The row processors (Resampler, Agc, ToneSquelch, AfskDemod, CodeSquelch) with rows 2^31 - delta bytes apart: rows 1, 2 and 4 of five start just
below byte 2^31, 2^32 and 2^33 of the buffer (element 2^31 and 2^32 in int16, W-sample 2^31 at width 2), and two calls of ~2400
samples per row read (the input pitched) or write (the output pitched) across each line -- the second call with the carried history
in front.  The pitch is 16-byte aligned in one case and not in the other, so the vector and the element paths both cross.

The wide buffer is allocated and never filled: only its windows (tests/big_cases.py) hold data -- the live rows, and around them and
at every place a 32-bit wrap of an offset would lead to, decoy samples (a buffer that is read) or the sentinel (one that is
written).  Outputs against the test-side definitions (resample_ref, agc_ref, tonesq_ref, afsk_ref) bit for bit after every call;
every window compared with its mirror: nothing but the outputs is written, the input is unchanged.  tests/test_big_cases.py shows
without a GPU that a kernel with any of the wrong arithmetics fails here."""
import numpy as np
import pytest

import afsk_ref as ar
import agc_ref as ag
import big_cases as bc
import dcs_ref as dr
import resample_ref as rr
import tonesq_ref as tr
from big_gpu import Pitched

pytestmark = pytest.mark.gpu

CASES = bc.row_cases()


def _tq_cfg():
    q = bc.TQ
    return tr.Cfg(q.block, q.guard, q.dom_shift, q.confirm, q.hang, q.ramp, q.min_power, q.accept)


def _make(fmd, c, rng):
    """(handle, reference with push(x [rows, n, width]) -> [rows, n_out, width])"""
    if c.handle == "resample":
        g = rng.integers(-4000, 4001, (bc.RS.L, bc.RS.T)).astype(np.int16)
        return fmd.Resampler(g, bc.RS.L, bc.RS.M, bc.RS.shift, n_rows=bc.ROWS, width=c.width, device_id=0), rr.Resampler(g, bc.RS.L, bc.RS.M, bc.RS.shift)
    if c.handle == "agc":
        a = bc.AGC
        return (fmd.Agc(n_rows=bc.ROWS, width=c.width, target=a.target, block=a.block, hang=a.hang, decay=a.decay, gain_max=a.gain_max, device_id=0),
                ag.Agc(a))
    if c.handle == "tonesq":
        q = bc.TQ
        tab = fmd.tone_table(q.rate, q.freqs, q.block)
        return (fmd.ToneSquelch(tab, n_rows=bc.ROWS, width=c.width, accept=q.accept, guard=q.guard, dom_shift=q.dom_shift, min_power=q.min_power,
                                confirm=q.confirm, hang=q.hang, ramp=q.ramp, device_id=0), tr.ToneSquelch(tab, _tq_cfg()))
    if c.handle == "dcs":
        q = bc.DCS
        cfg = dr.Cfg(q.block, q.box, list(q.lp), q.lshift, list(q.tap), q.tol, q.min_hits, q.confirm, q.hang, q.ramp, q.accept)
        return (fmd.CodeSquelch(list(q.words), q.block, q.box, cfg.lp, q.lshift, cfg.tap, n_rows=bc.ROWS, width=c.width, accept=q.accept, tol=q.tol,
                                min_hits=q.min_hits, confirm=q.confirm, hang=q.hang, ramp=q.ramp, device_id=0), dr.CodeSquelch(list(q.words), cfg))
    tab, pre, out = fmd.afsk_table(bc.AF.rate, taps=bc.AF.taps)
    ref = ar.AfskDemod(tab, bc.AF.stride, pre, out, rows=bc.ROWS)

    class Mono:                                                   # afsk_ref takes and gives [rows, n]
        def push(self, x):
            return ref.push(x[:, :, 0])[:, :, None]
    return fmd.AfskDemod(tab, bc.AF.stride, pre, out, n_rows=bc.ROWS, device_id=0), Mono()


def _input(c, rng, n, first):
    """int16 [rows, n, width]: full-range noise (the code squelch's configuration opens on it); for the tone squelch row r carries
    tone r mod 3 of its table under the noise, so that the gate opens and the output depends on every sample."""
    if c.handle != "tonesq":
        return rng.integers(-32768, 32768, (bc.ROWS, n, c.width)).astype(np.int16)
    t = (first + np.arange(n))[None, :, None]
    f = np.array([bc.TQ.freqs[r % 3] for r in range(bc.ROWS)])[:, None, None]
    x = 9000 * np.cos(2 * np.pi * f * t / bc.TQ.rate) + rng.integers(-3000, 3001, (bc.ROWS, n, c.width))
    return np.rint(x).astype(np.int16)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_rows_across_the_lines(fmd, c):
    import torch
    rng = np.random.default_rng([2031, CASES.index(c)])
    h, ref = _make(fmd, c, rng)
    W, geo = c.width, c.geo
    big = Pitched(geo, c.peak, "decoy" if c.side == "in" else "sentinel", CASES.index(c))
    try:
        first = 0
        for call, n_in in enumerate(c.n_in):
            x = _input(c, rng, n_in, first)
            exp = ref.push(x)
            assert exp.shape == (bc.ROWS, c.n_out[call], W), (exp.shape, c.n_out)
            if c.side == "in":
                for r in range(bc.ROWS):
                    big.put(r, x[r])
                cap = (c.n_out[call] + 3) | 1
                d_out = torch.full((bc.ROWS, cap, W), bc.SENT, dtype=torch.int16, device="cuda")
                torch.cuda.synchronize()
                n = h.run_device(big.ptr, n_in, geo.cap, d_out.data_ptr(), cap)
                h.check()
                got = d_out.cpu().numpy()
                assert n == c.n_out[call] and (got[:, n:] == bc.SENT).all()
                assert np.array_equal(got[:, :n], exp), "call %d: rows %r differ" % (call, [r for r in range(bc.ROWS) if not np.array_equal(got[r, :n], exp[r])])
                big.check("the input after call %d" % call)
            else:
                in_cap = n_in + 1 + n_in % 2
                host = np.full((bc.ROWS, in_cap, W), 12321, np.int16)
                host[:, :n_in] = x
                d_in = torch.from_numpy(host).cuda()
                big.clear()
                torch.cuda.synchronize()
                n = h.run_device(d_in.data_ptr(), n_in, in_cap, big.ptr, geo.cap)
                h.check()
                assert n == c.n_out[call]
                for r in range(bc.ROWS):
                    big.put(r, exp[r], device=False)
                big.check("the output of call %d" % call)
                assert np.array_equal(d_in.cpu().numpy(), host)
            first += n_in
        assert h.counts() == (first, sum(c.n_out))
        if c.handle == "tonesq":
            tone, power, gate = h.status()
            rt, rp, rg = ref.status()
            assert [int(v) for v in tone] == rt and [int(v) for v in power] == rp and [bool(v) for v in gate] == rg
            assert all(rg) and rt == [r % 3 for r in range(bc.ROWS)]     # the gates are open: the outputs carried the samples
        if c.handle == "dcs":
            code, hits, gate = h.status()
            rc, rh, rg = ref.status()
            assert code.tolist() == rc and [int(v) for v in hits] == rh and gate.tolist() == rg
            # every completed block decided on an accepted word: the gate ramps up over block 1 and is open from block 2 on
            assert all(rg) and len(ref.hits) == 18 * bc.ROWS and all(hit != dr.NONE for _, _, hit, _, _ in ref.hits)
    finally:
        big.release()
        h.close()
