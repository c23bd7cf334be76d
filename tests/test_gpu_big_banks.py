"""The down-converter banks (stations, channelizer, stereo, RDS, receiver -- each of its two outputs --, narrow-band, uniform channelizer
and band-plan) with their S x K = 5 output rows 2^31 - delta bytes apart, once as five streams of one station and once as one stream
of five (the kernels form s * K * out_cap and k * out_cap separately): rows 1, 2 and 4 are written across byte 2^31, 2^32 and 2^33 of
the buffer, and across element 2^31 and 2^32 in int16.  The banks that store (a, b) pairs as one uint32 run once more at a pitch of
2^32 - delta bytes, where row 2 is written across uint32 element 2^31 and row 4 across 2^32.  Two calls each, the second on the
carried histories.

The wide buffer is allocated and never filled: its windows (tests/big_cases.py) hold the sentinel, and after every call they are
compared as a whole with the definition's output in place (stations_ref, channelizer_ref, stereo_ref, rds_ref, receiver_ref,
narrow_ref, uniform_ref, bandplan_ref) -- bit for bit, and nothing else written next to the rows, behind their ends or where a
32-bit wrap of an offset would lead.  tests/test_big_cases.py shows without a GPU that a kernel with any of the wrong arithmetics
fails here.  The shapes and taps are those of tests/test_gpu_ddc_handles.py."""
import numpy as np
import pytest

import bandplan_ref as br
import big_cases as bc
import channelizer_ref as cr
import domain_cases as dmc
import narrow_ref as nr
import rds_ref as rr
import receiver_ref as rv
import stations_ref as sr
import stereo_ref as st
import uniform_ref as ur
from big_gpu import Pitched, need, random_bytes

pytestmark = pytest.mark.gpu

CASES = bc.bank_cases()
B = bc.BK
SEL = [1, 3, 4, 6, 7]                                        # the five channels of the plan of 8 (one stream of five)


def _make(fmd, oracle, kind, S, K, B, rng, streams=None, wide=False):
    """(bank, {stream: its definition} whose feed(bytes) gives [K, n, ...] of the output under test, run(d_iq, nbytes, ptr, cap, stream)
    -> n).  The receiver's other output goes to a buffer of its own, which is checked against the definition as well.  `streams`: the
    streams that get a definition (all of them where None); `wide`: many streams, so the shifts come from domain_cases' rules
    instead of the wrappers' search over every stream."""
    import torch
    uniform = kind in ("uniform", "bandplan")
    h = rng.integers(-900, 901, B.TU if uniform else B.T).astype(np.int16)
    g = rng.integers(-1500, 1501, B.TA).astype(np.int16)
    gi = rng.integers(-1500, 1501, B.TA).astype(np.int16)
    incs = rng.integers(0, 1 << 32, (S, K), dtype=np.uint64).astype(np.uint32)
    sel = SEL[:K] if B.N == 8 else list(range(K))
    streams = range(S) if streams is None else streams
    shift = None
    if wide:
        shift = ur.min_shift(h, ur.channel_incs(B.N, sel)) if uniform else dmc.shift_for(h, incs, 16384)
    return _build(fmd, oracle, kind, S, K, B, rng, h, g, gi, incs, sel, streams, shift)


def _build(fmd, oracle, kind, S, K, B, rng, h, g, gi, incs, sel, streams, shift):
    import torch
    if kind == "stations":
        bank = fmd.StationBank(h, B.D, incs, B.FAST, B.SLOW, n_streams=S, shift=shift, device_id=0)
        refs = {s: sr.StationsRef(oracle, h, B.D, incs[s], B.FAST, B.SLOW, bank.shift, z=sr.z_corr) for s in streams}
        return bank, refs, bank.demodulate_device
    if kind == "channelizer":
        bank = fmd.Channelizer(h, B.D, incs, n_streams=S, shift=shift, device_id=0)
        return bank, {s: cr.ChannelizerRef(h, B.D, incs[s], bank.shift, z=sr.z_corr) for s in streams}, bank.run_device
    if kind == "stereo":
        bank = fmd.StereoBank(h, B.D, incs, B.RATE, g, B.R, n_streams=S, block=B.PILOT_BLOCK, pilot_min=1, shift=shift, device_id=0)
        return bank, {s: st.StereoRef(h, B.D, incs[s], bank.shift, B.RATE, g, B.R, B.PILOT_BLOCK, 1, bank.audio_shift, z=sr.z_corr) for s in streams}, bank.run_device
    if kind == "rds":
        bank = fmd.RdsBank(h, B.D, incs, B.RATE, g, B.R, n_streams=S, block=B.PILOT_BLOCK, pilot_min=1, shift=shift, device_id=0)
        return bank, {s: rr.RdsRef(h, B.D, incs[s], bank.shift, B.RATE, g, B.R, bank.rds_shift, B.PILOT_BLOCK, 1, z=sr.z_corr) for s in streams}, bank.run_device
    if kind == "narrow":
        cs = None if shift is None else dmc.chan_shift_for(h, incs, shift, g, None, 16384)
        bank = fmd.NarrowBank(h, B.D, incs, g, B.R, mode="fm", n_streams=S, block=B.BLOCK, squelch=0, chan_shift=cs, shift=shift, device_id=0)
        return bank, {s: nr.NarrowRef(h, B.D, incs[s], bank.shift, bank.gr, bank.gi, bank.mode, B.R, bank.chan_shift, B.BLOCK, 0, bank.gain, z=sr.z_corr)
                      for s in streams}, bank.run_device
    if kind == "uniform":
        bank = fmd.UniformChannelizer(h, B.N, B.HOP, channels=sel, n_streams=S, shift=shift, device_id=0)
        return bank, {s: ur.UniformRef(h, B.N, B.HOP, bank.shift, channels=sel) for s in streams}, bank.run_device
    if kind == "bandplan":
        bank = fmd.BandPlanBank(h, B.N, B.HOP, (g, gi), B.R, mode="am", channels=sel, n_streams=S, block=B.BLOCK, squelch=0, shift=shift, device_id=0)
        return bank, {s: br.BandPlanRef(h, B.N, B.HOP, bank.shift, bank.gr, bank.gi, bank.mode, B.R, bank.chan_shift, B.BLOCK, 0, bank.gain, channels=sel)
                      for s in streams}, bank.run_device
    assert kind in ("receiver-audio", "receiver-rds")
    g2 = rng.integers(-1500, 1501, B.TA).astype(np.int16)
    bank = fmd.ReceiverBank(h, B.D, incs, B.RATE, g, B.R, g2, B.R, n_streams=S, block=B.PILOT_BLOCK, pilot_min=1, shift=shift, device_id=0)
    refs = {s: rv.ReceiverRef(h, B.D, incs[s], bank.shift, B.RATE, g, B.R, bank.audio_shift, g2, B.R, bank.rds_shift, B.PILOT_BLOCK, 1, z=sr.z_corr)
            for s in streams}
    mine = 0 if kind == "receiver-audio" else 1

    class Pick:                                              # the pitched output's definition; the other output is kept for `run`
        def __init__(self, ref):
            self.ref, self.other = ref, None

        def feed(self, buf):
            both = self.ref.feed(buf)
            self.other = both[1 - mine]
            return both[mine]
    picks = {s: Pick(r) for s, r in refs.items()}

    def run(d_iq, nbytes, ptr, cap, stream):
        small_cap = max(bank.out_caps(nbytes)) + 3
        d_small = torch.full((S, K, small_cap, 2), bc.SENT, dtype=torch.int16, device="cuda")
        args = (ptr, cap, d_small.data_ptr(), small_cap) if mine == 0 else (d_small.data_ptr(), small_cap, ptr, cap)
        n = bank.run_device(d_iq, nbytes, *args, stream)
        torch.cuda.synchronize()
        for s in picks:
            exp = np.asarray(picks[s].other)
            got = d_small[s].cpu().numpy()
            assert exp.shape[1] == n[1 - mine] and np.array_equal(got[:, :exp.shape[1]], exp), "the receiver's other output, stream %d" % s
        assert bool((d_small[:, :, n[1 - mine]:] == bc.SENT).all())
        return n[mine]
    return bank, picks, run


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_bank_output_rows_across_the_lines(fmd, oracle, c):
    import torch
    rng = np.random.default_rng([2032, CASES.index(c)])
    bank, refs, run = _make(fmd, oracle, c.kind, c.S, c.K, B, rng)
    big = None
    try:
        big = Pitched(c.geo, c.peak, "sentinel", CASES.index(c))
        for call, nbytes in enumerate(bc.BANK_CALLS):
            iq = rng.integers(0, 256, (c.S, nbytes), dtype=np.uint8)
            exp = [refs[s].feed(iq[s]) for s in range(c.S)]        # before the call: the receiver's `run` compares its other output
            d_iq = torch.from_numpy(iq).cuda()
            big.clear()
            torch.cuda.synchronize()
            n = run(d_iq.data_ptr(), nbytes, big.ptr, c.geo.cap, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            bank.check()
            assert n == c.ns[call], (n, c.ns)
            for s in range(c.S):
                for k in range(c.K):
                    e = np.asarray(exp[s][k])
                    assert e.shape[0] == n and e.size == n * c.width and np.abs(e).max() <= 32768
                    big.put(s * c.K + k, e.astype(np.int16), device=False)
            big.check("%s: the output of call %d" % (c.name, call))
            assert np.array_equal(d_iq.cpu().numpy(), iq)
    finally:
        if big is not None:
            big.release()
        bank.close()


# ---- inputs of 2^32 bytes and more --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", bc.BANK_INPUTS)
def test_bank_input_beyond_4_gib(fmd, oracle, kind):
    """65535 streams x 65552 bytes of random input, filled on the device, one station (every channel of a plan of 4 for the uniform
    channelizer and the band-plan bank) and the smallest tap counts, two calls: the first and last streams, the streams that straddle
    byte 2^31 and 2^32 of the buffer and their neighbours against the definitions, which are fed the bytes read back from the device;
    nothing written behind any row's outputs.  The narrow-band and the band-plan bank's internal stage passes 2^32 bytes as well."""
    import torch
    S, K, nbytes = bc.BANK_IN_S, bc.BANK_IN_K.get(kind, 1), bc.IN_BYTES
    need(torch, bc.bank_input_peak(kind))
    picks = bc.sampled(S, nbytes)
    rng = np.random.default_rng([2033, bc.BANK_INPUTS.index(kind)])
    bank, refs, run = _make(fmd, oracle, kind, S, K, bc.BI, rng, streams=picks, wide=True)
    width = bc.BANKS[kind][0]
    d_iq = d_out = None
    try:
        cap = (max(bank.out_caps(nbytes)) if kind.startswith("receiver") else bank.out_cap(nbytes)) + 3
        d_iq = torch.empty((S, nbytes), dtype=torch.uint8, device="cuda")
        d_out = torch.empty((S, K, cap, width), dtype=torch.int16, device="cuda")
        for call in range(2):
            random_bytes(torch, d_iq, 500 + call)
            d_out.fill_(bc.SENT)
            iq = {s: d_iq[s].cpu().numpy() for s in picks}
            exp = {s: refs[s].feed(iq[s]) for s in picks}
            torch.cuda.synchronize()
            n = run(d_iq.data_ptr(), nbytes, d_out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            bank.check()
            for s in picks:
                got = d_out[s].cpu().numpy()
                for k in range(K):
                    e = np.asarray(exp[s][k])
                    assert e.shape[0] == n, (call, s, k, e.shape, n)
                    assert np.array_equal(got[k, :n].reshape(e.shape), e), "call %d stream %d row %d differs from the definition" % (call, s, k)
                assert np.array_equal(d_iq[s].cpu().numpy(), iq[s])
            assert bool((d_out[:, :, n:] == bc.SENT).all())
    finally:
        del d_iq, d_out
        bank.close()
        torch.cuda.empty_cache()


def test_spectrum_input_beyond_4_gib(fmd):
    """The power spectrum of 65535 streams x 65552 bytes, two calls of which the second accumulates: the sampled streams against
    spectrum_ref.power of the bytes read back from the device; the rows of all other streams are written too (no sentinel left)."""
    import torch
    import spectrum_ref as spr
    S, nbytes, q = bc.BANK_IN_S, bc.IN_BYTES, bc.SPEC
    need(torch, S * nbytes + (1 << 30) + bc.SLACK)
    picks = bc.sampled(S, nbytes)
    w = np.random.default_rng(2034).integers(-2047, 2048, q.N).astype(np.int16)
    sp = fmd.Spectrum(q.N, q.HOP, window=w, shift=q.SHIFT, n_streams=S, device_id=0)
    d_iq = d_pow = None
    try:
        d_iq = torch.empty((S, nbytes), dtype=torch.uint8, device="cuda")
        d_pow = torch.full((S, q.N), -1, dtype=torch.int64, device="cuda")
        total = np.zeros((len(picks), q.N), np.uint64)
        for call in range(2):
            random_bytes(torch, d_iq, 700 + call)
            iq = np.stack([d_iq[s].cpu().numpy() for s in picks])
            torch.cuda.synchronize()
            sp.power_device(d_iq.data_ptr(), nbytes, d_pow.data_ptr(), accumulate=call > 0, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            sp.check()
            total = total + spr.power_chunked(w, q.HOP, q.SHIFT, iq).astype(np.uint64)
            got = np.stack([d_pow[s].cpu().numpy() for s in picks]).view(np.uint64)
            assert np.array_equal(got, total), call
            assert bool((d_pow != -1).all())
            assert np.array_equal(np.stack([d_iq[s].cpu().numpy() for s in picks]), iq)
    finally:
        del d_iq, d_pow
        sp.close()
        torch.cuda.empty_cache()
