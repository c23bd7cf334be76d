"""The five down-converter handles (station bank, channelizer, stereo, narrow-band and RDS bank) alive at once on the MI355X: they
share one host layer (csrc/fmd_ddc.h), so each is checked bit for bit against its own definition while the others run, are reset,
refuse a call and are freed around it.  The stereo and the RDS bank, which share their second stage over the multiplex
(csrc/fmd_stereo_mpx.h), also run on the same bytes.  Likewise the narrow-band bank, the uniform channelizer and the band-plan bank: the two banks
share their second stage's host side (csrc/fmd_chan_stage.h), and the band-plan bank drives a uniform channelizer of its own."""
import numpy as np
import pytest

import bandplan_ref as br
import channelizer_ref as cr
import narrow_ref as nr
import rds_ref as rr
import stations_ref as sr
import stereo_ref as st
import uniform_ref as ur

pytestmark = pytest.mark.gpu

TOO_SHORT = -3
S, K, D, T = 2, 3, 4, 33
RATE = 480000                                                # >= 120000 * D, the RDS bank's floor (the stereo bank's is lower)
FAST, SLOW = RATE // D, 30000                                # the station bank's rates: 4 filter outputs per audio sample
TA, R = 9, 2                                                 # every second filter: 9 taps at stride 2
CUTS = (8 * 601, 8 * 513, 8 * 389)                           # 2404 + 2052 + 1556 samples: cut 2 crosses the first 1024-sample pilot block


def _same(got, exp):
    """got [S, K, ...] from a bank, exp[s] the definition's [K, ...] of stream s"""
    return all(np.array_equal(got[s, k], exp[s][k]) for s in range(S) for k in range(K))


def test_five_handles_interleaved_reset_refusal_and_free(fmd, oracle):
    rng = np.random.default_rng(515)
    h = rng.integers(-900, 901, T).astype(np.int16)          # |W| > 127: the two-digit tap form
    incs = np.array([[int(x) for x in rng.integers(0, 1 << 32, K)] for _ in range(S)], np.uint32)
    assert max(np.abs(w).max() for i in incs.ravel() for w in sr.complex_taps(h, int(i))) > 127
    g = rng.integers(-1500, 1501, TA).astype(np.int16)       # sum |g| <= 13500
    data = rng.integers(0, 256, (S, sum(CUTS)), dtype=np.uint8)
    cuts = np.split(data, np.cumsum(CUTS)[:-1], axis=1)

    bank = fmd.StationBank(h, D, incs, FAST, SLOW, n_streams=S, device_id=0)
    ch = fmd.Channelizer(h, D, incs, n_streams=S, device_id=0)
    sb = fmd.StereoBank(h, D, incs, RATE, g, R, n_streams=S, block=1024, pilot_min=1, device_id=0)
    nb = fmd.NarrowBank(h, D, incs, g, R, n_streams=S, block=16, device_id=0)
    rb = fmd.RdsBank(h, D, incs, RATE, g, R, n_streams=S, block=1024, pilot_min=1, device_id=0)

    def refs(kind):
        if kind == "bank":
            return [sr.StationsRef(oracle, h, D, incs[s], FAST, SLOW, bank.shift, z=sr.z_corr) for s in range(S)]
        if kind == "ch":
            return [cr.ChannelizerRef(h, D, incs[s], ch.shift, z=sr.z_corr) for s in range(S)]
        if kind == "sb":
            return [st.StereoRef(h, D, incs[s], sb.shift, RATE, g, R, 1024, 1, sb.audio_shift, z=sr.z_corr) for s in range(S)]
        if kind == "nb":
            return [nr.NarrowRef(h, D, incs[s], nb.shift, nb.gr, nb.gi, nb.mode, R, nb.chan_shift, 16, nb.squelch, nb.gain, z=sr.z_corr)
                    for s in range(S)]
        return [rr.RdsRef(h, D, incs[s], rb.shift, RATE, g, R, rb.rds_shift, 1024, 1, z=sr.z_corr) for s in range(S)]

    ref = {kind: refs(kind) for kind in ("bank", "ch", "sb", "nb", "rb")}
    run = {"bank": bank.demodulate_batch, "ch": ch.run_batch, "sb": sb.run_batch, "nb": nb.run_batch, "rb": rb.run_batch}

    def step(kind, cut):
        """one call of one handle, against its definition; every call completes at least one output"""
        exp = [ref[kind][s].feed(cut[s]) for s in range(S)]
        got = run[kind](cut)
        assert got.shape[2] == len(exp[0][0]) >= 1 and _same(got, exp), kind
        return got

    # cut 1, the handles interleaved call by call
    first = {kind: step(kind, cuts[0]) for kind in ("bank", "ch", "sb", "nb", "rb")}

    # two of them back to the start: the other three continue unbroken, the two reproduce their first outputs
    sb.reset()
    nb.reset()
    assert sb.outputs() == 0 and nb.outputs() == 0
    ref["sb"], ref["nb"] = refs("sb"), refs("nb")
    step("bank", cuts[1])
    assert np.array_equal(step("sb", cuts[0]), first["sb"])
    step("ch", cuts[1])
    assert np.array_equal(step("nb", cuts[0]), first["nb"])
    # a refused call on one handle between good calls on the others: nothing changes, there or elsewhere.  8 bytes are 4 samples,
    # one front-end output; after cut 1 (593 of them) that completes no output of the stride-2 second filter
    before = rb.outputs()
    assert ref["rb"][0].completes(8) < 1
    with pytest.raises(fmd.FmdError) as e:
        rb.run_batch(data[:, :8])
    assert e.value.status == TOO_SHORT and rb.outputs() == before
    step("sb", cuts[1])
    step("rb", cuts[1])
    step("nb", cuts[1])

    step("bank", cuts[2])
    step("ch", cuts[2])
    step("sb", cuts[2])
    step("rb", cuts[2])
    step("nb", cuts[2])
    assert ch.outputs() == ref["ch"][0].m_next and rb.outputs() == ref["rb"][0].n_next
    assert sb.outputs() == ref["sb"][0].n_next and nb.outputs() == ref["nb"][0].n_next

    # freed in another order than created; a handle created afterwards starts clean
    for hd in (sb, bank, rb, ch, nb):
        hd.close()
    ch2 = fmd.Channelizer(h, D, incs, n_streams=S, device_id=0)
    ref2 = [cr.ChannelizerRef(h, D, incs[s], ch2.shift, z=sr.z_corr) for s in range(S)]
    assert _same(ch2.run_batch(cuts[0]), [ref2[s].feed(cuts[0][s]) for s in range(S)])
    ch2.close()


def test_stereo_and_rds_banks_on_the_same_bytes(fmd):
    """The two banks share their second stage (csrc/fmd_stereo_mpx.h) and differ in what they stage, where in LDS, and what they
    store.  One front end, the same bytes call by call, at the smallest shape where the shared tile can go wrong in one bank only:
    40 second-stage taps (HX = 39), stride 5 against 32, D = 2 and T = 3, so that the first 4 n bytes are n - 1 multiplex samples."""
    S2, K2, D2, TA2 = 2, 2, 2, 40
    rng = np.random.default_rng(717)
    h = rng.integers(-900, 901, 3).astype(np.int16)
    incs = np.array([[int(x) for x in rng.integers(0, 1 << 32, K2)] for _ in range(S2)], np.uint32)
    g = rng.integers(-400, 401, TA2).astype(np.int16)        # sum |g| <= 16000
    data = rng.integers(0, 256, (S2, 64 + 8400 + 136 + 8400), dtype=np.uint8)
    short, a, b, c = np.split(data, np.cumsum((64, 8400, 136)), axis=1)

    sb = fmd.StereoBank(h, D2, incs, RATE, g, 5, n_streams=S2, block=1024, pilot_min=1, device_id=0)
    rb = fmd.RdsBank(h, D2, incs, RATE, g, 32, n_streams=S2, block=1024, pilot_min=1, device_id=0)
    sref = [st.StereoRef(h, D2, incs[s], sb.shift, RATE, g, 5, 1024, 1, sb.audio_shift, z=sr.z_corr) for s in range(S2)]
    rref = [rr.RdsRef(h, D2, incs[s], rb.shift, RATE, g, 32, rb.rds_shift, 1024, 1, z=sr.z_corr) for s in range(S2)]
    assert sb.shift == rb.shift

    def pilots_agree():
        want = [sref[s].pilot(k) for s in range(S2) for k in range(K2)]
        assert want == [rref[s].pilot(k) for s in range(S2) for k in range(K2)]
        return all([bank.pilot(s, k) for s in range(S2) for k in range(K2)] == want for bank in (sb, rb))

    def step(cut, n_stereo, n_rds):
        """one call of both banks against their definitions: `cut` completes n_stereo and n_rds outputs per row"""
        got = []
        for bank, ref, n in ((sb, sref, n_stereo), (rb, rref, n_rds)):
            exp = np.stack([ref[s].feed(cut[s]) for s in range(S2)])
            got.append(bank.run_batch(cut))
            assert got[-1].shape == (S2, K2, n, 2) and np.array_equal(got[-1], exp), bank._prefix
            assert bank.outputs() == ref[0].n_next
        assert pilots_agree()
        return got

    # 64 bytes are 15 multiplex samples, fewer than the 40 taps: both refuse, nothing changes
    for bank, ref in ((sb, sref), (rb, rref)):
        assert ref[0].completes(64) < 1
        with pytest.raises(fmd.FmdError) as e:
            bank.run_batch(short)
        assert e.value.status == TOO_SHORT and bank.outputs() == 0
    assert pilots_agree()
    # 2099 multiplex samples: two tiles per row in both second passes (256 + 156 audio samples, 60 + 5 RDS outputs), two pilot
    # blocks, and the RDS staging beyond slot 32 at stride 32
    first = step(a, 412, 65)
    assert any(sref[s].pilot(k)[0] for s in range(S2) for k in range(K2))
    # 34 multiplex samples, fewer than HX: the next history is the old history's tail and the call; one RDS output exactly
    step(b, 7, 1)
    step(c, 420, 66)
    # back to the start
    for hd in (sb, rb):
        hd.reset()
    for ref in sref + rref:
        ref.reset()
    assert sb.outputs() == 0 and rb.outputs() == 0 and pilots_agree()
    again = step(a, 412, 65)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    sb.close()
    rb.close()


N, HOP, SEL = 8, 8, [1, 4, 6]                                # the plan of the uniform channelizer and the band-plan bank: K channels
CUTS_HOPS = (16 * 301, 16 * 257, 16 * 195)                   # whole hops; blocks of 16 audio samples and windows end inside calls


def test_narrow_uniform_and_bandplan_interleaved_reset_refusal_and_free(fmd):
    rng = np.random.default_rng(616)
    h = rng.integers(-900, 901, T).astype(np.int16)          # the two-digit tap form
    incs = np.array([[int(x) for x in rng.integers(0, 1 << 32, K)] for _ in range(S)], np.uint32)
    assert max(np.abs(w).max() for i in ur.channel_incs(N, SEL) for w in sr.complex_taps(h, int(i))) > 127
    gr = rng.integers(-1500, 1501, TA).astype(np.int16)      # real taps for the narrow-band bank, complex ones for the band-plan
    gi = rng.integers(-1500, 1501, TA).astype(np.int16)      # bank: both variants of the second pass run
    data = rng.integers(0, 256, (S, sum(CUTS_HOPS)), dtype=np.uint8)
    cuts = np.split(data, np.cumsum(CUTS_HOPS)[:-1], axis=1)

    nb = fmd.NarrowBank(h, D, incs, gr, R, mode="fm", n_streams=S, block=16, squelch=0, device_id=0)
    uv = fmd.UniformChannelizer(h, N, HOP, channels=SEL, n_streams=S, device_id=0)
    mk_bp = lambda: fmd.BandPlanBank(h, N, HOP, (gr, gi), R, mode="am", channels=SEL, n_streams=S, block=16, squelch=0, device_id=0)
    bp = mk_bp()
    assert nb.kernel_name(1).endswith("<false>") and bp.kernel_name(1).endswith("<true>")

    def refs(kind):
        if kind == "nb":
            return [nr.NarrowRef(h, D, incs[s], nb.shift, nb.gr, nb.gi, nb.mode, R, nb.chan_shift, 16, 0, nb.gain, z=sr.z_corr)
                    for s in range(S)]
        if kind == "uv":
            return [ur.UniformRef(h, N, HOP, uv.shift, channels=SEL) for _ in range(S)]
        return [br.BandPlanRef(h, N, HOP, bp.shift, bp.gr, bp.gi, bp.mode, R, bp.chan_shift, 16, 0, bp.gain, channels=SEL) for _ in range(S)]

    ref = {kind: refs(kind) for kind in ("nb", "uv", "bp")}
    run = {"nb": nb.run_batch, "uv": uv.run_batch, "bp": lambda cut: bp.run_batch(cut)}

    def levels_agree():
        opn, rms = bp.levels()
        want = [[ref["bp"][s].level(k) for k in range(K)] for s in range(S)]
        return opn.tolist() == [[o for o, _ in row] for row in want] and rms.tolist() == [[r for _, r in row] for row in want]

    def step(kind, cut):
        """one call of one handle, against its definition; every call completes at least one output"""
        exp = [ref[kind][s].feed(cut[s]) for s in range(S)]
        got = run[kind](cut)
        assert got.shape[2] == len(exp[0][0]) >= 1 and _same(got, exp), kind
        assert kind != "bp" or levels_agree()
        return got

    # cut 1, the handles interleaved call by call
    first = {kind: step(kind, cuts[0]) for kind in ("nb", "uv", "bp")}
    assert first["bp"].any()

    # the band-plan bank back to the start: it reproduces its first output, the other two continue unbroken
    bp.reset()
    assert bp.outputs() == 0 and not bp.levels()[0].any() and not bp.levels()[1].any()
    ref["bp"] = refs("bp")
    step("nb", cuts[1])
    assert np.array_equal(step("bp", cuts[0]), first["bp"])
    step("uv", cuts[1])
    # a refused call on it between good calls on the others: nothing changes, its inner uniform channelizer included.  16 bytes
    # are one hop, one y; after cut 1 (297 of them, 145 audio samples) the stride-2 second filter needs two more
    before, lv = bp.outputs(), bp.levels()
    assert ref["bp"][0].completes(16) < 1
    with pytest.raises(fmd.FmdError) as e:
        bp.run_batch(data[:, :16])
    assert e.value.status == TOO_SHORT and bp.outputs() == before
    assert np.array_equal(bp.levels()[0], lv[0]) and np.array_equal(bp.levels()[1], lv[1])
    step("bp", cuts[1])                                      # (had the refused call advanced pass 1, this y would be one hop off)

    step("uv", cuts[2])
    step("bp", cuts[2])
    step("nb", cuts[2])
    assert uv.outputs() == ref["uv"][0].m_next and nb.outputs() == ref["nb"][0].n_next and bp.outputs() == ref["bp"][0].n_next
    assert all(nb.level(s, k) == ref["nb"][s].level(k) for s in range(S) for k in range(K))

    # freed in another order than created; a band-plan bank created afterwards starts clean
    for hd in (uv, bp, nb):
        hd.close()
    bp = mk_bp()
    ref["bp"] = refs("bp")
    step("bp", cuts[0])
    bp.close()
