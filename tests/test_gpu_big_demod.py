"""DemodBank through demodulate_device on both sides of the table prologue's switch, and with its output rows 2^31 - delta bytes
apart.  The table prologue forms a channel's output base as a 32-bit product, so fmd_fast_geometry takes it only while the whole
output array (n_channels * out_cap * 2 bytes) is below 2^32 bytes:
    8 channels, out_cap 2^28 - 8   the table, with channels 5 ... 7 past byte 2^31 and the array ending 128 bytes under 2^32;
    8 channels, out_cap 2^28       exactly 2^32 bytes: no table -- the closed form where the tiles repeat, else the general prologue;
    9 channels, out_cap 2^30 - delta / 2: channels 1, 2, 4 and 8 write across byte 2^31, 2^32, 2^33 and 2^34.
The cases and the kernel each call must run come from tests/big_cases.py and tests/demod_cases.py (fast_mode with out_cap);
tests/test_big_cases.py shows without a GPU where a wrapped offset would land.  The output buffer is allocated and never filled:
its windows hold the sentinel, and after every call they are compared as a whole with the oracle's audio in place -- so the audio
is the oracle's bit for bit and nothing else is written, next to the rows, behind their lengths or where a wrap would lead.  The
output lengths, the state of every channel and DemodBank.last_kernel() are compared as tests/test_gpu_demod_domain.py does."""
import numpy as np
import pytest

import big_cases as bc
import demod_cases as dc
from big_gpu import Pitched, need, random_bytes, rest_is_sentinel, rows_of
from test_gpu_demod_domain import compare, install_states
from test_gpu_parity import gpu_state, mkcfg

pytestmark = pytest.mark.gpu

SWITCH = bc.demod_switch_cases()


@pytest.mark.parametrize("case", SWITCH, ids=[c.name for c in SWITCH])
def test_table_prologue_switch(fmd, oracle, case):
    import torch
    bank = fmd.DemodBank(mkcfg(fmd, case.D, case.fast, case.slow), case.nch)
    big = None
    try:
        bank.set_tiling(case.kt)
        big = Pitched(case.geo, case.peak, "sentinel", SWITCH.index(case))
        want = dc.name(case.D, bc.demod_expected_modes(case))
        for ci, install, iq, audio, states in dc.reference(case, oracle):
            assert not install
            d_iq = torch.from_numpy(iq).cuda()
            d_len = torch.zeros(case.nch, dtype=torch.int32, device="cuda")
            big.clear()
            torch.cuda.synchronize()
            bank.demodulate_device(d_iq.data_ptr(), iq.shape[1], big.ptr, case.out_cap, d_len.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            bank.check()
            lens = d_len.cpu().numpy()
            assert np.array_equal(bank.last_out_len(), lens)
            got = [big.row(c, int(lens[c])) for c in range(case.nch)]
            ran = bank.last_kernel()
            compare(case, ci, got, lens, audio, states, bank, ran)
            assert ran == want, "call %d ran %s; at %d x %d x 2 bytes of output the switch says %s" % (ci, ran, case.nch, case.out_cap, want)
            for c in range(case.nch):
                big.put(c, audio[c], device=False)
            big.check("%s: the output of call %d" % (dc.describe(case), ci))
            assert np.array_equal(d_iq.cpu().numpy(), iq)
    finally:
        if big is not None:
            big.release()
        bank.close()


# ---- inputs of 2^32 bytes and more --------------------------------------------------------------------------------------------------

def test_synth_fill_beyond_4_gib(fmd):
    """fmd_synth_fill_device over a [65600][65552]-byte buffer against synth.synth_iq for the sampled channels: the channels that
    straddle byte 2^31 and 2^32 of the buffer, their neighbours, the first and the last."""
    import torch
    need(torch, bc.IN_CH * bc.IN_BYTES + bc.SLACK)
    d_iq = torch.empty((bc.IN_CH, bc.IN_BYTES), dtype=torch.uint8, device="cuda")
    try:
        for c in bc.sampled():
            d_iq[c] = 0
        fmd.synth.fill_device(d_iq.data_ptr(), bc.IN_CH, bc.IN_BYTES, sample_offset=12345, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for c in bc.sampled():
            exp = fmd.synth.synth_iq(1, bc.IN_BYTES, sample_offset=12345, first_channel=c)[0]
            assert np.array_equal(d_iq[c].cpu().numpy(), exp), c
    finally:
        del d_iq
        torch.cuda.empty_cache()


@pytest.mark.parametrize("name", list(bc.DEMOD_INPUTS))
def test_input_beyond_4_gib(fmd, oracle, name):
    """65600 channels x 65552 bytes of random input, two calls: the sampled channels (bc.sampled) against the oracle, which is fed
    the bytes read back from the device; their states; every channel's length; the kernel the model names; nothing written behind
    any channel's length.  One case per path that forms a channel's input address (bc.DEMOD_INPUTS)."""
    import torch
    case = bc.demod_input_case(name)
    need(torch, case.peak)
    picks = bc.sampled()
    bank = fmd.DemodBank(mkcfg(fmd, case.D, case.fast, case.slow), case.nch)
    obank = oracle.new_bank(oracle.config(case.D, case.fast, case.slow), len(picks))
    d_iq = d_out = None
    try:
        if case.kt:
            bank.set_tiling(case.kt)
        ahead = [c for c in picks if c % 2] if case.pre else []
        for c in ahead:                                            # (the odd sampled channels are a class of their own)
            j = picks.index(c)
            oracle.demodulate(obank[j], np.random.default_rng(c).integers(0, 256, case.pre, dtype=np.uint8))
            install_states(fmd, bank, {c: oracle.state_of(obank[j])})
        cap = bank.out_cap(case.nbytes) + 3
        d_iq = torch.empty((case.nch, case.nbytes), dtype=torch.uint8, device="cuda")
        d_out = torch.empty((case.nch, cap), dtype=torch.int16, device="cuda")
        d_len = torch.zeros(case.nch, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for call in range(2):
            random_bytes(torch, d_iq, 100 * call + len(name))
            d_out.fill_(bc.SENT)
            iq = rows_of(torch, d_iq, picks)
            torch.cuda.synchronize()
            bank.demodulate_device(d_iq.data_ptr(), case.nbytes, d_out.data_ptr(), cap, d_len.data_ptr(), stream)
            torch.cuda.synchronize()
            bank.check()
            assert bank.last_kernel() == case.kernels[call], (bank.last_kernel(), case.kernels[call])
            exp, elens = oracle.demodulate_batch(obank, iq)
            got, lens = rows_of(torch, d_out, picks), d_len.cpu().numpy()
            for j, c in enumerate(picks):
                assert lens[c] == elens[j], (call, c, lens[c], elens[j])
                assert np.array_equal(got[j, :elens[j]], exp[j, :elens[j]]), "call %d channel %d differs from the oracle" % (call, c)
                assert gpu_state(bank, c) == oracle.state_of(obank[j]), (call, c)
            others = np.ones(case.nch, bool)
            others[ahead] = False
            assert (lens[others] == lens[0]).all() and (not case.K or lens[0] == case.K[call][0])
            assert np.array_equal(bank.last_out_len(), lens)
            assert rest_is_sentinel(torch, d_out, d_len)
            assert np.array_equal(rows_of(torch, d_iq, picks), iq)
    finally:
        del d_iq, d_out
        bank.close()
        torch.cuda.empty_cache()


# ---- FirBank and FirDemodBank ------------------------------------------------------------------------------------------------------

FIR = bc.fir_cases()


def _fir_taps():
    return np.random.default_rng(bc.FIR_SEED).integers(-2047, 2048, bc.FIR_T).astype(np.int16)


def _fir_pair(fmd, oracle, op, nch, nref):
    """(bank, call(d_iq, nbytes, d_out, cap) -> n, the oracle's handles, ref(h, bytes) -> output, free)"""
    taps = _fir_taps()
    if op == "fir":
        bank = fmd.FirBank(taps, bc.FIR_M, nch, device_id=0)
        return bank, bank.filter_device, [oracle.fir_new(taps, bc.FIR_M) for _ in range(nref)], oracle.fir_filter, oracle.lib.fmo_fir_free
    bank = fmd.FirDemodBank(taps, bc.FIR_M, bc.FIR_FAST, bc.FIR_SLOW, nch, device_id=0)
    hs = [oracle.firdemod_new(taps, bc.FIR_M, bank.shift, bc.FIR_FAST, bc.FIR_SLOW) for _ in range(nref)]
    return bank, bank.demodulate_device, hs, oracle.firdemod, oracle.lib.fmo_firdemod_free


def _fused_state(bank, c):
    s = bank.get_state(c).as_dict()
    return (s["now_lpr"], s["prev_lpr_index"], list(s["demod_pre"]))


@pytest.mark.parametrize("case", FIR, ids=[c.name for c in FIR])
def test_fir_output_rows_across_the_lines(fmd, oracle, case):
    """Five channels whose output rows are 2^31 - delta bytes apart, two calls (the second on the carried filter history): the
    (re, im) int32 pairs of the FIR and the int16 audio of the fused bank across byte 2^31, 2^32 and 2^33, and across pair 2^31
    where the pitch is 8-byte elements; the windows as a whole against the oracle's output in place."""
    import torch
    bank, run, hs, ref, free = _fir_pair(fmd, oracle, case.op, bc.ROWS, bc.ROWS)
    big = None
    try:
        big = Pitched(case.geo, case.peak, "sentinel", FIR.index(case))
        rng = np.random.default_rng([31, FIR.index(case)])
        for call, nbytes in enumerate(bc.FIR_CALLS):
            iq = rng.integers(0, 256, (bc.ROWS, nbytes), dtype=np.uint8)
            d_iq = torch.from_numpy(iq).cuda()
            big.clear()
            torch.cuda.synchronize()
            n = run(d_iq.data_ptr(), nbytes, big.ptr, case.geo.cap, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            if case.op == "fused":
                bank.check()
            assert n == case.ns[call], (n, case.ns)
            for c in range(bc.ROWS):
                exp = ref(hs[c], iq[c])
                assert exp.shape[0] == n
                big.put(c, exp, device=False)
                if case.op == "fused":
                    assert _fused_state(bank, c) == _fused_state_of(oracle, hs[c]), (call, c)
            big.check("%s: the output of call %d" % (case.name, call))
            assert np.array_equal(d_iq.cpu().numpy(), iq)
    finally:
        if big is not None:
            big.release()
        for h in hs:
            free(h)
        bank.close()


def _fused_state_of(oracle, h):
    s = oracle.firdemod_state(h)
    return (s["now_lpr"], s["prev_lpr_index"], list(s["demod_pre"]))


@pytest.mark.parametrize("op", ["fir", "fused"])
def test_fir_input_beyond_4_gib(fmd, oracle, op):
    """65600 channels x 65552 bytes of random input through FirBank and FirDemodBank, two calls (the second reads every channel's
    filter history): the sampled channels against the oracle, fed the bytes read back from the device; the fused bank's states;
    nothing written behind the outputs of any channel."""
    import torch
    picks = bc.sampled()
    width = 2 if op == "fir" else 1
    bank, run, hs, ref, free = _fir_pair(fmd, oracle, op, bc.IN_CH, len(picks))
    d_iq = d_out = None
    try:
        cap = bank.out_cap(bc.IN_BYTES) + 3
        need(torch, bc.IN_CH * bc.IN_BYTES + bc.IN_CH * cap * 4 * width * 2 + bc.SLACK)
        d_iq = torch.empty((bc.IN_CH, bc.IN_BYTES), dtype=torch.uint8, device="cuda")
        d_out = torch.empty((bc.IN_CH, cap, width), dtype=torch.int32 if op == "fir" else torch.int16, device="cuda")
        for call in range(2):
            random_bytes(torch, d_iq, 300 + call)
            d_out.view(torch.int16).fill_(bc.SENT)
            iq = rows_of(torch, d_iq, picks)
            torch.cuda.synchronize()
            n = run(d_iq.data_ptr(), bc.IN_BYTES, d_out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            if op == "fused":
                bank.check()
            got = rows_of(torch, d_out, picks)
            for j, c in enumerate(picks):
                exp = ref(hs[j], iq[j])
                assert exp.shape[0] == n, (call, c, exp.shape, n)
                assert np.array_equal(got[j, :n].reshape(exp.shape), exp), "call %d channel %d differs from the oracle" % (call, c)
                if op == "fused":
                    assert _fused_state(bank, c) == _fused_state_of(oracle, hs[j]), (call, c)
            assert bool((d_out[:, n:].reshape(bc.IN_CH, -1).view(torch.int16) == bc.SENT).all())
            assert np.array_equal(rows_of(torch, d_iq, picks), iq)
    finally:
        del d_iq, d_out
        for h in hs:
            free(h)
        bank.close()
        torch.cuda.empty_cache()
