"""The demodulation kernels (fmd_demod_*) over every instantiation fmd_launch_tile can pick and every prologue, against the
oracle: the cases of tests/demod_cases.py, each of which names the kernel every one of its calls must run.  After every call
the audio of every channel (bit for bit), the output lengths, the state of every channel and DemodBank.last_kernel() are
compared; a case that does not run the path it claims fails.  The last test asserts that the kernels seen are exactly the
kernels the table claims.  tests/test_demod_cases.py checks the table itself without a GPU."""
import numpy as np
import pytest

import demod_cases as dc
from test_gpu_parity import gpu_state, mkcfg

pytestmark = pytest.mark.gpu

TABLE = dc.deterministic()
SPECIAL = ("stream", "blocks")
SEEN, RAN = set(), set()                                           # kernel names reported / deterministic cases run


def group(g):
    if g in SPECIAL:
        return [c for c in TABLE if c.cause.startswith(g)]
    return [c for c in TABLE if c.D == g and not c.cause.startswith(SPECIAL)]


def install_states(fmd, bank, install):
    for c, s in install.items():
        bank.set_state(c, fmd.DemodState(prev_index=s["prev_index"], now_lpr=s["now_lpr"], prev_lpr_index=s["prev_lpr_index"],
                                         lp_now_re=s["lp_now"][0], lp_now_im=s["lp_now"][1],
                                         demod_pre_re=s["demod_pre"][0], demod_pre_im=s["demod_pre"][1]))


def compare(case, ci, got, lens, audio, states, bank, ran):
    for c in range(case.nch):
        assert lens[c] == audio[c].size, "call %d channel %d: %d samples, oracle %d" % (ci, c, lens[c], audio[c].size)
        if not np.array_equal(got[c], audio[c]):
            bad = np.nonzero(got[c] != audio[c])[0]
            raise AssertionError("call %d channel %d: %d of %d samples differ, first at %d: gpu %d oracle %d" % (
                ci, c, bad.size, audio[c].size, bad[0], got[c][bad[0]], audio[c][bad[0]]))
    for c in range(case.nch):
        assert gpu_state(bank, c) == states[c], "call %d channel %d: state %r, oracle %r" % (ci, c, gpu_state(bank, c), states[c])
    assert ran == case.calls[ci].kernel, "call %d ran %s, the case claims %s" % (ci, ran, case.calls[ci].kernel)


def run_case(fmd, oracle, case, device=False, seen=None):
    """Feeds the case to a DemodBank and to the oracle.  FmdError passes through (the random leg replaces a refused draw)."""
    bank = fmd.DemodBank(mkcfg(fmd, case.D, case.fast, case.slow), case.nch)
    ran = "(nothing)"
    try:
        if case.kt:
            bank.set_tiling(case.kt)
        if case.block:
            bank.set_block_len(case.block)
        for ci, install, iq, audio, states in dc.reference(case, oracle):
            install_states(fmd, bank, install)
            if device:
                import torch
                n, cap = iq.shape[1], bank.out_cap(iq.shape[1])
                d_iq = torch.from_numpy(iq).cuda()
                d_out = torch.zeros((case.nch, cap), dtype=torch.int16, device="cuda")
                d_len = torch.zeros(case.nch, dtype=torch.int32, device="cuda")
                bank.demodulate_device(d_iq.data_ptr(), n, d_out.data_ptr(), cap, d_len.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                bank.check()
                lens, out = d_len.cpu().numpy(), d_out.cpu().numpy()
                assert np.array_equal(bank.last_out_len(), lens), "call %d: d_out_len %r, last_out_len %r" % (ci, lens, bank.last_out_len())
                got = [out[c, :lens[c]] for c in range(case.nch)]
            else:
                got = bank.demodulate_batch(iq)
                lens = [g.size for g in got]
            ran = bank.last_kernel()
            if seen is not None:
                seen.add(ran)
            compare(case, ci, got, lens, audio, states, bank, ran)
    except AssertionError as e:
        raise AssertionError("%s\n%s\nlast kernel: %s" % (e, dc.describe(case), ran))
    finally:
        bank.close()


@pytest.mark.parametrize("g", dc.ALL_FACTORS + SPECIAL, ids=str)
def test_instantiation(fmd, oracle, g):
    """Every deterministic case of one downsample factor (or: the streaming kernel's cases, the block cases)."""
    cases = group(g)
    assert cases
    for case in cases:
        try:
            run_case(fmd, oracle, case, seen=SEEN)
        except fmd.FmdError as e:                                  # no refusal in the deterministic table
            raise AssertionError("refused (%d): %s\n%s" % (e.status, e, dc.describe(case)))
        RAN.add(case.i)


@pytest.mark.parametrize("k", range(3))
def test_device_entry(fmd, oracle, k):
    """One case per prologue through demodulate_device on torch-owned buffers, with d_out_len."""
    case = dc.device_cases(TABLE)[k]
    assert {c.mode for c in case.calls} >= {(2, 1, 0)[k]}
    run_case(fmd, oracle, case, device=True)


def test_random_leg(fmd, oracle):
    """Seeded random cases over the whole instantiation list (FMD_FUZZ_CASES / FMD_FUZZ_SEED scale and move it): >= 8 channels
    and lengths that are multiples of 16, so the fast prologues are what they mostly run.  A legal refusal (too short,
    capacity, unsupported) replaces the draw -- up to 10 replacements per wanted case: a library that refuses nearly everything fails."""
    n, source = dc.fuzz_source()
    done = refused = 0
    while done < n:
        case = next(source)
        try:
            run_case(fmd, oracle, case)
        except fmd.FmdError as e:
            assert e.status in (-3, -5, -6), "%s\n%s" % (e, dc.describe(case))
            refused += 1
            assert refused <= 10 * n, "%d draws refused for %d run; the last: %s\n%s" % (refused, done, e, dc.describe(case))
            continue
        done += 1


def test_every_claimed_kernel_ran():
    """Path coverage of the deterministic sweep above: the kernels that ran are exactly the kernels the table claims."""
    assert RAN == {c.i for c in TABLE}, "this assertion needs the whole file: the deterministic sweep did not run (or did not pass) completely"
    claimed = {call.kernel for c in TABLE for call in c.calls}
    assert SEEN == claimed, (sorted(claimed - SEEN), sorted(SEEN - claimed))
