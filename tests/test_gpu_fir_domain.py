"""The tapped FIR and the fused FIR-demod kernels over every instantiation the shipped library can launch, against the oracle: the
cases of tests/fir_cases.py, each of which names the kernel every one of its calls must run.  After every call the output of every
channel (bit for bit), the output lengths, for the fused kernel the state of every channel, and kernel_name(), tap_digits() and the
tiling are compared with the claim; a case that does not run the path it claims fails.  The families that ran before this table come
first, the table-less launches last.  The last test asserts that the kernels seen are exactly the kernels the table claims.
tests/test_fir_cases.py checks the table itself without a GPU."""
import numpy as np
import pytest

import fir_cases as fc

pytestmark = pytest.mark.gpu

FIR, FUSED = fc.deterministic()
TABLELESS = [c for c in FUSED if "tableless" in c.tags]
SEEN, RAN = {"fir": set(), "fused": set()}, set()                  # kernel names reported / deterministic cases run


def diff(got, exp):
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))
    first = tuple(int(b[0]) for b in bad)
    return "%d of %d values differ, first at %r: gpu %r oracle %r" % (bad[0].size, np.asarray(exp).size, first, got[first], exp[first])


def run_fir(fmd, oracle, case, seen=None):
    bank = fmd.FirBank(case.taps, case.M, case.nch)
    ran, ci = "(nothing)", -1
    try:
        assert bank.tap_digits() == case.sel.digits, "tap_digits %d, the case claims %d" % (bank.tap_digits(), case.sel.digits)
        for ci, iq, exp in fc.reference_fir(case, oracle):
            call = case.calls[ci]
            if case.device:
                import torch
                cap = max(1, bank.out_cap(call.nbytes))
                d_iq = torch.from_numpy(iq).cuda()
                d_out = torch.zeros((case.nch, cap, 2), dtype=torch.int32, device="cuda")
                n = bank.filter_device(d_iq.data_ptr(), call.nbytes, d_out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                got = d_out.cpu().numpy()[:, :n]
            else:
                got = bank.filter_batch(iq)
            ran = bank.kernel_name()
            if seen is not None:
                seen.add(ran)
            assert got.shape == (case.nch, call.n_out, 2), "call %d: output %r, the case claims %d per channel" % (ci, got.shape, call.n_out)
            for c in range(case.nch):
                assert exp[c].shape == (call.n_out, 2)
                assert np.array_equal(got[c], exp[c]), "call %d (%s) channel %d: %s" % (ci, call.label, c, diff(got[c], exp[c]))
            assert ran == call.kernel, "call %d ran %s, the case claims %s" % (ci, ran, call.kernel)
            assert bank.tap_digits() == case.sel.digits
    except AssertionError as e:
        raise AssertionError("%s\n%s\ncall %d, last kernel: %s" % (e, fc.describe(case), ci, ran))
    finally:
        bank.close()


def gpu_state(bank, c):
    return fc.state_tuple(bank.get_state(c).as_dict())


def run_fused(fmd, oracle, case, seen=None):
    def new():
        return fmd.FirDemodBank(case.taps, case.M, case.fast, case.slow, case.nch, shift=case.shift)
    bank = new()
    ran, ci = "(nothing)", -1
    try:
        tl = bank.tiling()
        assert (tl["audio_per_tile"], tl["lds_bytes"]) == (case.sel.kt, case.sel.lds), "tiling %r, the case claims %r" % (tl, (case.sel.kt, case.sel.lds))
        assert bank.kernel_name() == fc.fused_name(case.sel), bank.kernel_name()           # before the first launch: with the table
        for ci, iq, audio, states in fc.reference_fused(case, oracle):
            call = case.calls[ci]
            if case.device:
                import torch
                cap = max(1, bank.out_cap(call.nbytes))
                d_iq = torch.from_numpy(iq).cuda()
                d_out = torch.zeros((case.nch, cap), dtype=torch.int16, device="cuda")
                k = bank.demodulate_device(d_iq.data_ptr(), call.nbytes, d_out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                bank.check()
                got = d_out.cpu().numpy()[:, :k]
            else:
                got = bank.demodulate_batch(iq)
            ran = bank.kernel_name()
            if seen is not None:
                seen.add(ran)
            assert got.shape == (case.nch, call.K), "call %d: output %r, the case claims %d per channel" % (ci, got.shape, call.K)
            for c in range(case.nch):
                assert audio[c].size == call.K
                assert np.array_equal(got[c], audio[c]), "call %d (%s) channel %d: %s" % (ci, call.label, c, diff(got[c], audio[c]))
            for c in range(case.nch):
                assert gpu_state(bank, c) == states[c], "call %d (%s) channel %d: state %r, oracle %r" % (ci, call.label, c, gpu_state(bank, c), states[c])
            assert ran == call.kernel, "call %d ran %s, the case claims %s" % (ci, ran, call.kernel)
            assert bank.tiling()["audio_per_tile"] == case.sel.kt
            if case.ckpt == ci:                                    # a fresh bank resumed from the blob takes over in the middle of the case
                blob = bank.checkpoint()
                fresh = new()
                fresh.resume(blob)
                bank.close()
                bank = fresh
                assert [gpu_state(bank, c) for c in range(case.nch)] == states
    except AssertionError as e:
        raise AssertionError("%s\n%s\ncall %d, last kernel: %s" % (e, fc.describe(case), ci, ran))
    finally:
        bank.close()


def run_group(fmd, oracle, cases, run, seen):
    assert cases
    for case in cases:
        try:
            run(fmd, oracle, case, seen=seen)
        except fmd.FmdError as e:                                  # no refusal in the deterministic table
            raise AssertionError("refused (%d): %s\n%s" % (e.status, e, fc.describe(case)))
        RAN.add((case.op, case.i))


@pytest.mark.parametrize("fam,nku", fc.groups_of(FIR), ids=lambda v: str(v))
def test_fir_instantiation(fmd, oracle, fam, nku):
    """Every deterministic case of one FIR kernel family and NKU (both single- and multi-pass shapes of that NKU)."""
    run_group(fmd, oracle, [c for c in FIR if (c.sel.family, c.sel.nku) == (fam, nku)], run_fir, SEEN["fir"])


@pytest.mark.parametrize("fam,nku", fc.groups_of(FUSED), ids=lambda v: str(v))
def test_fused_instantiation(fmd, oracle, fam, nku):
    """Every deterministic case of one fused kernel family and NKU (every column parameter NG of that NKU), one of them through
    demodulate_device + check and one with a checkpoint / resume in the middle at the family's lowest or highest NKU."""
    run_group(fmd, oracle, [c for c in FUSED if (c.sel.family, c.sel.nku) == (fam, nku) and "tableless" not in c.tags], run_fused, SEEN["fused"])


def test_fir_random_leg(fmd, oracle):
    """Seeded random cases drawn uniformly over the classes (FMD_FUZZ_CASES / FMD_FUZZ_SEED scale and move it).  No refusal is allowed."""
    n, source = fc.fuzz_source("fir")
    for _ in range(n):
        case = next(source)
        try:
            run_fir(fmd, oracle, case)
        except fmd.FmdError as e:
            raise AssertionError("refused (%d): %s\n%s" % (e.status, e, fc.describe(case)))


def test_fused_random_leg(fmd, oracle):
    """The same for the fused kernel: drawn inside the documented domain only (gain, rate range, >= 2 filter outputs per call), so no
    refusal is allowed either."""
    n, source = fc.fuzz_source("fused")
    for _ in range(n):
        case = next(source)
        try:
            run_fused(fmd, oracle, case)
        except fmd.FmdError as e:
            raise AssertionError("refused (%d): %s\n%s" % (e.status, e, fc.describe(case)))


@pytest.mark.parametrize("k", range(len(TABLELESS)), ids=lambda k: "%s-%d" % (TABLELESS[k].sel.family, TABLELESS[k].sel.cls[2]))
def test_tableless_launch(fmd, oracle, k):
    """Calls of exactly 160 and 161 tiles on one channel: the second has no per-tile table and runs the <..., false> instantiation of
    the register forms (the use_rows == 0 path of the LDS-array kernel) -- the only large cases, a few megabytes each."""
    case = TABLELESS[k]
    assert [c.nt for c in case.calls[1:3]] == [fc.FD_ROWS, fc.FD_ROWS + 1]
    run_group(fmd, oracle, [case], run_fused, SEEN["fused"])


def test_every_claimed_kernel_ran():
    """Path coverage of the deterministic sweep above: the kernels that ran are exactly the kernels the table claims."""
    assert RAN == {(c.op, c.i) for c in FIR + FUSED}, "this assertion needs the whole file: the deterministic sweep did not run (or did not pass) completely"
    for op, cases in (("fir", FIR), ("fused", FUSED)):
        claimed = {call.kernel for c in cases for call in c.calls}
        assert SEEN[op] == claimed, (sorted(claimed - SEEN[op]), sorted(SEEN[op] - claimed))
