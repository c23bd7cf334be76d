"""The pulse bank's domain cases without a GPU: the case table of tests/test_gpu_pulses_domain.py checking itself -- the owed edges and
keep tiles at the seams of the summaries, the boxes, the threshold limits -- the helper that stands in for 2^30 constant samples
against a real run, the saturation script's expectation, and two plausible wrong kernels modelled on the definition's data."""
import numpy as np
import pytest

import pulses_cases as pc
import pulses_domain_cases as dc
import pulses_ref as ref


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_case_table_checks_itself(name):
    assert dc.case(name).name == name
    dc.check_case(name)


def test_case_names_are_the_cases():
    assert [c.name for c in dc.all_cases()] == dc.CASE_NAMES and not set(dc.CASE_NAMES) & set(pc.CASE_NAMES)
    assert {c.cfg["pulse_cap"] for c in dc.all_cases()} >= {3, 100}              # capacities that are no power of two


def test_the_scaled_settings_put_medium_between_the_thresholds():
    for W in dc.BOXES:
        _, lo, hi = dc.scaled(W)
        assert W * pc.M_QUIET < lo <= W * pc.M_MEDIUM < hi <= W * pc.M_STRONG
    assert dc.scaled(8) == pc.SETTINGS[8]


@pytest.mark.parametrize("lvl,state", [(pc.QUIET, 0), (pc.STRONG, 1), (pc.MEDIUM, 0), (pc.MEDIUM, 1)])
def test_advance_is_a_real_run_of_constant_samples(lvl, state):
    """n = 10^5 samples equal to the carried ones: `advance` leaves the stream as Stream.run over the materialised bytes does."""
    n = 100000
    lead = dc.small((pc.QUIET, 50), (pc.STRONG, 50), (pc.QUIET if state == 0 else pc.STRONG, 30), (lvl, 70))
    a, b = (ref.Stream(*pc.SETTINGS[8]) for _ in range(2))
    assert a.run(lead[0]) == b.run(lead[0]) and a.state == state
    assert dc.advance(a, n) == b.run(dc.small((lvl, n))[0]) == (0, [])
    assert a.info == b.info and (a.pos, a.state, a.run_len, a.gap) == (b.pos, b.state, b.run_len, b.gap) and np.array_equal(a.tail, b.tail)
    tail = dc.small((pc.QUIET, 80), (pc.STRONG, 40), (pc.QUIET, 80))
    assert a.run(tail[0]) == b.run(tail[0]) and a.info == b.info
    mixed = dc.small((pc.QUIET, 30), (pc.STRONG, 30))
    a.run(mixed[0])
    with pytest.raises(AssertionError):
        dc.advance(a, 10)                                    # the carried samples differ: the box would move


def test_the_saturation_script_reaches_2_32():
    out = dc.check_saturation()
    assert all(x.shape[1] % 8 == 0 for kind, x in dc.saturation_script() if kind == "bytes")
    assert 2 * dc.STRETCH == 1 << 31                         # the largest call the bank takes


# ---- wrong kernels --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 64])
def test_a_gather_that_stops_at_64_tiles_loses_records_and_state(W):
    """One call: records fall in tiles 64 and beyond, and the final state and run are made there.  Three calls: the third has 66
    tiles, with records behind its 64th."""
    T = dc.tile()
    per_call, info = dc.expected("tiles_many_%d_one" % W)
    counts, recs = per_call[0]
    for s in range(8):
        assert any(r["k_rel"] // T >= 64 for r in recs[s]), s
    stop = ref.run_bank(dc.case("tiles_many_%d_one" % W).cfg, [dc.case("tiles_many_%d_one" % W).calls[0][:, :2 * 64 * T]], 8)
    assert stop[0][0][0] != counts and [i["state"] for i in stop[1]] != [i["state"] for i in info]
    per_call, _ = dc.expected("tiles_many_%d_three" % W)
    assert any(r["k_rel"] // T >= 64 for rr in per_call[2][1] for r in rr)


@pytest.mark.parametrize("W", dc.BOXES)
def test_a_box_rounded_to_a_power_of_two_gives_other_records(W):
    """Q[x] - Q[x - W'] with W' the next power of two (or one sample off) in place of W: the traffic's records differ."""
    c = dc.case("boxes_%d_pair" % W)
    per_call, _ = dc.expected(c.name)
    for other in (1 << W.bit_length(), W - 1, W + 1):
        assert ref.run_bank(dict(c.cfg, W=other), c.calls, c.n_streams)[0] != per_call, (W, other)


def test_a_comparator_off_by_one_at_hi_sets_nothing_at_the_limits():
    """`e > hi` in place of `e >= hi`: the block of saturated samples never sets."""
    for name in ("limits_top", "limits_wide"):
        c = dc.case(name)
        st = ref.Stream(c.cfg["W"], c.cfg["lo"], c.cfg["hi"])
        st.hi += 1
        for iq in c.calls:
            st.run(iq[0])
        assert st.info["rises"] == 0 and dc.expected(name)[1][0]["rises"] == 1, name


def test_without_saturation_the_gap_the_width_and_the_run_wrap():
    """sat32 missing: the low 32 bits of a run beyond 2^32 are neither 2^32 - 1 nor the run."""
    out = dc.saturation_expected()
    runs = (out[5][2]["run"], out[11][2]["run"])
    for run in runs:
        assert run > ref.SAT and (run & ref.SAT) != ref.SAT and (run & ref.SAT) + 200 < ref.SAT
    recs = [r for _, rr, _ in out for r in rr]
    assert recs[1]["gap"] == ref.SAT and recs[2]["width"] == ref.SAT
