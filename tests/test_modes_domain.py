"""The Mode S bank's domain cases without a GPU: the case table of tests/test_gpu_modes_domain.py checking itself -- the queue indices,
the per-tile counts, the accepted formats, the tiles and the power each case is there for -- the sender against the library's, and,
for each path the cases enter, a plausible wrong kernel modelled on the definition's data: the case's comparison would differ."""
import numpy as np
import pytest

import modes_cases as mc
import modes_domain_cases as dc
import modes_ref as ref


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_case_table_checks_itself(name):
    assert dc.case(name).name == name
    dc.check_case(name)


def test_case_names_are_the_cases():
    assert [c.name for c in dc.all_cases()] == dc.CASE_NAMES and not set(dc.CASE_NAMES) & set(mc.CASE_NAMES)


def test_sender_is_the_librarys_at_its_level(fmd):
    """`put` at the default level writes what modes_encode writes, for the published messages and a DF 11 reply; frame_bits gives a
    zero syndrome (or the overlay) by the library's syndrome as well."""
    for msg in mc.LONG + [mc.short_msg(3)]:
        bits = np.unpackbits(np.frombuffer(msg, np.uint8)).tolist()
        iq = dc.quiet(1, 16 + 2 * len(bits) + 8)
        dc.put(iq, 0, 4, bits)
        assert np.array_equal(iq[0], fmd.modes_encode(msg, 60, lead=4, trail=4))
    for df, overlay in ((17, 0), (18, 0), (11, 0x55), (24, 0), (0, 0)):
        assert fmd.modes_syndrome(dc.as_bytes(dc.frame_bits(df, 9, overlay))) == overlay
    full = dc.quiet(1, 4, dc.FLOOR)
    full[0, 0:2], full[0, 2:4] = (255, 255), (0, 0)
    assert ref.magnitude(full[0]).tolist() == [dc.M_FULL, dc.M_FULL, 1, 1]


def test_a_comb_is_a_candidate_per_tooth_that_decodes_as_df_24():
    iq = dc.quiet(1, 3000)
    dc.comb(iq, 0, 100, 160)
    assert dc.candidates(iq[0]).tolist() == list(range(100, 100 + 16 * 160, 16))
    st = ref.Stream(fix_errors=1, df11=1)
    assert st.run(iq[0])[0] == 0 and st.info["candidates"] == 160
    a = np.concatenate([np.zeros(239, np.int64), ref.magnitude(iq[0])])[239 + 100:]
    assert [int(a[16 + 2 * t] > a[17 + 2 * t]) for t in range(5)] == [1, 1, 0, 0, 0]


# ---- wrong kernels --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [2, 32])
def test_a_ranking_restarted_at_every_chunk_keeps_other_positions(cap):
    """fmd_modes_tile_kernel without n_acc carried across the chunks of 64 queue entries: an acceptance's rank is its rank inside its
    own chunk, and a later chunk overwrites the kept positions of an earlier one."""
    c = dc.case("queue_long_%d" % cap)
    at, _ = dc.queue_indices(c, 0, 1)
    true = at[:cap]
    wrong = {}
    for i in at:
        rank = sum(1 for j in at if j // 64 == i // 64 and j < i)
        if rank < cap:
            wrong[rank] = i
    assert [wrong[r] for r in sorted(wrong)] != true


def test_a_fix_without_its_second_ballot_misses_the_bits_from_64_on():
    every, _ = dc.check_case("fix_every_bit_1")
    low = {ref.T112[t]: t for t in range(5, 64)}             # f0 alone
    for t in range(64, 112):
        assert ref.T112[t] not in low and every[t] and every[t][0]["fixed_bit"] == t
    # and a seam pair is no single bit's syndrome for either ballot alone
    assert all(ref.T112[a] ^ ref.T112[b] not in low for a, b in dc.DOUBLES)


def test_a_selection_without_df_18_differs():
    for df11 in (0, 1):
        c = dc.case("df_selection_%d" % df11)
        every, _ = dc.check_case(c.name)
        s = [df for df, _, _ in c.want["frames"]].index(18)
        assert every[s] and every[s][0]["df"] == 18


@pytest.mark.parametrize("name", ["tiles_many_one", "tiles_many_two"])
def test_a_gather_that_stops_at_64_tiles_loses_records_and_candidates(name):
    """Both calls of the cut case have more than 64 tiles, and acceptances and noise candidates in the tiles from 64 on."""
    c, T = dc.case(name), dc.tile()
    per_call, _ = dc.expected(name)
    pos = 0
    for (counts, recs), iq in zip(per_call, c.calls):
        n = iq.shape[1] // 2
        assert (n + T - 1) // T > 64
        assert any((r["k_rel"] + 239) // T >= 64 for r in recs[0]) and any((r["k_rel"] + 239) // T < 64 for r in recs[0])
        cand = dc.candidates(np.concatenate([x[1] for x in c.calls]))
        assert ((cand >= pos + 64 * T) & (cand < pos + n - 239)).any()
        pos += n


def test_a_power_in_too_few_bits_differs_at_full_scale():
    """m = 65025 needs all 16 bits of the plane's entries and S = 260100 more than 16: a plane of int16, or S summed in 16 bits, gives
    another power, and with it another verdict of `min_power` on one of the two sides."""
    every, _ = dc.check_case("full_scale_at")
    assert dc.M_FULL > 0x7FFF and all(r["power"] > 0xFFFF and r["power"] & 0xFFFF < dc.case("full_scale_at").cfg["min_power"] for e in every for r in e)
    assert dc.check_case("full_scale_above")[0] == [[]] * 4
    # and 6 a_j < S over the floor: a quiet slot at full scale would fail the test that a wrapped 6 * 65025 passes
    assert 6 * dc.M_FULL > 4 * dc.M_FULL > (6 * dc.M_FULL) & 0xFFFF


def test_a_cap_applied_per_tile_only_differs_over_many_tiles():
    """dense_short at 40 and 256: every tile holds fewer than msg_cap, the stream more -- only `total + k < msg_cap` cuts."""
    for cap in (40, 256):
        c = dc.case("dense_short_%d" % cap)
        every, _ = dc.check_case(c.name)
        n = c.calls[0].shape[1] // 2
        assert max(dc.dense_per_tile(dc.tile(), n, c.want["dense"])) < cap < len(every[0])
