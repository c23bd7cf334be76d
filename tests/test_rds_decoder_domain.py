"""RDS decoder (include/fmd.h, fmd_rds_decoder_*) over what its header documents, without a GPU: every sample rate class from
4 kHz to 32 kHz, a residual carrier up to +-20 Hz at any phase, version-B groups with C', the text A/B flag, 0x0D, a group type it
does not interpret, and its block synchronisation under damage -- one failed block, 9 and 10 failed blocks in a row, a lost bit.

The signal is tests/rds_ref.py's baseband_direct: the biphase waveform of a BIT stream on a residual carrier, plus noise, at the
level of the full-chain fixture of tests/test_rds.py (the first test anchors the shortcut to that fixture).  A bit flipped before
the differential coding is exactly one wrong decoded bit, so every expectation is exact: which blocks fail, which groups come
out, when the lock goes and returns.  Every case is decoded twice, in one push and in random pieces (pieces of 0 and 1 samples
among them), and both must agree."""
import numpy as np
import pytest

import rds_ref as rr
from test_rds import baseband  # noqa: F401  (module fixture: the full chain's baseband of 0.7 s of the test station)

FS = 8000.0
CYCLE = rr.groups_0a_2a(rr.PI, rr.PS, rr.RT)                      # 8 groups: 0A, 2A, 0A, 2A ...
FILL = [CYCLE[1]]                                            # after the last group under test: the decoder lags by about a bit


def _fmd():
    import rtl_sdr_rs_amd as fmd
    return fmd


def _push(num, den, u, pieces):
    dec = _fmd().RdsDecoder(num, den)
    groups, pos = [], 0
    for n in pieces:
        groups += dec.push(u[pos:pos + n])
        pos += n
    assert pos == u.shape[0]
    return groups, dec.info()


def decode(u, num=8000, den=1):
    """(groups, info) of u, pushed whole -- and pushed in random pieces, which must give the same."""
    whole = _push(num, den, u, [u.shape[0]])
    rng = np.random.default_rng(u.shape[0])
    pieces = [1, 0, 2, 0, 1]
    while sum(pieces) < u.shape[0]:
        pieces.append(min(int(rng.choice([0, 1, int(rng.integers(2, 40)), int(rng.integers(40, 3000))])), u.shape[0] - sum(pieces)))
    assert pieces.count(0) >= 3 and pieces.count(1) >= 3
    assert _push(num, den, u, pieces) == whole
    return whole


def flip(bits, block, j=5):
    """One flipped bit (bit j, an information bit) in block `block` (counted from the stream's start).  The damaged block cannot
    pass: the remainder of one bit is not zero, and here it is not the difference of C and C' either."""
    e = rr.remainder(1 << (25 - j), 26)
    assert e != 0 and e != rr.OFFSETS["C"] ^ rr.OFFSETS["C'"]
    bits[26 * block + j] ^= 1


def sample_of_bit(k, fs=FS, bit_rate=rr.BIT_RATE, start_bit=0.0):
    """The sample at which bit k (as received: after any deleted bit) has passed."""
    return int((k - start_bit) * fs / bit_rate)


def check_sent(groups, sent, masks=None, fs=FS, bit_rate=rr.BIT_RATE, start_bit=0.0, lost_bits=0, last=None):
    """Every delivered group after the first is a group of `sent`: its first_sample is the centre of the first bit of sent group
    idx (within a bit), consecutive groups have consecutive idx, every block flagged valid holds what was sent, and ok_mask is
    masks[idx] (15 where not given).  The first delivered group may begin before the lock: its valid blocks are checked against
    the group before the second.  Returns the idx of the delivered groups.  `lost_bits`: bits deleted from the stream before
    these groups.  `last`: the delivered groups reach at least this idx."""
    assert len(groups) >= 3
    idx = []
    for g in groups[1:]:
        k = g["first_sample"] * bit_rate / fs + start_bit - 0.5 + lost_bits
        i = int(round(k / 104))
        assert abs(k - 104 * i) <= 1.0, (g, k)
        idx.append(i)
    assert idx == list(range(idx[0], idx[0] + len(idx)))
    idx = [idx[0] - 1] + idx
    for n, (g, i) in enumerate(zip(groups, idx)):
        if n > 0:
            assert g["ok_mask"] == (masks or {}).get(i, 15), (i, g)
        for b in range(4):
            if g["ok_mask"] >> b & 1:
                assert g["blocks"][b] == sent[i][b], (i, b)
    if last is not None:
        assert idx[-1] >= last
    return idx


def locks_early(groups, fs=FS, bit_rate=rr.BIT_RATE):
    """The first delivered group begins within the first three groups of the signal."""
    return groups[0]["first_sample"] < 3 * 104 * fs / bit_rate


# ---- the shortcut is the full chain's baseband ----------------------------------------------------------------------------------

def test_direct_baseband_decodes_as_the_full_chain(baseband):  # noqa: F811
    """The same station, bit clock (pilot / 16), start (10 bits into the cycle) and residual (+6 Hz): the same groups with the same
    checks, PI, PS and RadioText from both.  first_sample differs by the delay of the bank's two filters, a constant."""
    fmd = _fmd()
    u, sent = baseband
    dec = fmd.RdsDecoder(rr.FS, rr.D * rr.R)
    want, info = dec.push(u), dec.info()
    d = rr.baseband_direct(np.tile(rr.group_bits(sent), 2), FS, f_res=6.0, phase=0.3, seed=1, start_bit=rr.START_BIT,
                           bit_rate=rr.PILOT_HZ / 16)[:u.shape[0]]
    rms = lambda a: float(np.sqrt((a.astype(np.float64) ** 2).sum(axis=1).mean()))
    assert 0.8 < rms(d) / rms(u[300:]) < 1.25                       # the level of the fixture (after its filters have filled)
    got, ginfo = decode(d)
    assert [(g["blocks"], g["ok_mask"]) for g in got] == [(g["blocks"], g["ok_mask"]) for g in want] and len(got) == 8
    assert ginfo == info and info["pi"] == rr.PI and info["ps"] == rr.PS and info["rt"] == rr.RT
    lag = {g["first_sample"] - w["first_sample"] for g, w in zip(got[1:], want[1:])}
    assert max(lag) - min(lag) <= 1 and got[0]["first_sample"] == want[0]["first_sample"] == 0


# ---- rates and residual carrier -----------------------------------------------------------------------------------------------------

def _clean_case(num, den, f_res, phase, seed):
    fs = num / den
    sent = CYCLE * 2 + FILL
    u = rr.baseband_direct(rr.group_bits(sent), fs, f_res=f_res, phase=phase, seed=seed)
    assert 1.0 <= u.shape[0] / fs <= 2.0
    groups, info = decode(u, num, den)
    assert locks_early(groups, fs)
    idx = check_sent(groups, sent, fs=fs, last=len(sent) - 2)
    assert idx[0] <= 2 and info["synced"] and info["blocks_bad"] == 0
    assert info["groups_ok"] >= len(groups) - 1
    assert (info["pi"], info["ps"], info["rt"]) == (rr.PI, rr.PS, rr.RT)


@pytest.mark.parametrize("num,den", [(4000, 1), (4750, 1), (8000, 1), (256000, 27), (32000, 1)])
def test_rates(num, den):
    """The limits, 4 samples per bit exactly (4750), the bank's usual rate, a rate that is no integer (9481.48 Hz)."""
    _clean_case(num, den, 3.0, 1.0, num)


@pytest.mark.parametrize("phase", [0.0, np.pi / 2, np.pi, 3 * np.pi / 2])
@pytest.mark.parametrize("f_res", [-20.0, -6.0, 0.0, 6.0, 20.0])
def test_residual_carrier(f_res, phase):
    _clean_case(8000, 1, f_res, phase, int(f_res) + 100)


# ---- content ----------------------------------------------------------------------------------------------------------------------

def test_version_b_groups_and_pi_from_c_prime():
    text = "Thirty-two characters through 2B"
    assert len(text) == 32
    sent = rr.groups_0b_2b(rr.PI, rr.PS, text) + FILL
    assert len(sent) == 21 and all(g[1] >> 11 & 1 for g in sent[:-1])
    bits = rr.group_bits(sent)
    c_prime = rr.encode_block(rr.PI, "C'")
    assert rr.remainder(c_prime, 26) == 0x350 and [int(b) for b in bits[52:78]] == [c_prime >> i & 1 for i in range(25, -1, -1)]
    groups, info = decode(rr.baseband_direct(bits, FS, f_res=4.0, seed=2))
    check_sent(groups, sent, last=19)
    assert (info["pi"], info["ps"], info["rt"], info["blocks_bad"]) == (rr.PI, rr.PS, text, 0)
    # block A of every group damaged: the PI can only come from C'
    for g in range(len(sent)):
        flip(bits, 4 * g)
    groups, info = decode(rr.baseband_direct(bits, FS, f_res=4.0, seed=2))
    idx = check_sent(groups, sent, masks={i: 14 for i in range(len(sent))}, last=19)
    assert (info["pi"], info["ps"], info["rt"]) == (rr.PI, rr.PS, text) and info["groups_ok"] == 0 and info["synced"]
    # locked on blocks B and C' of group 0; from there block A of every group, the filler's too, fails once and the lock holds
    assert idx[0] == 0 and groups[0]["ok_mask"] == 14 and info["blocks_bad"] == len(sent) - 1


def test_64_characters_through_2a():
    text = "Sixty-four characters of RadioText fill all sixteen 2A segments."
    assert len(text) == 64
    sent = rr.groups_0a_2a(rr.PI, rr.PS, text) + FILL
    groups, info = decode(rr.baseband_direct(rr.group_bits(sent), FS, f_res=-5.0, seed=3))
    check_sent(groups, sent, last=19)
    assert (info["pi"], info["ps"], info["rt"], info["blocks_bad"]) == (rr.PI, rr.PS, text, 0)


def test_carriage_return_ends_the_text():
    text = "RDS ends here\rthis is not shown."
    assert len(text) == 32 and text[13] == "\r"
    sent = rr.groups_0a_2a(rr.PI, rr.PS, text) + FILL
    groups, info = decode(rr.baseband_direct(rr.group_bits(sent), FS, seed=4))
    check_sent(groups, sent, last=11)
    assert info["rt"] == "RDS ends here" and info["ps"] == rr.PS


def test_text_flag_flip_clears_the_buffer():
    one, two = "The first text, all of it, 32 ch", "Second text."
    assert len(one) == 32 and len(two) == 12
    first = rr.groups_0a_2a(rr.PI, rr.PS, one, flag=0)                          # 12 groups
    flipped = [g for g in rr.groups_0a_2a(rr.PI, rr.PS, two, flag=1) if g[1] >> 12 == 2]
    assert len(first) == 12 and len(flipped) == 3 and all(g[1] >> 4 & 1 for g in flipped)
    sent = first + [CYCLE[0]] + flipped + FILL
    u = rr.baseband_direct(rr.group_bits(sent), FS, f_res=2.0, seed=5)
    _, before = decode(u[:sample_of_bit(104 * 13)])               # up to the end of the 0A group behind the first text
    assert before["rt"] == one
    groups, info = decode(u)
    check_sent(groups, sent, last=15)
    assert info["rt"] == two and info["ps"] == rr.PS and info["blocks_bad"] == 0


def test_a_group_type_the_decoder_does_not_read_comes_out_raw():
    odd = rr.raw_group(rr.PI, 4 << 12 | 0x2A5, 0x1234, 0xABCD)                  # 4A
    sent = CYCLE + [odd] + CYCLE[:2] + FILL
    groups, info = decode(rr.baseband_direct(rr.group_bits(sent), FS, f_res=-3.0, seed=6))
    idx = check_sent(groups, sent, last=10)
    g = groups[idx.index(8)]
    assert g["blocks"] == odd and g["ok_mask"] == 15
    assert (info["pi"], info["ps"], info["rt"], info["blocks_bad"]) == (rr.PI, rr.PS, rr.RT, 0)


# ---- damage -------------------------------------------------------------------------------------------------------------------------

def test_a_failed_block_is_not_used():
    """PS "TEST FM " complete, then a cycle with "ABCDEFGH" whose segment 1 ("CD") has one flipped bit in block D."""
    sent = CYCLE + rr.groups_0a_2a(rr.PI, "ABCDEFGH", rr.RT) + FILL
    bad = 10                                                       # 0A, segment 1 of the second cycle
    assert sent[bad][1] >> 11 == 0 and sent[bad][1] & 3 == 1 and sent[bad][3] == ord("C") << 8 | ord("D")
    bits = rr.group_bits(sent)
    flip(bits, 4 * bad + 3)
    groups, info = decode(rr.baseband_direct(bits, FS, f_res=5.0, seed=7))
    idx = check_sent(groups, sent, masks={bad: 7}, last=15)
    assert groups[idx.index(bad)]["ok_mask"] & 8 == 0
    assert info["ps"] == "ABSTEFGH" and info["rt"] == rr.RT and info["pi"] == rr.PI
    assert info["blocks_bad"] == 1 and info["synced"]
    assert info["groups_ok"] == sum(g["ok_mask"] == 15 for g in groups) == len(groups) - 1 - (groups[0]["ok_mask"] != 15)


def _damaged(n_blocks):
    """Three cycles; one flipped bit in each of n_blocks consecutive blocks from block A of group 6 on."""
    sent = CYCLE * 3 + FILL
    bits = rr.group_bits(sent)
    for b in range(24, 24 + n_blocks):
        flip(bits, b)
    masks = {}
    for b in range(24, 24 + n_blocks):
        masks[b // 4] = masks.get(b // 4, 15) & ~(1 << b % 4)
    return sent, rr.baseband_direct(bits, FS, f_res=-4.0, phase=2.0, seed=8), masks


def test_nine_failed_blocks_in_a_row_keep_the_lock():
    sent, u, masks = _damaged(9)
    assert masks == {6: 0, 7: 0, 8: 14}
    _, mid = decode(u[:sample_of_bit(26 * 33 + 8)])               # right after the ninth
    assert mid["synced"] and mid["blocks_bad"] == 9
    groups, info = decode(u)
    idx = check_sent(groups, sent, masks=masks, last=23)
    assert info["synced"] and info["blocks_bad"] == 9
    # the grid never moved: the groups after the damage begin where those before it lead, 104 bits apart.  Both strobes of a
    # difference are rounded to a sample (+-1/2 each) and the timing estimate may move by one more under noise.
    after = [g["first_sample"] for g, i in zip(groups, idx) if i >= 5]
    spg = 104 * FS / rr.BIT_RATE
    assert len(after) >= 15 and all(abs(b - a - spg) <= 2 for a, b in zip(after[:-1], after[1:]))
    assert (info["pi"], info["ps"], info["rt"]) == (rr.PI, rr.PS, rr.RT)


def test_ten_failed_blocks_in_a_row_drop_the_lock():
    sent, u, masks = _damaged(10)
    assert masks == {6: 0, 7: 0, 8: 12}
    _, mid = decode(u[:sample_of_bit(26 * 33 + 8)])               # right after the ninth: still locked
    assert mid["synced"] and mid["blocks_bad"] == 9
    _, mid = decode(u[:sample_of_bit(26 * 34 + 8)])               # right after the tenth; two valid blocks need 52 bits more
    assert not mid["synced"] and mid["blocks_bad"] == 10
    groups, info = decode(u)
    # locked again on blocks C and D of group 8, the first two valid blocks in sequence, and group 8 comes out with those two.
    # Five bits behind block C the stream happens to hold 26 bits that divide to offset word B: a decoder that remembers one
    # candidate only loses block C to that match and locks a block later, without group 8.
    check_sent(groups, sent, masks=masks, last=23)
    assert info["synced"] and info["blocks_bad"] == 10
    assert (info["pi"], info["ps"], info["rt"]) == (rr.PI, rr.PS, rr.RT)


def test_a_lost_bit_drops_the_lock_and_it_returns():
    """One bit deleted inside block B of group 6: every block from there on is cut one bit late and fails, the lock goes with the
    tenth (blocks 25 ... 34 of the old grid) and returns on the new grid, where the groups are the ones sent."""
    sent = CYCLE * 3 + FILL
    bits = np.delete(rr.group_bits(sent), 6 * 104 + 30)
    u = rr.baseband_direct(bits, FS, f_res=4.0, phase=1.0, seed=9)
    _, mid = decode(u[:sample_of_bit(26 * 35 + 8)])
    assert not mid["synced"] and mid["blocks_bad"] == 10
    groups, info = decode(u)
    assert info["synced"] and info["blocks_bad"] == 10
    cut = next(n for n, g in enumerate(groups) if g["first_sample"] > sample_of_bit(104 * 6))
    head = check_sent(groups[:cut], sent)
    assert head[-1] == 5 and locks_early(groups)
    # groups 6 ... 8 of the old grid come out empty; the first group of the new grid may lack the blocks before the lock
    tail = [g for g in groups[cut:] if g["ok_mask"]]
    assert [g["ok_mask"] for g in groups[cut:] if not g["ok_mask"]] == [0] * (len(groups) - cut - len(tail)) and len(tail) >= 14
    idx = check_sent(tail, sent, lost_bits=1, last=23)
    assert idx[0] <= 10
    assert (info["pi"], info["ps"], info["rt"]) == (rr.PI, rr.PS, rr.RT)
