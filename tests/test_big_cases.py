"""The layout table of the beyond-2-GiB tests (tests/big_cases.py), checked without a GPU: every case straddles the lines it claims,
and under every wrong-arithmetic model the address a wrong kernel would touch differs from the true one, lies inside the allocation
and lies inside a window that the GPU test fills and checks -- so a kernel that wraps fails an assertion instead of passing or
faulting.  Also each case's peak device memory, from its own arithmetic, against the cap of 32 GiB."""
import numpy as np
import pytest

import big_cases as bc

ROW_CASES = bc.row_cases()
DEMOD_CASES = bc.demod_switch_cases()
FIR_CASES = bc.fir_cases()
BANK_CASES = bc.bank_cases()
ALL = ([(c.name, c.geo, c.geo.claims(), c.peak) for c in ROW_CASES + FIR_CASES + BANK_CASES] + [(c.name, c.geo, c.claims, c.peak) for c in DEMOD_CASES])
IDS = [a[0] for a in ALL]


def _watched(geo, name, wrong, true):
    """The three assertions of one model over the elements `wrong` / `true` (byte offsets from the pointer)."""
    assert (wrong != true).all(), (name, "the wrong address is the true one")
    assert (wrong >= -geo.margin).all() and (wrong + geo.elem <= geo.end).all(), (name, "outside the allocation")
    assert geo.inside(wrong).all() and geo.inside(wrong + geo.elem - 1).all(), (name, "outside every window")


@pytest.mark.parametrize("name,geo,claims,peak", ALL, ids=IDS)
def test_every_claimed_line_is_straddled_and_every_alias_is_watched(name, geo, claims, peak):
    models = geo.models()
    assert claims
    for r, k, u, kind in claims:
        line = (1 << k) * u
        for n in geo.ns:
            j = np.arange(n, dtype=np.int64)
            if kind == "straddle":
                assert geo.base(r) + bc.EDGE * geo.elem <= line <= geo.base(r) + (n - bc.EDGE) * geo.elem, (name, r, k, u, n)
                beyond = j[geo.true(r, j) >= line]                 # the elements at and behind the line
                assert beyond.size >= bc.EDGE
                which = "whole"
            else:
                assert geo.base(r) >= line, (name, r, k, u)
                beyond, which = j, "product"
            seen = 0
            for signed in (False, True):
                if bc.watches(which, k, signed):
                    _watched(geo, (name, r, k, u, which, signed), models[(which, u, signed)](r, beyond), geo.true(r, beyond))
                    seen += 1
            assert seen


@pytest.mark.parametrize("name,geo,claims,peak", ALL, ids=IDS)
def test_no_alias_of_any_access_goes_unwatched(name, geo, claims, peak):
    """Every element every call touches, under every model: the address is the true one, or it is inside the allocation and inside a
    window.  The true addresses are inside windows too (they are what the test reads back)."""
    for n in geo.ns:
        j = np.arange(n, dtype=np.int64)
        for r in range(geo.rows):
            true = geo.true(r, j)
            assert geo.inside(true).all() and (true + geo.elem <= geo.end).all(), (name, r)
            # the 64 elements on each side of the live span are watched as well
            assert geo.inside(true[0] - bc.EDGE * geo.elem) and geo.inside(true[-1] + (bc.EDGE + 1) * geo.elem - 1), (name, r)
            for key, f in geo.models().items():
                wrong = f(r, j)
                bad = wrong != true
                if bad.any():
                    _watched(geo, (name, r, key), wrong[bad], true[bad])


@pytest.mark.parametrize("name,geo,claims,peak", ALL, ids=IDS)
def test_windows_and_memory(name, geo, claims, peak):
    w = geo.windows()
    assert all(a[1] <= b[0] for a, b in zip(w, w[1:])) and w[0][0] >= -geo.margin and w[-1][1] <= geo.end
    assert sum(hi - lo for lo, hi in w) < 64 << 20                 # what a test writes and reads back is small
    assert geo.margin == (1 << 31) * max(geo.units) and geo.size == geo.margin + geo.end
    assert geo.size < peak <= bc.MEMORY_CAP, (name, peak / bc.GiB)
    assert geo.cap * geo.elem == geo.pitch


def test_the_table_covers_what_it_should():
    """Every row processor at each of its widths, input and output pitched, a 16-byte aligned and an unaligned pitch; rows 1, 2 and 4
    straddle bytes 2^31, 2^32 and 2^33; both element lines are crossed at width 1 and the W-sample line at width 2."""
    seen = {(c.handle, c.width, c.side, c.geo.aligned) for c in ROW_CASES}
    assert seen == {(h, w, s, a) for h in bc.HANDLES for w in bc.WIDTHS[h] for s in ("in", "out") for a in (True, False)}
    for c in ROW_CASES:
        claims = set(c.geo.claims())
        assert {(1, 31, 1, "straddle"), (2, 32, 1, "straddle"), (4, 33, 1, "straddle"), (2, 31, 2, "straddle"), (4, 32, 2, "straddle")} <= claims
        assert (c.width == 1) or (4, 31, 4, "straddle") in claims
        assert c.geo.ns == (c.n_in if c.side == "in" else c.n_out)


def test_demod_switch_cases():
    """The three sizes of the switch: just under 2^32 bytes of output the table, at exactly 2^32 bytes and with 9 rows of 2^31 - delta
    bytes never; the model's claim (demod_cases.fast_mode with out_cap) is what the statement of the switch says."""
    names = {c.name for c in DEMOD_CASES}
    assert len(names) == len(DEMOD_CASES) == 8
    for c in DEMOD_CASES:
        size = c.nch * c.out_cap * 2
        assert (size < 1 << 32) == c.name.startswith("under")
        assert c.name.startswith("under") == (size == (1 << 32) - 128) and c.name.startswith("exact") == (size == 1 << 32)
        want = bc.demod_expected_modes(c)
        assert [call.mode for call in c.calls] == [want] * len(c.calls), (c.name, [call.mode for call in c.calls])
        assert all(call.nt <= 32 for call in c.calls) == (not c.name.startswith("wide"))
        assert all(call.nbytes % 16 == 0 and call.nbytes < 1 << 20 for call in c.calls)


def test_input_cases_are_beyond_4_gib():
    """The unpitched inputs: 65600 channels of 65552 bytes are more than 2^32 bytes, a channel straddles each of byte 2^31 and 2^32 at
    least 64 bytes from either end, at least 8 channels are compared, every call is a multiple of 16 bytes (the fast prologues), the
    cases run the prologues and kernels they are there for, and none needs more than the cap."""
    assert bc.IN_CH * bc.IN_BYTES >= 1 << 32 and bc.IN_BYTES > 65536 and bc.IN_BYTES % 16 == 0 and bc.IN_CH > 65535
    assert (1 << 31) % bc.IN_BYTES and (1 << 32) % bc.IN_BYTES
    picks = bc.sampled()
    assert len(picks) >= 8 and picks[0] == 0 and picks[-1] == bc.IN_CH - 1
    for k in (31, 32):
        c = (1 << k) // bc.IN_BYTES
        assert {c - 1, c, c + 1} <= set(picks) and c * bc.IN_BYTES + bc.EDGE <= 1 << k <= (c + 1) * bc.IN_BYTES - bc.EDGE
    import demod_cases as dc
    seen = set()
    for name in bc.DEMOD_INPUTS:
        c = bc.demod_input_case(name)
        assert c.peak <= bc.MEMORY_CAP and len(c.kernels) == 2
        if name == "generic":
            assert c.D > 128
            continue
        stream = name == "stream"
        assert c.kernels == [dc.name(c.D, bc.DEMOD_INPUT_MODES[name], stream)] * 2, (name, c.kernels)
        assert (len(c.K[0]) == 2) == (name == "classes")
        seen.add("stream" if stream else "even" if c.D % 2 == 0 and c.D <= 14 else "odd" if c.D % 2 else "wide")
    assert seen == {"stream", "even", "odd", "wide"}               # fmd_tile_stream.hip, fmd_tile_lds_even / _odd / _wide.hip


def test_fir_cases():
    md, K = bc.fir_counts()
    assert md == [2289, 2048] and K == [763, 682]
    assert {c.name for c in FIR_CASES} == {"fir-out-1024", "fir-out-1032", "fused-out-256", "fused-out-264"}
    assert [c.geo.aligned for c in FIR_CASES] == [True, False, True, False]


def test_bank_cases():
    """Every bank as 5 x 1 and as 1 x 5 rows, one of them on 16-byte rows and one not; every bank of packed uint32 outputs once more
    with row 4 across element 2^32."""
    for kind, (width, _) in bc.BANKS.items():
        mine = [c for c in BANK_CASES if c.kind == kind]
        assert {(c.S, c.K) for c in mine} == {(5, 1), (1, 5)} and {c.geo.aligned for c in mine} == {True, False}
        assert all(c.S * c.K == c.geo.rows == 5 and c.geo.elem == 2 * width for c in mine)
        wide = [c for c in mine if c.geo.grid == 1 << 32]
        assert len(wide) == (1 if width == 2 else 0)
        for c in wide:
            assert (4, 32, 4, "straddle") in c.geo.claims() and (2, 31, 4, "straddle") in c.geo.claims()


def test_bank_input_cases():
    """65535 streams of 65552 bytes are more than 2^32 bytes and a stream straddles each line; the narrow-band and the band-plan bank's
    internal stage ([S K][ystride] packed uint32) passes 2^32 bytes as well; none needs more than the cap."""
    S, n = bc.BANK_IN_S, bc.IN_BYTES
    assert S * n >= 1 << 32 and n % (2 * bc.BI.HOP) == 0 and S == 65535
    picks = bc.sampled(S, n)
    assert len(picks) >= 8 and picks[-1] == S - 1 and {(1 << k) // n for k in (31, 32)} <= set(picks)
    for kind in bc.BANK_INPUTS:
        i, o, stage = bc.bank_input_bytes(kind)
        assert i >= 1 << 32 and bc.bank_input_peak(kind) <= bc.MEMORY_CAP, (kind, bc.bank_input_peak(kind) / bc.GiB)
        if kind in ("narrow", "bandplan"):
            assert stage >= 1 << 32, (kind, stage)
