"""The case table of the demodulation kernels (tests/demod_cases.py) against the references alone, without a GPU: the table
covers exactly the instantiations fmd_launch_tile dispatches to, every (instantiation, prologue cause) pair is present, every
call is legal, the two independent references (the C oracle and tests/pyref.py) agree on every case, and the cases contain
what they claim.  The GPU file (tests/test_gpu_demod_domain.py) then holds the kernels to the claims."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import demod_cases as dc
import oracle_lib
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = dc.deterministic()
SPECIAL = ("stream", "blocks")
CAUSES = ("table", "closed", "general-tiles", "general-channels", "general-length", "general-classes")


def dh_of(D):
    return D // 2 if D % 2 == 0 else -D


def one_class(case):
    return not case.pre


def test_table_matches_the_launch_switch():
    """An instantiation added to fmd_launch_tile without cases here fails: the FMD_CASE list IS the table's LDS list."""
    src = open(os.path.join(ROOT, "rtl-sdr-rs_amd", "csrc", "fmd_tile_launch.hip")).read()
    switch = {int(x) for x in re.findall(r"FMD_CASE\((-?\d+)\)", src)}
    assert len(switch) >= 34 and switch == {dh_of(D) for D in dc.LDS_FACTORS}
    assert {int(x) for x in re.findall(r"launch_stream<(\d+)>\(K", src)} == {D // 2 for D in dc.STREAM}
    assert "default: launch_lds<0>" in src
    assert dc.CATCH_ALL == (33, 34, 63, 65, 66, 96, 127) and not set(dc.CATCH_ALL) & set(dc.LDS_FACTORS)
    assert int(re.search(r"#define FMD_FAST_ROWS (\d+)", open(os.path.join(ROOT, "rtl-sdr-rs_amd", "csrc", "fmd_kernels.h")).read()).group(1)) == dc.FAST_ROWS
    # the names: DH = D / 2, -D for the odd factors, 0 for the catch-all
    assert dc.name(6, 2) == "fmd_tk::fmd_demod_tile_kernel<3, 2>" and dc.name(7, 0) == "fmd_tk::fmd_demod_tile_kernel<-7, 0>"
    assert dc.name(96, 1) == "fmd_tk::fmd_demod_tile_kernel<0, 1>" and dc.name(4, 2, True) == "fmd_tk::fmd_demod_stream_kernel<2, 2>"


def test_every_instantiation_and_prologue_cause():
    lds = [c for c in TABLE if not c.cause.startswith(SPECIAL)]
    for D in dc.ALL_FACTORS:
        mine = [c for c in lds if c.D == D]
        assert {c.cause for c in mine} >= set(CAUSES), (D, set(CAUSES) - {c.cause for c in mine})
        want = {"table": 2, "closed": 1, "general-tiles": 0, "general-channels": 0, "general-length": 0, "general-classes": 0}
        for c in mine:
            assert c.kt and len(c.calls) >= 3
            if c.cause in want:
                modes = [k.mode for k in c.calls]
                assert want[c.cause] in modes, dc.describe(c)
                assert all(k.kernel == dc.name(D, k.mode) for k in c.calls)
        by = {cause: [c for c in mine if c.cause == cause] for cause in CAUSES}
        assert all(k.mode == 2 and k.nt <= 32 for c in by["table"] for k in c.calls)
        assert {k.nt for c in by["table"] for k in c.calls} >= {1, 2, 32}
        # the table's boundary with tiles that repeat (33 -> closed form) and with tiles that do not (33 -> general)
        for cause, beyond in (("closed", 1), ("general-tiles", 0)):
            pairs = {(k.nt, k.mode) for c in by[cause] for k in c.calls}
            assert pairs >= {(32, 2), (33, beyond)} and all(m == (2 if nt <= 32 else beyond) for nt, m in pairs), (D, cause, pairs)
            rt = {dc.make_tiling(dc.rates(D, c.fast, c.slow, c.kt)).Rt != 0 for c in by[cause]}
            assert rt == {beyond == 0}
        assert {c.nch for c in by["general-channels"]} == {1, 7} and all(k.mode == 0 for c in by["general-channels"] for k in c.calls)
        assert any(k.nt > 32 for c in by["general-channels"] for k in c.calls)
        for c in by["general-length"]:
            assert c.nch >= 8 and all((k.nbytes % 16 == 8) == (k.mode == 0) and k.nt <= 32 for k in c.calls) and {k.mode for k in c.calls} == {0, 2}
        for c in by["general-classes"]:
            assert c.nch >= 8 and c.pre and all(k.mode == 0 and k.nbytes % 16 == 0 and k.nt <= 32 and len(set(zip(k.p0, k.i0r))) == 2 for k in c.calls)
    assert {c.nch for c in lds if c.cause in ("table", "closed")} == set(dc.FAST_CHANNELS)
    # both LDS kernels that share their factor with a streaming kernel: explicit tile, < 8 channels, odd phase
    for D in dc.STREAM:
        assert any(c.cause == "phases" and k.p0[0] % 2 and k.kernel == dc.name(D, 2) for c in lds if c.D == D for k in c.calls)


def test_streaming_cases():
    for D in dc.STREAM:
        mine = [c for c in TABLE if c.cause.startswith("stream") and c.D == D]
        assert all(c.kt is None and c.nch >= 8 and not c.block for c in mine)
        tiles = {(k.nt, k.kernel) for c in mine for k in c.calls if k.stream}
        assert tiles >= {(n, dc.name(D, 2, True)) for n in (1, 2, 32)} and all(k == dc.name(D, 2, True) for _, k in tiles)
        # 33 tiles that do not repeat: the library plans the call again for the LDS kernel, general prologue
        assert any(not k.stream and k.kernel == dc.name(D, 0) and max(k.K) > 32 * dc.stream_tile(D, c.fast, c.slow) for c in mine for k in c.calls)
        # an odd phase and back: stream -> LDS -> stream
        seq = [c for c in mine if c.cause == "stream-phase"]
        assert seq
        for c in seq:
            kinds = [(k.stream, k.p0[0] % 2) for k in c.calls]
            assert kinds[0] == (True, 0) and kinds[1] == (False, 1) and (True, 0) in kinds[2:], kinds
            assert all(k.kernel == dc.name(D, 2) and max(k.K) <= 32 for k in c.calls if not k.stream)
            assert any(not k.stream and k.p0[0] % 2 == 0 and k.nbytes < 64 * D for k in c.calls)        # too short for the streaming kernel
    # the planner's tile: 400 ... 1000 audio samples at the rates of the tests that exist
    assert dc.stream_tile(4, 256000, 48000) % 32 == 0 and 64 <= dc.stream_tile(4, 256000, 48000) <= 4096
    assert dc.stream_tile(6, 170000, 32000) is None


def test_block_cases():
    blocks = [c for c in TABLE if c.cause.startswith("blocks")]
    assert {c.D for c in blocks} == set(dc.BLOCK_FACTORS) and any(c.D not in dc.LDS_FACTORS for c in blocks)
    for D in dc.BLOCK_FACTORS:
        mine = [c for c in blocks if c.D == D]
        assert all(c.nch >= 8 and c.block % 16 == 0 and c.block // 2 >= 2 * D for c in mine)
        seen = {(k.nbytes // c.block, k.mode) for c in mine for k in c.calls}
        assert {b for b, _ in seen} == set(dc.BLOCK_COUNTS)
        assert seen >= {(1, 2), (2, 2), (5, 2), (33, 2), (33, 1)}, (D, seen)
        rel = set()
        for c in mine:
            r = dc.rates(D, c.fast, c.slow, c.kt)
            g = dc.make_tiling(r)
            if g.Rt == 0:
                tile = 2 * D * g.Qt                                # bytes of one tile
                rel.add("less" if c.block < tile else "one" if c.block == tile else "several" if c.block % tile == 0 else "other")
            if (c.block // 2) % D:
                assert len({k.p0[0] for k in c.calls}) > 1 or D == 1
                rel.add("phase")
        assert rel >= {"less", "one", "several"} | ({"phase"} if D != 2 else set()), (D, rel)


def test_phases_and_small_calls():
    calls = [(c, k) for c in TABLE for k in c.calls]
    for D in (1, 3, 5, 7):                                         # odd factors: call lengths reach every boxcar phase
        assert {k.p0[0] for c, k in calls if c.D == D and k.set_p0 is None and one_class(c)} == set(range(D)), D
    for D in range(2, 17, 2):                                      # even: the odd ones by set_state
        assert {k.p0[0] for c, k in calls if c.D == D and k.mode == 2 and not k.stream} == set(range(D)), D
    assert sum(1 for c, k in calls if max(k.K) == 0) >= 10         # calls that produce no audio
    assert {min(k.M) for c, k in calls} >= {2, 3}                  # the shortest legal calls
    # the first tile of every call has jfirst = -1 (it starts from demod_pre); tiles that start AT sample 0 or 1 (jfirst = 0) occur too
    n0 = 0
    for c, k in calls:
        if c.kt and one_class(c) and k.nt > 1:
            r = dc.rates(c.D, c.fast, c.slow, c.kt)
            P = dc.make_plan(r, k.p0[0], k.i0r[0], k.nbytes // 2)
            n0 += dc.tile_fast(r, P, dc.make_tiling(r), k.nbytes // 2, 1).jA == 1
    assert n0 >= 5


def test_data_kinds_per_case():
    for c in TABLE:
        kinds = [k.kind for k in c.calls]
        assert "random" in kinds and set(kinds) & set(dc.KINDS[1:]), dc.describe(c)
    assert {k.kind for c in TABLE for k in c.calls} == set(dc.KINDS)
    assert all(c.D >= 64 for c in TABLE for k in c.calls if k.kind == "dcflip")
    c = next(c for c in TABLE if c.nch == 17)
    iq = dc.data(c, 0)
    assert iq.shape == (17, c.calls[0].nbytes) and len({iq[ch].tobytes() for ch in range(17)}) == 17     # every channel its own data
    assert np.array_equal(iq, dc.data(c, 0))


def test_tile_limit_decides_the_names_at_32_and_33_tiles():
    """The claimed names depend on FMD_FAST_ROWS exactly at the boundary: with a limit of 31 every 32-tile call would leave the table, with
    33 every 33-tile call would stay in it."""
    n32 = n33 = 0
    for c in TABLE:
        if not c.kt or not one_class(c) or c.nch < 8:
            continue
        r = dc.rates(c.D, c.fast, c.slow, c.kt)
        for k in c.calls:
            if k.nbytes % 16:
                continue
            P = dc.make_plan(r, k.p0[0], k.i0r[0], k.nbytes // 2)
            assert P.nt == k.nt and dc.fast_mode(r, P, c.nch, k.nbytes, False) == k.mode
            if k.nt == 32:
                assert k.mode == 2 and dc.fast_mode(r, P, c.nch, k.nbytes, False, tiles_limit=31) != 2
                n32 += 1
            if k.nt == 33:
                assert k.mode != 2 and dc.fast_mode(r, P, c.nch, k.nbytes, False, tiles_limit=33) == 2
                n33 += 1
    assert n32 >= 2 * len(dc.ALL_FACTORS) and n33 >= 2 * len(dc.ALL_FACTORS)


def test_output_size_decides_the_table():
    """fmd_fast_geometry takes the table only while n_channels * out_stride * 2 < 2^32 (it addresses the output with 32-bit products):
    at the three sizes of tests/test_gpu_big_demod.py every table call of the deterministic sweep stays a table call just under 2^32
    bytes, and leaves the table at exactly 2^32 bytes and at a pitch of 2^31 - 256 bytes -- for the closed form where the tiles repeat
    and the call has what the closed form needs, else for the general prologue.  A call that is no table call is not changed by
    any of the sizes, and the default is the output far below the line that every other caller has."""
    src = open(os.path.join(ROOT, "rtl-sdr-rs_amd", "csrc", "fmd_tile_launch.hip")).read()
    assert "(uint64_t)L.n_channels * L.out_stride * 2ull < (1ull << 32)" in src
    seen = {0: 0, 1: 0}
    for c in TABLE:
        if not c.kt or not one_class(c) or c.nch < 8:
            continue
        r = dc.rates(c.D, c.fast, c.slow, c.kt)
        under = -(-(1 << 31) // c.nch) - 1                         # the largest out_cap with nch * out_cap * 2 < 2^32
        for k in c.calls:
            if k.nbytes % 16:
                continue
            P = dc.make_plan(r, k.p0[0], k.i0r[0], k.nbytes // 2)
            modes = [dc.fast_mode(r, P, c.nch, k.nbytes, False, out_cap=cap) for cap in (None, k.K[0], under, under + 1, ((1 << 31) - 256) // 2)]
            assert modes[:3] == [k.mode] * 3 and c.nch * under * 2 < 1 << 32 <= c.nch * (under + 1) * 2
            if k.mode != 2:
                assert modes[3:] == [k.mode] * 2
                continue
            closed = dc.fast_mode(r, P, c.nch, k.nbytes, False, tiles_limit=0)
            assert modes[3:] == [closed] * 2 and closed in (0, 1) and (closed == 0 or dc.make_tiling(r).Rt == 0)
            seen[closed] += 1
    assert seen[0] >= len(dc.ALL_FACTORS) and seen[1] >= len(dc.ALL_FACTORS)
    # 8 channels: out_cap 2^28 - 8 is under the line (the array ends 128 bytes below 2^32), 2^28 is on it
    assert 8 * ((1 << 28) - 8) * 2 == (1 << 32) - 128 and 8 * (1 << 28) * 2 == 1 << 32


# ---- the references ----------------------------------------------------------------------------------------------------------------

def group(g):
    if g in SPECIAL:
        return [c for c in TABLE if c.cause.startswith(g)]
    return [c for c in TABLE if c.D == g and not c.cause.startswith(SPECIAL)]


def cf_lib(oracle):
    lib = oracle.lib
    u8p, i16p = C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
    lib.fmcf_demodulate_blocks.argtypes = [C.c_uint32] * 5 + [C.POINTER(oracle_lib.ChanState), u8p, C.c_size_t, i16p, C.c_size_t]
    lib.fmcf_demodulate_blocks.restype = C.c_long
    lib.fmcf_check_plan.argtypes = [C.c_uint32] * 7
    lib.fmcf_check_plan.restype = C.c_int
    return lib


def products(D, st, buf):
    """The discriminator's complex products of one call, from the independent restatement: [(re, im)], unwrapped inputs."""
    d = pyref.Demod(D, 1, 1)
    d.prev_index, d.lp_now = st["prev_index"], tuple(st["lp_now"])
    rot = pyref.rotate_90(bytes(buf))
    lp = d.low_pass_complex([(rot[i] - 127, rot[i + 1] - 127) for i in range(0, len(rot), 2)])
    return [pyref.mul_conj(lp[i], lp[i - 1]) for i in range(1, len(lp))]


def kind_holds(D, kind, st, buf, ch):
    """What an extreme data kind is there for, on the references' own intermediate values (the discriminator's products x + j y).
    -> None where the channel carries no claim, else whether the claim holds."""
    if kind == "square":
        return set(np.unique(buf)) <= {0, 255}
    pr = products(D, st, buf)[1:]                                  # (the first product still holds the previous call's partial sum)
    F = 127 * D
    if kind == "silence":
        if ch != 0:
            return all(abs(x) + abs(y) <= 2 * (3 * D) ** 2 for x, y in pr)
        # channel 0: every decimated sample is (0, s), so every product has y == 0, with x of either sign (signed zeros)
        return all(y == 0 for x, y in pr) and any(x > 0 for x, y in pr) and any(x < 0 for x, y in pr)
    if kind == "axis":
        # full scale on an axis: two whole windows of one stretch give y = +-0 with |x| >= F^2 (x = +-0 with |y| >= F^2 needs a change of
        # axis exactly between two windows, which the boxcar phase of the call decides)
        return any(y == 0 and abs(x) >= F * F for x, y in pr)
    if kind == "diag":
        if ch % 4 not in (1, 2):
            return None
        # (4096 * s) as i32 wraps from s = 2^19 on, which 2 (128 D)^2 reaches at downsample 4; below that the diagonal product itself
        wraps = [abs(4096 * ((x - abs(y)) if x >= 0 else (x + abs(y)))) >= 1 << 31 for x, y in pr]
        if D < 4:
            return not any(wraps) and any(y == 0 and x >= 2 * F * F for x, y in pr)
        return all(wraps) if ch % 4 == 2 else any(wraps)           # channel 2 is the saturated constant: every product is the wrap point
    if kind == "dcflip":
        if ch != 0:
            return None
        # rotated full-scale DC: two whole windows of one sign (the largest product) and a flip between windows of opposite sign
        return any(y == 0 and x >= 2 * F * F for x, y in pr) and any(x <= -F * F for x, y in pr)
    raise ValueError(kind)


def test_data_kinds_hold_at_every_factor(oracle):
    """Every extreme kind sits, at every factor, on a call of a table or closed-form case that is long enough to hold it (>= 96
    decimated samples), and there the references show what the kind is for -- e.g. the diagonal calls contain the wrap product of
    `(4096 * s) as i32` at every factor from 4 on."""
    seen = set()
    for case in TABLE:
        if case.cause not in ("table", "closed"):
            continue
        od = oracle.new_bank(oracle.config(case.D, case.fast, case.slow), case.nch)
        for ci, call in enumerate(case.calls):
            iq = dc.data(case, ci)
            if call.kind != "random" and min(call.M) >= 96:
                assert call.nbytes <= 65536 and call.mode in (1, 2)
                for ch in (0, 1, 2):
                    ok = kind_holds(case.D, call.kind, oracle.state_of(od[ch]), iq[ch], ch)
                    assert ok is not False, (dc.describe(case), ci, ch)
                    if ok:
                        seen.add((call.kind, case.D, ch))
            oracle.demodulate_batch(od, iq)
    for D in dc.ALL_FACTORS:
        for kind, chs in (("square", (0, 1, 2)), ("axis", (0, 1, 2)), ("silence", (0, 1, 2)), ("diag", (1, 2)), ("dcflip", (0,) if D >= 64 else ())):
            assert {ch for k, d, ch in seen if (k, d) == (kind, D)} >= set(chs), (kind, D)


@pytest.mark.parametrize("g", dc.ALL_FACTORS + SPECIAL, ids=str)
def test_references_agree_and_calls_are_legal(oracle, g):
    """Per case: no call is refused or would make the reference panic; the model's phases and sample counts are the oracle's;
    pyref gives the oracle's audio and state (two channels per case: one in rotation and the last, the last alone where a call exceeds 256 KiB; the channels are independent in both
    references); the closed-form model of the kernels' decomposition (oracle/closed_form.cpp) with the case's tile gives them too, within
    the LDS sizing -- that and fmcf_check_plan are what the fmcf_* entry points expose of the prologue decision; the choice between
    table, closed form and general prologue itself (fmd_fast_geometry) is host code of the library that they do not expose, so the
    claimed mode is left to the GPU assertion (tests/demod_cases.py restates it; test_tile_limit_decides_the_names_at_32_and_33_tiles
    pins the restatement's boundary)."""
    lib = cf_lib(oracle)
    cases = group(g)
    assert cases
    for case in cases:
        D, nch = case.D, case.nch
        chs = sorted({case.i % nch, nch - 1})
        if max(k.nbytes for k in case.calls) > 1 << 18:
            chs = chs[-1:]                                         # (pyref is a per-sample Python loop: the MiB calls of the streaming cases on the last channel only)
        panics0 = oracle.lib.fmo_would_panic()
        pds = {ch: pyref.Demod(D, case.fast, case.slow) for ch in chs}
        for ch in chs:
            if case.pre and ch % 2:
                pds[ch].demodulate(dc.prefeed(case))
        gdiv = dc.rates(D, case.fast, case.slow, 1).g
        for ci, install, iq, audio, states in dc.reference(case, oracle):
            call = case.calls[ci]
            n = call.nbytes
            assert n % 8 == 0 and iq.shape == (nch, n) and min(call.M) >= 2, dc.describe(case)
            assert {a.size for a in audio} == set(call.K), (dc.describe(case), ci)
            for ch in chs:
                pd = pds[ch]
                if call.set_p0 is not None:
                    pd.prev_index, pd.lp_now = call.set_p0, dc.lp_for(call.set_p0, ch)
                if ch in install:
                    assert pd.state() == install[ch], (dc.describe(case), ci)
                st0 = pd.state()
                # the model's bookkeeping is the oracle's
                cls = 1 if case.pre and ch % 2 else 0
                assert st0["prev_index"] == call.p0[cls] and st0["prev_lpr_index"] == call.i0r[cls] * gdiv, (dc.describe(case), ci)
                assert audio[ch].size == call.K[cls], (dc.describe(case), ci)
                step = case.block or n
                got = [v for o in range(0, n, step) for v in pd.demodulate(iq[ch, o:o + step])]
                assert np.array_equal(np.array(got, np.int16), audio[ch]), (dc.describe(case), ci, ch)
                assert pd.state() == states[ch], (dc.describe(case), ci, ch)
                if not case.kt:
                    continue
                assert lib.fmcf_check_plan(D, case.fast, case.slow, case.kt, call.p0[cls], call.i0r[cls], n // 2) == 0
                st = oracle_lib.ChanState(st0["prev_index"], st0["prev_lpr_index"] // gdiv, st0["now_lpr"], st0["lp_now"][0], st0["lp_now"][1],
                                          st0["demod_pre"][0], st0["demod_pre"][1], 0)
                buf = np.ascontiguousarray(iq[ch])
                out = np.empty(n // 2 + 16, np.int16)
                K = lib.fmcf_demodulate_blocks(D, case.fast, case.slow, case.kt, case.block // 2, C.byref(st), buf.ctypes.data_as(C.POINTER(C.c_uint8)), n,
                                               out.ctypes.data_as(C.POINTER(C.c_int16)), out.size)
                assert K == audio[ch].size and np.array_equal(out[:K], audio[ch]), (dc.describe(case), ci, ch, K)     # (< 0: -100 / -101 the LDS sizing)
                assert max(1, -(-K // case.kt)) == max(1, -(-max(call.K) // case.kt)) or case.pre
                assert (st.prev_index, st.lpr_index_r * gdiv, st.now_lpr, [st.lp_now_re, st.lp_now_im], [st.demod_pre_re, st.demod_pre_im]) == (
                    states[ch]["prev_index"], states[ch]["prev_lpr_index"], states[ch]["now_lpr"], states[ch]["lp_now"], states[ch]["demod_pre"])
        assert oracle.lib.fmo_would_panic() == panics0, dc.describe(case)


def test_random_leg_is_legal_and_reproducible():
    n, source = dc.fuzz_source()
    a = [next(source) for _ in range(n)]
    n2, source2 = dc.fuzz_source()
    b = [next(source2) for _ in range(n2)]
    assert n >= 40 and [dc.describe(c) for c in a] == [dc.describe(c) for c in b]
    for c in a:
        assert 8 <= c.nch <= 40 and len(c.calls) >= 3 and all(k.nbytes % 16 == 0 and min(k.M) >= 2 for k in c.calls)
        assert c.kt or c.D in dc.STREAM
    assert len({c.D for c in a}) >= 15 and {k.mode for c in a for k in c.calls} == {0, 1, 2}
    assert any(c.block for c in a) and any(k.stream for c in a for k in c.calls)
