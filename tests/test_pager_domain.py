"""The page bank's domain cases (tests/pager_domain_cases.py) without a GPU: what each case reaches, that the kernel's step in Python
(pager_cases.Model) equals the definition on it, and that it tells a wrong kernel -- a Model with one thing changed -- from the
definition.  The wrong kernels are subclasses of Model over its hooks, or change its state on entry to a call; none copies the step.

Two things the wave's copy does are not in Model, which delivers a message's bytes as Python slices: what it takes of the row's kept
320 bytes (pager_domain_cases.package) and which slot it writes (pager_domain_cases.wave_slots).  Both are held to the definition's
records here and got wrong on purpose.

What no case can tell: nothing.  Every carried field of the 32 state dwords is told by a call edge of table C (TELLS), the four high
dwords and the 64-bit n by table B (BEYOND_TELLS)."""
import numpy as np
import pytest

import pager_cases as pc
import pager_domain_cases as dc
import pager_ref as gr

U32, T32 = pc.U32, 1 << 32


def _through(dec, soft, hits, cuts, hit_cap=16):
    """([messages per call], info) of a decoder or a model pushed `soft` in calls of `cuts` and then the rest"""
    lo, out = 0, []
    for m in list(cuts) + [len(soft)]:
        part = soft[lo:lo + m]
        if len(part) == 0:
            break
        out.append(dec.push(part, [(k - lo, d, c, t) for k, d, c, t in hits if lo <= k < lo + len(part)][:hit_cap]))
        lo += len(part)
    return out, dec.info()


def _decoder(rate, e=1, n0=0):
    ref = gr.Pager(rate[0], rate[1], rate[2], e, 4, 1)
    if n0:
        dc.skip(ref, n0)
    return ref.decs[0]


def _model(cls, rate, e=1, n0=0):
    m = cls(rate[0], rate[1], rate[2], e)
    m.n0 = n0
    return m


def _differs(cls, rate, soft, hits, cuts, n0=0, want=None, e=1):
    """the first call at which the model `cls` gives other messages or counters than the definition, or None"""
    want = _through(_decoder(rate, e, n0), soft, hits, cuts) if want is None else want
    mod, lo = _model(cls, rate, e, n0), 0
    for c, m in enumerate(list(cuts) + [len(soft)]):
        part = soft[lo:lo + m]
        if len(part) == 0:
            break
        try:
            got = mod.push(part, [(k - lo, d, cc, t) for k, d, cc, t in hits if lo <= k < lo + len(part)][:16])
        except (AssertionError, IndexError):                 # a bit outside the tail and the call: no kernel to speak of
            return c
        if got != want[0][c]:
            return c
        lo += len(part)
    return None if mod.info() == want[1] else c


def _flat(per_call):
    return [m for call in per_call for m in call]


def _entry(change):
    """Model with `change` made to its state on entry to every call"""
    class Changed(pc.Model):
        def push(self, soft, hits=()):
            change(self)
            return super().push(soft, hits)
    return Changed


def _zeroed(field):
    return _entry(lambda m: setattr(m, field, type(getattr(m, field))(0)))


def _low_dword(field):
    return _entry(lambda m: setattr(m, field, getattr(m, field) & U32))


class Sum32(pc.Model):
    """the carry sum formed in 32 bits"""

    def _sum(self):
        return (self.rem + self.rd) & U32


class N32(pc.Model):
    """n = n0 + i formed in 32 bits"""

    def _n(self, n0, i):
        return (n0 + i) & U32


class SignedAbs(pc.Model):
    """mag as abs() in int32: -2^31 stays -2^31"""

    @staticmethod
    def _mag(c):
        return ((abs(c) + (1 << 31)) & U32) - (1 << 31)


class NarrowSlot(pc.Model):
    def _near(self, n):
        return abs(n - self.kp) < self.half


class NarrowSearch(pc.Model):
    def _inside(self, n):
        return n < self.kp + self.r


class AnyPolarity(pc.Model):
    def _pol(self, hinv):
        return True


# ---- A ------------------------------------------------------------------------------------------------------------------------------------
def test_the_carry_sum_passes_2_to_the_32_at_the_two_new_rates_only():
    """max(R(n) + rd) over a batch's 544 bits is above 2^32 - 1 at "wide-a", and at "wide-b" as well (there R(3) + rd = 4359738360:
    a sum kept in 32 bits is 64771064 < 2 step, the carry is missed, and p(4) comes out one sample early), and at no name of
    pager_cases.RATES."""
    over = sorted(name for name in dc.RATES if max(dc.carry_sums(name)) > U32)
    assert over == ["wide-a", "wide-b"]
    assert dc.carry_sums("wide-b")[2] == 4359738360
    first = next(n for n, t in enumerate(dc.carry_sums("wide-a"), 1) if t > U32)
    assert first <= 5                                        # p(5) is the first bit position a 32-bit sum gets wrong


@pytest.mark.parametrize("name", sorted(dc.RATES))
def test_rate_rows_model_equals_the_definition_and_the_32_bit_sum_does_not(name):
    rate = dc.RATES[name]
    x, hits = dc.rate_rows(name)
    told = []
    for row in range(5):
        for cuts in (dc.CUTS, ()):
            want = _through(_decoder(rate), x[row], hits[row], cuts)
            assert _differs(pc.Model, rate, x[row], hits[row], cuts, want=want) is None, (name, row, cuts)
            if _differs(Sum32, rate, x[row], hits[row], cuts, want=want) is not None:
                told.append(row)
        for e in (0, 2):
            assert _differs(pc.Model, rate, x[row], hits[row], (333, 1, 1, 2000), e=e) is None, (name, row, e)
        msgs, info = _flat(want[0]), want[1]
        if row < 2:
            assert [(m["address"], m["n_bits"], m["inverted"]) for m in msgs] == [(1234560, 40, row), (765437, 140, row), (9, 0, row), (77, 100, row)]
        elif row < 4:
            assert info["batches"] >= 1 and (info["bad_codewords"] or sum(m["corrected"] for m in msgs)), (name, row)
        else:
            assert info["batches"] >= 1 and len(hits[row]) >= 10
    assert (0 in told and 1 in told) == (name in ("wide-a", "wide-b")), (name, told)     # and nothing else tells it
    assert bool(told) == (name in ("wide-a", "wide-b"))


# ---- B ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
def test_skip_is_a_push_of_zeros(m):
    rng = np.random.default_rng(m)
    noise = rng.integers(-9000, 9000, (2, 100)).astype(np.int16)
    a, b = gr.Pager(*dc.B_RATE, 1, 4, 2), gr.Pager(*dc.B_RATE, 1, 4, 2)
    for ref in (a, b):
        ref.run(noise[:, :37])                               # (fewer than 64 samples before: the kept samples are not all zero)
    a.run(np.zeros((2, m), np.int16))
    dc.skip(b, m)
    assert a.pos == b.pos == 37 + m
    for x, y in zip(a.decs, b.decs):
        assert vars(x) == vars(y)
    assert np.array_equal(a.last[0], b.last[0]) and a.last[1].tobytes() == b.last[1].tobytes() and a.last[2] == b.last[2]
    a.run(noise, np.array([1, 1], np.uint32), np.array([[(5, 0, 900, 3)], [(7, 1 << 31, -900, 3)]], gr.HIT_DTYPE))
    b.run(noise, np.array([1, 1], np.uint32), np.array([[(5, 0, 900, 3)], [(7, 1 << 31, -900, 3)]], gr.HIT_DTYPE))
    assert [vars(d) for d in a.decs] == [vars(d) for d in b.decs]


# the wrong kernel and a run of pager_domain_cases.beyond_runs() that tells it, on row 0
BEYOND_TELLS = {"pnext": "b-edge", "kp": "b-edge", "xk": "a-edge", "c_end": "c-edge", "n": "a-edge"}


def _beyond_models():
    return dict({f: _low_dword(f) for f in ("pnext", "kp", "xk", "c_end")}, n=N32)


def test_beyond_runs_reach_2_to_the_32_and_tell_every_dropped_high_dword():
    x, hits = dc.beyond_rows()
    runs = dc.beyond_runs()
    assert [r[0] for r in runs] == ["a-edge", "a-inside", "b-edge", "b-inside", "c-edge", "c-inside", "d-edge", "d-inside"]
    k = hits[0][0][0]
    assert len(hits[0]) == 3 and hits[1][0][0] == k + 1 and hits[0][1][0] == k + 2720 and hits[0][2][0] + 1 == k + dc.B_THIRD
    at0 = [_flat(_through(_decoder(dc.B_RATE), x[row], hits[row], ())[0]) for row in (0, 1)]
    assert [[(m["address"] >> 3, m["function"], m["n_bits"]) for m in msgs] for msgs in at0] == [[(0x2A5A5, 1, 160), (0x155, 2, 40), (0x3FFFF, 3, 20)]] * 2
    told = {}
    for name, L, cuts in runs:
        n0 = T32 - L
        assert cuts[0] in (L, L - 2) and sum(cuts) == k + dc.B_THIRD
        for row in (0, 1):
            want = _through(_decoder(dc.B_RATE, 1, n0), x[row], hits[row], cuts)
            msgs = _flat(want[0])
            assert [dict(m, end_sample=m["end_sample"] - n0) for m in msgs] == at0[row], (name, row)
            assert all(m["end_sample"] > T32 for m in msgs)
            assert _differs(pc.Model, dc.B_RATE, x[row], hits[row], cuts, n0, want) is None, (name, row)
            if row == 0:
                for what, cls in _beyond_models().items():
                    if _differs(cls, dc.B_RATE, x[row], hits[row], cuts, n0, want) is not None:
                        told.setdefault(what, []).append(name)
    for what, name in BEYOND_TELLS.items():
        assert name in told.get(what, []), (what, told)
    # at position 0 none of them is told: it takes the position
    for what, cls in _beyond_models().items():
        assert _differs(cls, dc.B_RATE, x[0], hits[0], runs[0][2]) is None, what


# ---- C ------------------------------------------------------------------------------------------------------------------------------------
# carried field -> (rate, row, call): zeroed on entry to every call, the model first leaves the definition in that call of that row
TELLS = {"word": ("2", 0, 37), "nbm1": ("2", 0, 45), "rem": ("wide-a", 0, 63), "thr": ("2", 0, 45), "xthr": ("2", 1, 68), "xcorr": ("2", 1, 70),
         "xk": ("2", 1, 67), "kp": ("2", 0, 34), "pnext": ("2", 0, 5), "inv": ("2", 35, 32), "xinv": ("2", 41, 32), "best": ("2", 1, 70),
         "open": ("2", 0, 45), "cinv": ("2", 35, 45), "window": ("2", 6, 45), "locked": ("2", 0, 45), "c_addr": ("2", 0, 45),
         "c_func": ("2", 0, 45), "c_nbits": ("2", 0, 45), "c_corr": ("2", 0, 45), "c_end": ("2", 0, 45)}     # (rem is 0 throughout at "2" and "5")
FIELDS = ["word", "nbm1", "rem", "thr", "xthr", "xcorr", "xk", "kp", "pnext", "inv", "xinv", "best", "open", "cinv", "window", "locked",
          "c_addr", "c_func", "c_nbits", "c_corr", "c_end"]


@pytest.mark.parametrize("name", dc.C_RATES)
def test_edge_rows_model_equals_the_definition(name):
    rate = dc.RATES[name]
    x, hits, cuts = dc.edge_rows(name)
    assert x.shape[0] == 2 * dc.S and len(cuts) > 20 and set(cuts) == {dc.S}
    starts = set()
    for row in range(2 * dc.S):
        want = _through(_decoder(rate), x[row], hits[row], cuts)
        assert _differs(pc.Model, rate, x[row], hits[row], cuts, want=want) is None, (name, row)
        msgs, info = _flat(want[0]), want[1]
        first = msgs[0]
        assert (first["address"] >> 3, first["function"], first["n_bits"], first["corrected"], first["inverted"]) == (0x1B3C7, 2, 140, 1, int(row >= dc.S))
        assert info["batches"] == 3 and info["locked"] == 0      # the lock is lost behind the third batch, a message open
        assert (len(msgs), msgs[-1]["n_bits"]) == ((2, 40 + 16 * 20) if row >= dc.S else (18, 0))
        assert msgs[-1]["end_sample"] > hits[row][4][0]
        starts.add((hits[row][0][0] - hits[0][0][0], row >= dc.S))
    assert starts == {(j, inv) for j in range(dc.S) for inv in (False, True)}     # every phase of the calls against the line


@pytest.mark.parametrize("field", FIELDS)
def test_edge_rows_tell_every_carried_field(field):
    name, row, call = TELLS[field]
    x, hits, cuts = dc.edge_rows(name)
    assert _differs(_zeroed(field), dc.RATES[name], x[row], hits[row], cuts) == call


def test_edge_rows_single_sample_calls():
    x, hits, cuts = dc.edge_rows_single()
    assert cuts[1:] == [1] * 200 and hits[1][0][0] == hits[0][0][0]
    for row in (0, 1):
        assert _differs(pc.Model, dc.RATES["2"], x[row], hits[row], cuts) is None


# ---- D ------------------------------------------------------------------------------------------------------------------------------------
class Keeps(pc.Model):
    """the model, keeping the row's 320 bytes as they stand when a message closes"""
    kept = None

    def _close(self, out):
        if self.open:
            self.kept = (self.kept or []) + [bytes(self.bits)]
        super()._close(out)


def test_length_rows_every_length_and_stale_bytes_behind_a_short_message():
    (x1, h1, c1), (x2, h2, c2) = dc.length_rows(), dc.short_rows()
    lens, starts, told = set(), set(), {"behind": [], "mask": []}
    for w in dc.D_WORDS:
        dec, mod = _decoder(dc.D_RATE), _model(Keeps, dc.D_RATE)
        got = []
        for x, h, c in ((x1, h1, c1), (x2, h2, c2)):
            want = _through(dec, x[w], h[w], c)
            assert _through(mod, x[w], h[w], c) == want, w
            got += _flat(want[0])
        assert [m["n_bits"] for m in got] == [20 * w, 20 * ((w + 1) % 4)] and len(mod.kept) == 2
        assert (got[0]["address"], got[0]["inverted"]) == (8 * (w + 1), int(w % 7 == 3))
        if 0 < w <= 128:
            tail = np.unpackbits(np.frombuffer(got[0]["bits"], np.uint8))[:min(20 * w, 2560)][-20:]
            assert tail.all()                                # the last word's ones
            starts.add((20 * (w - 1)) % 8)
        lens.add(len(got[0]["bits"]) % 4)
        for m, kept in zip(got, mod.kept):
            full = m["bits"] + bytes(320 - len(m["bits"]))
            assert dc.package(kept, m["n_bits"]) == full, w
        full = got[1]["bits"] + bytes(320 - len(got[1]["bits"]))
        if dc.package(mod.kept[1], got[1]["n_bits"], zero_behind=False) != full:
            told["behind"].append(w)
        if dc.package(mod.kept[1], got[1]["n_bits"], mask=False) != full:
            told["mask"].append(w)
    assert lens == {0, 1, 2, 3} and starts == {0, 4}
    assert {dc.n_bytes(20 * ((w + 1) % 4)) % 4 for w in dc.D_WORDS} == {0, 1, 3}
    # every row but the tone-only ones in front shows bytes left behind; the rows whose second message ends inside a dword show the mask
    assert set(told["behind"]) >= set(range(8, 131)) and set(told["mask"]) >= {w for w in range(8, 131) if (w + 1) % 4 in (1, 2)}


# ---- E ------------------------------------------------------------------------------------------------------------------------------------
def _records(every, cap, **kw):
    rec = np.zeros((len(every), cap), gr.MSG_DTYPE)
    for r, slot, m in dc.wave_slots(every, cap, **kw):
        for f in ("address", "function", "n_bits", "corrected", "inverted", "end_sample"):
            rec[r, slot][f] = m[f]
        rec[r, slot]["bits"][:len(m["bits"])] = np.frombuffer(m["bits"], np.uint8)
    return rec


@pytest.mark.parametrize("cap", [1, 2, 4, 15, 16])
def test_closing_rows_close_together_at_every_slot(cap):
    x, hits = dc.closing_rows(cap)
    ref = gr.Pager(*dc.E_RATE, 1, cap, dc.E_ROWS)
    counts, rec, every = ref.run(x, *pc.pack(hits, 0, x.shape[1]))
    assert counts.tolist() == [j % (cap + 2) + 1 for j in range(dc.E_ROWS)] and counts.max() == cap + 2 and counts.min() == 1
    assert len({e[-1]["end_sample"] for e in every}) == 1 and [e[-1]["address"] >> 3 for e in every] == [0x30000 + j for j in range(dc.E_ROWS)]
    assert _records(every, cap).tobytes() == rec.tobytes()
    assert _records(every, cap, one_slot=True).tobytes() != rec.tobytes()
    if cap == 4:                                             # across two calls the count is the call's own
        two = gr.Pager(*dc.E_RATE, 1, cap, dc.E_ROWS)
        cut = hits[0][0][0] + dc.E_CUT
        a = two.run(x[:, :cut], *pc.pack(hits, 0, cut))[0].copy()
        b = two.run(x[:, cut:], *pc.pack(hits, cut, x.shape[1] - cut))[0]
        assert (a + b).tolist() == counts.tolist() and a.max() == 3 and sorted(set(b.tolist())) == [1, 2, 3]


# ---- F ------------------------------------------------------------------------------------------------------------------------------------
# the wrong kernel -> the items of F_ITEMS that tell it
RULE_TELLS = {SignedAbs: ["-2^31 after 2^31 - 1", "2^31 - 1 after -2^31", "slot 16: -2^31 after 2^31 - 1", "slot 16: 2^31 - 1 after -2^31"], NarrowSlot: ["slot 16 - half", "slot 16 + half"],
              NarrowSearch: ["second at k1 + r"], AnyPolarity: ["slot 16 other polarity"]}


@pytest.mark.parametrize("name", dc.F_RATES)
def test_rule_rows_give_what_the_table_states_and_tell_the_wrong_rules(name):
    rate = dc.RATES[name]
    x, hits = dc.rule_rows(name)
    told = {cls: [] for cls in RULE_TELLS}
    for row, item in enumerate(dc.F_ITEMS):
        want = _through(_decoder(rate), x[row], hits[row], ())
        info = want[1]
        assert (info["batches"], info["locked"], info["messages"]) == dc.RULES[name][row], (name, item)
        assert _differs(pc.Model, rate, x[row], hits[row], (), want=want) is None, (name, item)
        for cls in RULE_TELLS:
            if _differs(cls, rate, x[row], hits[row], (), want=want) is not None:
                told[cls].append(item)
    for cls, items in RULE_TELLS.items():
        assert told[cls] == items, (name, cls.__name__, told[cls])


# ---- G ------------------------------------------------------------------------------------------------------------------------------------
def test_many_rows_sample():
    sample = dc.many_sample()
    assert set([0, 63, 64, 65, 39935, 39936, 39999]) <= set(sample) and 190 <= len(sample) <= 200
    assert {dc.many_kind(r) for r in sample} == set(dc.G_KINDS)
    assert len({(r % dc.G_LINES, r % dc.G_LEADS) for r in range(dc.G_LINES * dc.G_LEADS)}) == dc.G_LINES * dc.G_LEADS
    assert len({s.tobytes() for s, _ in dc.many_lines()}) == dc.G_LINES
    for r in sample[:40]:
        soft, hits = dc.many_row(r)
        msgs, info = _through(_decoder(dc.G_RATE), soft, hits, dc.G_CUTS)
        if dc.many_kind(r) in ("page", "inverted"):
            assert info["messages"] == 1 and info["batches"] == 1 and _flat(msgs)[0]["inverted"] == int(dc.many_kind(r) == "inverted")
