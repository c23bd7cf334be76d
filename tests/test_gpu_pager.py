"""The page bank (include/fmd.h, fmd_pager_*) on the MI355X: after every call the counts, the message records of all rows (every
byte), the counters and the position bit for bit against the test-side definition (tests/pager_ref.py: a pocsag_ref.Decoder per row),
over the lane, wave and workgroup edges, rates, cuts, events on a call's first and last sample, the message cases, both capacities,
lanes that close together, records that must be passed over, unaligned rows, refusals, reset, streams, rows 2 GiB apart, and composed
with the narrow-band bank, the FSK front end and the command-line tool.

No case reads a bit from the carried tail: a bit is read at the sample that makes it due (p(1) of a new batch is never behind the
sample that anchors it: tests/test_pager.py holds that over the rate domain), so the tail is carried as the definition keeps it and
the nearest reachable cases -- a bit, a window and slot 16 due on a call's first sample -- stand in."""
import os
import subprocess

import numpy as np
import pytest

import big_cases as bc
import narrow_ref as nr
import pager_cases as pc
import pager_ref as gr
import stereo_ref as st
from big_gpu import Pitched

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, CAPACITY, UNSUPPORTED = -1, -5, -6
CUTS = (1, 7, 1000, 333)
R5 = pc.RATES["5"]
SENT16, SENT32 = 12321, 0x5A5A5A5A
U32 = pc.U32


def _pager(fmd, rate=R5, max_errors=1, cap=4, rows=1):
    return fmd.Pager(rate[0], rate[1], rate[2], max_errors, cap, n_rows=rows, device_id=0)


def _ref(rate=R5, max_errors=1, cap=4, rows=1):
    return gr.Pager(rate[0], rate[1], rate[2], max_errors, cap, rows)


def _records(fmd, pg, rows):
    rows = np.ascontiguousarray(rows, np.uint32)
    rec = np.full((len(rows), pg.msg_cap), 0x5A, np.uint8).repeat(gr.MSG_DTYPE.itemsize, axis=1).view(gr.MSG_DTYPE)
    fmd.check(fmd.lib().fmd_pager_msgs(pg._h, rows.ctypes.data, len(rows), rec.ctypes.data))
    return rec


def _same(fmd, pg, ref, what=None):
    """counts, the records of all rows (every byte), the counters and the position are the definition's after its last call"""
    counts, rec, every = ref.last
    got = _records(fmd, pg, np.arange(pg.n_rows))
    assert np.array_equal(pg.counts(), counts), (what, pg.counts().tolist(), counts.tolist())
    bad = [r for r in range(pg.n_rows) if got[r].tobytes() != rec[r].tobytes()]
    assert not bad, (what, bad)
    assert pg.info() == ref.info(), what
    assert pg.inputs() == ref.pos
    assert pg.msgs(list(range(pg.n_rows))) == [e[:pg.msg_cap] for e in every]


def _device(soft, counts, rec, in_cap=None, off=0):
    """the call in device buffers with sentinels around: soft rows in_cap apart, `off` samples behind a 16-byte boundary"""
    import torch
    rows, n = soft.shape
    in_cap = max(1, n) if in_cap is None else in_cap
    host = np.full(rows * in_cap + off + 16, SENT16, np.int16)
    host[off:off + rows * in_cap].reshape(rows, in_cap)[:, :n] = soft
    hc = np.full(rows + 8, SENT32, np.uint32)
    hc[4:4 + rows] = counts
    hr = np.full((rows * rec.shape[1] + 8) * 4, SENT32, np.uint32)
    hr[16:16 + rows * rec.shape[1] * 4] = rec.view(np.uint32).reshape(-1)
    d, dc, dr = torch.from_numpy(host).cuda(), torch.from_numpy(hc.view(np.int32)).cuda(), torch.from_numpy(hr.view(np.int32)).cuda()
    torch.cuda.synchronize()
    return (d, dc, dr), (d.data_ptr() + 2 * off, dc.data_ptr() + 16, dr.data_ptr() + 64), in_cap, (host, hc.view(np.int32), hr.view(np.int32))


def _call(fmd, pg, ref, part, counts, rec, batch=False, stream=None, off=0, odd=False, what=None):
    ref.run(part, counts, rec)
    if batch:
        pg.run_batch(part, counts, rec)
    else:
        bufs, ptrs, in_cap, hosts = _device(part, counts, rec, (part.shape[1] + 2) | 1 if odd else None, off)
        pg.run_device(ptrs[0], part.shape[1], in_cap, ptrs[1], ptrs[2], rec.shape[1], stream)
        pg.check()
        for b, h in zip(bufs, hosts):                        # the inputs and the sentinels around them
            assert np.array_equal(b.cpu().numpy(), h), what
    _same(fmd, pg, ref, what)


def _feed(fmd, pg, ref, x, hits, cuts, hit_cap=16, **kw):
    """x [rows, n] with every row's records through handle and definition in calls of `cuts` and then the rest, compared after
    every call; the messages that closed"""
    lo, total = 0, 0
    for m in list(cuts) + [x.shape[1]]:
        part = np.ascontiguousarray(x[:, lo:lo + m])
        if part.shape[1] == 0:
            break
        counts, rec = pc.pack(hits, lo, part.shape[1], hit_cap)
        _call(fmd, pg, ref, part, counts, rec, what=(lo, m), **kw)
        lo += part.shape[1]
        total += int(ref.last[0].sum())
    assert lo == x.shape[1]
    return total


def _page(fmd, r, rate=R5, **kw):
    """row r's own page: its address, function and text"""
    mode = ("alpha", "numeric", "tone")[r % 3]
    text = {"alpha": "row %d says hello" % r, "numeric": "%d-%d" % (r, 7 * r + 1), "tone": ""}[mode]
    bits = fmd.pocsag_encode([((r * 7919 + 5) & 0x1FFFFF, r % 4, text, mode)], preamble=32 + 2 * (r % 5))
    return pc.line(bits, rate, lead=8 + r % 13, invert=r % 4 == 3, dc=10 * (r % 7), **kw)


def _rows(fmd, rng, rows, rate=R5):
    """every row content of its own: a page, noise with records of its own, or nothing"""
    lines = []
    for r in range(rows):
        if r % 3 == 0 or rows < 3:
            lines.append(_page(fmd, r, rate))
        elif r % 3 == 1:
            n = 2000 + 10 * r
            ks = sorted(set(rng.integers(0, n, 6).tolist()))
            lines.append((rng.integers(-20000, 20000, n).astype(np.int16),
                          [(k, int(rng.integers(0, 3)) | (int(rng.integers(0, 2)) << 31), int(rng.integers(-99999, 99999)), int(rng.integers(-9999, 9999)))
                           for k in ks]))
        else:
            lines.append((np.zeros(100, np.int16), []))
    return pc.stack(lines)


# ---- rows, rates, cuts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 63, 64, 65, 70, 257])
def test_every_row_count_cut_and_uncut_through_both_entries(fmd, rows):
    rng = np.random.default_rng(rows)
    x, hits = _rows(fmd, rng, rows)
    pg = _pager(fmd, rows=rows)
    assert pg.kernel_name() == "fmd_pg::fmd_pager_kernel" and pg.inputs() == 0 and not pg.counts().any()
    total = _feed(fmd, pg, _ref(rows=rows), x, hits, [], batch=rows % 2 == 1)
    assert total >= (rows + 2) // 3
    pg.reset()
    assert _feed(fmd, pg, _ref(rows=rows), x, hits, CUTS, batch=rows % 2 == 0, odd=True) == total


@pytest.mark.parametrize("name", ["2", "5", "32", "11025-2400", "wide-2", "wide-32"])
def test_rates_cut_and_uncut(fmd, name):
    rate = pc.RATES[name]
    rows = 5
    x, hits = pc.stack([_page(fmd, r, rate) for r in range(rows)])
    pg = _pager(fmd, rate, rows=rows)
    assert _feed(fmd, pg, _ref(rate, rows=rows), x, hits, []) == rows
    pg.reset()
    assert _feed(fmd, pg, _ref(rate, rows=rows), x, hits, CUTS, batch=True) == rows


def test_calls_of_one_sample(fmd):
    rate = pc.RATES["2"]
    x, hits = pc.stack([_page(fmd, r, rate) for r in (2, 3)])
    k = hits[0][0][0]
    pg = _pager(fmd, rate, rows=2)
    assert _feed(fmd, pg, _ref(rate, rows=2), x, hits, [k - 20] + [1] * 120) == 2


# ---- events on a call's first and last sample ----------------------------------------------------------------------------------------------
def test_records_windows_bits_and_slot_16_at_the_call_edges(fmd):
    """With the record at sample k and r = 5: the window closes at k + 5, which is also bit 1; bit 2 lies at k + 10; slot 16 is due at
    p544 + 2 = k + 2722.  Every one of them as a call's last sample and as the next call's first; the record on a call's last sample
    has its window close in the next call."""
    bits = fmd.pocsag_encode([(77, 1, "edge", "alpha"), (85, 2, "", "tone")], preamble=32)
    two = np.concatenate([bits, bits[32:]])                  # a second batch behind the first: slot 16 finds its sync word
    x, hits = pc.stack([pc.line(two, R5), pc.line(two, R5, invert=True, lead=41), pc.line(bits, R5)])
    k = hits[0][0][0]
    assert hits[1][0][0] == k + 1 and len(hits[0]) == 4
    want = None
    for edge in (k, k + 5, k + 10, k + 2722, k + 2720):
        for cut in ([edge + 1], [edge], [edge - 1, 1, 1, 1]):
            pg, ref = _pager(fmd, rows=3), _ref(rows=3)
            got = _feed(fmd, pg, ref, x, hits, cut)
            want = got if want is None else want
            assert got == want == 10 and [i["batches"] for i in ref.info()] == [4, 4, 2]
            pg.close()


# ---- the message cases ---------------------------------------------------------------------------------------------------------------------
def _cases(fmd):
    from rtl_sdr_rs_amd.pocsag import POCSAG_IDLE as IDLE, pocsag_codeword as cw
    rng = np.random.default_rng(4)
    a1, a2 = cw(0x155 << 2 | 1), cw(0x2AA << 2 | 2)
    m = [cw(1 << 20 | v) for v in (0x12345, 0xABCDE, 0xFFFFF)]
    long_a, long_b = rng.integers(0, 2, 2560).tolist(), rng.integers(0, 2, 2580).tolist()
    lines = [pc.line(fmd.pocsag_encode([(5, 1, long_a, "bits")], preamble=32), R5),                    # 2560 bits
             pc.line(fmd.pocsag_encode([(6, 2, long_b, "bits")], preamble=32), R5, invert=True),       # 2580 bits, inverted
             pc.line(fmd.pocsag_encode([(8 * i, i % 4, "", "tone") for i in range(3)], preamble=32), R5),
             # an orphan; address 1 and a word; idle, then an orphan again; a tone-only page closed by the address behind it, whose
             # message runs to the end of the batch and is closed by the lost lock
             pc.line(fmd.pocsag_encode(None, preamble=32, words=[m[0], IDLE, a1, m[1], IDLE, m[2], a2, a1] + m * 2 + [m[0], m[1]]), R5)]
    # bad codewords inside a message: one, two and three bits off, in three message words
    w = [a1] + m * 4 + [IDLE] * 3
    bits = fmd.pocsag_encode(None, preamble=32, words=w)
    for word, flips in ((2, (3,)), (5, (7, 19)), (8, (1, 12, 30))):
        for f in flips:
            bits[32 + 32 + 32 * word + f] ^= 1
    lines.append(pc.line(bits, R5))
    return pc.stack(lines)


@pytest.mark.parametrize("max_errors", [0, 1, 2])
def test_message_cases_at_every_max_errors(fmd, max_errors):
    """2560 and 2580 message bits (open across many calls), an inverted line, tone-only pages, orphans, an idle word inside a
    message, a lost lock inside a message, and codewords one, two and three bits off inside a message."""
    x, hits = _cases(fmd)
    pg, ref = _pager(fmd, max_errors=max_errors, rows=5), _ref(max_errors=max_errors, rows=5)
    total = _feed(fmd, pg, ref, x, hits, [3000, 4000, 5000, 64, 1], batch=max_errors == 1)
    info = ref.info()
    assert info[4]["bad_codewords"] == 3 - max_errors and info[3]["orphans"] == 2 and info[2]["messages"] == 3
    assert total == sum(i["messages"] for i in info) and info[0]["messages"] == info[1]["messages"] == 1
    pg.reset()
    ref = _ref(max_errors=max_errors, rows=5)
    got = [[] for _ in range(5)]
    lo = 0
    for m in (x.shape[1] // 3, x.shape[1] // 3, x.shape[1]):             # the long messages are open across three calls
        part = np.ascontiguousarray(x[:, lo:lo + m])
        counts, rec = pc.pack(hits, lo, part.shape[1])
        _call(fmd, pg, ref, part, counts, rec)
        for r, ms in enumerate(pg.msgs(range(5))):
            got[r] += ms
        lo += m
    assert [(g[0]["n_bits"], len(g[0]["bits"]), g[0]["inverted"]) for g in got[:2]] == [(2560, 320, 0), (2580, 320, 1)]
    assert got[2][0]["n_bits"] == 0 and got[2][0]["bits"] == b""


@pytest.mark.parametrize("cap,pages", [(1, 3), (1, 17), (16, 3), (16, 17)])
def test_msg_cap_1_and_16_under_three_and_seventeen_pages_in_one_call(fmd, cap, pages):
    from rtl_sdr_rs_amd.pocsag import POCSAG_IDLE as IDLE, pocsag_codeword as cw
    words = [cw((100 + i) << 2 | i % 4) for i in range(pages)] + [IDLE]
    words += [IDLE] * (-len(words) % 16)
    rate = pc.RATES["2"]
    one = pc.line(fmd.pocsag_encode(None, preamble=32, words=words), rate)
    x, hits = pc.stack([one, pc.line(fmd.pocsag_encode(None, preamble=32, words=words), rate, invert=True), (np.zeros(10, np.int16), [])])
    pg, ref = _pager(fmd, rate, cap=cap, rows=3), _ref(rate, cap=cap, rows=3)
    assert _feed(fmd, pg, ref, x, hits, []) == 2 * pages
    assert pg.counts().tolist() == [pages, pages, 0] and [i["messages"] for i in pg.info()] == [pages, pages, 0]
    got = pg.msgs([0])[0]
    assert [m["address"] >> 3 for m in got] == [100 + i for i in range(min(cap, pages))] and pg.max_messages(x.shape[1]) >= pages


@pytest.mark.parametrize("hit_cap", [1, 64])
def test_hit_cap_1_and_64(fmd, hit_cap):
    """Both ends of the per-call domain: with hit_cap 1 a call keeps its first record only, as the definition does."""
    bits = fmd.pocsag_encode([(40, 1, "hit cap", "alpha"), (48, 2, "", "tone")], preamble=32)
    two = np.concatenate([bits, bits[32:]])
    x, hits = pc.stack([pc.line(two, R5), pc.line(two, R5, invert=True, lead=11), (np.zeros(10, np.int16), [])])
    for batch in (True, False):
        pg, ref = _pager(fmd, rows=3), _ref(rows=3)
        total = _feed(fmd, pg, ref, x, hits, [3000], hit_cap=hit_cap, batch=batch)
        assert total == (8 if hit_cap == 64 else sum(i["messages"] for i in ref.info())) and ref.info()[0]["batches"] == (4 if hit_cap == 64 else 2)
        pg.close()


def test_lanes_of_one_wave_closing_on_the_same_and_on_adjacent_steps(fmd):
    """Rows 0, 1 and 3 carry lines of one timing and close in the same turn of the wave's loop; row 2 runs a sample behind; row 63
    takes a record more (ignored while locked), which costs it a turn, so it closes a turn behind rows it shares its samples with."""
    pages = [[(8 * (r + 1), r % 4, "lane %d" % r, "alpha"), (16, 0, "", "tone")] for r in range(4)]
    lines = [pc.line(fmd.pocsag_encode(p, preamble=32), R5, lead=20 + (r == 2)) for r, p in enumerate(pages)]
    lines += [(np.zeros(10, np.int16), [])] * 59
    s, h = pc.line(fmd.pocsag_encode(pages[0], preamble=32), R5, lead=20)
    lines.append((s, h[:1] + [(h[0][0] + 400, 1, 5000, 0)] + h[1:]))
    x, hits = pc.stack(lines)
    pg, ref = _pager(fmd, rows=64), _ref(rows=64)
    assert _feed(fmd, pg, ref, x, hits, []) == 10
    ends = [[m["end_sample"] for m in ref.last[2][r]] for r in (0, 1, 2, 3, 63)]
    assert ends[0] == ends[1] == ends[3] == ends[4] and ends[2] == [e + 1 for e in ends[0]]
    assert [m[0]["address"] for m in pg.msgs([0, 1, 2, 3, 63])] == [8, 16, 24, 32, 8]


# ---- records that must be passed over -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [True, False], ids=["host", "device"])
def test_records_out_of_order_behind_the_call_and_beyond_hit_cap(fmd, batch):
    """Records with k_rel = n_in, n_in + 1 and 2^32 - 1, records out of order, and a count above hit_cap: equal to the definition,
    which passes them over, and nothing around the buffers is touched."""
    rows = 6
    x, hits = pc.stack([_page(fmd, r) for r in range(rows)])
    n = x.shape[1]
    k = [h[0][0] for h in hits]
    good = [h[0] for h in hits]
    recs = [[good[0], (n, 0, 10 ** 6, 0), good[0]],                          # k_rel = n_in blocks what is behind it
            [(n + 1, 0, 10 ** 6, 0), good[1]],
            [(U32, 1 << 31, -10 ** 6, 0), good[2]],
            [good[3], (k[3] - 5, good[3][1], 10 ** 6, 7), (k[3], good[3][1], 10 ** 6, good[3][3] + 7), (k[3] + 1, good[3][1], -3 * 10 ** 6, good[3][3] + 9)],     # out of order, then taken again
            [(k[4] - 300, 0, 1, 0)] * 3 + [good[4]],                         # four records, hit_cap 3: the page's is never read
            [good[5], (k[5] + 1, good[5][1], 2 * good[5][2], good[5][3])]]   # a better candidate inside the window
    hit_cap = 4
    counts = np.array([len(r) for r in recs], np.uint32)
    rec = np.zeros((rows, hit_cap), gr.HIT_DTYPE)
    for r, rr in enumerate(recs):
        for j, h in enumerate(rr[:hit_cap]):
            rec[r, j] = h
    counts[4], rec[4, 3] = 9, (U32, U32, -1, -1)             # count above hit_cap; hit_cap is 4 here, so the fourth is read: beyond the call
    pg, ref = _pager(fmd, rows=rows), _ref(rows=rows)
    _call(fmd, pg, ref, x, counts, rec, batch=batch)
    info = ref.info()
    assert [i["batches"] for i in info[:4]] == [1, 0, 0, 1] and info[4]["batches"] >= 1 and info[5]["batches"] == 1
    assert [i["messages"] for i in info[:4]] == [1, 0, 0, 1] and info[5]["messages"] == 1



# ---- the addresses -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [1, 3, 7])
def test_rows_at_odd_offsets_with_an_odd_in_cap(fmd, off):
    rows = 9
    x, hits = pc.stack([_page(fmd, r) for r in range(rows)])
    pg, ref = _pager(fmd, rows=rows), _ref(rows=rows)
    assert _feed(fmd, pg, ref, x, hits, [257, 64, 1001, 30, 31], off=off, odd=True) == rows


# ---- refusals and the handle's state ---------------------------------------------------------------------------------------------------
def test_refused_calls_and_calls_of_no_samples_leave_the_last_results(fmd):
    rows = 5
    x, hits = pc.stack([_page(fmd, r) for r in range(rows)])
    half = x.shape[1] - 600
    pg, ref = _pager(fmd, rows=rows), _ref(rows=rows)
    _feed(fmd, pg, ref, x[:, :half], hits, [])
    m = x.shape[1] - half
    counts, rec = pc.pack(hits, half, m)
    bufs, ptrs, in_cap, hosts = _device(np.ascontiguousarray(x[:, half:]), counts, rec)
    for args, status in (((ptrs[0], m, m - 1, ptrs[1], ptrs[2], 16), CAPACITY), ((ptrs[0] + 1, m, m, ptrs[1], ptrs[2], 16), INVALID_ARG),
                         ((0, m, m, ptrs[1], ptrs[2], 16), INVALID_ARG), ((ptrs[0], m, m, ptrs[1], ptrs[2], 0), UNSUPPORTED),
                         ((ptrs[0], m, m, ptrs[1], ptrs[2], 65), UNSUPPORTED), ((ptrs[0], m, m, ptrs[1] + 2, ptrs[2], 16), INVALID_ARG),
                         ((ptrs[0], m, m, ptrs[1], ptrs[2] + 4, 16), INVALID_ARG), ((ptrs[0], m, m, None, ptrs[2], 16), INVALID_ARG)):
        with pytest.raises(fmd.FmdError) as e:
            pg.run_device(*args)
        assert e.value.status == status, args
        _same(fmd, pg, ref)
    assert fmd.lib().fmd_pager_run_batch(pg._h, x.ctypes.data, 5, 4, counts.ctypes.data, rec.ctypes.data, 16) == CAPACITY
    _same(fmd, pg, ref)
    sel = np.array([0, rows], np.uint32)                     # a row index at or beyond n_rows: nothing is written
    out = np.full((2, pg.msg_cap), 0x5A, np.uint8).repeat(352, axis=1)
    assert fmd.lib().fmd_pager_msgs(pg._h, sel.ctypes.data, 2, out.ctypes.data) == INVALID_ARG and (out == 0x5A).all()
    before = pg.counts().copy()                              # no samples: no launch, the last call's counts and messages stay
    pg.run_device(ptrs[0], 0, m, ptrs[1], ptrs[2], 16)
    pg.run_batch(x[:, :0], counts, rec)
    ref.run(x[:, :0])
    _same(fmd, pg, ref)
    assert np.array_equal(pg.counts(), before)
    pg.run_device(ptrs[0], m, in_cap, ptrs[1], ptrs[2], 16)  # and the refused samples are taken when handed over again
    pg.check()
    ref.run(x[:, half:], counts, rec)
    _same(fmd, pg, ref)
    assert sum(i["messages"] for i in pg.info()) == rows


def test_a_selection_out_of_order_with_a_repeat_and_a_selection_of_no_rows(fmd):
    rows, rate = 5, pc.RATES["2"]                         # (about 2000 soft decisions, a page in every row)
    x, hits = pc.stack([_page(fmd, r, rate) for r in range(rows)])
    pg, ref = _pager(fmd, rate, rows=rows), _ref(rate, rows=rows)
    assert _feed(fmd, pg, ref, x, hits, [], batch=True) == rows
    every = _records(fmd, pg, np.arange(rows))
    assert every[0].tobytes() != every[4].tobytes()
    # each listed row's records in the order listed, byte for byte the identity selection's
    got = _records(fmd, pg, [4, 0, 0])
    assert [g.tobytes() for g in got] == [every[r].tobytes() for r in (4, 0, 0)]
    assert pg.msgs([4, 0, 0]) == [ref.last[2][r][:pg.msg_cap] for r in (4, 0, 0)]
    # no rows: null pointers pass, and nothing is written where there is a buffer
    assert fmd.lib().fmd_pager_msgs(pg._h, None, 0, None) == 0
    out = np.full(pg.msg_cap * gr.MSG_DTYPE.itemsize, 0x5A, np.uint8)
    assert fmd.lib().fmd_pager_msgs(pg._h, None, 0, out.ctypes.data) == 0 and (out == 0x5A).all()
    assert pg.msg_records([]) == [] and pg.msgs([]) == []
    _same(fmd, pg, ref)


def test_reset_inside_a_batch_a_callers_stream_and_two_handles(fmd):
    import torch
    xa, ha = pc.stack([_page(fmd, r) for r in range(70)])
    rate_b = pc.RATES["11025-2400"]
    xb, hb = pc.stack([_page(fmd, r, rate_b) for r in range(2)])
    a, b = _pager(fmd, rows=70), _pager(fmd, rate_b, 2, 1, rows=2)
    ra, rb = _ref(rows=70), _ref(rate_b, 2, 1, rows=2)
    stream = torch.cuda.Stream()
    n = min(xa.shape[1], xb.shape[1])
    for lo, hi in ((0, 1500), (1500, 1501), (1501, n)):      # the two handles interleaved, a on the caller's stream, b on the default one
        ca, ka = pc.pack(ha, lo, hi - lo)
        _call(fmd, a, ra, np.ascontiguousarray(xa[:, lo:hi]), ca, ka, stream=stream.cuda_stream)
        cb, kb = pc.pack(hb, lo, hi - lo)
        _call(fmd, b, rb, np.ascontiguousarray(xb[:, lo:hi]), cb, kb)
    first = _ref(rows=70)
    c0, k0 = pc.pack(ha, 0, 1500)
    first.run(xa[:, :1500], c0, k0)
    assert max(i["locked"] for i in first.info()) == 1       # sample 1500 lies inside batches
    a.reset()
    a.run_batch(xa[:, :1500], c0, k0)
    a.reset()
    assert a.inputs() == 0 and not a.counts().any() and a.info() == _ref(rows=70).info()
    assert _feed(fmd, a, _ref(rows=70), xa, ha, []) == 70
    assert b.inputs() == n and b.info() == rb.info()


def test_rows_2_gib_apart(fmd):
    """Five rows 2^31 - 6 bytes apart in the input: rows 1, 2 and 4 start just below byte 2^31, 2^32 and 2^33, and the pitch is no
    multiple of 16 bytes.  Two calls; the wide buffer is allocated and never filled, only its windows hold data (decoy samples around
    the rows), and they are unchanged behind the calls."""
    import torch
    rows = 5
    x, hits = pc.stack([_page(fmd, r) for r in range(rows)])
    cut = x.shape[1] // 2
    ns = (cut, x.shape[1] - cut)
    geo = bc.Geo(rows, 2, (1 << 31) - 6, ns, (1, 2), 6)
    big = Pitched(geo, geo.size + bc.SLACK, "decoy", 20)
    pg, ref = _pager(fmd, rows=rows), _ref(rows=rows)
    try:
        lo = 0
        for n in ns:
            part = np.ascontiguousarray(x[:, lo:lo + n])
            counts, rec = pc.pack(hits, lo, n)
            for r in range(rows):
                big.put(r, part[r])
            dc, dr = torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(rec.view(np.int32).copy()).cuda()
            torch.cuda.synchronize()
            pg.run_device(big.ptr, n, geo.cap, dc.data_ptr(), dr.data_ptr(), 16)
            pg.check()
            ref.run(part, counts, rec)
            _same(fmd, pg, ref, lo)
            big.check("the input after the call at %d" % lo)
            lo += n
        assert [i["messages"] for i in pg.info()] == [1] * rows
    finally:
        big.release()
        pg.close()


# ---- composed --------------------------------------------------------------------------------------------------------------------------
def test_narrow_bank_nfm_into_pages_into_the_page_bank_and_the_tool(fmd, tmp_path):
    """The two pages of test_gpu_fsk.py's chain, FM-modulated onto station 0 of a 240 kHz capture: NarrowBank (NFM, 12 kHz) ->
    pages(bank) -> paged(demod), each taking the one before's device buffers as they stand, the records through hits_device().  Both
    messages are delivered, equal to the host decoders over the same soft decisions and records and to the definition;
    decode_pages_gpu equals decode_pages over the same calls; pocsag_gpu -G prints what pocsag_gpu prints."""
    import torch
    from test_gpu_fsk import _fm
    fs, D, T, R, Ta, S, K = 240000, 4, 64, 5, 127, 1, 3
    rate, baud = fs // D // R, 1200
    h = st.lowpass(T, 20000 / fs)
    offs = np.array([[-70000, 20000, 85000]])
    incs = np.array([[fmd.phase_inc(int(o), fs) for o in offs[s]] for s in range(S)], np.uint32)
    nb = fmd.NarrowBank(h, D, incs, fmd.narrow_taps(fs // D, Ta, -6000, 6000), R, mode=nr.FM, n_streams=S, block=64, squelch=0, gain=256,
                        device_id=0)
    dem = fmd.pages(nb, rate, baud, device_id=0)
    pg = fmd.paged(dem, device_id=0)
    assert (pg.n_rows, pg.rate_num, pg.rate_den, pg.baud, pg.max_errors, pg.msg_cap) == (S * K, rate, dem.D, baud, 1, 4)
    ref = gr.Pager(rate, dem.D, baud, 1, 4, rows=S * K)
    sent = [(1234567, 3, "first page", "alpha"), (7654, 0, "0123-456", "numeric")]
    bits = fmd.pocsag_encode(sent, preamble=96)
    lens = (8 * 24003, 8 * 10001, 8 * 60000)
    total = sum(lens) // 2
    idx = np.floor(np.arange(total) * baud / fs).astype(np.int64) - 40
    on = (idx >= 0) & (idx < len(bits))
    msg = np.where(on, 3000.0 * (2.0 * bits[np.clip(idx, 0, len(bits) - 1)] - 1.0), 0.0)
    z = _fm(total, fs, float(offs[0, 0]), 40.0, msg) + nr.carrier(total, fs, float(offs[0, 1]), 40.0)
    data_all = nr.to_u8(z, noise=1.0, seed=0)[None]
    decs = [fmd.PocsagDecoder(rate, dem.D, baud) for _ in range(S * K)]
    lo, got, host, audio_all = 0, [[] for _ in range(S * K)], [[] for _ in range(S * K)], []
    for n in lens:
        data = np.ascontiguousarray(data_all[:, lo:lo + n])
        lo += n
        cap = nb.out_cap(n) + 3
        d_audio = torch.full((S, K, cap), -12345, dtype=torch.int16, device="cuda")
        s_cap = (dem.out_cap(cap) + 2) | 1
        d_soft = torch.full((S * K, s_cap), -12345, dtype=torch.int16, device="cuda")
        d_iq = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        m = nb.run_device(d_iq.data_ptr(), n, d_audio.data_ptr(), cap)
        k = dem.run_device(d_audio.data_ptr(), m, cap, d_soft.data_ptr(), s_cap)           # the bank's out_cap is the in_cap
        d_counts, d_hits = dem.hits_device()
        pg.run_device(d_soft.data_ptr(), k, s_cap, d_counts, d_hits, dem.hit_cap)           # the demodulator's out_cap is the in_cap
        pg.check()
        soft = d_soft.cpu().numpy()
        assert (soft[:, k:] == -12345).all()
        c, r = dem.hits()
        ref.run(soft[:, :k], c, r)
        _same(fmd, pg, ref, lo)
        audio_all.append(d_audio.cpu().numpy().reshape(S * K, cap)[:, :m])
        for row, ms in enumerate(pg.msgs(list(range(S * K)))):
            got[row] += ms
            host[row] += decs[row].push(soft[row, :k], r[row, :min(int(c[row]), dem.hit_cap)])
    texts = [fmd.pocsag_text(m, baud) for m in got[0]]
    assert texts == ["POCSAG1200: Address: 1234567  Function: 3  Alpha: first page", "POCSAG1200: Address: 0007654  Function: 0  Numeric: 0123-456  "]
    assert got == host and got[1] == [] and pg.info() == [d.info() for d in decs]
    # the same calls through both row decoders
    a = fmd.decode_pages(fmd.pages(nb, rate, baud, device_id=0), audio_all)
    b = fmd.decode_pages_gpu(fmd.pages(nb, rate, baud, device_id=0), audio_all)
    assert [{k_: v for k_, v in row.items() if k_ != "pushes"} for row in a] == b and b[0]["messages_list"] == got[0]
    # the tool over row 0's audio, with and without -G
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "pocsag_gpu")
    (tmp_path / "row0.s16").write_bytes(np.concatenate([r[0] for r in audio_all]).tobytes())
    p = subprocess.run([exe, "-r", str(rate), str(tmp_path / "row0.s16")], capture_output=True, timeout=300)
    g = subprocess.run([exe, "-r", str(rate), "-G", str(tmp_path / "row0.s16")], capture_output=True, timeout=300)
    assert p.returncode == 0 and g.returncode == 0, (p.stderr.decode(), g.stderr.decode())
    assert g.stdout == p.stdout and g.stderr == p.stderr
    assert g.stdout.decode().splitlines() == texts and g.stderr.decode().startswith("messages 2 ")
