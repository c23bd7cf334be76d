"""FSK front end of the pager decoder (include/fmd.h, fmd_fsk_*) on the MI355X: every output, every count and every record bit for bit
against the test-side definition (tests/fsk_ref.py) after every call, and the composed chain narrow-band bank -> FskDemod ->
PocsagDecoder against narrow_ref -> fsk_ref -> the decoder, with decode_pages and pocsag_gpu over the same audio."""
import os
import subprocess

import numpy as np
import pytest

import fsk_ref as fr
import narrow_ref as nr
from rows_gpu import SENT, call as _call, call_at
import stereo_ref as st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = -5


def _demod(fmd, cfg, rows):
    return fmd.FskDemod(cfg.D, cfg.W, cfg.shift, cfg.tap, cfg.sync, cfg.tol, cfg.min_corr, cfg.hit_cap, n_rows=rows, device_id=0)


def _hits_equal(dem, counts, rec):
    c, r = dem.hits()
    return np.array_equal(c, counts) and np.array_equal(r.view(np.uint32), rec.view(np.uint32)) and np.array_equal(dem.hit_counts(), counts)


def _feed(dem, ref, x, cuts, batch=False):
    """x [rows, n] through handle and definition in calls of `cuts`, compared after every call; the total hits"""
    lo, total = 0, 0
    for m in cuts:
        part = x[:, lo:lo + m]
        want, counts, rec = ref.run(part)
        got = dem.run_batch(part) if batch else _call(dem, part[:, :, None])[:, :, 0]
        assert got.shape == want.shape and np.array_equal(got, want), (lo, m)
        if part.shape[1]:                                    # (a call of no samples launches nothing: the last call's hits stay)
            assert _hits_equal(dem, counts, rec), (lo, m)
        assert dem.counts() == (ref.pos, ref.outputs())
        lo += part.shape[1]
        total += int(counts.sum())
    assert lo == x.shape[1]
    return total


SHAPES = [(1, 1, 31), (1, 5, 155), (2, 4, 155), (9, 5, 255), (19, 5, 155), (64, 16, 255)]


@pytest.mark.parametrize("D,W,last", SHAPES, ids=["D%d-W%d-t%d" % s for s in SHAPES])
def test_definition_parity_cut_and_uncut(fmd, D, W, last):
    rng = np.random.default_rng(1000 * D + W)
    cfg = fr.random_cfg(rng, D, W, last, tol=3, min_corr=0, hit_cap=64)
    rows, n = 3, min(30000, 700 * D + 5)
    x = fr.laid_signal(rng, cfg, rows, n)
    x[1] = rng.integers(-32768, 32768, n)                    # a random row
    x[2, : n // 2] = 0                                       # a row that begins with zeros
    dem = _demod(fmd, cfg, rows)
    assert dem.kernel_name() == "fmd_fk::fmd_fsk_kernel" and dem.counts() == (0, 0)
    total = _feed(dem, fr.FskDemod(cfg, rows), x, [n])
    assert total >= 3
    dem.reset()
    assert _feed(dem, fr.FskDemod(cfg, rows), x, [7, 1000, 333, n], batch=True) == total
    dem.reset()
    # calls that end before, on and behind a box end and a chunk end (64 boxes), and calls of one sample
    span = 64 * D
    cuts = [D - 1, 1, 1, span - D - 1, 1, 1, span + 1, 2 * span - 1, 1, 0, 3 * span] if D > 1 else [1, 1, 62, 1, 1, 65, 127, 1, 0, 192]
    cuts = [c for c in cuts if c >= 0] + [1] * 5 + [n]
    assert _feed(dem, fr.FskDemod(cfg, rows), x, cuts) == total


@pytest.mark.parametrize("rows", [1, 3, 70])
def test_every_row_count_with_the_designed_detector_through_both_entries(fmd, rows):
    rng = np.random.default_rng(rows)
    d = fmd.fsk_design(12000, 1200)
    cfg = fr.Cfg(d.D, d.W, d.shift, d.tap, d.sync, d.tol, d.min_corr, d.hit_cap)
    bits = fmd.pocsag_encode([(1234, 1, "row", "alpha")], preamble=64)
    n = 10 * len(bits) + 400
    x = np.zeros((rows, n), np.int16)
    for r in range(rows):                                    # the word at another phase, polarity and DC in every row
        lvl = np.where(np.repeat(bits, 10) == 1, 3000, -3000) * (-1 if r % 3 == 2 else 1)
        dc = int(rng.integers(-2500, 2500))
        x[r] = dc + rng.normal(0, 300, n)
        x[r, 37 + 3 * r % 300:37 + 3 * r % 300 + len(lvl)] += lvl.astype(np.int16)
    x[rows // 2] = 0                                         # an all-zero row
    ref = fr.FskDemod(cfg, rows)
    dem = _demod(fmd, cfg, rows)
    assert _feed(dem, ref, x, [1000, 3001, n]) >= 2 * (rows - 1)
    dem.reset()
    assert _feed(dem, fr.FskDemod(cfg, rows), x, [4096, n], batch=True) >= 2 * (rows - 1)
    c, rec = dem.hits()
    assert c[rows // 2] == 0 and not rec[rows // 2].view(np.uint32).any()


def test_rows_at_odd_offsets_in_and_out(fmd):
    rng = np.random.default_rng(5)
    cfg = fr.random_cfg(rng, 3, 5, 100, hit_cap=16)
    rows, n = 5, 3 * 64 * 4 + 11
    x = fr.laid_signal(rng, cfg, rows, 3 * n)
    for off_in, off_out in ((1, 0), (0, 3), (7, 5), (2, 2)):
        dem, ref = _demod(fmd, cfg, rows), fr.FskDemod(cfg, rows)
        for lo in (0, n, 2 * n):
            want, counts, rec = ref.run(x[:, lo:lo + n])
            got = call_at(dem, x[:, lo:lo + n, None], off_in, off_out)[:, :, 0]
            assert np.array_equal(got, want) and _hits_equal(dem, counts, rec)


def test_refused_calls_leave_everything_and_are_taken_when_handed_over_again(fmd):
    import torch
    rng = np.random.default_rng(7)
    cfg = fr.random_cfg(rng, 4, 5, 155, hit_cap=8)
    rows, n = 6, 2000
    x = fr.laid_signal(rng, cfg, rows, 2 * n)
    dem, ref = _demod(fmd, cfg, rows), fr.FskDemod(cfg, rows)
    first = _call(dem, x[:, :n - 3, None])[:, :, 0]          # (1997 samples: a box stays open)
    want0, counts0, rec0 = ref.run(x[:, :n - 3])
    assert np.array_equal(first, want0) and _hits_equal(dem, counts0, rec0)
    rest = np.ascontiguousarray(x[:, n - 3:])
    m = rest.shape[1]
    outs = (3 + m) // 4                                      # the call's outputs
    d_in = torch.from_numpy(rest).cuda()
    d_out = torch.full((rows, outs + 5), SENT, dtype=torch.int16, device="cuda")
    before = dem.counts()
    for n_in, in_cap, out_cap in ((m, m - 1, outs + 5), (m, m, outs - 1), (m, m, 0)):
        with pytest.raises(fmd.FmdError) as e:
            dem.run_device(d_in.data_ptr(), n_in, in_cap, d_out.data_ptr(), out_cap)
        assert e.value.status == CAPACITY and dem.counts() == before
    dem.check()
    assert (d_out.cpu().numpy() == SENT).all() and np.array_equal(d_in.cpu().numpy(), rest) and _hits_equal(dem, counts0, rec0)
    d_tight = torch.full((rows * outs + 8,), SENT, dtype=torch.int16, device="cuda")      # exactly enough room, sentinels behind it
    assert dem.run_device(d_in.data_ptr(), m, m, d_tight.data_ptr(), outs) == outs
    dem.check()
    want, counts, rec = ref.run(rest)
    got = d_tight.cpu().numpy()
    assert np.array_equal(got[:rows * outs].reshape(rows, outs), want) and (got[rows * outs:] == SENT).all() and _hits_equal(dem, counts, rec)
    # a call that completes no box is taken; a call of no samples changes nothing
    assert dem.run_batch(x[:, :2]).shape == (rows, 0) and dem.counts() == (2 * n + 2, (2 * n + 2) // 4)
    assert dem.hit_counts().tolist() == [0] * rows
    assert dem.run_batch(x[:, :0]).shape == (rows, 0) and dem.counts() == (2 * n + 2, (2 * n + 2) // 4)


def test_full_scale_rows_at_the_largest_box_and_filter(fmd):
    tap = np.minimum(8 * np.arange(32), 255).astype(np.uint32)
    cfg = fr.Cfg(64, 16, 10, tap, 0xFFFF0000, 15, 0, 64)
    n = 64 * 300
    x = np.full((2, n), -32768, np.int16)
    x[1, ::2] = 32767
    x[1, 64 * 150:] = -32768
    dem, ref = _demod(fmd, cfg, 2), fr.FskDemod(cfg, 2)
    _feed(dem, ref, x, [64 * 20 + 5, 64 * 200, n])
    assert ref.soft.min() == -32768


@pytest.mark.parametrize("hit_cap", [1, 64])
def test_hit_cap_1_and_64(fmd, hit_cap):
    rng = np.random.default_rng(11)
    cfg = fr.random_cfg(rng, 2, 4, 60, tol=15, min_corr=0, hit_cap=hit_cap)     # (tol 15: most k hit)
    x = rng.integers(-20000, 20000, (3, 2 * 700)).astype(np.int16)
    dem, ref = _demod(fmd, cfg, 3), fr.FskDemod(cfg, 3)
    want, counts, rec = ref.run(x)
    got = _call(dem, x[:, :, None])[:, :, 0]
    assert np.array_equal(got, want) and _hits_equal(dem, counts, rec) and counts.min() > 64
    assert (np.diff(rec["k_rel"].astype(np.int64), axis=1) > 0).all() if hit_cap > 1 else rec.shape == (3, 1)


def test_reset_inside_a_word_a_callers_stream_and_two_handles(fmd):
    import torch
    rng = np.random.default_rng(13)
    ca, cb = fr.random_cfg(rng, 3, 5, 155, hit_cap=16), fr.random_cfg(rng, 1, 1, 31, hit_cap=4)
    xa, xb = fr.laid_signal(rng, ca, 7, 6000), fr.laid_signal(rng, cb, 2, 6000)
    a, b = _demod(fmd, ca, 7), _demod(fmd, cb, 2)
    ra, rb = fr.FskDemod(ca, 7), fr.FskDemod(cb, 2)
    stream = torch.cuda.Stream()
    first = None
    for lo, hi in ((0, 1700), (1700, 1701), (1701, 6000)):  # the two handles interleaved, a on the caller's stream, b on the default one
        ya = _call(a, xa[:, lo:hi, None], stream=stream.cuda_stream)[:, :, 0]
        wa, cnta, reca = ra.run(xa[:, lo:hi])
        assert np.array_equal(ya, wa) and _hits_equal(a, cnta, reca)
        yb = _call(b, xb[:, lo:hi, None])[:, :, 0]
        wb, cntb, recb = rb.run(xb[:, lo:hi])
        assert np.array_equal(yb, wb) and _hits_equal(b, cntb, recb)
        first = (ya, cnta, reca) if first is None else first
    _call(a, xa[:, :100, None])                              # inside a word and inside a box, everything carried
    a.reset()
    assert a.counts() == (0, 0) and a.hit_counts().tolist() == [0] * 7
    assert np.array_equal(_call(a, xa[:, :1700, None])[:, :, 0], first[0]) and _hits_equal(a, first[1], first[2])
    assert b.counts() == (6000, 6000)


@pytest.mark.parametrize("side", ["in", "out"])
def test_rows_beyond_the_2_gib_and_4_gib_lines(fmd, side):
    """Five rows 2^31 - 6 bytes apart in the input or in the output (rows 1, 2 and 4 start just below byte 2^31, 2^32 and 2^33; the
    pitch is no multiple of 16 bytes), two calls: the wide buffer is allocated and never filled, only the rows' samples are put
    there, and behind every output row the sentinel stays."""
    import torch
    rng = np.random.default_rng(17)
    cfg = fr.random_cfg(rng, 3, 5, 100, hit_cap=16)
    rows, n, pitch = 5, 2405, (1 << 30) - 3
    x = fr.laid_signal(rng, cfg, rows, 2 * n)
    dem, ref = _demod(fmd, cfg, rows), fr.FskDemod(cfg, rows)
    big = torch.empty((rows, pitch), dtype=torch.int16, device="cuda")
    try:
        for lo in (0, n):
            part = np.ascontiguousarray(x[:, lo:lo + n])
            want, counts, rec = ref.run(part)
            k = want.shape[1]
            if side == "in":
                big[:, :n] = torch.from_numpy(part).cuda()
                d_out = torch.full((rows, k + 5), SENT, dtype=torch.int16, device="cuda")
                torch.cuda.synchronize()
                assert dem.run_device(big.data_ptr(), n, pitch, d_out.data_ptr(), k + 5) == k
                dem.check()
                got = d_out.cpu().numpy()
                assert np.array_equal(big[:, :n].cpu().numpy(), part)
            else:
                big[:, :k + 8] = SENT
                d_in = torch.from_numpy(part).cuda()
                torch.cuda.synchronize()
                assert dem.run_device(d_in.data_ptr(), n, n, big.data_ptr(), pitch) == k
                dem.check()
                got = big[:, :k + 8].cpu().numpy()
            assert np.array_equal(got[:, :k], want), [r for r in range(rows) if not np.array_equal(got[r, :k], want[r])]
            assert (got[:, k:] == SENT).all() and _hits_equal(dem, counts, rec) and counts.sum() > 0
    finally:
        del big
        torch.cuda.empty_cache()


def _fm(n, fs, off, amp, msg_hz):
    """A carrier at `off` whose frequency moves by msg_hz[i] Hz"""
    ph = 2 * np.pi * np.cumsum(msg_hz) / fs
    return amp * np.exp(1j * (2 * np.pi * off * np.arange(n) / fs + ph))


def test_narrow_bank_nfm_into_the_pager_decoder_and_the_tool(fmd, tmp_path):
    """The narrow-band bank in NFM mode on a synthetic 240 kHz capture whose first station sends two pages (1200 baud, 3 kHz
    deviation): its d_out at 12 kHz, as it stands and with its out_cap as in_cap, through pages(bank) equals narrow_ref -> fsk_ref
    call by call, the decoder behind it delivers both messages, and decode_pages and pocsag_gpu find them in the same audio."""
    import torch
    import pocsag_ref as pr
    fs, D, T, R, Ta, S, K = 240000, 4, 64, 5, 127, 1, 3
    rate, baud = fs // D // R, 1200
    h = st.lowpass(T, 20000 / fs)
    offs = np.array([[-70000, 20000, 85000]])
    incs = np.array([[fmd.phase_inc(int(o), fs) for o in offs[s]] for s in range(S)], np.uint32)
    g = fmd.narrow_taps(fs // D, Ta, -6000, 6000)
    nb = fmd.NarrowBank(h, D, incs, g, R, mode=nr.FM, n_streams=S, block=64, squelch=0, gain=256, device_id=0)
    refs = [nr.NarrowRef(nb.taps, nb.decim, incs[s], nb.shift, nb.gr, nb.gi, nb.mode, nb.chan_decim, nb.chan_shift, nb.block, nb.squelch,
                         nb.gain) for s in range(S)]
    dem = fmd.pages(nb, rate, baud, device_id=0)
    d = fmd.fsk_design(rate, baud)
    assert (dem.n_rows, dem.width, dem.D, dem.W) == (S * K, 1, d.D, d.W)
    fref = fr.FskDemod(fr.Cfg(d.D, d.W, d.shift, d.tap, d.sync, d.tol, d.min_corr, d.hit_cap), S * K)
    sent = [(1234567, 3, "first page", "alpha"), (7654, 0, "0123-456", "numeric")]
    bits = fmd.pocsag_encode(sent, preamble=96)
    lens = (8 * 24003, 8 * 10001, 8 * 60000)
    total = sum(lens) // 2
    t = np.arange(total)
    idx = np.floor(t * baud / fs).astype(np.int64) - 40
    on = (idx >= 0) & (idx < len(bits))
    msg = np.where(on, 3000.0 * (2.0 * bits[np.clip(idx, 0, len(bits) - 1)] - 1.0), 0.0)
    assert idx.max() > len(bits) + 40                        # the carrier outlasts the transmission
    z = np.zeros((S, total), np.complex128)
    z[0] = _fm(total, fs, float(offs[0, 0]), 40.0, msg) + nr.carrier(total, fs, float(offs[0, 1]), 40.0)
    data_all = np.stack([nr.to_u8(z[s], noise=1.0, seed=s) for s in range(S)])
    decs = [fmd.PocsagDecoder(rate, d.D, baud) for _ in range(S * K)]
    rdecs = [pr.Decoder(rate, d.D, baud) for _ in range(S * K)]
    lo, got, audio_all = 0, [[] for _ in range(S * K)], []
    for n in lens:
        data = np.ascontiguousarray(data_all[:, lo:lo + n])
        lo += n
        cap = nb.out_cap(n) + 3
        d_audio = torch.full((S, K, cap), SENT, dtype=torch.int16, device="cuda")
        s_cap = (dem.out_cap(cap) + 2) | 1
        d_soft = torch.full((S * K, s_cap), SENT, dtype=torch.int16, device="cuda")
        d_iq = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        m = nb.run_device(d_iq.data_ptr(), n, d_audio.data_ptr(), cap)
        k = dem.run_device(d_audio.data_ptr(), m, cap, d_soft.data_ptr(), s_cap)           # the bank's out_cap is the in_cap
        dem.check()
        audio = np.stack([refs[s].feed(data[s]) for s in range(S)]).reshape(S * K, m).astype(np.int16)
        audio_all.append(audio)
        want, counts, rec = fref.run(audio)
        soft = d_soft.cpu().numpy()
        assert k == want.shape[1] and np.array_equal(soft[:, :k], want) and (soft[:, k:] == SENT).all()
        assert _hits_equal(dem, counts, rec)
        c, r = dem.hits()
        for row in range(S * K):
            msgs = decs[row].push(soft[row, :k], r[row, :min(int(c[row]), d.hit_cap)])
            assert msgs == rdecs[row].push(want[row], rec[row, :min(int(counts[row]), d.hit_cap)].tolist())
            got[row] += msgs
    texts = [(m["address"], m["function"], fmd.pocsag_text(m, baud)) for m in got[0]]
    assert texts == [(1234567, 3, "POCSAG1200: Address: 1234567  Function: 3  Alpha: first page"),
                     (7654, 0, "POCSAG1200: Address: 0007654  Function: 0  Numeric: 0123-456  ")]
    assert got[1] == [] and got[2] == [] and [dc.info() for dc in decs] == [rd.info() for rd in rdecs]
    # the same audio through decode_pages: the rows without a sync word never reach their decoders
    dem.reset()
    res = fmd.decode_pages(dem, audio_all)
    assert [m["bits"] for m in res[0]["messages_list"]] == [m["bits"] for m in got[0]]
    assert [m["end_sample"] for m in res[0]["messages_list"]] == [m["end_sample"] for m in got[0]]
    assert res[0]["messages"] == 2 and res[0]["pushes"] >= 1 and res[1]["pushes"] == 0 and res[2]["pushes"] == 0
    # and through the tool
    (tmp_path / "in.s16").write_bytes(np.concatenate(audio_all, axis=1)[0].tobytes())
    exe = os.path.join(ROOT, "rtl-sdr-rs_amd", "pocsag_gpu")
    p = subprocess.run([exe, "-r", str(rate), str(tmp_path / "in.s16")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode().splitlines() == [t[2] for t in texts]
    assert p.stderr.decode() == "messages 2 batches %d bad_codewords 0 orphans 0\n" % decs[0].info()["batches"]
