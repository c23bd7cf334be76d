#!/usr/bin/env python3
"""Time the page bank (fmd_pager_*) on one MI355X over the soft decisions and records the FSK front end leaves at two banks' shapes,
both at 1200 baud:

    narrow:    4096 rows x 327/328 soft decisions, from  4096 x  655 samples at 12 kHz (D 2)
    bandplan: 65536 rows x 256     soft decisions, from 65536 x 1024 samples at 24 kHz (D 4)

Every 64th row carries continuous POCSAG 1200 traffic from pocsag_encode, the others audio-level noise (a level per row); the records
are the FskDemod's own of the same calls.  Eight consecutive calls of soft decisions, counts and records are kept on the device and
handed to the page bank in turn (the traffic repeats with them, so a traffic row loses and regains its lock where the eighth call
meets the first).  HIP events, the median of 3 x 200 consecutive calls after a warm-up.  Beside it, in the same process and on the same
rows: a plain device-to-device copy of one call's soft rows, and the path the page bank replaces -- the copy of the busy rows (a
record, or a decoder locked or searching) to pinned host memory, fmd_pocsag_decoder_push over the busy rows on one thread and on 16
(tools/pager_hostbench.cpp, timed without the interpreter), and one call of Python's decode_pages end to end (the fourth of four
calls, timed between two requests for input).  Four sampled rows, two of them traffic rows, are compared with tests/pager_ref.py over twelve calls: counts,
records and counters.  Writes profiles/pager_bench.json."""
import ctypes as C
import time

import bench_common as bc
from bench_common import fmd, np, torch

import pager_ref as gr

SHAPES = [("narrow", 4096, 655, 12000), ("bandplan", 65536, 1024, 24000)]
BAUD, PERIOD, MSG_CAP = 1200, 8, 4
FSK_MS_COMMITTED = {"narrow": 0.0278, "bandplan": 0.1953}    # profiles/pocsag_bench.json
PUSH_ARGS = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint,
             C.POINTER(C.c_uint64)]


def bench(name, rows, n, rate, iters, host):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    d = fmd.fsk_design(rate, BAUD)
    dem = fmd.FskDemod(d.D, d.W, d.shift, d.tap, d.sync, d.tol, d.min_corr, d.hit_cap, n_rows=rows, device_id=0, rate=rate, baud=BAUD)
    cap = dem.out_cap(n)
    # the traffic rows' audio: 2 PERIOD calls of one transmission, pages on end
    text = "the quick brown fox jumps over the lazy dog"
    bits = fmd.pocsag_encode([(8 * k + k % 8, k % 4, text[:10 + 3 * k], "alpha") for k in range(12)], preamble=64)
    total = 2 * PERIOD * n
    idx = np.floor(np.arange(total) * BAUD / rate).astype(np.int64)
    if idx[-1] >= len(bits):
        raise SystemExit("%s: the transmission is too short" % name)
    tone = torch.from_numpy((4000 * (2 * bits[idx].astype(np.int32) - 1)).reshape(2 * PERIOD, n)).cuda().to(torch.int32)
    level = torch.randint(50, 3000, (rows, 1), generator=gen, device="cuda", dtype=torch.int32)
    traffic = (torch.arange(rows, device="cuda") % 64 == 0).to(torch.int32)[:, None]
    soft = torch.zeros((PERIOD, rows, cap), dtype=torch.int16, device="cuda")
    d_cnt = torch.zeros((PERIOD, rows), dtype=torch.int32, device="cuda")
    d_hit = torch.zeros((PERIOD, rows, d.hit_cap * 4), dtype=torch.int32, device="cuda")
    ks, h_cnt, h_hit, audio_host = [0] * PERIOD, [None] * PERIOD, [None] * PERIOD, []
    for call in range(2 * PERIOD):                           # (the second lap is kept: the front end's taps are full from the first sample on)
        p = call % PERIOD
        noise = torch.randint(-1024, 1025, (rows, n), generator=torch.Generator(device="cuda").manual_seed(p), device="cuda", dtype=torch.int32)
        audio = (((level * noise) >> 10) + traffic * tone[call][None, :]).clamp(-32768, 32767).to(torch.int16).contiguous()
        torch.cuda.synchronize()
        ks[p] = dem.run_device(audio.data_ptr(), n, n, soft[p].data_ptr(), cap, stream)
        dem.check()
        c, r = dem.hits()
        h_cnt[p], h_hit[p] = c, r
        d_cnt[p].copy_(torch.from_numpy(c.view(np.int32)))
        d_hit[p].copy_(torch.from_numpy(r.view(np.int32).reshape(rows, -1)))
        if call >= 2 * PERIOD - 4:
            audio_host.append(audio.cpu().numpy())
    del noise, audio
    torch.cuda.synchronize()

    def handle():
        return fmd.Pager(rate, d.D, BAUD, 1, MSG_CAP, n_rows=rows, device_id=0)

    def run(pg, i):
        p = i % PERIOD
        pg.run_device(soft[p].data_ptr(), ks[p], cap, d_cnt[p].data_ptr(), d_hit[p].data_ptr(), d.hit_cap, stream)

    # parity of four sampled rows over twelve calls, two of them traffic rows
    sample = sorted([0, 64 * (rows // 128)] + [r | 1 for r in bc.parity_sample(rows, 2)])
    ref = gr.Pager(rate, d.D, BAUD, 1, MSG_CAP, rows=len(sample))
    pg = handle()
    found = 0
    for i in range(12):
        p = i % PERIOD
        run(pg, i)
        pg.check()
        counts, rec, every = ref.run(soft[p][sample][:, :ks[p]].cpu().numpy(), h_cnt[p][sample], h_hit[p][sample])
        got = np.zeros((len(sample), MSG_CAP), gr.MSG_DTYPE)
        fmd.check(fmd.lib().fmd_pager_msgs(pg._h, np.array(sample, np.uint32).ctypes.data, len(sample), got.ctypes.data))
        info = pg.info()
        if not np.array_equal(pg.counts()[sample], counts) or got.tobytes() != rec.tobytes() or [info[r] for r in sample] != ref.info():
            raise SystemExit("%s: rows %s differ from tests/pager_ref.py in call %d" % (name, sample, i))
        found += int(counts.sum())
    if found < 2:
        raise SystemExit("%s: the sampled rows delivered no message" % name)
    del pg

    pg = handle()
    ms, all_ms = bc.time_calls(lambda i: run(pg, i), iters)
    pg.check()
    info = pg.info()
    calls = 3 + 3 * iters
    last = (iters - 1) % PERIOD
    busy = np.nonzero((h_cnt[last] > 0) | np.array([i["locked"] or i["searching"] for i in info]))[0].astype(np.uint32)
    # the path this replaces: the busy rows to the host, and a host decoder for each of them
    d_busy = torch.from_numpy(busy.astype(np.int64)).cuda()
    (copy_ms, copy_all), (d2h_ms, d2h_all) = bc.copy_baselines(name, soft, iters, lambda s: s.index_select(0, d_busy))
    t0 = time.perf_counter()
    for r in busy.tolist():                                  # as decode_pages copies them: a copy per row
        soft[last][r, :ks[last]].cpu()
    d2h_rows_ms = 1e3 * (time.perf_counter() - t0)
    decs = (C.c_void_p * rows)()
    for r in busy.tolist():
        dd = C.c_void_p()
        fmd.check(fmd.lib().fmd_pocsag_decoder_new(rate, d.D, BAUD, 1, C.byref(dd)))
        decs[r] = dd
    got = C.c_uint64(0)
    push = bc.host_push(soft, lambda p, h_rows, threads: host.hostbench_push(
        decs, h_rows, ks[p], cap, h_cnt[p].ctypes.data, h_hit[p].ctypes.data, d.hit_cap, busy.ctypes.data, len(busy), threads, C.byref(got)))
    for r in busy.tolist():
        fmd.lib().fmd_pocsag_decoder_free(C.c_void_p(decs[r]))
    # decode_pages end to end: the calls come from a generator that notes when each is asked for, so the time between two requests is
    # one call of decode_pages, the upload of its input included; the last call's, whose rows are busy from the calls before, is taken
    asked = []

    def feed():
        for x in audio_host:
            asked.append(time.perf_counter())
            yield x
        asked.append(time.perf_counter())
    dm = fmd.FskDemod(d.D, d.W, d.shift, d.tap, d.sync, d.tol, d.min_corr, d.hit_cap, n_rows=rows, device_id=0, rate=rate, baud=BAUD)
    res = fmd.decode_pages(dm, feed())
    pages_ms = [1e3 * (b - a) for a, b in zip(asked, asked[1:])]
    pushed = sum(1 for r_ in res if r_["pushes"])
    del res, dm
    n_soft = rows * ks[0]
    return bc.emit({"shape": name, "rows": rows, "samples": n, "rate": rate, "baud": BAUD, "D": d.D, "soft_per_call": ks, "msg_cap": MSG_CAP,
                    "hit_cap": d.hit_cap, "kernel": pg.kernel_name(), "ms_per_call": round(ms, 5), "ms_runs": [round(t_, 5) for t_ in all_ms],
                    "gsoft_per_s": round(n_soft / ms / 1e6, 2), "copy_ms": round(copy_ms, 5), "copy_runs": [round(t_, 5) for t_ in copy_all],
                    "copy_bytes": 4 * rows * cap, "ratio_to_copy": round(ms / copy_ms, 3),
                    "fsk_ms_committed": FSK_MS_COMMITTED[name], "ratio_to_fsk_committed": round(ms / FSK_MS_COMMITTED[name], 3),
                    "busy_rows_last_call": int(len(busy)), "rows_with_a_record_last_call": int((h_cnt[last] > 0).sum()),
                    "d2h_busy_rows_ms": round(d2h_ms, 5), "d2h_busy_rows_runs": [round(t_, 5) for t_ in d2h_all],
                    "d2h_busy_rows_one_copy_each_ms": round(d2h_rows_ms, 3),
                    "host_push_busy_ms_1_thread": round(push[1], 4), "host_push_busy_ms_16_threads": round(push[16], 4),
                    "replaced_path_ms_16_threads": round(d2h_ms + push[16], 4), "ratio_replaced_to_kernel": round((d2h_ms + push[16]) / ms, 2),
                    "decode_pages_one_call_ms": round(pages_ms[-1], 2), "decode_pages_calls_ms": [round(t_, 2) for t_ in pages_ms],
                    "decode_pages_rows_pushed": pushed,
                    "timed_calls": calls, "messages_all_rows": int(sum(i["messages"] for i in info)),
                    "batches_all_rows": int(sum(i["batches"] for i in info)), "bad_codewords_all_rows": int(sum(i["bad_codewords"] for i in info)),
                    "locked_rows_after": int(sum(i["locked"] for i in info)),
                    "parity_rows": sample, "parity_messages": found, "parity": "exact"})


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    bc.add_out(ap, "pager_bench.json")
    a = ap.parse_args()
    host = bc.hostbench("pager", PUSH_ARGS)
    rows = [bench(*s, a.iters, host) for s in SHAPES]
    bc.write_rows(a.out, baud=BAUD, iters=a.iters, period=PERIOD, rows=rows)


if __name__ == "__main__":
    main()
