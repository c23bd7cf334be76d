#!/usr/bin/env python3
"""Time the frame bank (fmd_hdlc_*) on one MI355X over the soft decisions the packet demodulator leaves at two banks' shapes, both at
1200 baud:

    narrow:    4096 rows x 328 soft decisions, from  4096 x  655 samples at 12 kHz (stride 2)
    bandplan: 65536 rows x 256 soft decisions, from 65536 x 1024 samples at 24 kHz (stride 4)

The input is what AfskDemod writes for audio-level noise rows (a level per row), every 64th row carrying continuous-phase AFSK: flags,
and one 25-byte frame every eight calls.  Eight consecutive calls of soft decisions are kept on the device and handed to the framer
in turn.  HIP events, the median of 3 x 200 consecutive calls after a warm-up.  Beside it, in the same process and on the same rows:
a plain device-to-device copy of one call's soft rows, and the path the frame bank replaces -- the copy of the soft rows to pinned
host memory, and fmd_ax25_decoder_push over all rows on one thread and on 16 (tools/hdlc_hostbench.cpp, timed without the
interpreter).  Four sampled rows, two of them frame rows, are compared with tests/hdlc_ref.py over twelve calls: counts, records and
counters.  Writes profiles/hdlc_bench.json."""
import ctypes as C

import bench_common as bc
from bench_common import fmd, np, torch

import ax25_ref as xr
import hdlc_ref as hr

SHAPES = [("narrow", 4096, 655, 12000), ("bandplan", 65536, 1024, 24000)]
BAUD, PERIOD = 1200, 8
PUSH_ARGS = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.POINTER(C.c_uint64)]


def bench(name, rows, n, rate, iters, host):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    pk = fmd.AfskDemod(*_design(rate), n_rows=rows, device_id=0, rate=rate, baud=BAUD)
    cap = pk.out_cap(n)
    # the frame rows' audio: PERIOD calls of flags with one frame in them, the same in every period
    total_bits = PERIOD * n * BAUD // rate
    frame = xr.frame_bits(xr.ui_frame(("APRS", 0), ("N0CALL", 7), b"bench"), flags=4, closing=1)
    bits = (frame + xr.FLAG * (total_bits // 8 + 1))[:total_bits + 1]
    tone = xr.to_s16(xr.afsk_audio(xr.nrzi(bits), rate, BAUD, amp=6000.0)[0])[:PERIOD * n]
    tone = torch.from_numpy(np.ascontiguousarray(tone.reshape(PERIOD, n))).cuda().to(torch.int32)
    level = torch.randint(50, 3000, (rows, 1), generator=gen, device="cuda", dtype=torch.int32)
    framed = (torch.arange(rows, device="cuda") % 64 == 0).to(torch.int32)[:, None]
    soft = torch.zeros((PERIOD, rows, cap), dtype=torch.int16, device="cuda")
    ks = [0] * PERIOD
    for lap in range(2):                                     # (the second lap: the demodulator's window is full from the first sample on)
        for p in range(PERIOD):
            noise = torch.randint(-1024, 1025, (rows, n), generator=torch.Generator(device="cuda").manual_seed(p), device="cuda", dtype=torch.int32)
            audio = (((level * noise) >> 10) + framed * tone[p][None, :]).clamp(-32768, 32767).to(torch.int16).contiguous()
            torch.cuda.synchronize()
            ks[p] = pk.run_device(audio.data_ptr(), n, n, soft[p].data_ptr(), cap, stream)
            pk.check()
    del noise, audio

    def handle():
        return fmd.Ax25Framer(rate, pk.stride, BAUD, 4, n_rows=rows, device_id=0)

    def run(fb, i):
        fb.run_device(soft[i % PERIOD].data_ptr(), ks[i % PERIOD], cap, stream)

    # parity of four sampled rows over twelve calls, two of them frame rows
    sample = sorted([0, 64 * (rows // 128)] + [r | 1 for r in bc.parity_sample(rows, 2)])
    ref = hr.Framer(rate, pk.stride, BAUD, 4, rows=len(sample))
    fb = handle()
    found = 0
    for i in range(12):
        run(fb, i)
        fb.check()
        counts, rec, every = ref.run(soft[i % PERIOD][sample][:, :ks[i % PERIOD]].cpu().numpy())
        got = np.zeros((len(sample), 4), hr.FRAME_DTYPE)
        fmd.check(fmd.lib().fmd_hdlc_frames(fb._h, np.array(sample, np.uint32).ctypes.data, len(sample), got.ctypes.data))
        info = fb.info()
        if not np.array_equal(fb.counts()[sample], counts) or got.tobytes() != rec.tobytes() or [info[r] for r in sample] != ref.info():
            raise SystemExit("%s: rows %s differ from tests/hdlc_ref.py in call %d" % (name, sample, i))
        found += int(counts.sum())
    if found < 2:
        raise SystemExit("%s: the sampled rows delivered no frame" % name)
    del fb

    fb = handle()
    ms, all_ms = bc.time_calls(lambda i: run(fb, i), iters)
    fb.check()
    info = fb.info()
    calls = 3 + 3 * iters
    # the path this replaces: the soft rows to the host, and a host decoder per row
    (copy_ms, copy_all), (d2h_ms, d2h_all) = bc.copy_baselines(name, soft, iters)
    decs = (C.c_void_p * rows)()
    for r in range(rows):
        d = C.c_void_p()
        fmd.check(fmd.lib().fmd_ax25_decoder_new(rate, pk.stride, BAUD, C.byref(d)))
        decs[r] = d
    got = C.c_uint64(0)
    push = bc.host_push(soft, lambda p, h_rows, threads: host.hostbench_push(decs, h_rows, rows, ks[p], cap, threads, C.byref(got)))
    for r in range(rows):
        fmd.lib().fmd_ax25_decoder_free(C.c_void_p(decs[r]))
    n_soft = rows * ks[0]
    return bc.emit({"shape": name, "rows": rows, "samples": n, "rate": rate, "baud": BAUD, "stride": pk.stride, "soft_per_call": ks,
                    "frame_cap": 4, "kernel": fb.kernel_name(), "ms_per_call": round(ms, 5), "ms_runs": [round(t_, 5) for t_ in all_ms],
                    "gsoft_per_s": round(n_soft / ms / 1e6, 2), "copy_ms": round(copy_ms, 5), "copy_runs": [round(t_, 5) for t_ in copy_all],
                    "copy_bytes": 4 * rows * cap, "ratio_to_copy": round(ms / copy_ms, 3),
                    "d2h_ms": round(d2h_ms, 5), "d2h_runs": [round(t_, 5) for t_ in d2h_all], "d2h_bytes": 2 * rows * cap,
                    "host_push_ms_1_thread": round(push[1], 3), "host_push_ms_16_threads": round(push[16], 3),
                    "host_msoft_per_s_1_thread": round(n_soft / push[1] / 1e3, 1),
                    "replaced_path_ms_16_threads": round(d2h_ms + push[16], 3), "ratio_replaced_to_kernel": round((d2h_ms + push[16]) / ms, 1),
                    "timed_calls": calls, "frames_ok_all_rows": int(sum(i["frames_ok"] for i in info)),
                    "bad_fcs_all_rows": int(sum(i["bad_fcs"] for i in info)), "aborts_all_rows": int(sum(i["aborts"] for i in info)),
                    "parity_rows": sample, "parity_frames": found, "parity": "exact"})


def _design(rate):
    tab, pre, out = fmd.afsk_table(rate, BAUD)
    return tab, fmd.afsk_stride(tab.shape[1]), pre, out


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    bc.add_out(ap, "hdlc_bench.json")
    a = ap.parse_args()
    host = bc.hostbench("hdlc", PUSH_ARGS)
    rows = [bench(*s, a.iters, host) for s in SHAPES]
    bc.write_rows(a.out, baud=BAUD, iters=a.iters, period=PERIOD, rows=rows)


if __name__ == "__main__":
    main()
