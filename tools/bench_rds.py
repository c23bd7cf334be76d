#!/usr/bin/env python3
"""RDS bank (fmd_rds_*): S streams x 262144 B per call at 2.4 Msps, decimate 10 (f_m = 240 kHz), 64 front-end taps, output
decimation 32 (7.5 kHz) with 255 RDS taps, pilot blocks of 4096, K stations.  Per K (--k 1,4,8,16): ms per call (HIP events, both
passes and the block-sum reset), a parity bit against the test-side definition (tests/rds_ref.py) on a seeded sample of streams, and
two baselines timed in the same process at the same K and front-end shift: the stereo station bank (R = 5, 127 audio taps) and the
channelizer.  Then the host decoder: fmd_rds_decoder_push in samples per second on one thread, on the definition's baseband of a
synthesized station.  Writes every line to --out (profiles/rds_bench.json)."""
import time

import numpy as np
import torch

import bench_common as bc
from bench_common import fmd, time_calls

FS, D, T, R, TA, P = 2400000, 10, 64, 32, 255, 4096


def run(K, S, n, iters, parity_streams):
    import rds_ref as rr
    import stations_ref as sr
    h = bc.lowpass(T, 130000 / FS)
    g, rs = fmd.rds_taps(FS // D, R, TA)
    incs = bc.station_incs(K, S, FS)
    rb = fmd.RdsBank(h, D, incs, FS, g, R, n_streams=S, block=P, rds_shift=rs, device_id=0)
    bufs, stream = bc.device_buffers(S, n)
    cap = rb.out_cap(n)
    out = torch.empty((S, K, cap, 2), dtype=torch.int16, device="cuda")
    got = {}

    def launch(i):
        got["n"] = rb.run_device(bufs[i % 2].data_ptr(), n, out.data_ptr(), cap, stream)

    ms, ts = time_calls(launch, iters)
    rb.check()
    # baseline 1: the stereo station bank at the same K and shift (the same pass 0; its pass 1 at R = 5 with 127 taps)
    sb = fmd.StereoBank(h, D, incs, FS, fmd.stereo_taps(FS // D, 5, 127), 5, n_streams=S, block=P, shift=rb.shift, device_id=0)
    scap = sb.out_cap(n)
    sout = torch.empty((S, K, scap, 2), dtype=torch.int16, device="cuda")
    ms_st, ts_st = time_calls(lambda i: sb.run_device(bufs[i % 2].data_ptr(), n, sout.data_ptr(), scap, stream), iters)
    sb.check()
    del sb, sout
    # baseline 2: the channelizer at the same K and shift
    ch = fmd.Channelizer(h, D, incs, n_streams=S, shift=rb.shift, device_id=0)
    ccap = ch.out_cap(n)
    cout = torch.empty((S, K, ccap, 2), dtype=torch.int16, device="cuda")
    ms_ch, ts_ch = time_calls(lambda i: ch.run_device(bufs[i % 2].data_ptr(), n, cout.data_ptr(), ccap, stream), iters)
    ch.check()
    del ch, cout
    torch.cuda.empty_cache()
    # parity: a fresh bank, two calls, sampled streams against the definition
    pb = fmd.RdsBank(h, D, incs, FS, g, R, n_streams=S, block=P, rds_shift=rs, device_id=0)
    sample = bc.parity_sample(S, parity_streams)
    refs = {s: rr.RdsRef(h, D, incs[s], pb.shift, FS, g, R, rs, P, pb.pilot_min, z=sr.z_corr) for s in sample}
    ok = True
    for b in range(2):
        host = bufs[b].cpu().numpy()
        pout = torch.empty((S, K, cap, 2), dtype=torch.int16, device="cuda")
        m = pb.run_device(bufs[b].data_ptr(), n, pout.data_ptr(), cap, stream)
        pb.check()
        a = pout[sample, :, :m].cpu().numpy()
        for i, s in enumerate(sample):
            ok &= bool(np.array_equal(a[i], refs[s].feed(host[s])))
    return {"tool": "bench_rds", "K": K, "streams": S, "nbytes": n, "decim": D, "taps": T, "out_decim": R, "rds_taps": TA,
            "block": P, "shift": rb.shift, "rds_shift": rb.rds_shift, "kernels": [rb.kernel_name(0), rb.kernel_name(1)],
            "out_per_station": got["n"], "ms": round(ms, 4), "ms_all": [round(t, 4) for t in ts], "in_bytes": S * n,
            "out_bytes": S * K * got["n"] * 4,
            "stereo_ms": round(ms_st, 4), "stereo_ms_all": [round(t, 4) for t in ts_st], "ratio_vs_stereo": round(ms / ms_st, 3),
            "channelizer_ms": round(ms_ch, 4), "channelizer_ms_all": [round(t, 4) for t in ts_ch],
            "ratio_vs_channelizer": round(ms / ms_ch, 3), "parity": bool(ok), "parity_streams": sample}


def decoder_rate(seconds=2.0, reps=5):
    """fmd_rds_decoder_push on one thread: samples per second over `seconds` of the test station's baseband (the definition's)."""
    import rds_ref as rr
    import stations_ref as sr
    iq, _ = rr.station_capture(seconds)
    h = rr.front_taps()
    incs = [sr.phase_inc(40000, rr.FS)]
    g, rs = fmd.rds_taps(rr.FS // rr.D, rr.R, rr.T_RDS)
    ref = rr.RdsRef(h, rr.D, incs, fmd.stations_auto_shift(h, incs, limit=256), rr.FS, g, rr.R, rs, z=sr.z_corr)
    u = np.ascontiguousarray(ref.feed(iq)[0].astype(np.int16))
    ts, info = [], None
    for _ in range(reps):
        dec = fmd.RdsDecoder(rr.FS, rr.D * rr.R)
        t0 = time.perf_counter()
        dec.push(u)
        ts.append(time.perf_counter() - t0)
        info = dec.info()
    t = sorted(ts)[len(ts) // 2]
    return {"tool": "bench_rds", "decoder": True, "samples": int(u.shape[0]), "sample_rate": rr.FS / (rr.D * rr.R),
            "push_seconds": round(t, 6), "samples_per_second": round(u.shape[0] / t), "realtime_stations_per_thread": round(u.shape[0] / t / (rr.FS / (rr.D * rr.R))),
            "groups_ok": info["groups_ok"], "blocks_bad": info["blocks_bad"], "ps": info["ps"], "rt": info["rt"]}


def main():
    ap = bc.parser()
    ap.add_argument("--k", default="1,4,8,16")
    ap.add_argument("--parity-streams", type=int, default=2)
    bc.add_out(ap, "rds_bench.json")
    a = ap.parse_args()
    rows = []
    for K in [int(x) for x in a.k.split(",")]:
        rows.append(run(K, a.streams, a.nbytes, a.iters, a.parity_streams))
        bc.emit(rows[-1])
    dec = decoder_rate()
    bc.emit(dec)
    bc.write_rows(a.out, rows=rows, decoder=dec)


if __name__ == "__main__":
    main()
