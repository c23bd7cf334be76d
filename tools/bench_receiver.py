#!/usr/bin/env python3
"""FM receiver bank (fmd_receiver_*): S streams x 262144 B per call at 2.4 Msps, decimate 10 (f_m = 240 kHz), 64 front-end taps,
pilot blocks of 4096, audio at R = 5 with 127 taps, RDS at R = 32 with 255 taps, K stations.  Per K (--k 1,4,8,16), all in one
process: ms per call of the receiver (HIP events: the block-sum reset, the multiplex pass, the fused second pass), of a stereo bank
and of an RDS bank at the same K and shift -- what a caller who wants both runs today -- ratio = receiver / (stereo + rds), and a
parity bit against the test-side definitions (tests/stereo_ref.py, tests/rds_ref.py through tests/receiver_ref.py) on a seeded sample
of streams.  Writes every line to --out (profiles/receiver_bench.json).  For the per-kernel split run it under
`rocprofv3 --kernel-trace --stats` with --k 8 --out ''."""
import numpy as np
import torch

import bench_common as bc
from bench_common import fmd, time_calls

FS, D, T, P = 2400000, 10, 64, 4096
RA, TA, RR, TR = 5, 127, 32, 255


def banks(K, S, n):
    """(receiver, stereo bank, RDS bank, their launch closures) on the tool's two device buffers."""
    h = bc.lowpass(T, 130000 / FS)
    ga = fmd.stereo_taps(FS // D, RA, TA)
    gr, rs = fmd.rds_taps(FS // D, RR, TR)
    incs = bc.station_incs(K, S, FS)
    rx = fmd.ReceiverBank(h, D, incs, FS, ga, RA, gr, RR, n_streams=S, block=P, rds_shift=rs, device_id=0)
    sb = fmd.StereoBank(h, D, incs, FS, ga, RA, n_streams=S, block=P, shift=rx.shift, audio_shift=rx.audio_shift, device_id=0)
    rb = fmd.RdsBank(h, D, incs, FS, gr, RR, n_streams=S, block=P, rds_shift=rs, shift=rx.shift, device_id=0)
    return h, ga, gr, rs, incs, rx, sb, rb


def run(K, S, n, iters, parity_streams):
    import receiver_ref as rxr
    import stations_ref as sr
    h, ga, gr, rs, incs, rx, sb, rb = banks(K, S, n)
    bufs, stream = bc.device_buffers(S, n)
    ca, cr = rx.out_caps(n)
    audio = torch.empty((S, K, ca, 2), dtype=torch.int16, device="cuda")
    rds = torch.empty((S, K, cr, 2), dtype=torch.int16, device="cuda")
    got = {}

    def launch(i):
        got["n"] = rx.run_device(bufs[i % 2].data_ptr(), n, audio.data_ptr(), ca, rds.data_ptr(), cr, stream)

    ms, ts = time_calls(launch, iters)
    rx.check()
    ms_st, ts_st = time_calls(lambda i: sb.run_device(bufs[i % 2].data_ptr(), n, audio.data_ptr(), ca, stream), iters)
    sb.check()
    ms_rd, ts_rd = time_calls(lambda i: rb.run_device(bufs[i % 2].data_ptr(), n, rds.data_ptr(), cr, stream), iters)
    rb.check()
    # the three once more in the other order, so that a drift over the run shows as a spread and not as a ratio
    ms2, ts2 = time_calls(launch, iters)
    rx.check()
    ts, ms = ts + ts2, sorted(ts + ts2)[len(ts)]
    # parity: a fresh receiver, two calls, sampled streams against the definition
    pb = fmd.ReceiverBank(h, D, incs, FS, ga, RA, gr, RR, n_streams=S, block=P, rds_shift=rs, device_id=0)
    sample = bc.parity_sample(S, parity_streams)
    refs = {s: rxr.ReceiverRef(h, D, incs[s], pb.shift, FS, ga, RA, pb.audio_shift, gr, RR, rs, P, pb.pilot_min, z=sr.z_corr) for s in sample}
    ok = True
    for b in range(2):
        host = bufs[b].cpu().numpy()
        na, nr = pb.run_device(bufs[b].data_ptr(), n, audio.data_ptr(), ca, rds.data_ptr(), cr, stream)
        pb.check()
        a, u = audio[sample, :, :na].cpu().numpy(), rds[sample, :, :nr].cpu().numpy()
        for i, s in enumerate(sample):
            ea, eu = refs[s].feed(host[s])
            ok &= bool(np.array_equal(a[i], ea)) and bool(np.array_equal(u[i], eu))
    both = ms_st + ms_rd
    return {"tool": "bench_receiver", "K": K, "streams": S, "nbytes": n, "decim": D, "taps": T, "block": P, "audio_decim": RA,
            "audio_taps": TA, "rds_decim": RR, "rds_taps": TR, "shift": rx.shift, "audio_shift": rx.audio_shift, "rds_shift": rx.rds_shift,
            "kernels": [rx.kernel_name(0), rx.kernel_name(1)], "audio_per_station": got["n"][0], "rds_per_station": got["n"][1],
            "ms": round(ms, 4), "ms_all": [round(t, 4) for t in ts], "in_bytes": S * n,
            "stereo_ms": round(ms_st, 4), "stereo_ms_all": [round(t, 4) for t in ts_st],
            "rds_ms": round(ms_rd, 4), "rds_ms_all": [round(t, 4) for t in ts_rd],
            "stereo_plus_rds_ms": round(both, 4), "ratio": round(ms / both, 3),
            # the least favourable pairing of the repetitions: the receiver's slowest against the two banks' fastest
            "ratio_worst": round(max(ts) / (min(ts_st) + min(ts_rd)), 3),
            "parity": bool(ok), "parity_streams": sample}


def main():
    ap = bc.parser()
    ap.add_argument("--k", default="1,4,8,16")
    ap.add_argument("--parity-streams", type=int, default=2)
    bc.add_out(ap, "receiver_bench.json")
    a = ap.parse_args()
    rows = []
    for K in [int(x) for x in a.k.split(",")]:
        rows.append(run(K, a.streams, a.nbytes, a.iters, a.parity_streams))
        bc.emit(rows[-1])
    bc.write_rows(a.out, rows=rows)


if __name__ == "__main__":
    main()
