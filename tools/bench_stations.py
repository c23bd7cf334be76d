#!/usr/bin/env python3
"""Station bank (fmd_stations_*): S streams x 262144 B per call at 2.4 Msps, decimate 10, 64 taps, K stations -> 32 kHz audio,
against the same S streams through K fmd_firdemod launches (what a user can do today, without even the mixing).  One JSON
line per K (--k 1,4,8,16): ms per call (HIP events), input TB/s, station-outputs/s, and a parity bit against the test-side
definition (tests/stations_ref.py) on a seeded sample of streams."""
import numpy as np
import torch

import bench_common as bc
from bench_common import fmd, time_calls

FS, D, T, FAST, SLOW = 2400000, 10, 64, 240000, 32000


def run(K, S, n, iters, parity_streams):
    import oracle_lib
    import stations_ref as sr
    h = bc.lowpass(T, 100000 / FS)
    incs = bc.station_incs(K, S, FS)
    bank = fmd.StationBank(h, D, incs, FAST, SLOW, n_streams=S, device_id=0)
    bufs, stream = bc.device_buffers(S, n)
    cap = bank.out_cap(n)
    out = torch.zeros((S, K, cap), dtype=torch.int16, device="cuda")
    got = {}

    def launch(i):
        got["n"] = bank.demodulate_device(bufs[i % 2].data_ptr(), n, out.data_ptr(), cap, stream)

    ms, ts = time_calls(launch, iters, warmup=5)
    bank.check()
    # K fmd_firdemod launches over the same streams (real taps, no mixing)
    fd = fmd.FirDemodBank(h, D, FAST, SLOW, S, device_id=0)
    fcap = fd.out_cap(n)
    fout = torch.zeros((S, fcap), dtype=torch.int16, device="cuda")

    def launch_fd(i):
        for _ in range(K):
            fd.demodulate_device(bufs[i % 2].data_ptr(), n, fout.data_ptr(), fcap, stream)

    ms_fd, ts_fd = time_calls(launch_fd, max(2, iters // max(1, K // 2)), warmup=5)
    fd.check()
    # parity: a fresh bank, two calls, sampled streams against the definition
    pb = fmd.StationBank(h, D, incs, FAST, SLOW, n_streams=S, device_id=0)
    sample = bc.parity_sample(S, parity_streams)
    o = oracle_lib.load()
    refs = {s: sr.StationsRef(o, h, D, incs[s], FAST, SLOW, pb.shift) for s in sample}
    ok = True
    for b in range(2):
        a = pb.demodulate_batch(bufs[b].cpu().numpy())
        host = bufs[b].cpu().numpy()
        for s in sample:
            exp = refs[s].feed(host[s])
            ok &= all(np.array_equal(a[s, k], exp[k]) for k in range(K))
    outputs = S * K * ((n // 2) // D)
    return {"tool": "bench_stations", "K": K, "streams": S, "nbytes": n, "decim": D, "taps": T, "shift": bank.shift,
            "kernel": bank.kernel_name(), "ms": round(ms, 4), "ms_all": [round(t, 4) for t in ts],
            "input_TBps": round(S * n / ms / 1e9, 3), "station_outputs_per_s": float("%.4g" % (outputs / ms * 1e3)),
            "firdemod_x_K_ms": round(ms_fd, 4), "firdemod_x_K_ms_all": [round(t, 4) for t in ts_fd],
            "ratio_vs_firdemod_x_K": round(ms / ms_fd, 3), "audio_per_station": got["n"],
            "parity": bool(ok), "parity_streams": sample}


def main():
    ap = bc.parser()
    ap.add_argument("--k", default="1,4,8,16")
    ap.add_argument("--parity-streams", type=int, default=2)
    a = ap.parse_args()
    for K in [int(x) for x in a.k.split(",")]:
        bc.emit(run(K, a.streams, a.nbytes, a.iters, a.parity_streams))


if __name__ == "__main__":
    main()
