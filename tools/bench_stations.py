#!/usr/bin/env python3
"""Station bank (fmd_stations_*): S streams x 262144 B per call at 2.4 Msps, decimate 10, 64 taps, K stations -> 32 kHz audio,
against the same S streams through K fmd_firdemod launches (what a user can do today, without even the mixing).  One JSON
line per K (--k 1,4,8,16): ms per call (HIP events), input TB/s, station-outputs/s, and a parity bit against the test-side
definition (tests/stations_ref.py) on a seeded sample of streams."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import rtl_sdr_rs_amd as fmd

FS, D, T, FAST, SLOW = 2400000, 10, 64, 240000, 32000


def lowpass(T, cutoff):
    n = np.arange(T) - (T - 1) / 2
    h = np.sinc(2 * cutoff * n) * np.hamming(T)
    h = h / np.abs(h).max()
    return np.round(h * 2047).astype(np.int16)


def time_calls(launch, iters, reps=3):
    for _ in range(5):
        launch(0)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            launch(i)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return sorted(ts)[len(ts) // 2], ts


def run(K, S, n, iters, parity_streams):
    import oracle_lib
    import stations_ref as sr
    h = lowpass(T, 100000 / FS)
    rng = np.random.default_rng(K)
    offs = np.linspace(-1000000, 1000000, K) if K > 1 else np.array([300000.0])
    incs = np.array([[fmd.phase_inc(int(o) + int(rng.integers(-5000, 5000)), FS) for o in offs] for _ in range(S)], np.uint32)
    bank = fmd.StationBank(h, D, incs, FAST, SLOW, n_streams=S, device_id=0)
    stream = torch.cuda.current_stream().cuda_stream
    bufs = []
    for b in range(2):
        t = torch.empty((S, n), dtype=torch.uint8, device="cuda")
        fmd.synth.fill_device(t.data_ptr(), S, n, sample_offset=b * (n // 2), stream=stream)
        bufs.append(t)
    cap = bank.out_cap(n)
    out = torch.zeros((S, K, cap), dtype=torch.int16, device="cuda")
    got = {}

    def launch(i):
        got["n"] = bank.demodulate_device(bufs[i % 2].data_ptr(), n, out.data_ptr(), cap, stream)

    ms, ts = time_calls(launch, iters)
    bank.check()
    # K fmd_firdemod launches over the same streams (real taps, no mixing)
    fd = fmd.FirDemodBank(h, D, FAST, SLOW, S, device_id=0)
    fcap = fd.out_cap(n)
    fout = torch.zeros((S, fcap), dtype=torch.int16, device="cuda")

    def launch_fd(i):
        for _ in range(K):
            fd.demodulate_device(bufs[i % 2].data_ptr(), n, fout.data_ptr(), fcap, stream)

    ms_fd, ts_fd = time_calls(launch_fd, max(2, iters // max(1, K // 2)))
    fd.check()
    # parity: a fresh bank, two calls, sampled streams against the definition
    pb = fmd.StationBank(h, D, incs, FAST, SLOW, n_streams=S, device_id=0)
    sample = sorted(np.random.default_rng(7).choice(S, min(parity_streams, S), replace=False).tolist())
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="1,4,8,16")
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--nbytes", type=int, default=fmd.DEFAULT_BUF_LENGTH)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parity-streams", type=int, default=2)
    a = ap.parse_args()
    for K in [int(x) for x in a.k.split(",")]:
        print(json.dumps(run(K, a.streams, a.nbytes, a.iters, a.parity_streams)), flush=True)


if __name__ == "__main__":
    main()
