#!/usr/bin/env python3
"""Stereo station bank (fmd_stereo_*): S streams x 262144 B per call at 2.4 Msps, decimate 10 (f_m = 240 kHz), 64 front-end taps,
audio decimation 5 (48 kHz) with 127 audio taps, pilot blocks of 4096, K stations.  Per K (--k 1,4,8,16): ms per call (HIP events,
both passes and the block-sum reset), a parity bit against the test-side definition (tests/stereo_ref.py) on a seeded sample of
streams, and three baselines timed in the same process: the channelizer and the station bank at the same K, and the same chain in
float torch (u8 -> mix -> conv1d -> angle -> block pilot correlation -> carrier -> conv1d with stride R).  Writes every line to --out
(profiles/stereo_bench.json)."""
import numpy as np
import torch

import bench_common as bc
from bench_common import fmd, time_calls

FS, D, T, R, TA, P = 2400000, 10, 64, 5, 127, 4096


def run(K, S, n, iters, parity_streams):
    import stations_ref as sr
    import stereo_ref as st
    h = bc.lowpass(T, 130000 / FS)
    g = fmd.stereo_taps(FS // D, R, TA)
    incs = bc.station_incs(K, S, FS)
    sb = fmd.StereoBank(h, D, incs, FS, g, R, n_streams=S, block=P, device_id=0)
    bufs, stream = bc.device_buffers(S, n)
    cap = sb.out_cap(n)
    out = torch.empty((S, K, cap, 2), dtype=torch.int16, device="cuda")
    got = {}

    def launch(i):
        got["n"] = sb.run_device(bufs[i % 2].data_ptr(), n, out.data_ptr(), cap, stream)

    ms, ts = time_calls(launch, iters)
    sb.check()
    # baseline 1: the channelizer at the same K (its y is pass 1's input)
    ch = fmd.Channelizer(h, D, incs, n_streams=S, shift=sb.shift, device_id=0)
    ccap = ch.out_cap(n)
    cout = torch.empty((S, K, ccap, 2), dtype=torch.int16, device="cuda")
    ms_ch, ts_ch = time_calls(lambda i: ch.run_device(bufs[i % 2].data_ptr(), n, cout.data_ptr(), ccap, stream), iters)
    ch.check()
    del ch, cout
    # baseline 2: the mono station bank at the same K
    bank = fmd.StationBank(h, D, incs, 240000, 48000, n_streams=S, device_id=0)
    bcap = bank.out_cap(n)
    bout = torch.empty((S, K, bcap), dtype=torch.int16, device="cuda")
    ms_bank, ts_bank = time_calls(lambda i: bank.demodulate_device(bufs[i % 2].data_ptr(), n, bout.data_ptr(), bcap, stream), iters)
    bank.check()
    del bank, bout
    # baseline 3: the same chain in float torch
    N = n // 2
    M = (N - T) // D + 1
    ph = torch.from_numpy(incs.astype(np.float64) / 2.0 ** 32).cuda()
    tn = torch.arange(N, device="cuda", dtype=torch.float64)
    w = torch.from_numpy(h.astype(np.float32)[::-1].copy()).cuda().view(1, 1, T).repeat(2, 1, 1)
    ga = torch.from_numpy(g.astype(np.float32)[::-1].copy()).cuda().view(1, 1, TA)
    nb = M // P
    tm = torch.arange(nb * P, device="cuda", dtype=torch.float64) * (19000.0 / (FS / D))
    th = (2 * np.pi * torch.remainder(tm, 1.0)).float()
    cth, sth = torch.cos(th).view(nb, P), torch.sin(th).view(nb, P)

    def launch_torch(i):
        x = bufs[i % 2].view(S, N, 2).float() - 127.0
        xc = torch.complex(x[..., 0], x[..., 1])
        a = (-2 * np.pi * torch.remainder(ph[:, :, None] * tn, 1.0)).float()
        mixed = xc[:, None, :] * torch.complex(torch.cos(a), torch.sin(a))                       # [S, K, N]
        r = torch.view_as_real(mixed).permute(0, 1, 3, 2).reshape(S * K, 2, N)
        y = torch.nn.functional.conv1d(r, w, stride=D, groups=2)                                 # [S K, 2, M]
        yc = torch.complex(y[:, 0], y[:, 1])
        mpx = torch.angle(yc[:, 1:] * torch.conj(yc[:, :-1]))[:, :nb * P].reshape(S * K, nb, P)
        I = (mpx * cth).sum(-1)
        Q = (mpx * sth).sum(-1)
        alpha = torch.atan2(I, Q)                                                                # pilot sin(theta + alpha)
        prev = torch.cat([alpha[:, :1], alpha[:, :-1]], dim=1)[:, :, None]
        s = (mpx * 2 * torch.sin(2 * th.view(1, nb, P) + 2 * prev)).reshape(S * K, 1, nb * P)
        both = torch.cat([mpx.reshape(S * K, 1, nb * P), s], dim=0)
        au = torch.nn.functional.conv1d(both, ga, stride=R)
        return au[:S * K] + au[S * K:], au[:S * K] - au[S * K:]

    try:
        ms_torch, ts_torch = time_calls(launch_torch, max(2, iters // 4))
    except torch.cuda.OutOfMemoryError:
        ms_torch, ts_torch = None, []
    torch.cuda.empty_cache()
    # parity: a fresh bank, two calls, sampled streams against the definition
    pb = fmd.StereoBank(h, D, incs, FS, g, R, n_streams=S, block=P, device_id=0)
    sample = bc.parity_sample(S, parity_streams)
    refs = {s: st.StereoRef(h, D, incs[s], pb.shift, FS, g, R, P, pb.pilot_min, pb.audio_shift, z=sr.z_corr) for s in sample}
    ok = True
    for b in range(2):
        host = bufs[b].cpu().numpy()
        pout = torch.empty((S, K, cap, 2), dtype=torch.int16, device="cuda")
        m = pb.run_device(bufs[b].data_ptr(), n, pout.data_ptr(), cap, stream)
        pb.check()
        a = pout[sample, :, :m].cpu().numpy()
        for i, s in enumerate(sample):
            ok &= bool(np.array_equal(a[i], refs[s].feed(host[s])))
    x_bytes = S * K * (2 * ((n // 2 - T) // D + 1))
    return {"tool": "bench_stereo", "K": K, "streams": S, "nbytes": n, "decim": D, "taps": T, "audio_decim": R, "audio_taps": TA,
            "block": P, "shift": sb.shift, "audio_shift": sb.audio_shift, "pilot_min": sb.pilot_min,
            "kernels": [sb.kernel_name(0), sb.kernel_name(1)], "audio_per_station": got["n"],
            "ms": round(ms, 4), "ms_all": [round(t, 4) for t in ts], "in_bytes": S * n, "x_bytes": x_bytes,
            "out_bytes": S * K * got["n"] * 4,
            "channelizer_ms": round(ms_ch, 4), "channelizer_ms_all": [round(t, 4) for t in ts_ch],
            "ratio_vs_channelizer": round(ms / ms_ch, 3),
            "bank_ms": round(ms_bank, 4), "bank_ms_all": [round(t, 4) for t in ts_bank], "ratio_vs_bank": round(ms / ms_bank, 3),
            "torch_ms": None if ms_torch is None else round(ms_torch, 3), "torch_ms_all": [round(t, 3) for t in ts_torch],
            "speedup_vs_torch": None if ms_torch is None else round(ms_torch / ms, 1),
            "parity": bool(ok), "parity_streams": sample}


def main():
    ap = bc.parser()
    ap.add_argument("--k", default="1,4,8,16")
    ap.add_argument("--parity-streams", type=int, default=2)
    bc.add_out(ap, "stereo_bench.json")
    a = ap.parse_args()
    rows = []
    for K in [int(x) for x in a.k.split(",")]:
        rows.append(run(K, a.streams, a.nbytes, a.iters, a.parity_streams))
        bc.emit(rows[-1])
    bc.write_rows(a.out, rows=rows)


if __name__ == "__main__":
    main()
