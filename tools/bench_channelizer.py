#!/usr/bin/env python3
"""Channelizer (fmd_channelizer_*): S streams x 262144 B per call at 2.4 Msps, decimate 10, 64 taps, K stations -> complex baseband
at 240 kHz.  Per K (--k 1,4,8,16): ms per call (HIP events), input and output bytes and their TB/s, a parity bit against the
test-side definition (tests/channelizer_ref.py) on a seeded sample of streams, and two baselines timed in the same process: the
station bank at the same K (which computes the same y and then demodulates), and what a user writes today in torch (u8 -> float,
a complex mix per station, conv1d with stride D).  Writes every line to --out (profiles/channelizer_bench.json)."""
import numpy as np
import torch

import bench_common as bc
from bench_common import fmd, time_calls

FS, D, T, FAST, SLOW = 2400000, 10, 64, 240000, 32000


def run(K, S, n, iters, parity_streams):
    import channelizer_ref as cr
    import stations_ref as sr
    h = bc.lowpass(T, 100000 / FS)
    incs = bc.station_incs(K, S, FS)
    ch = fmd.Channelizer(h, D, incs, n_streams=S, device_id=0)
    bufs, stream = bc.device_buffers(S, n)
    cap = ch.out_cap(n)
    out = torch.empty((S, K, cap, 2), dtype=torch.int16, device="cuda")
    got = {}

    def launch(i):
        got["n"] = ch.run_device(bufs[i % 2].data_ptr(), n, out.data_ptr(), cap, stream)

    ms, ts = time_calls(launch, iters)
    ch.check()
    # baseline 1: the station bank at the same K (the same y, then fm_demod + low_pass_real; its own default shift)
    bank = fmd.StationBank(h, D, incs, FAST, SLOW, n_streams=S, device_id=0)
    bcap = bank.out_cap(n)
    bout = torch.empty((S, K, bcap), dtype=torch.int16, device="cuda")

    def launch_bank(i):
        bank.demodulate_device(bufs[i % 2].data_ptr(), n, bout.data_ptr(), bcap, stream)

    ms_bank, ts_bank = time_calls(launch_bank, iters)
    bank.check()
    del bank, bout
    # baseline 2: torch -- u8 -> float, a complex mix per station, conv1d(stride D) on (re, im) with the same prototype
    ph = torch.from_numpy(incs.astype(np.float64) / 2.0 ** 32).cuda()                          # cycles per sample, [S, K]
    tn = torch.arange(n // 2, device="cuda", dtype=torch.float64)
    w = torch.from_numpy(h.astype(np.float32)[::-1].copy()).cuda().view(1, 1, T).repeat(2, 1, 1)

    def launch_torch(i):
        x = bufs[i % 2].view(S, n // 2, 2).float() - 127.0
        xc = torch.complex(x[..., 0], x[..., 1])                                                # [S, N]
        a = (-2 * np.pi * torch.remainder(ph[:, :, None] * tn, 1.0)).float()
        lo = torch.complex(torch.cos(a), torch.sin(a))
        mixed = xc[:, None, :] * lo                                                            # [S, K, N]
        r = torch.view_as_real(mixed).permute(0, 1, 3, 2).reshape(S * K, 2, n // 2)
        return torch.nn.functional.conv1d(r, w, stride=D, groups=2)

    torch_iters = max(2, iters // 4)
    try:
        ms_torch, ts_torch = time_calls(launch_torch, torch_iters)
    except torch.cuda.OutOfMemoryError:
        ms_torch, ts_torch = None, []
    torch.cuda.empty_cache()
    # parity: a fresh channelizer, two calls, sampled streams against the definition
    pc = fmd.Channelizer(h, D, incs, n_streams=S, device_id=0)
    sample = bc.parity_sample(S, parity_streams)
    refs = {s: cr.ChannelizerRef(h, D, incs[s], pc.shift, z=sr.z_corr) for s in sample}
    ok = True
    for b in range(2):
        host = bufs[b].cpu().numpy()
        pout = torch.empty((S, K, cap, 2), dtype=torch.int16, device="cuda")
        m = pc.run_device(bufs[b].data_ptr(), n, pout.data_ptr(), cap, stream)
        pc.check()
        a = pout[sample, :, :m].cpu().numpy()
        for i, s in enumerate(sample):
            ok &= bool(np.array_equal(a[i], refs[s].feed(host[s])))
    in_bytes, out_bytes = S * n, S * K * got["n"] * 4
    return {"tool": "bench_channelizer", "K": K, "streams": S, "nbytes": n, "decim": D, "taps": T, "shift": ch.shift,
            "kernel": ch.kernel_name(), "outputs_per_station": got["n"], "ms": round(ms, 4), "ms_all": [round(t, 4) for t in ts],
            "in_bytes": in_bytes, "out_bytes": out_bytes, "io_TBps": round((in_bytes + out_bytes) / ms / 1e9, 3),
            "bank_ms": round(ms_bank, 4), "bank_ms_all": [round(t, 4) for t in ts_bank], "ratio_vs_bank": round(ms / ms_bank, 3),
            "torch_ms": None if ms_torch is None else round(ms_torch, 3), "torch_ms_all": [round(t, 3) for t in ts_torch],
            "speedup_vs_torch": None if ms_torch is None else round(ms_torch / ms, 1),
            "parity": bool(ok), "parity_streams": sample}


def main():
    ap = bc.parser()
    ap.add_argument("--k", default="1,4,8,16")
    ap.add_argument("--parity-streams", type=int, default=2)
    bc.add_out(ap, "channelizer_bench.json")
    a = ap.parse_args()
    rows = []
    for K in [int(x) for x in a.k.split(",")]:
        rows.append(run(K, a.streams, a.nbytes, a.iters, a.parity_streams))
        bc.emit(rows[-1])
    bc.write_rows(a.out, rows=rows)


if __name__ == "__main__":
    main()
