#!/usr/bin/env python3
"""Narrow-band bank (fmd_narrow_*): S streams x 262144 B per call at 2.4 Msps, decimate 10 (240 kHz), 64 front-end taps, channel
decimation 20 (12 kHz) with 256 channel taps, squelch blocks of 256, K stations.  Per K (--k 1,4,8,16,32) and mode (iq, fm, am, usb):
ms per call (HIP events, both passes), a parity bit against the test-side definition (tests/narrow_ref.py) on a seeded sample of
streams, and two baselines timed in the same process: the channelizer at the same K and shift (pass 1 alone: the floor), and the
same chain in float torch (u8 -> mix -> conv1d stride D -> complex conv1d stride R -> abs / angle / real).  Writes every line to
--out (profiles/narrow_bench.json)."""
import numpy as np
import torch

import bench_common as bc
from bench_common import fmd, time_calls

FS, D, T, R, TA, P = 2400000, 10, 64, 20, 256, 256
BANDS = {"iq": (-5000, 5000), "fm": (-6000, 6000), "am": (-4000, 4000), "usb": (300, 3000)}


def torch_chain(bufs, incs, h, gr, gi, mode, S, K, n, chunk):
    """The same chain in float torch, `chunk` streams at a time (the mixed signal of all of them at once does not fit for large K)."""
    N = n // 2
    tn = torch.arange(N, device="cuda", dtype=torch.float64)
    w = torch.from_numpy(h.astype(np.float32)).cuda().view(1, 1, T).repeat(2, 1, 1)
    g_r = torch.from_numpy(gr.astype(np.float32)).cuda()
    g_i = torch.from_numpy((np.zeros_like(gr) if gi is None else gi).astype(np.float32)).cuda()
    wc = torch.stack([torch.stack([g_r, -g_i]), torch.stack([g_i, g_r])])                      # [2 out, 2 in, Ta]: vr, vi
    ph = torch.from_numpy(incs.astype(np.float64) / 2.0 ** 32).cuda()

    def launch(i):
        outs = []
        for s0 in range(0, S, chunk):
            x = bufs[i % 2][s0:s0 + chunk].view(-1, N, 2).float() - 127.0
            xc = torch.complex(x[..., 0], x[..., 1])
            a = (-2 * np.pi * torch.remainder(ph[s0:s0 + chunk, :, None] * tn, 1.0)).float()
            mixed = xc[:, None, :] * torch.complex(torch.cos(a), torch.sin(a))                 # [chunk, K, N]
            r = torch.view_as_real(mixed).permute(0, 1, 3, 2).reshape(-1, 2, N)
            y = torch.nn.functional.conv1d(r, w, stride=D, groups=2)                           # [chunk K, 2, M]
            v = torch.nn.functional.conv1d(y, wc, stride=R)                                    # [chunk K, 2, NA]
            vc = torch.complex(v[:, 0], v[:, 1])
            if mode == "fm":
                o = torch.angle(vc[:, 1:] * torch.conj(vc[:, :-1]))
            elif mode == "am":
                m = vc.abs()
                o = m - m.mean(dim=1, keepdim=True)
            elif mode == "usb":
                o = v[:, 0]
            else:
                o = v
            outs.append(o)
        return outs

    return launch


def run(K, S, n, iters, parity_streams, modes):
    import narrow_ref as nr
    import stations_ref as sr
    h = bc.lowpass(T, 100000 / FS)
    incs = bc.station_incs(K, S, FS)
    bufs, stream = bc.device_buffers(S, n)
    shift = fmd.stations_auto_shift(h, incs, limit=16384)
    # the floor: the channelizer at the same K and shift (pass 1 alone)
    ch = fmd.Channelizer(h, D, incs, n_streams=S, shift=shift, device_id=0)
    ccap = ch.out_cap(n)
    cout = torch.empty((S, K, ccap, 2), dtype=torch.int16, device="cuda")
    ms_ch, ts_ch = time_calls(lambda i: ch.run_device(bufs[i % 2].data_ptr(), n, cout.data_ptr(), ccap, stream), iters)
    ch.check()
    del ch, cout
    rows = []
    for mode in modes:
        gr, gi = fmd.narrow_taps(FS // D, TA, *BANDS[mode])
        mk = lambda: fmd.NarrowBank(h, D, incs, (gr, gi), R, mode=mode, n_streams=S, block=P, squelch=20, shift=shift, device_id=0)
        nb = mk()
        cap = nb.out_cap(n)
        out = torch.empty((S, K, cap, nb.width), dtype=torch.int16, device="cuda")
        got = {}

        def launch(i):
            got["n"] = nb.run_device(bufs[i % 2].data_ptr(), n, out.data_ptr(), cap, stream)

        ms, ts = time_calls(launch, iters)
        nb.check()
        try:
            ms_torch, ts_torch = time_calls(torch_chain(bufs, incs, h, gr, gi, mode, S, K, n, max(1, 256 // K)), 2, reps=2)
        except torch.cuda.OutOfMemoryError:
            ms_torch, ts_torch = None, []
        torch.cuda.empty_cache()
        # parity: a fresh bank, two calls, sampled streams against the definition
        pb = mk()
        sample = bc.parity_sample(S, parity_streams)
        refs = {s: nr.NarrowRef(h, D, incs[s], pb.shift, pb.gr, pb.gi, pb.mode, R, pb.chan_shift, P, pb.squelch, pb.gain, z=sr.z_corr)
                for s in sample}
        ok = True
        for b in range(2):
            host = bufs[b].cpu().numpy()
            m = pb.run_device(bufs[b].data_ptr(), n, out.data_ptr(), cap, stream)
            pb.check()
            a = out[sample, :, :m].cpu().numpy()
            for i, s in enumerate(sample):
                ok &= bool(np.array_equal(a[i] if pb.width == 2 else a[i][..., 0], refs[s].feed(host[s])))
        rows.append({"tool": "bench_narrow", "K": K, "mode": mode, "streams": S, "nbytes": n, "decim": D, "taps": T, "chan_decim": R,
                     "chan_taps": TA, "complex_taps": gi is not None, "block": P, "shift": nb.shift, "chan_shift": nb.chan_shift,
                     "kernels": [nb.kernel_name(0), nb.kernel_name(1)], "audio_per_station": got["n"],
                     "ms": round(ms, 4), "ms_all": [round(t, 4) for t in ts], "in_bytes": S * n,
                     "y_bytes": S * K * 4 * ((n // 2 - T) // D + 1), "out_bytes": S * K * got["n"] * 2 * nb.width,
                     "channelizer_ms": round(ms_ch, 4), "channelizer_ms_all": [round(t, 4) for t in ts_ch],
                     "ratio_vs_channelizer": round(ms / ms_ch, 3),
                     "torch_ms": None if ms_torch is None else round(ms_torch, 3), "torch_ms_all": [round(t, 3) for t in ts_torch],
                     "speedup_vs_torch": None if ms_torch is None else round(ms_torch / ms, 1),
                     "parity": bool(ok), "parity_streams": sample})
        bc.emit(rows[-1])
        del nb, pb, out
    return rows


def main():
    ap = bc.parser()
    ap.add_argument("--k", default="1,4,8,16,32")
    ap.add_argument("--modes", default="iq,fm,am,usb")
    ap.add_argument("--parity-streams", type=int, default=2)
    bc.add_out(ap, "narrow_bench.json")
    a = ap.parse_args()
    rows = []
    for K in [int(x) for x in a.k.split(",")]:
        rows += run(K, a.streams, a.nbytes, a.iters, a.parity_streams, a.modes.split(","))
    bc.write_rows(a.out, rows=rows)


if __name__ == "__main__":
    main()
