#!/usr/bin/env python3
"""Uniform channelizer (fmd_uniform_*): S streams x 262144 B per call at 2.4 Msps, prototype uniform_taps(N, T / N).  Per row
(N, hop, T, selected channels): ms per call (HIP events, warm-up, median of 3 x --iters calls), input TB/s, the i8 MAC/s the matrix
cores issue against the v_mfma_i32_16x16x64_i8 rate, a parity bit against the test-side definition (tests/uniform_ref.py) on one
stream and a few channels over two calls, and two baselines timed in the same process:
  - today's way to get the channels: ceil(selected / 32) fmd_channelizer launches at K <= 32 with decim = hop and the prototype CUT
    to its central 256 taps (a shorter, worse filter: the channelizer admits no more) -- only where hop <= 64;
  - what a torch user writes: u8 -> complex64, frames by unfold, window, fold to N, torch.fft.fft.
Writes every line to --out (profiles/uniform_bench.json)."""
import numpy as np
import torch

import bench_common as bc
from bench_common import fmd, time_calls

FS = 2400000
ROWS = [(16, 8, 128, None), (128, 64, 1024, None), (256, 128, 2048, None), (128, 64, 1024, 32)]
PEAK_MACS = 256 * 4 * (16 * 16 * 64 / 16.0) * 2.4e9        # 256 CUs x 4 SIMDs x one 16x16x64 MFMA per 16 cycles at 2.4 GHz


def torch_chain(bufs, h, N, hop, S, n, chunk):
    T = h.size
    w = torch.from_numpy(h.astype(np.float32)).cuda()

    def launch(i):
        outs = []
        for s0 in range(0, S, chunk):
            x = bufs[i % 2][s0:s0 + chunk].view(-1, n // 2, 2).float() - 127.0
            xc = torch.complex(x[..., 0], x[..., 1])
            fr = xc.unfold(1, T, hop) * w                                    # [chunk, frames, T]
            outs.append(torch.fft.fft(fr.view(fr.shape[0], fr.shape[1], T // N, N).sum(dim=2), dim=2))
        return outs

    return launch


def run(N, hop, T, nsel, S, n, iters):
    import uniform_ref as ur
    h = fmd.uniform_taps(N, T // N)
    sel = None if nsel is None else [int(k) for k in np.linspace(0, N - 1, nsel).astype(int)]
    bufs, stream = bc.device_buffers(S, n)
    mk = lambda: fmd.UniformChannelizer(h, N, hop, channels=sel, n_streams=S, device_id=0)
    u = mk()
    K = u.n_selected
    cap = u.out_cap(n)
    out = torch.empty((S, K, cap, 2), dtype=torch.int16, device="cuda")
    got = {}

    def launch(i):
        got["n"] = u.run_device(bufs[i % 2].data_ptr(), n, out.data_ptr(), cap, stream)

    ms, ts = time_calls(launch, iters)
    u.check()
    digits = u.tap_digits()
    nrt, nkc = -(-K // (8 if digits == 1 else 4)), -(-2 * T // 64)
    macs = S * got["n"] * nrt * nkc * 1024.0                                # per call: MFMAs x 16 x 16 x 64 / 16 columns
    row = {"tool": "bench_uniform", "n_channels": N, "hop": hop, "taps": T, "selected": K, "streams": S, "nbytes": n,
           "shift": u.shift, "digits": digits, "kernel": u.kernel_name(), "outputs_per_channel": got["n"],
           "ms": round(ms, 4), "ms_all": [round(t, 4) for t in ts], "in_bytes": S * n, "out_bytes": S * K * got["n"] * 4,
           "input_TBps": round(S * n / ms / 1e9, 4), "output_TBps": round(S * K * got["n"] * 4 / ms / 1e9, 4),
           "mfma_macs_per_s": round(macs / ms * 1e3, -9), "mfma_rate_fraction": round(macs / ms * 1e3 / PEAK_MACS, 4)}
    # baseline 1: fmd_channelizer launches of at most 32 stations, the prototype cut to its central 256 taps
    if hop <= 64:
        hc = h if T <= 256 else h[(T - 256) // 2:(T - 256) // 2 + 256]
        chans = list(range(N)) if sel is None else sel
        groups = [chans[i:i + 32] for i in range(0, len(chans), 32)]
        incs = [np.array([fmd.uniform_channel_inc(k, N) for k in g], np.uint32) for g in groups]
        shift_c = max(fmd.stations_auto_shift(hc, i, limit=16384) for i in incs)
        chs = [fmd.Channelizer(hc, hop, i, n_streams=S, shift=shift_c, device_id=0) for i in incs]
        ccap = chs[0].out_cap(n)
        couts = [torch.empty((S, len(g), ccap, 2), dtype=torch.int16, device="cuda") for g in groups]

        def launch_c(i):
            for c, o in zip(chs, couts):
                c.run_device(bufs[i % 2].data_ptr(), n, o.data_ptr(), ccap, stream)

        ms_c, ts_c = time_calls(launch_c, iters)
        for c in chs:
            c.check()
        row.update({"channelizer_launches": len(groups), "channelizer_taps": int(hc.size), "channelizer_ms": round(ms_c, 4),
                    "channelizer_ms_all": [round(t, 4) for t in ts_c], "speedup_vs_channelizer": round(ms_c / ms, 2)})
        del chs, couts
    else:
        row.update({"channelizer_launches": None, "channelizer_taps": None, "channelizer_ms": None, "speedup_vs_channelizer": None})
    # baseline 2: float torch, all N channels whatever the selection
    try:
        ms_t, ts_t = time_calls(torch_chain(bufs, h, N, hop, S, n, 64), 2, reps=2)
    except torch.cuda.OutOfMemoryError:
        ms_t, ts_t = None, []
    torch.cuda.empty_cache()
    row.update({"torch_ms": None if ms_t is None else round(ms_t, 3), "torch_ms_all": [round(t, 3) for t in ts_t],
                "speedup_vs_torch": None if ms_t is None else round(ms_t / ms, 1)})
    # parity: a fresh handle, two calls, one stream, a few of the rows against the definition
    pb = mk()
    chans = list(range(N)) if sel is None else sel
    pick = sorted(set([0, 1, K // 2 - 1, K // 2, K - 1]))
    s = S // 3
    ref = ur.UniformRef(h, N, hop, pb.shift, channels=[chans[i] for i in pick])
    ok = True
    for b in range(2):
        host = bufs[b][s].cpu().numpy()
        m = pb.run_device(bufs[b].data_ptr(), n, out.data_ptr(), cap, stream)
        pb.check()
        a = out[s, :, :m].cpu().numpy()[pick]
        ok &= bool(np.array_equal(a, ref.feed(host)))
    row.update({"parity": bool(ok), "parity_stream": s, "parity_rows": pick})
    bc.emit(row)
    return row


def main():
    ap = bc.parser()
    ap.add_argument("--rows", default="0,1,2,3")
    bc.add_out(ap, "uniform_bench.json")
    a = ap.parse_args()
    rows = [run(*ROWS[int(i)], a.streams, a.nbytes, a.iters) for i in a.rows.split(",")]
    bc.write_rows(a.out, peak_macs_per_s=PEAK_MACS, rows=rows)


if __name__ == "__main__":
    main()
