#!/usr/bin/env python3
"""Band-plan bank (fmd_bandplan_*): S streams x 262144 B per call (cut to whole hops) at 2.4 Msps, prototype uniform_taps(N, T / N), squelch blocks of
256.  Per row (N, hop, T, selected channels, mode, R, Ta): ms per call over BOTH passes (HIP events, warm-up, median of 3 x --iters
calls), a parity bit against the test-side definition (tests/bandplan_ref.py) on one stream and a few channels over two calls, and
two baselines timed in the same process:
  (a) the uniform channelizer alone at the same shape -- pass 1, the floor; ms - ms_uniform is what pass 2 costs;
  (b) the job without this handle: ceil(selected / 32) fmd_narrow launches with decim = hop, the prototype CUT to its central 256
      taps (the station front end admits no more) and the same second stage -- only where hop <= 64.
Writes every line to --out (profiles/bandplan_bench.json)."""
import numpy as np
import torch

import bench_common as bc
from bench_common import fmd, time_calls

FS, P, SQUELCH = 2400000, 256, 20
BANDS = {"am": (-4000, 4000), "fm": (-6000, 6000), "usb": (300, 3000)}
# N, hop, T, selected, mode, R, Ta
ROWS = [(96, 48, 768, None, "am", 4, 32), (128, 64, 1024, None, "fm", 2, 32), (256, 128, 2048, None, "usb", 2, 64),
        (128, 64, 1024, 32, "am", 4, 32)]


def run(N, hop, T, nsel, mode, R, Ta, S, n, iters):
    import bandplan_ref as br
    n = n // (2 * hop) * (2 * hop)                           # whole hops per call (hop 48: 262080 of the 262144 bytes)
    h = fmd.uniform_taps(N, T // N)
    sel = None if nsel is None else [int(k) for k in np.linspace(0, N - 1, nsel).astype(int)]
    chans = list(range(N)) if sel is None else sel
    gr, gi = fmd.narrow_taps(FS / hop, Ta, *BANDS[mode])
    bufs, stream = bc.device_buffers(S, n)
    mk = lambda: fmd.BandPlanBank(h, N, hop, (gr, gi), R, mode=mode, channels=sel, n_streams=S, block=P, squelch=SQUELCH, device_id=0)
    bp = mk()
    K = bp.n_selected
    cap = bp.out_cap(n)
    out = torch.empty((S, K, cap, bp.width), dtype=torch.int16, device="cuda")
    got = {}

    def launch(i):
        got["n"] = bp.run_device(bufs[i % 2].data_ptr(), n, out.data_ptr(), cap, stream)

    ms, ts = time_calls(launch, iters)
    bp.check()
    row = {"tool": "bench_bandplan", "n_channels": N, "hop": hop, "taps": T, "selected": K, "mode": mode, "chan_decim": R,
           "chan_taps": Ta, "complex_taps": gi is not None, "block": P, "squelch": SQUELCH, "streams": S, "nbytes": n,
           "shift": bp.shift, "chan_shift": bp.chan_shift, "kernels": [bp.kernel_name(0), bp.kernel_name(1)],
           "audio_per_channel": got["n"], "ms": round(ms, 4), "ms_all": [round(t, 4) for t in ts], "in_bytes": S * n,
           "y_bytes": S * K * 4 * (n // (2 * hop)), "out_bytes": S * K * got["n"] * 2 * bp.width}
    # (a) pass 1 alone
    u = fmd.UniformChannelizer(h, N, hop, channels=sel, n_streams=S, shift=bp.shift, device_id=0)
    ucap = u.out_cap(n)
    uout = torch.empty((S, K, ucap, 2), dtype=torch.int16, device="cuda")
    ms_u, ts_u = time_calls(lambda i: u.run_device(bufs[i % 2].data_ptr(), n, uout.data_ptr(), ucap, stream), iters)
    u.check()
    del u, uout
    row.update({"uniform_ms": round(ms_u, 4), "uniform_ms_all": [round(t, 4) for t in ts_u], "pass2_ms": round(ms - ms_u, 4),
                "pass2_over_pass1": round((ms - ms_u) / ms_u, 3)})
    # (b) fmd_narrow launches of at most 32 stations, the prototype cut to its central 256 taps
    if hop <= 64:
        hc = h if T <= 256 else h[(T - 256) // 2:(T - 256) // 2 + 256]
        groups = [chans[i:i + 32] for i in range(0, len(chans), 32)]
        incs = [np.array([fmd.uniform_channel_inc(k, N) for k in g], np.uint32) for g in groups]
        shift_c = max(fmd.stations_auto_shift(hc, i, limit=16384) for i in incs)
        nbs = [fmd.NarrowBank(hc, hop, i, (gr, gi), R, mode=mode, n_streams=S, block=P, squelch=SQUELCH, shift=shift_c, device_id=0)
               for i in incs]
        ncap = nbs[0].out_cap(n)
        nouts = [torch.empty((S, len(g), ncap, bp.width), dtype=torch.int16, device="cuda") for g in groups]

        def launch_n(i):
            for b, o in zip(nbs, nouts):
                b.run_device(bufs[i % 2].data_ptr(), n, o.data_ptr(), ncap, stream)

        ms_n, ts_n = time_calls(launch_n, iters)
        for b in nbs:
            b.check()
        row.update({"narrow_launches": len(groups), "narrow_taps": int(hc.size), "narrow_ms": round(ms_n, 4),
                    "narrow_ms_all": [round(t, 4) for t in ts_n], "speedup_vs_narrow": round(ms_n / ms, 2),
                    "not_slower_than_narrow": bool(ms <= ms_n)})
        del nbs, nouts
    else:
        row.update({"narrow_launches": None, "narrow_taps": None, "narrow_ms": None, "speedup_vs_narrow": None,
                    "not_slower_than_narrow": None})
    torch.cuda.empty_cache()
    # parity: a fresh handle, two calls, one stream, a few of the rows against the definition
    pb = mk()
    pick = sorted(set([0, 1, K // 2 - 1, K // 2, K - 1]))
    s = S // 3
    ref = br.BandPlanRef(h, N, hop, pb.shift, pb.gr, pb.gi, pb.mode, R, pb.chan_shift, P, SQUELCH, pb.gain, channels=[chans[i] for i in pick])
    ok = True
    for b in range(2):
        host = bufs[b][s].cpu().numpy()
        m = pb.run_device(bufs[b].data_ptr(), n, out.data_ptr(), cap, stream)
        pb.check()
        a = out[s, :, :m].cpu().numpy()[pick]
        ok &= bool(np.array_equal(a if pb.width == 2 else a[..., 0], ref.feed(host)))
    opn, rms = pb.levels()
    ok &= [(bool(opn[s, i]), int(rms[s, i])) for i in pick] == [ref.level(j) for j in range(len(pick))]
    row.update({"parity": bool(ok), "parity_stream": s, "parity_rows": pick})
    bc.emit(row)
    return row


def main():
    ap = bc.parser()
    ap.add_argument("--rows", default="0,1,2,3")
    bc.add_out(ap, "bandplan_bench.json")
    a = ap.parse_args()
    rows = [run(*ROWS[int(i)], a.streams, a.nbytes, a.iters) for i in a.rows.split(",")]
    bc.write_rows(a.out, rows=rows)


if __name__ == "__main__":
    main()
