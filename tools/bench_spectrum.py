#!/usr/bin/env python3
"""Power-spectrum scanner (fmd_spectrum_*): S streams x 262144 B per call, N bins, hop = N, one- and two-digit taps (integer Hann
windows of amplitude 127 and 2047), against the same power computed the way a user can today in torch (u8 -> complex64, unfold,
torch.fft.fft, |.|^2, sum over frames).  One JSON line per (N, digits) and all of them in --out: ms per call (HIP events), input
TB/s, i8 MACs per second (S F x 2 N digits rows x 2 N bytes), and a parity bit against the test-side definition
(tests/spectrum_ref.py) on a seeded sample of streams."""
import numpy as np
import torch

import bench_common as bc
from bench_common import fmd, time_calls


def run(N, digits, S, n, iters, parity_streams, bufs):
    import spectrum_ref as spr
    shift = 16
    w = fmd.hann_window(N, 127 if digits == 1 else 2047)
    sp = fmd.Spectrum(N, N, window=w, shift=shift, n_streams=S, device_id=0)
    assert sp.tap_digits() == digits
    stream = torch.cuda.current_stream().cuda_stream
    power = torch.zeros((S, N), dtype=torch.int64, device="cuda")

    def launch(i):
        sp.power_device(bufs[i % 2].data_ptr(), n, power.data_ptr(), accumulate=False, stream=stream)

    ms, ts = time_calls(launch, iters)
    sp.check()
    # the torch baseline over the same bytes
    wf = torch.from_numpy(w.astype(np.float32)).cuda()

    def baseline(i):
        x = bufs[i % 2].view(S, n // 2, 2).to(torch.float32) - 127.0
        c = torch.complex(x[..., 0], x[..., 1])
        fr = c.unfold(1, N, N) * wf
        return (torch.fft.fft(fr, dim=-1).abs() ** 2).sum(dim=1)

    ms_t, ts_t = time_calls(baseline, iters)
    # parity: the last timed call's buffer, sampled streams against the definition
    launch(iters - 1)
    torch.cuda.synchronize()
    got = power.cpu().numpy().view(np.uint64)
    host = bufs[(iters - 1) % 2].cpu().numpy()
    sample = bc.parity_sample(S, parity_streams)
    ok = all(np.array_equal(got[s], spr.power(w, N, shift, host[s:s + 1])[0]) for s in sample)
    F = sp.frames(n)
    macs = S * F * (2 * N * digits) * (2 * N)
    return {"tool": "bench_spectrum", "n_bins": N, "hop": N, "digits": digits, "streams": S, "nbytes": n, "frames": F,
            "shift": shift, "kernel": sp.kernel_name(), "ms": round(ms, 4), "ms_all": [round(t, 4) for t in ts],
            "input_TBps": round(S * n / ms / 1e9, 3), "i8_macs": macs, "i8_macs_per_s": float("%.4g" % (macs / ms * 1e3)),
            "torch_fft_ms": round(ms_t, 4), "torch_fft_ms_all": [round(t, 4) for t in ts_t],
            "speedup_vs_torch_fft": round(ms_t / ms, 2), "parity": bool(ok), "parity_streams": sample}


def main():
    ap = bc.parser()
    ap.add_argument("--bins", default="64,256")
    ap.add_argument("--parity-streams", type=int, default=3)
    bc.add_out(ap, "spectrum_bench.json")
    a = ap.parse_args()
    bufs, _ = bc.device_buffers(a.streams, a.nbytes)
    rows = []
    for N in [int(x) for x in a.bins.split(",")]:
        for d in (1, 2):
            r = run(N, d, a.streams, a.nbytes, a.iters, a.parity_streams, bufs)
            bc.emit(r)
            rows.append(r)
    bc.write_rows(a.out, rows=rows)


if __name__ == "__main__":
    main()
