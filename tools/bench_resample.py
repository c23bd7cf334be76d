#!/usr/bin/env python3
"""Time the rational resampler (fmd_resample_*) on one MI355X at the rows two banks leave behind at 512 streams x 8 stations:

    stereo:  4096 rows x 2621 samples x width 2 at 15 / 16   (the stereo bank's 51.2 kHz audio of one 262144 B call to 48 kHz)
    narrow:  4096 rows x  655 samples x width 1 at  4 /  1   (the narrow-band bank's 12 kHz audio to 48 kHz)

32 taps per phase (resample_taps).  HIP events, the median of 3 x 200 calls after a warm-up, every call on the same device rows (the
stream moves on, the work per call changes by at most one output).  The memory floor is measured in the same process: a plain
contiguous device-to-device copy of the same input rows.  Two sampled rows of the first three calls are compared with
tests/resample_ref.py on the host.  Writes profiles/resample_bench.json."""
import bench_common as bc
from bench_common import fmd, np, torch

import resample_ref as rr

SHAPES = [("stereo", 4096, 2621, 2, 15, 16), ("narrow", 4096, 655, 1, 4, 1)]
TAPS = 32


def bench(name, rows, n, width, L, M, iters):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    src = torch.randint(-32768, 32768, (rows, n, width), generator=gen, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    g, shift = fmd.resample_taps(L, M, TAPS)

    def handle():
        return fmd.Resampler(g, L, M, shift, n_rows=rows, width=width, device_id=0)
    rs = handle()
    cap = rs.out_cap(n)
    d_out = torch.zeros((rows, cap, width), dtype=torch.int16, device="cuda")

    sample = bc.parity_sample(rows, 2)
    host = src[sample].cpu().numpy()
    ref = rr.Resampler(g, L, M, shift)
    for _ in range(3):
        k = rs.run_device(src.data_ptr(), n, n, d_out.data_ptr(), cap, stream)
        rs.check()
        exp = ref.push(host)
        got = d_out[sample].cpu().numpy()[:, :k]
        if k != exp.shape[1] or not np.array_equal(got, exp):
            raise SystemExit("%s: rows %s differ from tests/resample_ref.py" % (name, sample))
    del rs

    rs = handle()
    in0, out0 = rs.counts()
    ms, all_ms = bc.time_calls(lambda i: rs.run_device(src.data_ptr(), n, n, d_out.data_ptr(), cap, stream), iters)
    rs.check()
    in1, out1 = rs.counts()
    calls = (in1 - in0) // n
    eb = 2 * width
    bytes_call = rows * eb * (n + (out1 - out0) / calls)     # input once, the call's outputs once (history not counted)
    macs = rows * width * TAPS * (out1 - out0) / calls

    dst = torch.empty_like(src)
    copy_ms, copy_all = bc.time_calls(lambda i: dst.copy_(src), iters)
    if not torch.equal(dst, src):
        raise SystemExit("%s: the copy did not copy" % name)
    return bc.emit({"shape": name, "rows": rows, "samples": n, "width": width, "L": L, "M": M, "taps_per_phase": TAPS, "shift": int(shift),
                    "kernel": rs.kernel_name(), "outputs_per_call": round((out1 - out0) / calls, 2),
                    "ms_per_call": round(ms, 5), "ms_runs": [round(t, 5) for t in all_ms], "bytes_per_call": int(bytes_call),
                    "gb_per_s": round(bytes_call / ms / 1e6, 1), "gmacs_per_s": round(macs / ms / 1e6, 1),
                    "copy_ms": round(copy_ms, 5), "copy_runs": [round(t, 5) for t in copy_all],
                    "copy_bytes": 2 * rows * n * eb, "copy_gb_per_s": round(2 * rows * n * eb / copy_ms / 1e6, 1),
                    "ratio_to_copy": round(ms / copy_ms, 3), "parity_rows": sample, "parity": "exact"})


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    bc.add_out(ap, "resample_bench.json")
    a = ap.parse_args()
    rows = [bench(*s, a.iters) for s in SHAPES]
    bc.write_rows(a.out, taps_per_phase=TAPS, iters=a.iters, rows=rows)


if __name__ == "__main__":
    main()
