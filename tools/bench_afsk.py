#!/usr/bin/env python3
"""Time the tone-pair demodulator (fmd_afsk_*) on one MI355X at the rows two banks leave behind:

    narrow:    4096 rows x  655 samples at 12 kHz (T 10, D 2)   (the narrow-band bank's audio of one 262144 B call at K = 8)
    bandplan: 65536 rows x 1024 samples at 24 kHz (T 20, D 4)   (a 128-channel band plan over 512 streams)

The designed table of each rate (afsk_table) and the default stride.  HIP events, the median of 3 x 200 consecutive calls after a
warm-up, every call on the same device rows (the stream moves on, the work per call changes by at most one output).  The memory
floor is measured in the same process: a plain contiguous device-to-device copy of the same input rows.  Two sampled rows of the
first three calls are compared with tests/afsk_ref.py on the host.  Writes profiles/afsk_bench.json."""
import bench_common as bc
from bench_common import fmd, np, torch

import afsk_ref as ar

SHAPES = [("narrow", 4096, 655, 12000), ("bandplan", 65536, 1024, 24000)]


def bench(name, rows, n, rate, iters):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    src = torch.randint(-32768, 32768, (rows, n), generator=gen, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    tab, pre, out = fmd.afsk_table(rate)
    T, D = tab.shape[1], fmd.afsk_stride(tab.shape[1])

    def handle():
        return fmd.AfskDemod(tab, D, pre, out, n_rows=rows, device_id=0)
    af = handle()
    cap = af.out_cap(n)
    d_out = torch.zeros((rows, cap), dtype=torch.int16, device="cuda")

    sample = bc.parity_sample(rows, 2)
    host = src[sample].cpu().numpy()
    ref = ar.AfskDemod(tab, D, pre, out, rows=2)
    for _ in range(3):
        k = af.run_device(src.data_ptr(), n, n, d_out.data_ptr(), cap, stream)
        af.check()
        exp = ref.push(host)
        got = d_out[sample].cpu().numpy()[:, :k]
        if k != exp.shape[1] or not np.array_equal(got, exp):
            raise SystemExit("%s: rows %s differ from tests/afsk_ref.py" % (name, sample))
    del af

    af = handle()
    in0, out0 = af.counts()
    ms, all_ms = bc.time_calls(lambda i: af.run_device(src.data_ptr(), n, n, d_out.data_ptr(), cap, stream), iters)
    af.check()
    in1, out1 = af.counts()
    calls = (in1 - in0) // n
    bytes_call = rows * 2 * (n + (out1 - out0) / calls)      # input once, the call's outputs once (history not counted)
    macs = rows * 4 * T * (out1 - out0) / calls

    dst = torch.empty_like(src)
    copy_ms, copy_all = bc.time_calls(lambda i: dst.copy_(src), iters)
    if not torch.equal(dst, src):
        raise SystemExit("%s: the copy did not copy" % name)
    return bc.emit({"shape": name, "rows": rows, "samples": n, "rate": rate, "taps": T, "stride": D, "pre_shift": int(pre), "out_shift": int(out),
                    "kernel": af.kernel_name(), "outputs_per_call": round((out1 - out0) / calls, 2),
                    "ms_per_call": round(ms, 5), "ms_runs": [round(t, 5) for t in all_ms], "bytes_per_call": int(bytes_call),
                    "gb_per_s": round(bytes_call / ms / 1e6, 1), "gmacs_per_s": round(macs / ms / 1e6, 1),
                    "copy_ms": round(copy_ms, 5), "copy_runs": [round(t, 5) for t in copy_all],
                    "copy_bytes": 2 * rows * n * 2, "copy_gb_per_s": round(2 * rows * n * 2 / copy_ms / 1e6, 1),
                    "ratio_to_copy": round(ms / copy_ms, 3), "parity_rows": sample, "parity": "exact"})


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    bc.add_out(ap, "afsk_bench.json")
    a = ap.parse_args()
    rows = [bench(*s, a.iters) for s in SHAPES]
    bc.write_rows(a.out, iters=a.iters, rows=rows)


if __name__ == "__main__":
    main()
