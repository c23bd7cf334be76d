#!/usr/bin/env python3
"""Time the automatic gain control (fmd_agc_*) on one MI355X at the rows two banks leave behind at 512 streams x 8 stations:

    stereo:  4096 rows x 2621 samples x width 2   (the stereo bank's audio of one 262144 B call at K = 8)
    narrow:  4096 rows x  655 samples x width 1   (the narrow-band bank's)

P = 256.  HIP events, the median of 3 x 200 calls after a warm-up, every call on the same device rows (the state moves on, the work
per call does not change).  The memory floor is measured in the same process: a plain contiguous device-to-device copy of the same
input rows into the output buffer (`dst.copy_(src)`; no gather, no index arithmetic).  Two sampled rows of the first three calls are
compared with tests/agc_ref.py on the host.  Writes profiles/agc_bench.json."""
import bench_common as bc
from bench_common import fmd, np, torch

import agc_ref as ar

SHAPES = [("stereo", 4096, 2621, 2), ("narrow", 4096, 655, 1)]
CFG = ar.Cfg(256, 12000, 65536, 4, 32)


def bench(name, rows, n, width, iters):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    # audio-like rows: a level per row (3 ... 24000) times noise, so that rows sit at different gains
    level = torch.randint(3, 24000, (rows, 1, 1), generator=gen, device="cuda", dtype=torch.int32)
    noise = torch.randint(-1024, 1025, (rows, n, width), generator=gen, device="cuda", dtype=torch.int32)
    src = ((level * noise) >> 10).to(torch.int16).contiguous()
    host = src.cpu().numpy()

    def handle():
        return fmd.Agc(n_rows=rows, width=width, target=CFG.target, block=CFG.block, hang=CFG.hang, decay=CFG.decay, gain_max=CFG.gain_max,
                       device_id=0)
    ag = handle()
    cap = ag.out_cap(n)
    d_out = torch.zeros((rows, cap, width), dtype=torch.int16, device="cuda")

    # parity of two sampled rows over three calls
    sample = bc.parity_sample(rows, 2)
    ref = ar.Agc(CFG)
    for _ in range(3):
        k = ag.run_device(src.data_ptr(), n, n, d_out.data_ptr(), cap, stream)
        ag.check()
        exp = ref.push(host[sample])
        got = d_out.cpu().numpy()[sample, :k]
        if k != exp.shape[1] or not np.array_equal(got, exp):
            raise SystemExit("%s: rows %s differ from tests/agc_ref.py" % (name, sample))
    del ag

    ag = handle()
    in0, out0 = ag.counts()
    ms, all_ms = bc.time_calls(lambda i: ag.run_device(src.data_ptr(), n, n, d_out.data_ptr(), cap, stream), iters)
    ag.check()
    in1, out1 = ag.counts()
    calls = (in1 - in0) // n
    eb = 2 * width
    bytes_call = rows * eb * (n + (out1 - out0) / calls)     # input once, the call's outputs once (history and state not counted)

    dst = d_out.view(-1)[:src.numel()].view_as(src)
    copy_ms, copy_all = bc.time_calls(lambda i: dst.copy_(src), iters)
    if not torch.equal(dst, src):
        raise SystemExit("%s: the copy did not copy" % name)
    return bc.emit({"shape": name, "rows": rows, "samples": n, "width": width, "block": CFG.block, "kernel": ag.kernel_name(),
                    "ms_per_call": round(ms, 5), "ms_runs": [round(t, 5) for t in all_ms], "bytes_per_call": int(bytes_call),
                    "gb_per_s": round(bytes_call / ms / 1e6, 1), "copy_ms": round(copy_ms, 5), "copy_runs": [round(t, 5) for t in copy_all],
                    "copy_bytes": 2 * rows * n * eb, "copy_gb_per_s": round(2 * rows * n * eb / copy_ms / 1e6, 1),
                    "ratio_to_copy": round(ms / copy_ms, 3), "parity_rows": sample, "parity": "exact"})


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    bc.add_out(ap, "agc_bench.json")
    a = ap.parse_args()
    rows = [bench(*s, a.iters) for s in SHAPES]
    bc.write_rows(a.out, config=CFG._asdict(), iters=a.iters, rows=rows)


if __name__ == "__main__":
    main()
