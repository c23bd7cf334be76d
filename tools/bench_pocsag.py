#!/usr/bin/env python3
"""Time the FSK front end of the pager decoder (fmd_fsk_*) on one MI355X at the rows two banks leave behind, the code squelch's two
shapes, both at 1200 baud:

    narrow:    4096 rows x  655 samples at 12 kHz (fsk_design: D = 2, W = 5)
    bandplan: 65536 rows x 1024 samples at 24 kHz (fsk_design: D = 4, W = 5)

HIP events, the median of 3 x 200 consecutive calls after a warm-up, every call on the same device rows: the stream moves on, so
box and chunk ends fall wherever the call length puts them.  Beside it, in the same process and on the same rows: a plain contiguous
device-to-device copy of the input rows (the memory floor), and the code squelch's committed figure from profiles/dcs_bench.json
(not re-measured).  Every 64th row carries the sync word once per call; two sampled rows of the first twelve calls, one of them
such a row, are compared with tests/fsk_ref.py on the host: outputs, counts and records.  Writes profiles/pocsag_bench.json."""
import json
import os

import bench_common as bc
from bench_common import fmd, np, torch

import fsk_ref as fr

SHAPES = [("narrow", 4096, 655, 12000), ("bandplan", 65536, 1024, 24000)]
BAUD = 1200


def bench(name, rows, n, rate, iters, dcs):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    d = fmd.fsk_design(rate, BAUD)
    cfg = fr.Cfg(d.D, d.W, d.shift, d.tap, d.sync, d.tol, d.min_corr, d.hit_cap)
    # audio-like rows: noise of a level per row on a DC per row, and on every 64th row ten bits of preamble, the sync word and
    # preamble again at amplitude 4000: every call finds the word once in each of those rows
    level = torch.randint(50, 3000, (rows, 1), generator=gen, device="cuda", dtype=torch.int32)
    noise = torch.randint(-1024, 1025, (rows, n), generator=gen, device="cuda", dtype=torch.int32)
    dc = torch.randint(-2500, 2501, (rows, 1), generator=gen, device="cuda", dtype=torch.int32)
    pattern = [1, 0] * 5 + [(d.sync >> b) & 1 for b in range(31, -1, -1)] + [1, 0] * 40
    bits = torch.tensor(pattern, dtype=torch.int32, device="cuda")
    idx = torch.floor(torch.arange(n, device="cuda", dtype=torch.float64) * BAUD / rate).to(torch.int64)
    paged = (torch.arange(rows, device="cuda") % 64 == 0).to(torch.int32)[:, None]
    src = (((level * noise) >> 10) + dc + paged * 4000 * (2 * bits[idx][None, :] - 1)).clamp(-32768, 32767).to(torch.int16).contiguous()
    del noise

    def handle():
        return fmd.FskDemod(d.D, d.W, d.shift, d.tap, d.sync, d.tol, d.min_corr, d.hit_cap, n_rows=rows, device_id=0)
    dem = handle()
    cap = dem.out_cap(n)
    d_out = torch.zeros((rows, cap), dtype=torch.int16, device="cuda")

    # parity of two sampled rows over twelve calls, one of them a row with the sync word
    sample = [0, bc.parity_sample(rows, 2)[1]]
    host = src[sample].cpu().numpy()
    ref = fr.FskDemod(cfg, 2)
    hits = 0
    for _ in range(12):
        k = dem.run_device(src.data_ptr(), n, n, d_out.data_ptr(), cap, stream)
        dem.check()
        want, counts, rec = ref.run(host)
        got = d_out[sample].cpu().numpy()
        c, r = dem.hits()
        if k != want.shape[1] or not np.array_equal(got[:, :k], want) or not np.array_equal(c[sample], counts) or \
                not np.array_equal(r[sample].view(np.uint32), rec.view(np.uint32)):
            raise SystemExit("%s: rows %s differ from tests/fsk_ref.py" % (name, sample))
        hits += int(counts.sum())
    if hits < 12:
        raise SystemExit("%s: the sampled rows found no sync word" % name)
    del dem

    dem = handle()
    ms, all_ms = bc.time_calls(lambda i: dem.run_device(src.data_ptr(), n, n, d_out.data_ptr(), cap, stream), iters)
    dem.check()
    rows_hit = int((dem.hit_counts() > 0).sum())
    carried = 2 * int(d.tap[31]) + 4 * d.W + 4 + 16 * d.hit_cap
    bytes_call = 2 * rows * n + 2 * rows * (n // d.D) + 2 * rows * carried     # samples in, soft out; what is carried read and written

    d_copy = torch.zeros_like(src)
    copy_ms, copy_all = bc.time_calls(lambda i: d_copy.copy_(src), iters)
    if not torch.equal(d_copy, src):
        raise SystemExit("%s: the copy did not copy" % name)
    ks = rows * (n // d.D)
    return bc.emit({"shape": name, "rows": rows, "samples": n, "rate": rate, "baud": BAUD, "D": d.D, "W": d.W, "tap31": int(d.tap[31]),
                    "kernel": dem.kernel_name(), "ms_per_call": round(ms, 5), "ms_runs": [round(t_, 5) for t_ in all_ms],
                    "bytes_per_call": int(bytes_call), "gb_per_s": round(bytes_call / ms / 1e6, 1), "copy_ms": round(copy_ms, 5),
                    "copy_runs": [round(t_, 5) for t_ in copy_all], "copy_bytes": 4 * rows * n,
                    "copy_gb_per_s": round(4 * rows * n / copy_ms / 1e6, 1), "ratio_to_copy": round(ms / copy_ms, 3),
                    "dcs_ms_committed": dcs.get(name), "ratio_to_dcs_committed": round(ms / dcs[name], 3) if dcs.get(name) else None,
                    "words_formed_per_call": ks, "gwords_per_s": round(ks / ms / 1e6, 2), "rows_with_a_hit_in_the_last_call": rows_hit,
                    "parity_rows": sample, "parity_hits": hits, "parity": "exact"})


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    bc.add_out(ap, "pocsag_bench.json")
    a = ap.parse_args()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dcs_bench.json")) as f:
        dcs = {r["shape"]: r["ms_per_call"] for r in json.load(f)["rows"]}
    rows = [bench(*s, a.iters, dcs) for s in SHAPES]
    bc.write_rows(a.out, baud=BAUD, iters=a.iters, rows=rows)


if __name__ == "__main__":
    main()
