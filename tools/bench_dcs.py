#!/usr/bin/env python3
"""Time the code squelch (fmd_dcs_*) on one MI355X at the rows two banks leave behind, the tone squelch's two shapes:

    narrow:    4096 rows x  655 samples x width 1 at 12 kHz (dcs_design: B = 8,  P = 4160)
    bandplan: 65536 rows x 1024 samples x width 1 at 24 kHz (dcs_design: B = 16, P = 8256)

F = 104 (every standard DCS word).  HIP events, the median of 3 x 200 consecutive calls after a warm-up, every call on the same
device rows: the stream moves on, so block ends fall inside the timed window.  Beside it, in the same process and on the same rows:
a plain contiguous device-to-device copy of the input rows into the output buffer (the memory floor), and the tone squelch's call (38
tones, P = 4096).  Two sampled rows of the first twelve calls are compared with tests/dcs_ref.py on the host.  Writes
profiles/dcs_bench.json."""
import bench_common as bc
from bench_common import fmd, np, torch

import dcs_ref as dr

SHAPES = [("narrow", 4096, 655, 1, 12000), ("bandplan", 65536, 1024, 1, 24000)]
WORDS = [fmd.dcs_word(c) for c in fmd.DCS_CODES]


def bench(name, rows, n, width, rate, iters):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    d = fmd.dcs_design(rate)
    cfg = dr.Cfg(d.block, d.box, d.lp, d.lshift, d.tap, d.tol, d.min_hits, d.confirm, d.hang, d.ramp, (1 << 104) - 1)
    # audio-like rows: noise of a level per row, and on every second row one DCS code NRZ at amplitude 300 ... 2000
    level = torch.randint(50, 4000, (rows, 1, 1), generator=gen, device="cuda", dtype=torch.int32)
    noise = torch.randint(-1024, 1025, (rows, n, width), generator=gen, device="cuda", dtype=torch.int32)
    cw = torch.tensor([fmd.dcs_codeword(c) for c in fmd.DCS_CODES], device="cuda", dtype=torch.int64)
    cw = cw[torch.randint(0, 104, (rows,), generator=gen, device="cuda")]
    amp = torch.randint(300, 2000, (rows,), generator=gen, device="cuda").to(torch.int32) * (torch.arange(rows, device="cuda") % 2).to(torch.int32)
    bit = torch.floor(torch.arange(n, device="cuda", dtype=torch.float64) * 134.4 / rate).to(torch.int64) % 23
    code = (((cw[:, None] >> bit[None, :]) & 1) * 2 - 1).to(torch.int32) * amp[:, None]
    src = (((level * noise) >> 10) + code[:, :, None]).clamp(-32768, 32767).to(torch.int16).contiguous()
    del noise, code

    def handle():
        return fmd.CodeSquelch(WORDS, d.block, d.box, d.lp, d.lshift, d.tap, n_rows=rows, width=width, accept=cfg.accept, tol=d.tol,
                               min_hits=d.min_hits, confirm=d.confirm, hang=d.hang, ramp=d.ramp, device_id=0)
    sq = handle()
    d_out = torch.zeros((rows, n, width), dtype=torch.int16, device="cuda")

    # parity of two sampled rows over twelve calls (block ends inside)
    sample = bc.parity_sample(rows, 2)
    host = src[sample].cpu().numpy()
    ref = dr.CodeSquelch(WORDS, cfg)
    for _ in range(12):
        k = sq.run_device(src.data_ptr(), n, n, d_out.data_ptr(), n, stream)
        sq.check()
        exp = ref.push(host)
        got = d_out[sample].cpu().numpy()
        code_, hits, gate = sq.status()
        if k != n or not np.array_equal(got, exp) or [int(code_[r]) for r in sample] != ref.status()[0] or \
                [int(hits[r]) for r in sample] != ref.status()[1] or [bool(gate[r]) for r in sample] != ref.status()[2]:
            raise SystemExit("%s: rows %s differ from tests/dcs_ref.py" % (name, sample))
    del sq

    sq = handle()
    ms, all_ms = bc.time_calls(lambda i: sq.run_device(src.data_ptr(), n, n, d_out.data_ptr(), n, stream), iters)
    sq.check()
    open_rows = int(sq.status()[2].sum())
    eb = 2 * width
    carried = 2 * (int(d.tap[22]) + len(d.lp) - 1) + 4 * 104 + 32
    bytes_call = 2 * rows * n * eb + 2 * rows * carried      # samples in and out; rings, counters and state read and written

    copy_ms, copy_all = bc.time_calls(lambda i: d_out.copy_(src), iters)
    if not torch.equal(d_out, src):
        raise SystemExit("%s: the copy did not copy" % name)
    tq = fmd.ToneSquelch(fmd.tone_table(rate, fmd.CTCSS_TONES, 4096), n_rows=rows, width=width, device_id=0)
    tq_ms, tq_all = bc.time_calls(lambda i: tq.run_device(src.data_ptr(), n, n, d_out.data_ptr(), n, stream), iters)
    tq.check()
    ks = rows * (n // d.box)
    return bc.emit({"shape": name, "rows": rows, "samples": n, "width": width, "rate": rate, "block": d.block, "box": d.box, "words": 104,
                    "kernel": sq.kernel_name(), "ms_per_call": round(ms, 5), "ms_runs": [round(t_, 5) for t_ in all_ms],
                    "bytes_per_call": int(bytes_call), "gb_per_s": round(bytes_call / ms / 1e6, 1), "copy_ms": round(copy_ms, 5),
                    "copy_runs": [round(t_, 5) for t_ in copy_all], "copy_bytes": 2 * rows * n * eb,
                    "copy_gb_per_s": round(2 * rows * n * eb / copy_ms / 1e6, 1), "ratio_to_copy": round(ms / copy_ms, 3),
                    "tonesq_ms": round(tq_ms, 5), "tonesq_runs": [round(t_, 5) for t_ in tq_all], "ratio_to_tonesq": round(ms / tq_ms, 3),
                    "words_formed_per_call": ks, "gcompares_per_s": round(ks * 104 / ms / 1e6, 2), "rows_open_at_end": open_rows,
                    "parity_rows": sample, "parity": "exact"})


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    bc.add_out(ap, "dcs_bench.json")
    a = ap.parse_args()
    rows = [bench(*s, a.iters) for s in SHAPES]
    bc.write_rows(a.out, words=104, iters=a.iters, rows=rows)


if __name__ == "__main__":
    main()
