#!/usr/bin/env python3
"""Time the tone squelch (fmd_tonesq_*) on one MI355X at the rows two banks leave behind:

    narrow:    4096 rows x  655 samples x width 1   (the narrow-band bank's audio of one 262144 B call at K = 8, about 12 kHz)
    bandplan: 65536 rows x 1024 samples x width 1   (a 128-channel band plan over 512 streams)

F = 38 (the CTCSS table at 12 kHz), P = 4096.  HIP events, the median of 3 x 200 consecutive calls after a warm-up, every call on the
same device rows: the stream moves on, so a block ends every 6.25 (narrow) or 4 (bandplan) calls inside the timed window.  The
memory floor is measured in the same process: a plain contiguous device-to-device copy of the same input rows into the output
buffer.  The multiply-adds per second are set against the packed 16-bit dot product's issue rate -- one wave instruction per SIMD
and 2 cycles, 4 SIMDs per CU, 2 multiply-adds per lane -- at the shader clock read while the kernel runs and the CU count the
device reports.  Two sampled rows of the first twelve calls are compared with tests/tonesq_ref.py on the host.  Writes
profiles/tonesq_bench.json."""
import bench_common as bc
import bench as flagship
from bench_common import fmd, np, torch

import tonesq_ref as tr

SHAPES = [("narrow", 4096, 655, 1), ("bandplan", 65536, 1024, 1)]
RATE, P = 12000, 4096
CFG = tr.Cfg(P, 1, 3, 2, 2, 64, 20_000_000, (1 << 38) - 1)


def bench(name, rows, n, width, iters):
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    tones = torch.tensor(fmd.CTCSS_TONES, device="cuda", dtype=torch.float64)
    # audio-like rows: noise of a level per row, and on every second row one CTCSS tone of amplitude 300 ... 2000
    level = torch.randint(50, 4000, (rows, 1, 1), generator=gen, device="cuda", dtype=torch.int32)
    noise = torch.randint(-1024, 1025, (rows, n, width), generator=gen, device="cuda", dtype=torch.int32)
    hz = tones[torch.randint(0, 38, (rows,), generator=gen, device="cuda")]
    amp = torch.randint(300, 2000, (rows,), generator=gen, device="cuda").to(torch.float64) * (torch.arange(rows, device="cuda") % 2)
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    tone = (amp[:, None] * torch.cos(2 * np.pi * hz[:, None] * t[None, :] / RATE)).round().to(torch.int32)
    src = (((level * noise) >> 10) + tone[:, :, None]).clamp(-32768, 32767).to(torch.int16).contiguous()
    del noise, tone
    table = fmd.tone_table(RATE, fmd.CTCSS_TONES, P)

    def handle():
        return fmd.ToneSquelch(table, n_rows=rows, width=width, accept=CFG.accept, guard=CFG.guard, dom_shift=CFG.dom_shift,
                               min_power=CFG.min_power, confirm=CFG.confirm, hang=CFG.hang, ramp=CFG.ramp, device_id=0)
    sq = handle()
    d_out = torch.zeros((rows, n, width), dtype=torch.int16, device="cuda")

    # parity of two sampled rows over twelve calls (block ends inside)
    sample = bc.parity_sample(rows, 2)
    host = src[sample].cpu().numpy()
    ref = tr.ToneSquelch(table, CFG)
    for _ in range(12):
        k = sq.run_device(src.data_ptr(), n, n, d_out.data_ptr(), n, stream)
        sq.check()
        exp = ref.push(host)
        got = d_out[sample].cpu().numpy()
        tone_, power, gate = sq.status()
        if k != n or not np.array_equal(got, exp) or [int(tone_[r]) for r in sample] != ref.status()[0] or \
                [int(power[r]) for r in sample] != ref.status()[1] or [bool(gate[r]) for r in sample] != ref.status()[2]:
            raise SystemExit("%s: rows %s differ from tests/tonesq_ref.py" % (name, sample))
    del sq

    sq = handle()
    ms, all_ms = bc.time_calls(lambda i: sq.run_device(src.data_ptr(), n, n, d_out.data_ptr(), n, stream), iters)
    sq.check()
    open_rows = int(sq.status()[2].sum())
    eb = 2 * width
    bytes_call = 2 * rows * n * eb + 2 * rows * (2 * 38 * 8 + 32)        # samples in and out; sums and state read and written
    macs = rows * n * 2 * 38

    copy_ms, copy_all = bc.time_calls(lambda i: d_out.copy_(src), iters)
    if not torch.equal(d_out, src):
        raise SystemExit("%s: the copy did not copy" % name)
    # the shader clock while the kernel runs back to back for a second (amdgpu's sysfs, as bench.py reads it); where no sensor is
    # readable, the 2.4 GHz that MI355X_MICROARCH.md quotes
    def burst():
        for i in range(50):
            sq.run_device(src.data_ptr(), n, n, d_out.data_ptr(), n, stream)
        torch.cuda.synchronize()
    sens = flagship.GpuSensors(torch, 0)
    sclk = sorted(sens.sample_while(burst, 1.0)[0]) if sens.dir else []
    clock_ghz, clock_source = (sclk[len(sclk) // 2] / 1e3, "pp_dpm_sclk, median while the kernel ran") if sclk else (2.4, "assumed: no sensor readable")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    peak = cus * 4 * 32 * 2 * clock_ghz * 1e9               # multiply-adds per second at the dot product's issue rate
    return bc.emit({"shape": name, "rows": rows, "samples": n, "width": width, "block": P, "tones": 38, "kernel": sq.kernel_name(),
                    "ms_per_call": round(ms, 5), "ms_runs": [round(t_, 5) for t_ in all_ms], "bytes_per_call": int(bytes_call),
                    "gb_per_s": round(bytes_call / ms / 1e6, 1), "copy_ms": round(copy_ms, 5), "copy_runs": [round(t_, 5) for t_ in copy_all],
                    "copy_bytes": 2 * rows * n * eb, "copy_gb_per_s": round(2 * rows * n * eb / copy_ms / 1e6, 1),
                    "ratio_to_copy": round(ms / copy_ms, 3), "macs_per_call": macs, "tmacs_per_s": round(macs / ms / 1e9, 2),
                    "clock_ghz": clock_ghz, "clock_source": clock_source, "cus": cus, "dot2_peak_tmacs_per_s": round(peak / 1e12, 1),
                    "fraction_of_dot2_peak": round(macs / (ms * 1e-3) / peak, 3), "rows_open_at_end": open_rows,
                    "parity_rows": sample, "parity": "exact"})


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    bc.add_out(ap, "tonesq_bench.json")
    a = ap.parse_args()
    rows = [bench(*s, a.iters) for s in SHAPES]
    bc.write_rows(a.out, config=CFG._asdict(), rate=RATE, iters=a.iters, rows=rows)


if __name__ == "__main__":
    main()
