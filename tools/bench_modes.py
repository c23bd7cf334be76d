#!/usr/bin/env python3
"""Time the Mode S bank (fmd_modes_*) on one MI355X at two shapes, 4096 and 512 streams x 262144 bytes (131072 samples of 2 Msample/s
u8 IQ per stream and call), each over an empty band -- Gaussian noise of sigma 12 LSB, where about 0.27 % of the positions pass the
preamble rule and none decodes -- and over a busy one: the same noise with about 100 extended squitters per buffer and stream, every
fourth with one bit damaged (fix_errors is on).  HIP events, the median of 3 x --iters consecutive calls on the same device buffer
after a warm-up; beside it, in the same process, a plain device-to-device copy of the same bytes.  Two sampled streams of every run are
compared with tests/modes_ref.py: counts, records and counters.  Writes profiles/modes_bench.json."""
import bench_common as bc
from bench_common import fmd, np, torch

import modes_cases as mc
import modes_ref

SHAPES = [("4096", 4096), ("512", 512)]
NBYTES, MSG_CAP, PER_BUFFER = 262144, 128, 100


def band(S, busy):
    """uint8 [S, NBYTES] on the device: seeded noise; `busy`: PER_BUFFER messages per stream, at places that differ between streams"""
    g = torch.Generator(device="cuda").manual_seed(S + busy)
    iq = torch.empty((S, NBYTES), dtype=torch.uint8, device="cuda")
    for lo in range(0, S, 256):                              # (in pieces: the float noise of all streams at once would be 4 GiB)
        hi = min(S, lo + 256)
        iq[lo:hi] = torch.normal(127.5, 12.0, (hi - lo, NBYTES), generator=g, device="cuda").round_().clamp_(0, 255).to(torch.uint8)
    if busy:
        msgs = [mc.LONG[k % 4] if k % 4 else mc.flip(mc.LONG[(k // 4) % 4], 5 + (7 * k) % 107) for k in range(PER_BUFFER)]
        enc = torch.from_numpy(np.stack([fmd.modes_encode(m, 60) for m in msgs])).cuda()
        step = (NBYTES // 2 - 600) // PER_BUFFER             # >= 1300 samples between two messages
        for grp in range(8):                                 # the streams s = grp mod 8 share their places
            for k in range(PER_BUFFER):
                p = 100 + 37 * grp + k * step + (11 * k * (grp + 1)) % 400
                iq[grp::8, 2 * p:2 * p + enc.shape[1]] = enc[k]
    return iq


def bench(name, S, busy, iters):
    stream = torch.cuda.current_stream().cuda_stream
    iq = band(S, busy)
    torch.cuda.synchronize()

    def handle():
        return fmd.ModeSBank(S, min_power=0, fix_errors=True, df11=False, msg_cap=MSG_CAP, device_id=0)

    # parity of two sampled streams over two calls
    sample = bc.parity_sample(S, 2)
    h_iq = iq[sample].cpu().numpy()
    cfg = mc.cfg(fix_errors=1, msg_cap=MSG_CAP)
    per_call, info = modes_ref.run_bank(cfg, [h_iq, h_iq], len(sample))
    bank = handle()
    found = 0
    for call in range(2):
        bank.run_device(iq.data_ptr(), NBYTES, NBYTES, stream)
        bank.check()
        counts, recs = per_call[call]
        if bank.counts()[sample].tolist() != counts or bank.messages(sample) != recs:
            raise SystemExit("%s: streams %s differ from tests/modes_ref.py in call %d" % (name, sample, call))
        found += sum(counts)
    got = bank.info()
    if [got[s] for s in sample] != info:
        raise SystemExit("%s: the counters of streams %s differ from tests/modes_ref.py" % (name, sample))
    if busy and found < PER_BUFFER:
        raise SystemExit("%s: the sampled streams delivered too few messages" % name)
    del bank

    bank = handle()
    ms, all_ms = bc.time_calls(lambda i: bank.run_device(iq.data_ptr(), NBYTES, NBYTES, stream), iters)
    bank.check()
    tot = bank.info()
    calls = 3 + 3 * iters
    d_copy = torch.empty_like(iq)
    copy_ms, copy_all = bc.time_calls(lambda i: d_copy.copy_(iq), iters)
    if not torch.equal(d_copy, iq):
        raise SystemExit("%s: the copy did not copy" % name)
    return bc.emit({"shape": name, "band": "busy" if busy else "empty", "streams": S, "nbytes": NBYTES, "msg_cap": MSG_CAP, "tile": fmd.modes_tile(),
                    "kernels": [bank.kernel_name(0), bank.kernel_name(1)], "ms_per_call": round(ms, 5), "ms_runs": [round(t, 5) for t in all_ms],
                    "gsamples_per_s": round(S * (NBYTES // 2) / ms / 1e6, 2), "copy_ms": round(copy_ms, 5),
                    "copy_runs": [round(t, 5) for t in copy_all], "copy_bytes": S * NBYTES, "ratio_to_copy": round(ms / copy_ms, 3),
                    "timed_calls": calls, "candidates_per_call": round(sum(t["candidates"] for t in tot) / calls, 1),
                    "messages_per_call": round(sum(t["messages"] for t in tot) / calls, 1), "fixed_per_call": round(sum(t["fixed"] for t in tot) / calls, 1),
                    "parity_streams": sample, "parity_messages": found, "parity": "exact"})


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    bc.add_out(ap, "modes_bench.json")
    a = ap.parse_args()
    rows = [bench(name, S, busy, a.iters) for name, S in SHAPES for busy in (0, 1)]
    bc.write_rows(a.out, iters=a.iters, rows=rows)


if __name__ == "__main__":
    main()
