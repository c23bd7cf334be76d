#!/usr/bin/env python3
"""Time the pulse bank (fmd_pulses_*) on one MI355X at two shapes, 4096 and 512 streams x 262144 bytes (131072 samples of u8 IQ per
stream and call), W = 8 and pulse_cap 64, each over OOK traffic -- Gaussian noise of sigma 6 LSB with strong pulses and gaps of 40 ...
400 samples, thresholds well apart -- and over the worst case: noise of sigma 12 with lo == hi at its median box, an edge on about
every fourth sample.  HIP events, the median of 3 x --iters consecutive calls on the same device buffer after a warm-up; beside it, in
the same process, a plain device-to-device copy of the same bytes and a Mode S bank call on the same buffer (the nearest kernel of the
same input).  Two sampled streams of every run are compared with tests/pulses_ref.py: counts, records and totals.  Writes
profiles/pulses_bench.json."""
import bench_common as bc
from bench_common import fmd, np, torch

import pulses_ref

SHAPES = [("4096", 4096), ("512", 512)]
NBYTES, W, PULSE_CAP = 262144, 8, 64
TRAFFIC = (10000, 30000)                                     # lo, hi of the traffic run


def band(S, worst):
    """uint8 [S, NBYTES] on the device: seeded noise; traffic: a carrier keyed on and off, at places that differ between streams"""
    g = torch.Generator(device="cuda").manual_seed(S + worst)
    n = NBYTES // 2
    iq = torch.empty((S, NBYTES), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(S)
    envs = []
    for k in range(8):                                       # the streams s = k mod 8 share their keying
        env, p = np.zeros(n, np.float32), 0
        while p < n:
            gap, width = int(rng.integers(40, 400)), int(rng.integers(40, 400))
            env[p + gap:p + gap + width] = 60.0
            p += gap + width
        envs.append(torch.from_numpy(np.repeat(env, 2)).cuda())
    for lo in range(0, S, 256):                              # (in pieces: the float noise of all streams at once would be 4 GiB)
        hi = min(S, lo + 256)
        x = torch.normal(127.5, 12.0 if worst else 6.0, (hi - lo, NBYTES), generator=g, device="cuda")
        if not worst:
            for k in range(8):
                x[(k - lo) % 8::8] += envs[k]                # (I and Q alike: m = 4 * 60^2 on a pulse)
        iq[lo:hi] = x.round_().clamp_(0, 255).to(torch.uint8)
    return iq


def worst_level(iq):
    """lo == hi: the median box of the first stream"""
    b = iq[0].cpu().numpy()
    e = pulses_ref.Stream(W, 1, 1).box(b)[0][W:]
    return int(np.median(e))


def bench(name, S, worst, iters):
    stream = torch.cuda.current_stream().cuda_stream
    iq = band(S, worst)
    torch.cuda.synchronize()
    lo, hi = (worst_level(iq),) * 2 if worst else TRAFFIC

    def handle():
        return fmd.PulseBank(S, W, lo, hi, PULSE_CAP, device_id=0)

    # parity of two sampled streams over two calls
    sample = bc.parity_sample(S, 2)
    h_iq = iq[sample].cpu().numpy()
    per_call, info = pulses_ref.run_bank({"W": W, "lo": lo, "hi": hi, "pulse_cap": PULSE_CAP}, [h_iq, h_iq], len(sample))
    bank = handle()
    found = 0
    for call in range(2):
        bank.run_device(iq.data_ptr(), NBYTES, NBYTES, stream)
        bank.check()
        counts, recs = per_call[call]
        if bank.counts()[sample].tolist() != counts or bank.pulses(sample) != recs:
            raise SystemExit("%s: streams %s differ from tests/pulses_ref.py in call %d" % (name, sample, call))
        found += sum(counts)
    got = bank.info()
    if [got[s] for s in sample] != info:
        raise SystemExit("%s: the totals of streams %s differ from tests/pulses_ref.py" % (name, sample))
    if found < 100:
        raise SystemExit("%s: the sampled streams delivered too few pulses" % name)
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
    del d_copy
    modes = fmd.ModeSBank(S, min_power=0, fix_errors=True, df11=False, msg_cap=32, device_id=0)
    modes_ms, modes_all = bc.time_calls(lambda i: modes.run_device(iq.data_ptr(), NBYTES, NBYTES, stream), iters)
    modes.check()
    return bc.emit({"shape": name, "band": "worst" if worst else "traffic", "streams": S, "nbytes": NBYTES, "W": W, "lo": lo, "hi": hi,
                    "pulse_cap": PULSE_CAP, "tile": fmd.pulses_tile(), "kernels": [bank.kernel_name(0), bank.kernel_name(1)],
                    "ms_per_call": round(ms, 5), "ms_runs": [round(t, 5) for t in all_ms],
                    "gsamples_per_s": round(S * (NBYTES // 2) / ms / 1e6, 2), "copy_ms": round(copy_ms, 5),
                    "copy_runs": [round(t, 5) for t in copy_all], "copy_bytes": S * NBYTES, "ratio_to_copy": round(ms / copy_ms, 3),
                    "modes_ms": round(modes_ms, 5), "modes_runs": [round(t, 5) for t in modes_all], "ratio_to_modes": round(ms / modes_ms, 3),
                    "timed_calls": calls, "pulses_per_call_and_stream": round(sum(t["pulses"] for t in tot) / calls / S, 1),
                    "parity_streams": sample, "parity_pulses": found, "parity": "exact"})


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    bc.add_out(ap, "pulses_bench.json")
    a = ap.parse_args()
    rows = [bench(name, S, worst, a.iters) for name, S in SHAPES for worst in (0, 1)]
    bc.write_rows(a.out, iters=a.iters, rows=rows)


if __name__ == "__main__":
    main()
