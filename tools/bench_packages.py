#!/usr/bin/env python3
"""Time the package bank (fmd_packages_*) on one MI355X behind the pulse bank at two shapes, 512 and 4096 streams x 262144 bytes of
tools/bench_pulses.py's OOK traffic (W = 8, thresholds well apart), with pulse_cap 512 -- the traffic gives about 300 pulses per stream
and call, and the tool stops if a stream overflows -- and a PWM slicer whose windows take most of the traffic's widths and whose reset
closes a package on the longer gaps.  HIP events, the median of 3 x --iters consecutive calls after a warm-up.  In one process:

    (a) fmd_packages_run_bank alone, on results that lie on the device;
    (b) the pulse bank and the package bank chained on one stream, beside the pulse bank alone;
    (c) the best host path: one copy of as many bytes as the counts, the records of all streams and the totals to pinned host memory,
        then an fmd_pulse_slicer per stream on sixteen threads (tools/packages_hostbench.cpp, timed without the interpreter);
    (d) a plain device-to-device copy of the records region.

Two sampled streams of every run are compared with tests/packages_ref.py over two calls: counts, packages and totals.  Writes
profiles/packages_bench.json."""
import ctypes as C

import bench_common as bc
import bench_pulses
from bench_common import fmd, np, torch

import packages_ref

SHAPES = [("512", 512), ("4096", 4096)]
NBYTES, W, PULSE_CAP = bench_pulses.NBYTES, bench_pulses.W, 512
LO, HI = bench_pulses.TRAFFIC
SLICER = {"modulation": "pwm", "short": 100, "long": 300, "tol": 100, "reset": 350}      # widths and gaps are 40 ... 400 samples
PUSH_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint, C.POINTER(C.c_uint64)]


def banks(S):
    pulses = fmd.PulseBank(S, W, LO, HI, PULSE_CAP, device_id=0)
    return pulses, fmd.sliced(pulses, min_bits=0, device_id=0, **SLICER)


def bench(name, S, iters, host):
    stream = torch.cuda.current_stream().cuda_stream
    iq = bench_pulses.band(S, 0)
    torch.cuda.synchronize()
    n_samples = NBYTES // 2

    # parity of two sampled streams over two calls, and the shape's premise: no stream overflows
    sample = bc.parity_sample(S, 2)
    pulses, pk = banks(S)
    ref = packages_ref.Bank(len(sample), packages_ref.PWM, SLICER["short"], SLICER["long"], SLICER["tol"], SLICER["reset"], 0, pk.pkg_cap)
    found = 0
    for call in range(2):
        pulses.run_device(iq.data_ptr(), NBYTES, NBYTES, stream)
        pk.run_bank(pulses, stream)
        pk.check()
        counts = pulses.counts()
        if counts.max() > PULSE_CAP:
            raise SystemExit("%s: a stream has %d pulses in a call: pulse_cap %d overflows" % (name, counts.max(), PULSE_CAP))
        info = pulses.info()
        want_n, want = ref.run(counts[sample], pulses.pulses(sample), PULSE_CAP, [info[s] for s in sample], n_samples)
        got = pk.info()
        if pk.counts()[sample].tolist() != want_n or pk.packages(sample) != want or [got[s] for s in sample] != ref.info:
            raise SystemExit("%s: streams %s differ from tests/packages_ref.py in call %d" % (name, sample, call))
        found += sum(want_n)
    if found < 10:
        raise SystemExit("%s: the sampled streams delivered too few packages" % name)

    # what the host path works on: the second call's results, fetched once
    h_counts = pulses.counts()
    h_recs = np.zeros((S, PULSE_CAP, 4), np.uint32)
    every = np.arange(S, dtype=np.uint32)
    fmd.check(fmd.lib().fmd_pulses_recs(pulses._h, every.ctypes.data, S, h_recs.ctypes.data))
    h_tot = (fmd.pulses.PulsesTotals * S)()
    fmd.check(fmd.lib().fmd_pulses_info(pulses._h, h_tot))

    # (a) run_bank alone on what lies on the device
    a_ms, a_all = bc.time_calls(lambda i: pk.run_bank(pulses, stream), iters)
    pk.check()
    per_call = int(pk.counts().sum())
    del pk, pulses

    # (b) chained, beside the pulse bank alone
    pulses, pk = banks(S)

    def chained(i):
        pulses.run_device(iq.data_ptr(), NBYTES, NBYTES, stream)
        pk.run_bank(pulses, stream)
    b_ms, b_all = bc.time_calls(chained, iters)
    pk.check()
    tot = pk.info()
    del pk, pulses
    pulses = fmd.PulseBank(S, W, LO, HI, PULSE_CAP, device_id=0)
    p_ms, p_all = bc.time_calls(lambda i: pulses.run_device(iq.data_ptr(), NBYTES, NBYTES, stream), iters)
    pulses.check()
    del pulses

    # (c) the host path: the bytes back in one copy, then the slicers on 16 threads
    back_bytes = 4 * S + 16 * S * PULSE_CAP + 48 * S           # counts, records, the bank's state of 12 dwords per stream
    d_res = torch.zeros(back_bytes, dtype=torch.uint8, device="cuda")
    h_res = torch.empty(back_bytes, dtype=torch.uint8, pin_memory=True)
    d2h_ms, d2h_all = bc.time_calls(lambda i: h_res.copy_(d_res, non_blocking=True), iters)
    slicers = (C.c_void_p * S)()
    for s in range(S):
        h = C.c_void_p()
        cfg = fmd.pulses.PulseSlicerConfig(0, SLICER["short"], SLICER["long"], SLICER["tol"], SLICER["reset"])
        fmd.check(fmd.lib().fmd_pulse_slicer_new(C.byref(cfg), C.byref(h)))
        slicers[s] = h
    got, push = C.c_uint64(0), {}
    for threads in (1, 16):
        ts = [1e3 * host.hostbench_push(slicers, h_counts.ctypes.data, h_recs.ctypes.data, PULSE_CAP, h_tot, n_samples, S, threads, C.byref(got))
              for _ in range(8)]
        push[threads] = float(np.median(ts[1:]))
    for s in range(S):
        fmd.lib().fmd_pulse_slicer_free(C.c_void_p(slicers[s]))

    # (d) a device copy of the records region
    d_rec = torch.zeros(16 * S * PULSE_CAP, dtype=torch.uint8, device="cuda")
    d_dst = torch.empty_like(d_rec)
    c_ms, c_all = bc.time_calls(lambda i: d_dst.copy_(d_rec), iters)
    r5 = lambda ts: [round(t, 5) for t in ts]
    calls = 3 + 3 * iters
    return bc.emit({"shape": name, "streams": S, "nbytes": NBYTES, "W": W, "lo": LO, "hi": HI, "pulse_cap": PULSE_CAP, "slicer": SLICER,
                    "pkg_cap": PULSE_CAP + 1, "kernel": "fmd_pk::fmd_packages_kernel",
                    "pulses_per_call_and_stream": round(float(h_counts.mean()), 1), "pulses_max": int(h_counts.max()),
                    "packages_per_call_all_streams": per_call,
                    "a_run_bank_ms": round(a_ms, 5), "a_runs": r5(a_all),
                    "b_chained_ms": round(b_ms, 5), "b_runs": r5(b_all), "b_pulses_alone_ms": round(p_ms, 5), "b_pulses_alone_runs": r5(p_all),
                    "b_added_ms": round(b_ms - p_ms, 5), "ratio_chained_to_pulses": round(b_ms / p_ms, 3),
                    "c_d2h_ms": round(d2h_ms, 5), "c_d2h_runs": r5(d2h_all), "c_d2h_bytes": back_bytes,
                    "c_host_slicers_ms_1_thread": round(push[1], 4), "c_host_slicers_ms_16_threads": round(push[16], 4),
                    "c_host_path_ms": round(d2h_ms + push[16], 4), "ratio_host_path_to_run_bank": round((d2h_ms + push[16]) / a_ms, 1),
                    "c_host_packages_per_call": int(got.value),
                    "d_copy_ms": round(c_ms, 5), "d_copy_runs": r5(c_all), "d_copy_bytes": 16 * S * PULSE_CAP, "ratio_run_bank_to_copy": round(a_ms / c_ms, 3),
                    "timed_calls": calls, "packages_all_streams": int(sum(t["packages"] for t in tot)), "bad_all_streams": int(sum(t["bad"] for t in tot)),
                    "parity_streams": sample, "parity_packages": found, "parity": "exact"})


def main():
    ap = bc.argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    bc.add_out(ap, "packages_bench.json")
    a = ap.parse_args()
    host = bc.hostbench("packages", PUSH_ARGS)
    rows = [bench(name, S, a.iters, host) for name, S in SHAPES]
    bc.write_rows(a.out, iters=a.iters, rows=rows)


if __name__ == "__main__":
    main()
