"""What the down-converter bench tools (bench_{stations,channelizer,stereo,narrow,rds,spectrum,uniform,bandplan}.py) share: the repository
and tests/ on sys.path, the front-end prototype, the stations' phase increments, the two synthetic device buffers, HIP-event timing,
the common arguments, and the tail that prints every row and writes them to --out; and what the record-bank tools (bench_hdlc.py,
bench_pager.py) share beside that: the host decoder pool's library, the copy baselines and the pool's timing."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import rtl_sdr_rs_amd as fmd


def lowpass(T, cutoff):
    """Hamming-windowed sinc, cutoff in cycles per sample, peak 2047 (the front end's prototype; tests/stereo_ref.lowpass)."""
    n = np.arange(T) - (T - 1) / 2
    h = np.sinc(2 * cutoff * n) * np.hamming(T)
    return np.round(h / np.abs(h).max() * 2047).astype(np.int16)


def station_incs(K, S, fs):
    """uint32 [S, K]: K stations spread over +-1 MHz (one: +300 kHz), each stream's a few kHz off, seeded by K."""
    rng = np.random.default_rng(K)
    offs = np.linspace(-1000000, 1000000, K) if K > 1 else np.array([300000.0])
    return np.array([[fmd.phase_inc(int(o) + int(rng.integers(-5000, 5000)), fs) for o in offs] for _ in range(S)], np.uint32)


def device_buffers(S, n):
    """Two synthetic uint8 [S, n] captures on the device, the second half a buffer later, and the stream they were filled on."""
    stream = torch.cuda.current_stream().cuda_stream
    bufs = []
    for b in range(2):
        t = torch.empty((S, n), dtype=torch.uint8, device="cuda")
        fmd.synth.fill_device(t.data_ptr(), S, n, sample_offset=b * (n // 2), stream=stream)
        bufs.append(t)
    return bufs, stream


def time_calls(launch, iters, reps=3, warmup=3):
    """(median, all) of `reps` HIP-event timings of `iters` calls launch(i), in ms per call, after `warmup` calls."""
    for _ in range(warmup):
        launch(0)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            launch(i)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return sorted(ts)[len(ts) // 2], ts


def hostbench(name, argtypes):
    """tools/<name>_hostbench.so, built from its .cpp where that is newer than it: hostbench_push(*argtypes) -> seconds."""
    so, src = (os.path.join(ROOT, "tools", "%s_hostbench.%s" % (name, ext)) for ext in ("so", "cpp"))
    pkg = os.path.join(ROOT, "rtl-sdr-rs_amd")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", so, "-L", pkg, "-lfmd_hip", "-Wl,-rpath," + pkg])
    lib = ctypes.CDLL(so)
    lib.hostbench_push.restype = ctypes.c_double
    lib.hostbench_push.argtypes = argtypes
    return lib


def copy_baselines(name, soft, iters, pick=lambda rows: rows):
    """Beside a record bank over soft[period][rows][cap] on the device, (ms, runs) each: a device-to-device copy of one call's rows,
    and the copy of pick(rows) of a call to pinned host memory."""
    d_copy = torch.zeros_like(soft[0])
    copy = time_calls(lambda i: d_copy.copy_(soft[i % len(soft)]), iters)
    if not torch.equal(d_copy, soft[(iters - 1) % len(soft)]):
        raise SystemExit("%s: the copy did not copy" % name)
    h_soft = torch.empty(pick(soft[0]).shape, dtype=torch.int16, pin_memory=True)
    return copy, time_calls(lambda i: h_soft.copy_(pick(soft[i % len(soft)]), non_blocking=True), 20)


def host_push(soft, push):
    """{threads: ms} of the host decoders on 1 and 16 threads: push(p, h_rows, threads) -> seconds over call p's rows in pinned host
    memory at h_rows; a lap to warm up, then the median of 24 calls."""
    h_all = torch.empty(soft[0].shape, dtype=torch.int16, pin_memory=True)
    res = {}
    for threads in (1, 16):
        ts = []
        for i in range(1 + 3 * len(soft)):
            h_all.copy_(soft[i % len(soft)])
            torch.cuda.synchronize()
            ts.append(1e3 * push(i % len(soft), h_all.data_ptr(), threads))
        res[threads] = float(np.median(ts[1:]))
    return res


def parity_sample(S, parity_streams):
    """The seeded sample of streams a tool checks against the test-side definition."""
    return sorted(np.random.default_rng(7).choice(S, min(parity_streams, S), replace=False).tolist())


def parser():
    """The arguments every tool has: --streams, --nbytes, --iters."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--nbytes", type=int, default=fmd.DEFAULT_BUF_LENGTH)
    ap.add_argument("--iters", type=int, default=20)
    return ap


def add_out(ap, name):
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", name))


def emit(row):
    print(json.dumps(row), flush=True)
    return row


def write_rows(out, **top):
    """{"device": ..., **top} to the file `out` (empty: nowhere)."""
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), **top), f, indent=1)
            f.write("\n")
