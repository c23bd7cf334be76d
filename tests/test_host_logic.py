"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol include/fmd.h
declares, status codes / helpers that need no GPU behave, the product fails loudly without a device,
the synthetic source is deterministic, and channel sharding over ranks (world_size 2, gloo) reassembles
exactly -- the N > 1 path of bench.py without GPUs."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "fmd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fmd_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(fmd):
    lib = fmd.lib()
    names = header_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), "libfmd_hip.so does not export %s" % n
    # the ctypes binding lists exactly the header's functions
    from rtl_sdr_rs_amd import _ffi
    assert sorted(_ffi.PROTOTYPES) == names


def test_no_oracle_in_product():
    """The shipped path must not reference oracle/ (SURVEY/prompt rule): grep the package sources."""
    pkg = os.path.join(ROOT, "rtl-sdr-rs_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".hpp")) or f == "Makefile":
                txt = open(os.path.join(dp, f), errors="ignore").read()
                for line in txt.split("\n"):
                    code = line.split("//")[0].split("#")[0] if not f.endswith(".py") else line.split("#")[0]
                    assert "fm_oracle" not in code and "oracle_lib" not in code and "libfm_oracle" not in code, (f, line)


def test_optimal_settings_and_out_cap_without_gpu(fmd):
    r, d = fmd.optimal_settings(94_900_000, 170_000)           # simple_fm.rs:48
    assert (d.downsample, d.rate_in, d.rate_out, d.rate_resample, d.output_scale) == (6, 170000, 170000, 32000, 42)
    assert (r.capture_rate, r.capture_freq) == (1_020_000, 95_155_000)
    with pytest.raises(fmd.FmdError) as ei:
        fmd.optimal_settings(1, 0)
    assert ei.value.status == -4
    cap = fmd.out_cap(d, fmd.DEFAULT_BUF_LENGTH)
    assert 4113 <= cap <= 4120                                  # 4112/4113 samples per reference block
    assert fmd.lib().fmd_strerror(-2).decode().startswith("buffer length")
    assert fmd.lib().fmd_version() == 3                      # FMD_VERSION_MAJOR * 1000 + FMD_VERSION_MINOR


def test_fails_loudly_without_device(fmd):
    if fmd.device_count() > 0:
        pytest.skip("a GPU is present")
    _, d = fmd.optimal_settings(94_900_000, 170_000)
    with pytest.raises(fmd.FmdError) as ei:
        fmd.Demod(d)
    assert ei.value.status == -8                                # FMD_ERR_NO_DEVICE: there is no CPU fallback
    cli = os.path.join(ROOT, "rtl-sdr-rs_amd", "simple_fm_gpu")
    if os.path.exists(cli):
        p = subprocess.run([cli, os.devnull], capture_output=True)
        assert p.returncode == 1 and b"no usable gfx950 device" in p.stderr


def test_fir_handles_refuse_their_domain_before_the_device(fmd):
    """Without a gfx950 the two FIR handles answer as every bank does: whatever their domain excludes is FMD_ERR_UNSUPPORTED, and
    only arguments they would accept reach the device check."""
    import numpy as np
    if fmd.device_count() > 0:
        pytest.skip("a GPU is present")
    UNSUPPORTED, NO_DEVICE = -6, -8
    ones = np.ones(8, np.int16)

    def status(make):
        with pytest.raises(fmd.FmdError) as ei:
            make()
        return ei.value.status, str(ei.value)

    assert status(lambda: fmd.FirBank(ones, 8))[0] == NO_DEVICE
    assert status(lambda: fmd.FirBank(ones, 3))[0] == UNSUPPORTED                       # odd decimation
    assert status(lambda: fmd.FirDemodBank(ones, 8, 2500000, 48000))[0] == NO_DEVICE
    assert status(lambda: fmd.FirDemodBank(np.ones(1024, np.int16), 64, 37500, 8000))[0] == NO_DEVICE   # (1024 taps at decimation 64 fit)
    for fast, text in ((48000 * 600, "rate ratio outside the exact-small-divide range"), (48000 * 500, "one audio sample does not fit a tile")):
        for taps in (ones, np.ones(1024, np.int16)):
            st, err = status(lambda: fmd.FirDemodBank(taps, 64, fast, 48000))
            assert st == UNSUPPORTED and text in err, (fast, taps.size, err)


def test_missing_library_is_an_error_not_a_fallback():
    """Without the built HIP library the package must raise, never compute on the CPU."""
    code = "import rtl_sdr_rs_amd as f\ntry:\n    f.lib()\nexcept ImportError as e:\n    print('IMPORTERROR', e)\n"
    env = dict(os.environ, FMD_LIB="/nonexistent/libfmd_hip.so", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, env=env, timeout=120)
    assert p.returncode == 0 and b"IMPORTERROR" in p.stdout and b"no CPU fallback" in p.stdout.replace(b"There is ", b"")


def test_shipped_library_reads_no_environment():
    """Tuning / test knobs (kernel variants, the f64 guard band, ablation bits) live in the -DFMD_EXPERIMENT build
    only: the shipped library must not even import getenv, and the sources may call it in one guarded place."""
    so = os.path.join(ROOT, "rtl-sdr-rs_amd", "libfmd_hip.so")
    syms = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, check=True).stdout.decode()
    assert "getenv" not in syms
    csrc = os.path.join(ROOT, "rtl-sdr-rs_amd", "csrc")
    hits = []
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".cpp", ".h", ".hpp")):
            for i, line in enumerate(open(os.path.join(csrc, f)), 1):
                if "getenv(" in line and not line.lstrip().startswith("//"):
                    hits.append((f, i))
    assert [h[0] for h in hits] == ["fmd_host.h"], hits          # fmd_knob(), inside #ifdef FMD_EXPERIMENT
    host = open(os.path.join(csrc, "fmd_host.h")).read()
    assert host.index("#ifdef FMD_EXPERIMENT") < host.index("getenv(") < host.index("#else")


def test_synth_is_deterministic_and_channel_offsettable(fmd):
    a = fmd.synth.synth_iq(3, 2048, sample_offset=1000)
    b = fmd.synth.synth_iq(3, 2048, sample_offset=1000)
    assert np.array_equal(a, b) and a.dtype == np.uint8
    whole = fmd.synth.synth_iq(1, 4096)
    assert np.array_equal(whole[0, 2048:], fmd.synth.synth_iq(1, 2048, sample_offset=1024)[0])   # streams continue
    assert np.array_equal(fmd.synth.synth_iq(4, 512)[2], fmd.synth.synth_iq(1, 512, first_channel=2)[0])
    assert 100 < a.mean() < 155 and a.min() >= 0


def test_channel_range_partition(fmd):
    for total, world in [(4096, 8), (10, 4), (7, 8), (32768, 8), (1, 1)]:
        seen = []
        for r in range(world):
            lo, hi = fmd.shard.channel_range(total, world, r)
            seen.extend(range(lo, hi))
            for c in range(lo, hi):
                assert fmd.shard.owner_of(c, total, world) == r
        assert seen == list(range(total))
    with pytest.raises(ValueError):
        fmd.shard.channel_range(4, 2, 2)


WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch.distributed as dist
import rtl_sdr_rs_amd as fmd, oracle_lib
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
total, n = 11, 16384
lo, hi = fmd.shard.channel_range(total, world, rank)
o = oracle_lib.load()
cfg = o.config(10, 240000, 32000)
# each rank demodulates ONLY its shard (the oracle stands in for the GPU kernel here: this test is about
# the sharding / gather logic of the N > 1 path; the kernel itself is covered by the -m gpu tests)
iq = fmd.synth.synth_iq(hi - lo, n, first_channel=lo)
bank = o.new_bank(cfg, hi - lo)
out, lens = o.demodulate_batch(bank, iq, threads=1)
local = [out[i, :lens[i]].copy() for i in range(hi - lo)]
full = fmd.shard.gather_audio(local, total, dst=0)
dist.barrier()
if rank == 0:
    ref_iq = fmd.synth.synth_iq(total, n)
    rbank = o.new_bank(cfg, total)
    rout, rlens = o.demodulate_batch(rbank, ref_iq, threads=1)
    assert len(full) == total
    for c in range(total):
        assert np.array_equal(full[c], rout[c, :rlens[c]]), c
    print("SHARD_OK")
else:
    assert full is None
dist.destroy_process_group()
'''


def test_sharded_run_world_size_2_gloo(tmp_path):
    """One process per rank (as bench.py --gpus N is launched), gloo backend, no collective on the data path:
    rank-local shards + the optional result gather reproduce the unsharded result exactly."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29517", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE) for r in range(2)]
    outs = [p.communicate(timeout=240) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se.decode()[-2000:]
    assert b"SHARD_OK" in outs[0][0]
