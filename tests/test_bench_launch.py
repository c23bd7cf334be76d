"""bench.py's launch paths.  `python bench.py --gpus N` must start N rank processes itself (`--gpus` was
parsed and ignored, so a plain `--gpus 8` measured one GPU).  CPU: the launcher really spawns N ranks and the whole
job fails loudly when there is no GPU (no silent CPU path, no silent single-rank run); a WORLD_SIZE / --gpus mismatch
is an error.  GPU: two ranks over gloo sharing the one GPU of the test box print ONE line with n_gpus == 2."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def clean_env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    return env


def test_gpus_flag_spawns_ranks_and_fails_loudly_without_gpu(fmd):
    if fmd.device_count() > 0:
        pytest.skip("a GPU is present: covered by the gpu test below")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--backend", "gloo", "--steps", "2", "--no-cpu"],
                       capture_output=True, env=clean_env(), timeout=600)
    err = p.stderr.decode()
    assert p.returncode != 0
    # both ranks ran and refused (on a box under load the launcher's 15 s grace can end the slower rank before it has said so:
    # then its exit code -- a kill -- still counts as a failure, and one refusal message is enough)
    assert "rank exit codes" in err and err.count("no gfx950 device") >= 1, err[-2000:]
    codes = err[err.index("rank exit codes"):].split("[", 1)[1].split("]", 1)[0].split(",")
    assert len(codes) == 2 and all(int(c) != 0 for c in codes), err[-2000:]
    assert p.stdout.decode().strip() == ""


def test_a_dead_rank_takes_the_job_down(monkeypatch):
    """One rank exits with an error while another would sit in the rendezvous: the launcher ends the job (after a grace
    period for the others' own messages) instead of waiting for a collective timeout."""
    import importlib.util
    import time
    import types
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    real = subprocess.Popen

    def fake(cmd, env=None, stdout=None):
        code = "import time; time.sleep(120)" if env["RANK"] == "0" else "import sys; sys.exit(3)"
        return real([sys.executable, "-c", code], stdout=stdout)

    monkeypatch.setattr(bench.subprocess, "Popen", fake)
    t0 = time.time()
    rc = bench.spawn_ranks(types.SimpleNamespace(gpus=2))
    assert rc == 1 and time.time() - t0 < 60


def test_a_dead_rank_zero_takes_the_job_down(monkeypatch):
    """The mirrored case: rank 0 (which hosts the rendezvous store) exits with an error first while rank 1 would wait
    for its own rendezvous / collective timeout: the launcher gives the others 15 s, then kills them by handle."""
    import importlib.util
    import time
    import types
    spec = importlib.util.spec_from_file_location("bench_under_test0", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    real = subprocess.Popen

    def fake(cmd, env=None, stdout=None):
        code = "import sys; sys.exit(4)" if env["RANK"] == "0" else "import time; time.sleep(300)"
        return real([sys.executable, "-c", code], stdout=stdout)

    monkeypatch.setattr(bench.subprocess, "Popen", fake)
    t0 = time.time()
    rc = bench.spawn_ranks(types.SimpleNamespace(gpus=2))
    assert rc == 1 and time.time() - t0 < 60


def test_world_size_must_match_gpus():
    env = dict(clean_env(), WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2"], capture_output=True, env=env, timeout=300)
    assert p.returncode != 0 and b"WORLD_SIZE=2" in p.stderr


def run_bench(args):
    p = subprocess.run([sys.executable, BENCH] + args, capture_output=True, env=clean_env(), timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_two_ranks_on_one_box():
    common = ["--steps", "5", "--warmup", "2", "--settle", "10", "--no-cpu", "--no-extra", "--channels", "1024", "--min-timed-s", "0.05"]
    one = run_bench(common)
    two = run_bench(["--gpus", "2", "--backend", "gloo"] + common)
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert len(two["per_gpu_msamples_per_s"]) == 2 and all(v > 0 for v in two["per_gpu_msamples_per_s"])
    assert two["config"]["parallelism"].startswith("channels sharded x2")
    assert "cpu_baseline" not in two and two["scaling"] == "weak"
    # both ranks share ONE GPU here, so the aggregate is about the one-rank rate (never 2x, never a silent 1-rank run)
    assert 0.4 * one["value"] < two["value"] < 1.6 * one["value"], (one["value"], two["value"])
    assert one["timing"]["regions"] >= 2 and one["timing"]["timed_ms_total"] >= 40.0
    for r in (one, two):
        assert 0.05 < r["roofline"]["frac"] < 1.0 and r["roofline"]["bound"] == "hbm"


@pytest.mark.gpu
def test_two_rank_line_is_self_verifying():
    """the N > 1 line must carry what makes it creditable -- a parity bit from EVERY rank (gathered), the CPU
    baseline (rank 0), every GPU's clock / power and the kernel name the library reports -- not only the N = 1 line.  Two
    gloo ranks share the test box's one GPU."""
    r = run_bench(["--gpus", "2", "--backend", "gloo", "--steps", "5", "--warmup", "2", "--settle", "10", "--channels", "1024",
                   "--min-timed-s", "0.05", "--cpu-seconds", "1", "--power-only"])
    assert r["n_gpus"] == 2
    p = r["parity"]
    assert p["ok"] is True and p["ranks_checked"] == 2 and p["ranks_ok"] == [True, True] and p["channels_checked"] >= 2 * 60
    cb = r["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1
    pg = r["extra"]["power_clock"]["per_gpu"]
    assert [g["rank"] for g in pg] == [0, 1] and all(g["ms_per_call"] is None or g["ms_per_call"] > 0 for g in pg)
    assert set(r["extra"]) == {"power_clock"}                   # the other side lines belong to the one-GPU line
    assert r["roofline"]["kernel"] == r["roofline"]["kernel_expected"] and r["roofline"]["kernel_is_expected"] is True


def torchrun_cmd(n, port, extra):
    """The driver's own launch line for N > 1 (one rank per GPU, rendezvous on 127.0.0.1)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
            "--master-port", str(port), BENCH, "--gpus", str(n)] + extra


def test_driver_launch_line_fails_loudly_without_gpu(fmd):
    """`python -m torch.distributed.run ... bench.py --gpus 2` on a box without a GPU: both ranks read RANK / LOCAL_RANK /
    WORLD_SIZE from the environment, refuse (no CPU path) and the job exits non-zero without printing a line."""
    if fmd.device_count() > 0:
        pytest.skip("a GPU is present: covered by the gpu test below")
    p = subprocess.run(torchrun_cmd(2, 29541, ["--backend", "gloo", "--steps", "2", "--no-cpu"]), capture_output=True, env=clean_env(), timeout=600)
    assert p.returncode != 0
    assert b"no gfx950 device" in p.stderr and not [l for l in p.stdout.decode().splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_driver_launch_line_two_ranks_on_one_box():
    """The same launch line with a GPU: ranks started by torch.distributed.run (not by bench.py's own launcher), gloo
    because both ranks share the box's one GPU; rank 0 prints ONE line with n_gpus == 2 and both per-GPU rates."""
    p = subprocess.run(torchrun_cmd(2, 29543, ["--backend", "gloo", "--steps", "5", "--warmup", "2", "--settle", "10", "--no-cpu", "--no-extra",
                                               "--channels", "1024", "--min-timed-s", "0.05"]), capture_output=True, env=clean_env(), timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and len(r["per_gpu_msamples_per_s"]) == 2 and r["scaling"] == "weak"
    assert r["config"]["torch_distributed"]["world_size"] == 2 and r["value"] > 0


RANKS_ON_ONE_BOX = 4        # + the pytest process, which holds the GPU too: five processes on one GPU, no more


@pytest.mark.gpu
def test_four_ranks_on_one_box_emit_the_line_a_multi_gpu_node_will():
    """the first real multi-GPU run (the driver's to launch) must not fail on plumbing.  The driver's launch
    line with RANKS_ON_ONE_BOX ranks over gloo, all sharing this box's one GPU (small banks: 256 channels each): one line, one
    per-GPU rate per rank, a parity bit from every rank, the world size, contiguous channel shards, no data-path collective.
    Not eight ranks: with the test process itself that would be nine processes holding one GPU at once."""
    n = RANKS_ON_ONE_BOX
    p = subprocess.run(torchrun_cmd(n, 29547, ["--backend", "gloo", "--steps", "3", "--warmup", "1", "--settle", "5", "--channels", "256",
                                               "--min-timed-s", "0.02", "--cpu-seconds", "0.5", "--power-only"]),
                       capture_output=True, env=clean_env(), timeout=1500)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    r = json.loads(lines[0])
    assert r["n_gpus"] == n and r["scaling"] == "weak" and r["value"] > 0
    assert len(r["per_gpu_msamples_per_s"]) == n and all(v > 0 for v in r["per_gpu_msamples_per_s"])
    assert r["config"]["torch_distributed"]["world_size"] == n
    assert r["config"]["parallelism"].startswith("channels sharded x%d" % n)
    pr = r["parity"]
    assert pr["ok"] is True and pr["ranks_checked"] == n and pr["ranks_ok"] == [True] * n
    assert [g["rank"] for g in r["extra"]["power_clock"]["per_gpu"]] == list(range(n))
    assert r["roofline"]["kernel_is_expected"] is True


def shape_of(x):
    """Keys and value types of a JSON line, recursively (numbers are one type): what "unchanged" means for a line."""
    if isinstance(x, dict):
        return {k: shape_of(v) for k, v in x.items()}
    if isinstance(x, list):
        return [shape_of(v) for v in x[:1]]
    return "num" if isinstance(x, (int, float)) and not isinstance(x, bool) else type(x).__name__


@pytest.mark.gpu
def test_force_dist_runs_the_rccl_branch_with_one_rank():
    """VERDICT r2 #1b: bench.py's torch.distributed branch (init_process_group("nccl", device_id=...), the barrier in every
    fence, all_reduce(MAX) per region, all_gather of the per-GPU rates, destroy) only ran with world > 1 -- never on any box
    the builder can reach.  --force-dist takes exactly that code with world size 1 over RCCL on the one GPU; the JSON line
    must keep its shape and its value."""
    common = ["--steps", "20", "--warmup", "2", "--settle", "50", "--no-cpu", "--no-extra", "--min-timed-s", "0.2"]
    plain = run_bench(common)
    forced = run_bench(common + ["--force-dist"])
    assert plain["config"]["torch_distributed"] is None
    assert forced["config"]["torch_distributed"] == {"backend": "nccl", "world_size": 1,
                                                     "collectives": forced["config"]["torch_distributed"]["collectives"]}
    a, b = shape_of(plain), shape_of(forced)
    a["config"].pop("torch_distributed"); b["config"].pop("torch_distributed")
    assert a == b
    assert forced["n_gpus"] == 1 and len(forced["per_gpu_msamples_per_s"]) == 1
    assert abs(forced["per_gpu_msamples_per_s"][0] - forced["value"]) < 0.05 * forced["value"]
    assert 0.7 * plain["value"] < forced["value"] < 1.4 * plain["value"], (plain["value"], forced["value"])
    assert forced["timing"]["regions"] >= 2
    # ... and with the parity bit, the CPU baseline and the per-GPU sensors gathered over RCCL (all_gather on device tensors)
    full = run_bench(["--steps", "20", "--warmup", "2", "--settle", "50", "--min-timed-s", "0.2", "--force-dist", "--cpu-seconds", "1", "--power-only"])
    assert full["parity"]["ok"] is True and full["parity"]["ranks_checked"] == 1 and full["parity"]["channels_checked"] >= 60
    assert full["cpu_baseline"]["value"] > 0 and len(full["extra"]["power_clock"]["per_gpu"]) == 1
    assert full["roofline"]["kernel_is_expected"] is True and full["roofline"]["kernel"].startswith("fmd_tk::fmd_demod_tile_kernel<5,")


@pytest.mark.gpu
def test_default_line_carries_parity_and_the_side_lines():
    """>= 1 s of timed launches, a parity bit against the oracle, and driver-visible lines for the
    reference's own configuration, config 2, the per-step completion point and the PCIe-inclusive sink."""
    r = run_bench(["--steps", "50", "--settle", "50", "--min-timed-s", "1"])
    assert r["timing"]["timed_ms_total"] >= 1000.0
    assert r["parity"]["ok"] is True and r["parity"]["channels_checked"] >= 32
    assert r["roofline"]["traffic_measured_in_this_run"] is False
    ex = r["extra"]
    assert r["roofline"]["kernel_is_expected"] is True and r["parity"]["ranks_checked"] == 1
    for k in ("cfg_ref", "check_per_step", "check_pipelined", "config2_1channel", "config4_fir", "config4_fir_demod_fused", "sink_pcie", "domain"):
        assert k in ex and "error" not in ex[k], (k, ex.get(k))
    # the completion points one and two launches back do not serialise host and device (fmd_demod_check_behind, round 6): within the
    # VERDICT's 1.03 x of the bare launches plus room for a host hiccup inside the 30 ms the side line times (measured 1.00 - 1.01 x
    # since guarded samples are settled without draining the queue, profiles/r06_experiments.md 9; launch + fmd_demod_check per
    # buffer is 1.12 x)
    assert ex["check_pipelined"]["ms_per_step"] <= 1.05 * r["ms_per_step"] and ex["check_pipelined"]["ms_per_step"] < ex["check_per_step"]["ms_per_step"]
    assert ex["check_pipelined"]["one_launch_back"]["ms_per_step"] < ex["check_per_step"]["ms_per_step"]
    assert ex["config4_fir"]["output_buffers"] == 4 and ex["config4_fir"]["kernel"].startswith("(anonymous namespace)::fmd_fir_mfma_kernel<")
    assert ex["config4_fir"]["one_output_buffer"]["frac"] > 0
    assert 0.3 < ex["cfg_ref"]["frac"] < 1.0 and ex["check_per_step"]["ms_per_step"] >= r["ms_per_step"] * 0.9
    assert ex["sink_pcie"]["all_status_ok"] and ex["sink_pcie"]["delivered"] >= 40
    rows = {row["downsample"]: row for row in ex["domain"]["rows"]}
    assert set(rows) == {1, 2, 3, 4, 5, 7, 8, 12, 16, 64} and all("error" not in row and 0.05 < row["frac"] < 1.0 for row in rows.values())
    assert rows[4]["kernel"].startswith("fmd_tk::fmd_demod_stream_kernel<2,") and rows[7]["kernel"].startswith("fmd_tk::fmd_demod_tile_kernel<-7,")
    assert ex["cfg_ref"]["kernel"].startswith("fmd_tk::fmd_demod_tile_kernel<3,")
    pc = ex["power_clock"]                                      # clock and power under load: sensors may be absent on a box,
    assert "error" in pc or (1000 <= pc["sclk_mhz"]["median"] <= 2500 and pc["power_w"]["median"] > pc["idle"]["power_w"]["median"]
                             and isinstance(pc["at_power_cap"], bool)), pc     # but when present they must read sensibly
    cb = r["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["cfg_ref_single_thread"]["value"] > 0
