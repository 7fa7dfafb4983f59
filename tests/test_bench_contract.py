"""-m gpu: bench.py's output contract (one JSON line, last on stdout, the keys the driver reads), on a small shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {"metric": str, "value": float, "unit": str, "n_gpus": int, "steps": int, "warmup": int, "ms_per_step": float,
            "higher_is_better": bool, "scaling": str, "dtype": str, "data": str, "config": dict, "roofline": dict}


def run_bench(extra, env=None):
    e = dict(os.environ)
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--shape", "small", "--steps", "6", "--warmup", "2",
                          "--batch-users", "128", "--num-dim", "32"] + extra, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    return json.loads(lines[-1])          # the JSON line is the LAST line of stdout


def check(d, n_gpus=1):
    for k, t in REQUIRED.items():
        assert k in d, k
        assert isinstance(d[k], t) or (t is float and isinstance(d[k], int)), (k, d[k])
    assert "vs_baseline" in d and d["vs_baseline"] is None            # BASELINE.md publishes no number for this metric
    assert d["unit"] == "users/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic"
    assert d["n_gpus"] == n_gpus and d["steps"] == 6 and d["warmup"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9


def test_default_line_with_cpu_baseline(built):
    d = run_bench(["--full", "--cpu-users", "300"])
    check(d)
    assert d["dtype"] == "f32" and d["roofline"]["bound"] == "hbm"
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and c["unit"] == "users/s" and isinstance(c["sample"], str)


def test_dump_outputs_are_what_the_timed_steps_left(built, tmp_path):
    """--dump-outputs: the parameters after the last timed step, float32 .npy.  Training is bit-deterministic
    (tests/test_gpu_parity.py::test_training_is_bit_deterministic_and_handles_reload), so the same arguments write the same arrays, also
    without the HIP events around the decode launches of the timed steps (--profile-every 0); one more timed step writes other arrays."""
    dumps = []
    for name, extra in (("a", []), ("b", ["--profile-every", "0"]), ("c", ["--steps", "7"])):
        d = run_bench(["--no-cpu-baseline", "--dump-outputs", str(tmp_path / name)] + extra)
        assert d["steps"] == (7 if name == "c" else 6) and d["ms_per_step"] > 0
        dumps.append({f[:-4]: np.load(tmp_path / name / f) for f in os.listdir(tmp_path / name)})
    a, b, c = dumps
    assert set(a) == {"W", "W_ag", "b", "b_ag", "bp", "bp_ag", "Wu", "Wu_ag"}
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= 64e6
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["W"], c["W"])


def test_full_output_line(built):
    d = run_bench(["--full-output", "--no-cpu-baseline"])
    check(d)
    assert d["dtype"] == "bf16" and d["roofline"]["bound"] == "mfma" and "cpu_baseline" not in d


def test_exchange_path_with_a_one_rank_rccl_group(built):
    """The N > 1 code path (process group after the handle, pipelined delta exchange, flush inside the timed region, JSON last
    after RCCL's banner) with a single rank — as much of `--gpus N` as one GPU can run."""
    d = run_bench(["--no-cpu-baseline"], env={"CDAE_BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29533",
                                              "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    check(d)
    assert d["config"]["exchange"] != "none"


def test_item_rows_layout_line(built):
    """--layout item-rows (the configs[4] layout) on one GPU with logical shards: same contract keys, strong scaling by definition"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--shape", "small", "--steps", "4", "--warmup", "1", "--batch-users", "128",
                          "--num-dim", "64", "--full-output", "--layout", "item-rows", "--logical-shards", "3", "--no-cpu-baseline"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip()][-1])
    for k, t in REQUIRED.items():
        assert k in d, k
    assert d["scaling"] == "strong" and d["n_gpus"] == 1 and d["value"] > 0 and d["roofline"]["bound"] == "mfma"
    assert "item-rows x3" in d["config"]["parallelism"]


def test_certified_schedule_line_is_what_gpus_n_runs_by_default(built):
    """What `--gpus N` (N > 1) runs by default since round 6 — user shards on the relay + synchronous-exchange + global-accumulator
    schedule, one process driving every GPU, with (--full) the single-GPU and item-rows figures of the same node beside the line — exercised on
    one GPU as logical shards (the sum kernel in RCCL's place).  K timed steps are exactly K exchanged steps (cdae_hip_multi_train_steps)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--shape", "small", "--steps", "20", "--warmup", "3", "--batch-users", "128",
                          "--num-dim", "32", "--layout", "certified", "--logical-shards", "4", "--sync-batch-users", "32", "--full", "--no-cpu-baseline"],
                         cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip()][-1])
    for k, t in REQUIRED.items():
        assert k in d, k
    assert d["scaling"] == "strong" and d["n_gpus"] == 1 and d["steps"] == 20 and d["value"] > 0 and d["dtype"] == "f32"
    c = d["config"]
    assert c["batch_users"] == 32 and 120 <= c["global_batch"] <= 128 and c["schedule"]["relay_epochs"] == 1.0 and c["schedule"]["steps_per_epoch"] > 0   # (shards finish together: a step takes ceil(n_s / steps) of each)
    assert abs(d["value"] - c["global_batch"] * 1e3 / d["ms_per_step"]) < 0.02 * d["value"]
    side = c["same_node_alternatives"]
    assert side["single_gpu"]["users_per_s"] > 0 and side["item_rows_same_gpus"]["users_per_s"] > 0, side
    assert c["vs_single_gpu"] > 0 and "relay" in c["accuracy"]
    assert abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-9


def test_sampled_item_rows_line(built):
    """The sampled decode in the item-rows layout — the multi-GPU schedule that is the single-GPU schedule exactly (the N > 1 default through
    round 5, now `--layout item-rows`) — exercised on one GPU as logical shards (--logical-shards selects the layout)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--shape", "small", "--steps", "20", "--warmup", "3", "--batch-users", "128",
                          "--num-dim", "32", "--logical-shards", "4", "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip()][-1])
    for k, t in REQUIRED.items():
        assert k in d, k
    assert d["scaling"] == "strong" and d["n_gpus"] == 1 and d["steps"] == 20 and d["value"] > 0 and d["dtype"] == "f32"
    assert d["roofline"]["bound"] == "hbm" and abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-9
    assert "item-rows x4" in d["config"]["parallelism"] and "single-GPU schedule exactly" in d["config"]["accuracy"]


FAMILIES = {"sample", "sort", "encode", "decode", "hidden", "input"}


def test_plain_run_is_lean_and_full_leaves_the_timed_steps_alone(built, tmp_path):
    """A plain run measures what the headline needs and nothing beside it: no CPU baseline, no untimed pass for the kernel families other
    than the decode (whose events sit inside the timed region).  --full adds both and changes nothing the timed steps compute: the same
    arguments dump the same arrays bit for bit either way."""
    plain = run_bench(["--dump-outputs", str(tmp_path / "plain")])
    full = run_bench(["--full", "--cpu-users", "300", "--dump-outputs", str(tmp_path / "full")])
    for d in (plain, full):
        check(d)
        assert d["dtype"] == "f32" and d["prewarm_steps"] == 298 and d["profiled_steps"] > 0
        assert d["kernel_ms_per_step"]["decode"] > 0 and d["roofline"]["avg_launch_ms"] > 0
    assert "cpu_baseline" not in plain and set(plain["kernel_ms_per_step"]) == {"decode"}
    assert full["cpu_baseline"]["value"] > 0 and set(full["kernel_ms_per_step"]) == FAMILIES
    assert all(full["kernel_ms_per_step"][k] > 0 for k in FAMILIES)
    assert plain["metric"] == full["metric"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and len(names) == 8
    for f in names:
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)), f


def test_plain_certified_line_starts_no_side_runs(built):
    """--layout certified without --full: the line of the exchanged schedule alone — no single-GPU or item-rows run in a process beside it"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--shape", "small", "--steps", "20", "--warmup", "3", "--batch-users", "128",
                          "--num-dim", "32", "--layout", "certified", "--logical-shards", "4", "--sync-batch-users", "32"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip()][-1])
    for k, t in REQUIRED.items():
        assert k in d, k
    c = d["config"]
    assert d["steps"] == 20 and d["value"] > 0 and c["batch_users"] == 32 and c["schedule"]["relay_epochs"] == 1.0
    assert c["same_node_alternatives"] == {} and c["vs_single_gpu"] is None


def test_plain_item_rows_line_has_no_untimed_pass(built):
    """--layout item-rows without --full: shard 0's launches are not timed in a pass of their own; with --full they are"""
    lines = []
    for extra in ([], ["--full"]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--shape", "small", "--steps", "4", "--warmup", "1", "--batch-users", "128",
                              "--num-dim", "32", "--logical-shards", "2"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads([l for l in out.stdout.splitlines() if l.strip()][-1]))
    plain, full = lines
    assert plain["value"] > 0 and "shard0_decode" not in plain["roofline"]
    assert full["value"] > 0 and full["roofline"]["shard0_decode"]["avg_launch_ms"] > 0
    assert abs(plain["roofline"]["frac"] - plain["roofline"]["achieved"] / plain["roofline"]["peak"]) < 1e-9
