"""bench.py contract tests (the driver's BENCH/SCALE entry point): the
JSON line matches BASELINE.json's metric/config fields, and the exact
multi-rank launch shape the driver uses (torch.distributed.run, gloo on
CPU here / RCCL on the GPU box) completes with n_gpus=WORLD_SIZE."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last_json(stdout: str) -> dict:
    for line in reversed(stdout.strip().splitlines()):
        line = line.strip()
        if line.startswith("{") and '"metric"' in line:
            return json.loads(line)
    raise AssertionError(f"no metric JSON in output:\n{stdout[-2000:]}")


def _check_contract(rec: dict, n: int):
    assert rec["metric"] == "lab1_price_match_agent_decisions_per_sec"
    assert rec["unit"] == "decisions/s"
    assert rec["n_gpus"] == n
    assert rec["higher_is_better"] is True
    assert rec["scaling"] == "weak"
    assert rec["data"] == "synthetic"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert rec["config"]["model"]
    assert rec["vs_baseline"] is None or rec["vs_baseline"] > 0


@pytest.mark.timeout(300)
def test_bench_single_rank_stub_contract():
    out = subprocess.run(
        [sys.executable, "bench.py", "--stub-llm", "--steps", "2",
         "--warmup", "1", "--batch", "4"],
        cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    _check_contract(_last_json(out.stdout), 1)


@pytest.mark.timeout(300)
def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's per-decision results
    as float32/float64 .npy files, one row per decision, identical from
    run to run for the same arguments; --full is accepted and still
    prints the contract line; --steps sets the timed step count."""
    import numpy as np

    def run(dirname, *extra):
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--stub-llm",
             "--steps", "2", "--warmup", "1", "--batch", "4",
             "--dump-outputs", str(tmp_path / dirname), *extra],
            cwd=ROOT, capture_output=True, text=True, timeout=240)
        assert out.returncode == 0, out.stderr[-2000:]
        rec = _last_json(out.stdout)
        _check_contract(rec, 1)
        assert rec["steps"] == 2 and rec["warmup"] == 1
        return {f[:-4]: np.load(tmp_path / dirname / f)
                for f in sorted(os.listdir(tmp_path / dirname))}

    a = run("a")
    b = run("b", "--full")
    assert set(a) == set(b) >= {"status", "iterations", "tool_calls",
                                "failures", "response_len",
                                "response_bytes"}
    total = 0
    for name, arr in a.items():
        assert arr.dtype in (np.float32, np.float64), name
        assert arr.shape[0] == 4, name          # one row per decision
        assert np.array_equal(arr, b[name]), name
        total += arr.nbytes
    assert total <= 64 * 2**20
    # the stub agent finishes every episode on its first turn
    assert a["status"].tolist() == [1.0] * 4
    assert (a["response_len"] > 0).all()
    first = bytes(a["response_bytes"][0][a["response_bytes"][0] >= 0]
                  .astype(np.uint8)).decode()
    assert first.startswith("[stub-llm] considering:")


@pytest.mark.timeout(300)
def test_bench_two_rank_driver_launch_shape():
    port = str(29700 + os.getpid() % 200)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", port, "bench.py", "--gpus", "2", "--stub-llm",
         "--steps", "1", "--warmup", "0", "--batch", "4"],
        cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = _last_json(out.stdout)
    _check_contract(rec, 2)
    # whole-job aggregate: 2 ranks of fixed per-rank work
    assert rec["steps"] == 1
