"""bench.py's multi-GPU launch on CPU (--dry-run: no GPU call): the ranks
bench.py spawns itself and the ranks torch.distributed.run starts (the
driver's N-GPU command line) read RANK / LOCAL_RANK / WORLD_SIZE, exchange the
rendezvous file rank 0 writes, and report the device each would open -- so a
real 8-GPU run cannot die in the launcher."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def clean_env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def check(p, n):
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    assert sorted(x["rank"] for x in lines) == list(range(n)), lines
    assert all(x["rendezvous_ok"] and x["world_size"] == n for x in lines), lines
    assert sorted(x["device"] for x in lines) == (list(range(n)) if n > 1 else [0])


@pytest.mark.parametrize("n", [1, 2, 4])
def test_spawned_ranks(n):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", str(n), "--dry-run"], cwd=ROOT, env=clean_env(),
                       capture_output=True, text=True, timeout=120)
    check(p, n)


@pytest.mark.parametrize("n", [2, 8])
def test_torchrun_ranks(n):
    # the driver's command: python -m torch.distributed.run --nnodes=1
    # --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), "bench.py", "--gpus", str(n), "--dry-run"]
    p = subprocess.run(cmd, cwd=ROOT, env=clean_env(), capture_output=True, text=True, timeout=240)
    check(p, n)


def test_dump_outputs_writes_every_result_field_as_float64(tmp_path):
    # --dump-outputs: one float64 .npy per ks_result field, values exact
    import importlib.util

    import numpy as np

    from ksched import _abi

    spec = importlib.util.spec_from_file_location("bench", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = 37
    raw = (_abi.KsResult * n)()
    for i in range(n):
        raw[i].node_index, raw[i].status, raw[i].total_score = i - 1, i % 3, (1 << 40) + i
        raw[i].feasible_nodes, raw[i].evaluated_nodes, raw[i].flags = 2 * i, 3 * i, i & 1
        raw[i].fail_counts[i % 8] = i
    bench.dump_outputs(tmp_path / "d", raw, n)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert sorted(got) == sorted(bench.DUMP_FIELDS) and all(a.dtype == np.float64 for a in got.values())
    i = np.arange(n)
    assert np.array_equal(got["node_index"], i - 1) and np.array_equal(got["status"], i % 3)
    assert np.array_equal(got["total_score"], (1 << 40) + i) and np.array_equal(got["flags"], i & 1)
    assert np.array_equal(got["feasible"], 2 * i) and np.array_equal(got["evaluated"], 3 * i)
    assert got["fail"].shape == (n, 8) and np.array_equal(got["fail"][i, i % 8], i) and got["fail"].sum() == i.sum()


def test_resolve_profile_needs_full():
    p = subprocess.run([sys.executable, "bench.py", "--resolve-profile", "--dry-run"], cwd=ROOT, env=clean_env(),
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--full" in p.stderr


def test_world_size_mismatch_is_refused():
    env = dict(clean_env(), WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--dry-run"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "WORLD_SIZE=2 but --gpus 4" in p.stderr
