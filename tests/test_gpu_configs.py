"""BASELINE.json configs 2, 3 and 4 at their workload shape (Gowalla-shaped T = 3 / L = 2 / d = 64,
MovieLens-shaped T = 6 / L = 2 / d = 128, Amazon-shaped T = 5 / L = 3 / d = 64 with the notebook's per-interval edge
counts) and the reference's fourth dataset shape (Yelp: T = 12 / L = 3 / d = 64), each as ONE run of the bench entry with its CPU leg: the timed configuration's propagated rows (user-side
sample, item-side hubs) against oracle/c/tf1_path.c and its fused embeddings (users AND items) against the numpy
oracle. The composite — every interval's SpMM stack into the strided slabs the fusion reads — is what the kernel
tests at other shapes do not cover. Edges are synthetic (the dataset blobs are absent: SURVEY §8c)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SHAPES = {"gowalla-shaped": dict(users=48_653, items=52_619, T=3, L=2, d=64),
          "movielens-shaped": dict(users=24_312, items=8_681, T=6, L=2, d=128),
          "amazon-shaped": dict(users=11_199, items=30_821, T=5, L=3, d=64),
          "yelp-shaped": dict(users=19_751, items=38_386, T=12, L=3, d=64)}      # yelp.sh:1 (not a BASELINE config): T = 12 fusion, L = 3


def _bench(*args):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "bench.py", *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(line) == 1, out.stdout[-2000:]
    return json.loads(line[0])


@pytest.mark.parametrize("launch", ["eager", "graph"])
@pytest.mark.parametrize("workload", sorted(SHAPES))
def test_dataset_shaped_config_against_the_oracle(workload, launch):
    r = _bench("--workload", workload, "--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "1",
               *(["--graph"] if launch == "graph" else []))
    w, c = SHAPES[workload], r["config"]
    assert (c["users"], c["items"], c["intervals_total"], c["gnn_layers"], c["embed_dim"]) == (w["users"], w["items"], w["T"], w["L"], w["d"])
    assert r["n_gpus"] == 1 and c["intervals_per_gpu"] == w["T"] and r["metric"] == "spmm_edges_per_sec" and r["value"] > 0
    if workload == "amazon-shaped":
        assert abs(c["edges_per_interval"] - sum([72280, 78997, 79692, 78096, 45651]) // 5) <= 700    # the notebook's counts (generator: <= target)
    # propagated rows: |got - want| <= 1e-5 + 1e-4 |want| (+ 3 eps32 sum|terms| on hub rows)
    assert r["cpu_baseline"]["kind"] == "port" and r["cpu_baseline"]["gpu_vs_cpu_max_abs_err"] <= 1e-5
    assert r["item_side_check"]["worst_over_tolerance"] <= 1.0, r["item_side_check"]
    # fused embeddings, users and items: |got - want| <= 2e-5 + 1e-4 |want|
    fc = r["fused_check"]
    assert set(fc["by_node_type"]) == {"users", "items"} and fc["intervals"] == w["T"]
    assert fc["worst_over_tolerance"] <= 1.0, fc
    assert fc["by_node_type"]["items"]["rows"] == min(65_536, w["items"])
    assert ("fusion_f32_engine" in r) == (launch == "eager")      # the same-run exact-fp32 block: eager steps only


def test_dump_outputs_hold_the_last_timed_step(tmp_path):
    """--dump-outputs writes the fused embeddings of the last timed step: on a dataset-sized graph every row fits the
    budget, so the files reproduce the result line's statistics of the full arrays (taken after the same-run fp32-engine
    passes, which end with one more f16 x 2 step on the same inputs)."""
    import numpy as np
    w = SHAPES["gowalla-shaped"]
    r = _bench("--workload", "gowalla-shaped", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
               "--dump-outputs", str(tmp_path))
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    for j, (name, n) in enumerate((("final_user_vector", w["users"]), ("final_item_vector", w["items"]))):
        x = np.load(tmp_path / (name + ".npy"))
        assert x.dtype == np.float32 and x.shape == (n, w["d"]) and np.isfinite(x).all()
        assert r["dumped_outputs"][name] == {"shape": [n, w["d"]], "rows_of": n}
        a = np.abs(x.astype(np.float64))
        assert abs(a.mean() - r["final_abs_mean"][j]) <= 1e-6 * r["final_abs_mean"][j]
        pos = float((a.sum(axis=1) * np.arange(1, n + 1)).sum() / (n * (n + 1) / 2.0))
        assert abs(pos - r["final_position_checksum"][j]) <= 1e-6 * r["final_position_checksum"][j]


def test_plain_run_leaves_the_full_blocks_out():
    """Without --full the line holds the timed steps' own figures (headline, in-run roofline, checksums) and nothing that
    needs work outside them: no exact-fp32 block, CPU baseline or oracle check, no recorded traffic."""
    r = _bench("--workload", "gowalla-shaped", "--steps", "2", "--warmup", "1")
    assert r["metric"] == "spmm_edges_per_sec" and r["value"] > 0 and r["ms_per_step"] > 0 and r["steps"] == 2
    assert r["roofline"]["launches"] > 0 and r["roofline"]["traffic_source"] is None
    assert len(r["final_abs_mean"]) == 2 and r["dumped_outputs"] is None
    assert not set(r) & {"fusion_f32_engine", "cpu_baseline", "item_side_check", "fused_check", "breakdown_ms"}
