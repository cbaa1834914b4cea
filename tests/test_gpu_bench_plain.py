"""bench.py without --full: only the headline line (no roofline / kernel events, no extra legs, no CPU work), and --dump-outputs
writes what the timed path returned in its last step.  Two runs with the same arguments see the same inputs, so their dumps agree."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_dtypes_and_seeded_sample(tmp_path, monkeypatch):
    import torch
    e = torch.randn(600, 64).bfloat16()
    d = torch.randn(600, 10)
    i = torch.arange(6000, dtype=torch.int64).view(600, 10)
    bench.dump_outputs(str(tmp_path / "a"), {"embeddings": e, "distances": d, "ids": i})
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("embeddings", "distances", "ids")}
    assert got["embeddings"].dtype == np.float32 and got["distances"].dtype == np.float32 and got["ids"].dtype == np.float64
    np.testing.assert_array_equal(got["embeddings"], e.float().numpy())
    np.testing.assert_array_equal(got["ids"], i.numpy().astype(np.float64))
    assert not (tmp_path / "a" / "rows.npy").exists()
    # over the limit: the same seeded rows of every array, their numbers in rows.npy, the whole under the limit
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    for sub in ("b", "c"):
        bench.dump_outputs(str(tmp_path / sub), {"embeddings": e, "distances": d, "ids": i}, rank=1, world=2)
    files = sorted(os.listdir(tmp_path / "b"))
    assert files == ["distances_rank1.npy", "embeddings_rank1.npy", "ids_rank1.npy", "rows_rank1.npy"]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in files) <= (64 << 10) // 2
    rows = np.load(tmp_path / "b" / "rows_rank1.npy").astype(np.int64)
    assert 0 < len(rows) < 600 and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "ids_rank1.npy"), i.numpy()[rows].astype(np.float64))
    for f in files:
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))


def _bench(out_dir, *extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--db-rows", "200000", "--clips", "256", "--dump-outputs", str(out_dir), *extra],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_and_dumps_the_last_step(gpu, tmp_path):
    out = _bench(tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
    assert abs(out["value"] - 256 * 1e3 / out["ms_per_step"]) / out["value"] < 1e-3
    for key in ("roofline", "kernels", "sustained", "scan_unstructured", "pcie_inclusive", "cpu_baseline", "parity_on_sample"):
        assert key not in out, key
    emb, dist, ids = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("embeddings", "distances", "ids"))
    assert emb.shape == (256, 512) and emb.dtype == np.float32
    assert dist.shape == (256, 10) and dist.dtype == np.float32 and ids.shape == (256, 10) and ids.dtype == np.float64
    # the store holds two near-duplicates of every clip: clip j's nearest row is its own planted row (bench.py, rank 0)
    np.testing.assert_array_equal(ids[:, 0], (np.arange(256) * 977 + 17) % 200000)
    assert np.all(np.diff(dist, axis=1) <= 0)
    # a second run with the same arguments: same inputs, same results
    _bench(tmp_path / "b")
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "ids.npy"), ids)
    np.testing.assert_allclose(np.load(tmp_path / "b" / "embeddings.npy"), emb, rtol=0, atol=1e-5)
