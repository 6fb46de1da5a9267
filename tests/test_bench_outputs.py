"""bench.py's plain run and --dump-outputs: the writer on the host, the plain line and its outputs on the device."""
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_test", REPO / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_write_outputs_keeps_small_outputs_whole(tmp_path):
    bench = _bench()
    pos = np.arange(20, dtype=np.float32).reshape(10, 2)
    ids = np.arange(10, dtype=np.uint32)
    bench.write_outputs(tmp_path, {"position": pos, "id": ids}, {"step_stats": np.array([0.5, 1.0, 3, 4], dtype=np.float64)})
    assert sorted(p.name for p in tmp_path.iterdir()) == ["id.npy", "position.npy", "step_stats.npy"]
    a = np.load(tmp_path / "position.npy")
    assert a.dtype == np.float32 and np.array_equal(a, pos)
    b = np.load(tmp_path / "id.npy")
    assert b.dtype == np.float64 and np.array_equal(b, ids)


def test_write_outputs_samples_large_outputs_the_same_way_every_time(tmp_path):
    bench = _bench()
    n = 5000
    pos = np.random.default_rng(1).random((n, 2), dtype=np.float32)
    rho = np.random.default_rng(2).random(n, dtype=np.float32)
    limit = 20000
    for d in ("a", "b"):
        bench.write_outputs(tmp_path / d, {"position": pos, "density": rho}, {"step_stats": np.zeros(4)}, limit_bytes=limit)
    total = sum(p.stat().st_size - 128 for p in (tmp_path / "a").iterdir())   # (.npy header: 128 bytes)
    assert total <= limit
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert idx.dtype == np.float64 and 0 < len(idx) < n and np.all(np.diff(idx) > 0)
    k = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "position.npy"), pos[k])
    assert np.array_equal(np.load(tmp_path / "a" / "density.npy"), rho[k])
    for name in ("sample_index", "position", "density", "step_stats"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")), name


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain run times exactly --steps steps, carries no --full leg, and two runs with the same arguments write the same outputs."""
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--workload", "dam_break_64k",
                            "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=600, cwd=str(REPO), env=dict(os.environ))
        assert r.returncode == 0, r.stderr[-4000:]
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    for d in lines:
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 3 and d["warmup"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
        for k in ("roofline", "kernels", "other_configs", "cpu_baseline", "strong_8m", "forced_count"):
            assert k not in d, k
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["density.npy", "position.npy", "pressure.npy", "step_stats.npy", "velocity.npy"]
    n = 256 * 256
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
    assert np.load(tmp_path / "a" / "position.npy").shape == (n, 2)
    assert np.all(np.isfinite(np.load(tmp_path / "a" / "density.npy")))
    st = np.load(tmp_path / "a" / "step_stats.npy")
    assert st.shape == (4,) and st[0] > 0
