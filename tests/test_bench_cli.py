"""bench.py's command line without a GPU: --dump-outputs (file format, the size cap and its fixed sample), the same
option through the scan workloads' CPU stand-in, and the argument check that runs before anything touches a GPU."""
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_dtypes_and_values(tmp_path):
    bench = _bench()
    d = np.arange(10, dtype=np.float32) / np.float32(3)
    i = np.arange(10, dtype=np.int32) * 1000003
    x = np.ones((2, 3)) / 3
    bench.dump_outputs(str(tmp_path / "o"), {"dist1": d, "idx1": i, "x": x})
    got = {k: np.load(str(tmp_path / "o" / (k + ".npy"))) for k in ("dist1", "idx1", "x")}
    assert got["dist1"].dtype == np.float32 and np.array_equal(got["dist1"], d)
    assert got["idx1"].dtype == np.float64 and np.array_equal(got["idx1"], i.astype(np.float64))
    assert got["x"].dtype == np.float64 and got["x"].shape == (2, 3) and np.array_equal(got["x"], x)


def test_dump_outputs_samples_above_the_cap(tmp_path):
    """Above the cap every array keeps the same seeded positions, in order, and the files stay under it."""
    bench = _bench()
    k = np.arange(1000)
    arrays = {"dist1": k.astype(np.float32), "idx1": k.astype(np.int32)}
    limit = 2 * 4096 + 3000                     # 12000 data bytes; 3000 left after the headers' room
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), arrays, limit=limit)
    d = np.load(str(tmp_path / "a" / "dist1.npy"))
    i = np.load(str(tmp_path / "a" / "idx1.npy"))
    assert d.size == i.size == 250 and np.all(np.diff(d) > 0)
    assert np.array_equal(d.astype(np.float64), i)
    assert d.nbytes + i.nbytes <= limit - 2 * 4096
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in ("dist1.npy", "idx1.npy")) <= limit
    for f in ("dist1.npy", "idx1.npy"):
        assert open(str(tmp_path / "a" / f), "rb").read() == open(str(tmp_path / "b" / f), "rb").read()


def test_dump_outputs_of_the_scan_workload_stub(tmp_path):
    """--workload c3 on the CPU stand-in (GENPC_BENCH_STUB=1): the gathered scan table is what is written."""
    env = dict(os.environ)
    env["GENPC_BENCH_STUB"] = "1"
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--workload", "c3", "--steps", "1", "--warmup", "0",
                        "--dump-outputs", str(tmp_path / "o")], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    t = np.load(str(tmp_path / "o" / "scan_metrics.npy")).astype(np.float64)
    assert t.shape == (13, 3) and line["steps"] == 1
    assert round(float(t.sum()), 9) == line["extra"]["scan_table_checksum"]


def test_bench_rejects_zero_steps():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--steps" in p.stderr
