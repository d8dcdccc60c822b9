"""A plain bench.py run: the headline line alone, --steps honoured, and --dump-outputs writing what the timed step
computed -- every distance and index of the bench input, bit-exact against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, gen_pair

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_timed_outputs(tmp_path, oracle):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["metric"] == "chamfer_nn_pair_dist_throughput" and line["unit"] == "Gpair-dist/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["value"] > 0
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert not {"ms_per_step_spread", "roofline", "roofline_hbm", "output_checked", "extra", "cpu_baseline"} & set(line)
    got = [np.load(str(out / (k + ".npy"))) for k in ("dist1", "dist2", "idx1", "idx2")]
    assert [g.dtype for g in got] == [np.float32, np.float32, np.float64, np.float64]
    assert all(g.shape == (1, 16384) for g in got)
    a, b = gen_pair(20250101, (1, 16384, 3), (1, 16384, 3))
    exp = oracle.chamfer_forward(a, b, 1)
    for g, e, name in zip(got, exp, ("dist1", "dist2", "idx1", "idx2")):
        np.testing.assert_array_equal(g, e.astype(g.dtype), err_msg=name)
