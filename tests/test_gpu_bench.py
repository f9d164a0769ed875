"""bench.py contract on the GPU: one short --full run of each workload prints ONE JSON line with the
fields its readers rely on (metric/value/unit, roofline, cpu_baseline slot, config); a plain
run prints the same headline fields without the companion measurements and --dump-outputs writes the
last timed step's arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"}


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "2", "--warmup", "1", *args],
                       capture_output=True, text=True, timeout=240, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("workload", ["line", "allforone", "train"])
def test_bench_prints_one_contract_line(workload):
    d = _bench("--full", "--no-cpu-baseline", "--workload", workload)
    assert KEYS <= set(d)
    assert d["value"] > 0 and d["n_gpus"] == 1 and d["scaling"] == "weak" and d["higher_is_better"] is True
    roof = d["roofline"]
    assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and 0 < roof["frac"] < 1
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    assert "workload" in d["config"]
    if workload == "line":
        assert d["metric"].startswith("Langevin denoising steps/sec") and d["unit"] == "image-steps/s"


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """Without --full the line carries the headline only (no roofline pass, sustained window, fp32 line
    or CPU baseline) and --dump-outputs leaves the last timed step's arrays: the 4-view megabatch and
    its likelihood gradient, float32, finite, within the 64 MB budget."""
    d = _bench("--gpus", "1", "--dump-outputs", str(tmp_path))
    assert KEYS <= set(d)
    assert d["metric"].startswith("Langevin denoising steps/sec") and d["unit"] == "image-steps/s"
    assert d["steps"] == 2 and d["dtype"] == "fp32x3" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 4 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None
    assert d["fp32_exact"] is None and d["sustained"] is None
    files = sorted(os.listdir(tmp_path))
    assert files == ["likelihood_grad.npy", "x.npy"]
    arrays = {f: np.load(tmp_path / f) for f in files}
    assert all(a.dtype == np.float32 and a.shape == (4, 2, 64, 1024) for a in arrays.values())
    assert all(np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
