"""The bench line's contract (one JSON line with `roofline` and `cpu_baseline`), at a size that takes seconds."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_roofline_and_cpu_baseline():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--haps", "4096", "--sites", "32768", "--steps", "2",
                        "--warmup", "1", "--full", "--no-other-configs", "--cpu-sample-cells", "2e7", "--cpu-threads", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and abs(d["value"] - 4096.0 * 32768 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and 0 < rf["frac"] < 1
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_same_outputs_twice(tmp_path):
    """Without --full the line is the headline alone (no CPU baseline, no other configurations) and --steps sets the
    timed steps; --dump-outputs writes the last step's outputs as float .npy files, the same in two runs."""
    import numpy as np
    got = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--haps", "4096", "--sites", "40000", "--steps", "3",
                            "--warmup", "1", "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["roundtrip_equal"] is True
        assert line["cpu_baseline"] is None and "other_configs" not in line and line["config"]["count_rows_ms"] is None
        files = sorted(os.listdir(d))
        assert files == ["block_offsets.npy", "decoded_rows_sample.npy", "sizes.npy", "xsi_blocks_sample.npy"], files
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        sizes = arrays["sizes.npy"]
        assert sizes[0] == line["config"]["xsi_bytes_this_gpu"] and sizes[2] == 40000
        assert arrays["block_offsets.npy"].shape == (line["config"]["blocks_this_gpu"],)
        assert 0 < arrays["xsi_blocks_sample.npy"].size <= min(line["config"]["xsi_bytes_this_gpu"], 4 << 20)
        assert arrays["decoded_rows_sample.npy"].shape[1] == line["config"]["row_stride_bytes"]
        got.append(arrays)
    for f in got[0]:
        assert np.array_equal(got[0][f], got[1][f]), f
