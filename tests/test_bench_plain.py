"""bench.py without --full: one block of exactly --steps ticks, the headline line and nothing else; --dump-outputs writes what the
last timed tick returned, the same from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _StubMPPI:
    steps = 50

    def getControls(self):
        return np.arange(2 * self.steps, dtype=np.float64).reshape(2, self.steps)


def test_dump_outputs_writes_float64_arrays(tmp_path):
    bench.dump_outputs(str(tmp_path / "out"), _StubMPPI(), (0.25, -0.5))
    c = np.load(tmp_path / "out" / "controls.npy")
    u = np.load(tmp_path / "out" / "control_sequence.npy")
    assert c.dtype == np.float64 and c.tolist() == [0.25, -0.5]
    assert u.dtype == np.float64 and u.shape == (2, 50) and np.array_equal(u, _StubMPPI().getControls())


def test_a_plain_line_names_no_detail_file_and_writes_none(tmp_path, monkeypatch, capsys):
    path = tmp_path / "bench_detail.json"
    monkeypatch.setattr(bench, "DETAIL_PATH", str(path))
    full = {"metric": "MPPI rollouts/s", "value": 1.0, "unit": "rollouts/s", "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 0.01,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "w", "noise": "n", "parallelism": "p"}, "roofline": None}
    bench.emit(full, detail_file=False)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["detail"] is None and line["ms_per_step"] == 0.01 and not path.exists()


def _plain_run(out_dir, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "5",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TBNAV_BENCH_DETAIL=str(out_dir) + ".detail.json"), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert not os.path.exists(str(out_dir) + ".detail.json")   # a plain run writes no detail file
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_times_steps_once_and_dumps_the_same_outputs_twice(gpu_pkg, tmp_path):
    a = _plain_run(tmp_path / "a", 20)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a, k
    assert a["metric"] == "MPPI rollouts/s" and a["unit"] == "rollouts/s" and a["higher_is_better"] is True and a["dtype"] == "f64"
    assert a["steps"] == 20 and a["repeats"] == 1 and a["ms_per_step"] > 0
    assert a["value"] == pytest.approx(1024 * 1000.0 / a["ms_per_step"], rel=1e-3)
    assert a["roofline"] is None and a["cpu_baseline"] is None and "rbpf" not in a and "sync_tick_ms" not in a
    b = _plain_run(tmp_path / "b", 20)
    for name, shape in (("controls", (2,)), ("control_sequence", (2, 50))):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float64 and x.shape == shape and np.all(np.isfinite(x))
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=0)
