"""bench.py's plain run (no --full): the headline alone, --steps timed steps, and --dump-outputs DIR with what the last
timed step returned — the same arrays again for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "3",
                        "--dump-outputs", str(out_dir)] + list(extra), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_dumps_the_last_forward(tmp_path):
    d = _bench(tmp_path / "a")
    assert d["metric"] == "graphs_per_sec" and d["unit"] == "graphs/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 40 and d["warmup"] == 3 and d["ms_per_step"] > 0
    assert abs(d["value"] - 1.0 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]      # cfg 2: one graph per step
    for k in ("ms_per_forward", "h2d_inclusive_graphs_per_sec", "roofline", "cpu_baseline", "multi_stream",
              "floorplans_sized"):
        assert d[k] is None, "%s measured without --full" % k
    a = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("pred_cls", "bbox")}
    assert a["pred_cls"].dtype == np.float32 and a["pred_cls"].shape == (400, 17) and np.isfinite(a["pred_cls"]).all()
    assert a["bbox"].dtype == np.float32 and a["bbox"].shape == (400, 4)
    _bench(tmp_path / "b")
    for n, want in a.items():
        np.testing.assert_allclose(np.load(str(tmp_path / "b" / (n + ".npy"))), want, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_plain_train_bench_run_dumps_the_loss_and_the_stepped_parameters(tmp_path):
    d = _bench(tmp_path, "--mode", "train")
    assert d["metric"] == "train_graphs_per_sec" and d["steps"] == 40 and d["ms_per_step"] > 0
    assert d["cpu_baseline"] is None and d["roofline"] is None
    loss = np.load(str(tmp_path / "loss.npy"))
    assert loss.dtype == np.float32 and loss.shape == () and np.isfinite(loss)
    params = [f for f in os.listdir(str(tmp_path)) if f.startswith("param.")]
    assert "param.cls_net.head.gconv.nn.0.weight.npy" in params
    assert all(np.isfinite(np.load(str(tmp_path / f))).all() for f in params)
