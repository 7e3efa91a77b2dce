"""bench.py --dump-outputs: what the last timed step computed, written as DIR/<name>.npy (float32 / float64, 64 MB at most),
so that two builds can be compared output for output on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_every_array_and_samples_large_ones(tmp_path):
    import bench
    B, Q, C, levels = 2, 5, 92, 3
    g = torch.Generator().manual_seed(0)
    logits = [torch.randn(B, Q, C, generator=g) for _ in range(levels)]
    boxes = [torch.rand(B, Q, 4, generator=g) for _ in range(levels)]
    out = {"pred_logits": logits[-1], "pred_boxes": boxes[-1],
           "aux": [{"pred_logits": logits[i], "pred_boxes": boxes[i]} for i in range(levels - 1)]}
    log = {"giou_loss": torch.tensor(0.5), "label_cost": torch.tensor(1.25), "backbone_lr": 1e-5}
    params = torch.randn(bench.DUMP_MAX_ELEMS + 1000, generator=g)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, torch.tensor(3.5), log, params)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["aux_pred_boxes", "aux_pred_logits", "loss", "losses", "params", "pred_boxes", "pred_logits"]
    assert np.array_equal(a["pred_logits"], logits[-1].numpy()) and a["pred_logits"].dtype == np.float32
    assert np.array_equal(a["aux_pred_boxes"], torch.stack(boxes[:-1]).numpy())
    assert a["loss"].dtype == np.float64 and float(a["loss"]) == 3.5
    assert a["losses"].tolist() == [0.5, 1.25]                      # loss entries only, in the dict's order
    # a large array becomes a fixed sample of its values: the same in every run, within the size budget
    assert a["params"].shape == (bench.DUMP_MAX_ELEMS,) and np.isin(a["params"], params.numpy()).all()
    assert np.array_equal(a["params"], np.load(tmp_path / "b" / "params.npy"))
    assert sum(v.nbytes for v in a.values()) <= 64 << 20


@pytest.mark.gpu
def test_bench_dump_outputs_of_the_timed_steps(hip, tmp_path):
    """A tiny bench run: --steps sets the timed steps, the line carries ms_per_step, the dump holds the last timed step's outputs."""
    env = dict(os.environ)
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--height", "64",
                        "--width", "96", "--launch", "eager", "--no-cpu-baseline", "--no-fp32-leg", "--no-configs",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["steps"] == 2 and j["ms_per_step"] > 0
    d = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert d["pred_logits"].shape == (2, 100, 92) and d["pred_boxes"].shape == (2, 100, 4)
    assert d["aux_pred_logits"].shape == (5, 2, 100, 92) and d["losses"].shape == (36,)
    assert abs(float(d["loss"]) - j["loss"]) <= 1e-4 * abs(j["loss"])
    assert all(np.isfinite(v).all() and v.dtype in (np.float32, np.float64) for v in d.values())
