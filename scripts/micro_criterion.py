"""Micro-benchmark: the four set-loss launches that take a criterion (cost, sums, finalize, gradient; csrc/setloss.hip) through
the entry points with the reference's criterion compiled in and through the _crit_ ones (run-time values, with and without class
weights), at the benchmark's loss shape -- 6 levels, B = 8, Q = 100, C = 92, R = 100 -- timed with HIP events on the launch alone.
usage: python scripts/micro_criterion.py [--out FILE.json]"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "detr-tensorflow_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

from detr_tf import _hip as hip
from detr_tf.loss.hungarian_matching import Matcher, make_desc
from oracle import set_loss_ref as L

LV, B, Q, C, R = 6, 8, 100, 92, 100


def timeit(fn, inner=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(7):
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / inner * 1e3)
    return best


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    hip.load()
    rng = np.random.default_rng(0)
    t_bbox, t_class = L.make_targets(B, seed=1235, max_rows=R)
    tb = torch.from_numpy(t_bbox).cuda()
    tc = torch.from_numpy(t_class).reshape(B, R).cuda()
    lg = torch.from_numpy(rng.normal(size=(LV, B, Q, C)).astype(np.float32)).cuda()
    bx = torch.from_numpy(np.concatenate([rng.uniform(0.2, 0.8, (LV, B, Q, 2)), rng.uniform(0.05, 0.4, (LV, B, Q, 2))], -1).astype(np.float32)).cuda()
    d = make_desc(lg, bx, tb, tc, C - 1)
    m = Matcher(LV, B, Q, R, lg.device)
    tfp = m.run(d, tb)
    sums = torch.zeros(LV * 10, device="cuda")
    losses, total = torch.zeros(LV, 6, device="cuda"), torch.zeros(1, device="cuda")
    dl, db = torch.zeros_like(lg), torch.zeros_like(bx)
    crit = (ctypes.c_float * hip.CRITERION_FLOATS)(1.0, 5.0, 2.0, 1.0, 5.0, 2.0, 0.1, 0.0)
    cw = torch.from_numpy((rng.integers(16, 257, size=C) / 64.0).astype(np.float32)).cuda()
    one = ctypes.c_float(1.0)
    dp = ctypes.byref(d)
    hip.call("detr_hip_set_loss_sums_f32", dp, tfp.data_ptr(), sums.data_ptr())            # sums for finalize / gradient to read
    fixed = {
        "cost": lambda: hip.call("detr_hip_match_cost_f32", dp, m.cost.data_ptr()),
        "sums": lambda: hip.call("detr_hip_set_loss_sums_f32", dp, tfp.data_ptr(), sums.data_ptr()),
        "finalize": lambda: hip.call("detr_hip_set_loss_finalize_f32", sums.data_ptr(), LV, losses.data_ptr(), total.data_ptr()),
        "grad": lambda: hip.call("detr_hip_set_loss_grad_f32", dp, tfp.data_ptr(), sums.data_ptr(), one, dl.data_ptr(), db.data_ptr()),
    }

    def runtime(w):
        return {
            "cost": lambda: hip.call("detr_hip_match_cost_crit_f32", dp, crit, m.cost.data_ptr()),
            "sums": lambda: hip.call("detr_hip_set_loss_sums_crit_f32", dp, crit, w, tfp.data_ptr(), sums.data_ptr()),
            "finalize": lambda: hip.call("detr_hip_set_loss_finalize_crit_f32", sums.data_ptr(), LV, crit, losses.data_ptr(), total.data_ptr()),
            "grad": lambda: hip.call("detr_hip_set_loss_grad_crit_f32", dp, crit, w, tfp.data_ptr(), sums.data_ptr(), one, dl.data_ptr(),
                                     db.data_ptr()),
        }
    res = {"shape": f"Lv{LV} B{B} Q{Q} C{C} R{R}"}
    for tag, calls in (("fixed", fixed), ("crit", runtime(None)), ("crit_class_weights", runtime(cw.data_ptr()))):
        res[tag + "_us"] = {k: round(timeit(fn), 2) for k, fn in calls.items()}
        res[tag + "_us"]["all"] = round(sum(res[tag + "_us"].values()), 2)
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
