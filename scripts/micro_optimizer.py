"""Optimiser phase of the training step (engine.phase("optimizer") .. "end", HIP events on the main stream) at the bench
shape -- DETR-R50 bf16, batch 8, 800x1333 -- for the three optimiser configurations:

  default      three Adam(clipnorm): 2 launches per group
  joint        config.global_clipnorm = 0.1: partial sums, finalize, one update for all groups
  joint+decay  the same with config.weight_decay = 1e-4

The configurations ALTERNATE step by step inside one process (same model, same batch), so box-to-box and drift effects
hit all three alike; the figure is the median over --steps steps each, after --warmup rounds.  The launches of the phase
are counted at the binding (every kernel goes through detr_tf._hip.call), hyper-parameter writes included.

  python scripts/micro_optimizer.py [--steps 20] [--warmup 3] [--batch 8] [--height 800] [--width 1333]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "detr-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = (("default", None, 0.0), ("joint", 0.1, 0.0), ("joint+decay", 0.1, 1e-4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--precision", default="bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_optimizer.py needs a GPU")
    from bench import make_targets
    from detr_tf import _hip, training
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.optimizers import setup_optimizers
    from detr_tf.training_config import TrainingConfig

    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.batch_size, cfg.target_batch = args.batch, None
    cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
    model = get_detr_model(cfg, include_top=True, device="cuda:0", seed=0, dropout=0.1, precision=args.precision)
    opt = setup_optimizers(model, cfg)
    rng = np.random.default_rng(1234)
    images = torch.from_numpy(rng.normal(size=(args.batch, args.height, args.width, 3)).astype(np.float32)).cuda()
    tb, tc = make_targets(args.batch, np.random.default_rng(1235))
    tb, tc = torch.from_numpy(tb).cuda(), torch.from_numpy(tc).cuda()

    counting = {"on": False, "names": []}
    real_call = _hip.call

    def counted(name, *a):
        if counting["on"]:
            counting["names"].append(name)
        return real_call(name, *a)
    _hip.call = counted
    real_phase = model.engine.phase

    def phase(name):
        counting["on"] = name == "optimizer"
        real_phase(name)
    model.engine.phase = phase

    ms = {n: [] for n, _, _ in CONFIGS}
    launches = {}
    for i in range(args.warmup + args.steps):
        for name, clip, wd in CONFIGS:
            cfg.global_clipnorm, cfg.weight_decay = clip, wd
            model.engine.phase_events = []
            counting["names"] = []
            training.train_step(model, images, tb, tc, opt, cfg, i)
            torch.cuda.synchronize()
            evs = dict(model.engine.phase_events)
            model.engine.phase_events = None
            if i >= args.warmup:
                ms[name].append(evs["optimizer"].elapsed_time(evs["end"]))
                launches[name] = list(counting["names"])
    out = {"shape": f"R50 {args.precision} B{args.batch} {args.height}x{args.width}", "steps": args.steps,
           "parameters": int(model.engine.P.total)}
    for name, _, _ in CONFIGS:
        v = sorted(ms[name])
        out[name] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
                     "launches": len(launches[name]),
                     "kernels": len([n for n in launches[name] if not n.startswith("detr_hip_set_floats")])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
