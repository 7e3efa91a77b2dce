"""What DC5 costs: (a) the dilated bf16 3x3 kernel at layer4's DC5 shape against the dense kernel on the contiguous tensor of the same
work, (b) the whole training step of resnet50-dc5 next to resnet50 (B = 8, 800 x 1333, bf16, dropout 0.1) with peak device memory.

    python scripts/bench_dc5.py --kernel            # one JSON line: microseconds and the ratio
    python scripts/bench_dc5.py --step [--batch 8]  # one JSON line per backbone
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


def _time_us(fn, warmup=20, reps=200):
    """Median of `reps` event-timed launches after `warmup`, flushing nothing: the operands (< 40 MB) stay L2 / MALL-warm for both sides."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


def bench_kernel():
    from detr_tf import _hip as hip
    hip.load()
    dev = "cuda"
    N, H, W, C = 8, 50, 84, 512
    gen = torch.Generator().manual_seed(0)
    b16 = lambda *s: torch.randn(*s, generator=gen).to(dev).to(torch.bfloat16)
    x, dy, w, msk = b16(N, H, W, C), b16(N, H, W, C), (b16(3, 3, C, C) / 64), b16(N, H, W, C)
    bias = torch.randn(C, generator=gen).to(dev)
    y = torch.empty(N, H, W, C, device=dev, dtype=torch.bfloat16)
    xs, ys = x.view(4 * N, H // 2, W // 2, C), y.view(4 * N, H // 2, W // 2, C)       # the same bytes as 32 dense 25 x 42 maps
    dys, ms = dy.view(4 * N, H // 2, W // 2, C), msk.view(4 * N, H // 2, W // 2, C)
    out = {}
    out["dilated_fwd_us"] = _time_us(lambda: hip.conv3x3(0, x, w, y, N, H, W, C, H, W, C, 1, pad=2, bias=bias, act=1, compute=1, dilation=2))
    out["dense_fwd_us"] = _time_us(lambda: hip.conv3x3(0, xs, w, ys, 4 * N, H // 2, W // 2, C, H // 2, W // 2, C, 1, bias=bias, act=1, compute=1))
    out["dilated_dgrad_us"] = _time_us(lambda: hip.conv3x3(1, dy, w, y, N, H, W, C, H, W, C, 1, pad=2, mask=msk, compute=1, dilation=2))
    out["dense_dgrad_us"] = _time_us(lambda: hip.conv3x3(1, dys, w, ys, 4 * N, H // 2, W // 2, C, H // 2, W // 2, C, 1, mask=ms, compute=1))
    out["fwd_ratio"] = out["dilated_fwd_us"] / out["dense_fwd_us"]
    out["dgrad_ratio"] = out["dilated_dgrad_us"] / out["dense_dgrad_us"]
    print(json.dumps({"bench": "dc5_kernel", "shape": [N, H, W, C], **{k: round(v, 3) for k, v in out.items()}}))


def bench_step(batch, steps, warmup):
    from detr_tf import training
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.optimizers import setup_optimizers
    from detr_tf.training_config import TrainingConfig
    from oracle import set_loss_ref as L
    for backbone in ("resnet50", "resnet50-dc5"):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        cfg = TrainingConfig()
        cfg.background_class = 91
        cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
        cfg.target_batch = None
        model = get_detr_model(cfg, include_top=True, backbone=backbone, precision="bf16", dropout=0.1, device="cuda:0")
        opt = setup_optimizers(model, cfg)
        images = torch.from_numpy(np.random.default_rng(0).normal(size=(batch, 800, 1333, 3)).astype(np.float32)).cuda()
        t_bbox, t_class = L.make_targets(batch, seed=5, force_full=False)

        def step():
            _, _, _, steps_ = training.run_train_step(model, images, t_bbox, t_class, opt, cfg)
            for name in steps_:
                training.aggregate_grad_and_apply(name, opt, steps_[name]["gradients"], 0, cfg)
        try:
            for _ in range(warmup):
                step()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                step()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / steps
            print(json.dumps({"bench": "dc5_step", "backbone": backbone, "batch": batch, "ms_per_step": round(ms, 2),
                              "images_per_s": round(batch / ms * 1e3, 1), "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))
        except torch.cuda.OutOfMemoryError:
            print(json.dumps({"bench": "dc5_step", "backbone": backbone, "batch": batch, "error": "out of memory"}))
        del model, opt


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.kernel:
        bench_kernel()
    if a.step:
        bench_step(a.batch, a.steps, a.warmup)
