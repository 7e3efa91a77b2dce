"""Micro-benchmark: the key-padding-masked attention kernels at the encoder site (B = 8, 8 heads, T = S = 1050: a 25 x 42 feature
map) next to the unmasked ones, all-bf16 operands (csrc/attention_dma.hip) and exact fp32 (csrc/attention_f32.hip):
  unmasked | masked, every key valid | masked, ~30 % padding (rectangular, whole 32-key tiles skipped) | masked, random 30 %
and one masked B = 8 training step (bf16, 800 x 1333 canvas, mixed extents) next to the unmasked step.
usage: python scripts/micro_attn_mask.py [--no-step]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "detr-tensorflow_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

from detr_tf import _hip as hip

hip.load()
dev = "cuda"
H, D = 8, 256
step = torch.tensor([0x1234567, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)


def timeit(fn, inner=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(5):
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / inner * 1e3)
    return best


def masks(B, rng):
    grid = np.zeros((B, 25, 42), bool)          # ~30 % padding: 25 x 42 -> valid 21 x 35 (70 %)
    grid[:, :21, :35] = True
    return {"all valid": np.ones((B, 1050), bool), "rect 30%": grid.reshape(B, -1), "random 30%": rng.random((B, 1050)) >= 0.3}


B, T, S = 8, 1050, 1050
rng = np.random.default_rng(0)
print(f"attention at the encoder site, B{B} H{H} T{T} S{S} (us, best of 5 x 20)")
print(f"{'operands':8s} {'p':>4s} {'mask':12s}   fwd     bwd   (vs unmasked)")
for io in ("bf16", "fp32"):
    for p in (0.1, 0.0):
        torch.manual_seed(0)
        dt = torch.bfloat16 if io == "bf16" else torch.float32
        q, k, v, do = (torch.randn(B * n, D, device=dev).to(dt) for n in (T, S, S, T))
        o = torch.zeros(B * T, D, dtype=dt, device=dev)
        lse, delta = torch.zeros(B * H, T, device=dev), torch.zeros(2 * B * H, T, device=dev)
        dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
        dm = None
        if io == "bf16" and p > 0.0:
            dm = torch.zeros(hip.attention_dropmask_words(B, H, T, S), dtype=torch.int32, device=dev)
            hip.attention_dropmask(dm, B, H, T, S, dropout_p=p, dropout_site=3, dropout_step=step)
        kw = dict(scale=32 ** -0.5, dropout_p=p, dropout_site=3, dropout_step=step, dropmask=dm, compute=0)
        base = None
        for name, valid in [("unmasked", None)] + list(masks(B, rng).items()):
            kv = None if valid is None else torch.from_numpy(hip.keymask_words_from_valid(valid)).to(dev)
            f = timeit(lambda: hip.attention(q, k, v, o, lse, B, H, T, S, key_valid=kv, **kw))
            b = timeit(lambda: hip.attention(q, k, v, o, lse, B, H, T, S, key_valid=kv, d_o=do, dq=dq, dk=dk, dv=dv, delta=delta, **kw))
            if base is None:
                base = (f, b)
            print(f"{io:8s} {p:4.1f} {name:12s} {f:7.1f} {b:7.1f}   ({f / base[0]:.3f}x, {b / base[1]:.3f}x)")

if "--no-step" not in sys.argv:
    from detr_tf import training
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.optimizers import setup_optimizers
    from detr_tf.training_config import TrainingConfig
    from oracle import detr_ref as R, set_loss_ref as L
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
    cfg.target_batch = None
    model = get_detr_model(cfg, include_top=True, precision="bf16")
    model.load_weights(R.make_params(1))
    opt = setup_optimizers(model, cfg)
    Hc, Wc = 800, 1333
    extents = [(800, 1333), (800, 533), (600, 800), (800, 1200), (533, 800), (750, 1000), (800, 600), (480, 1333)]
    images = torch.from_numpy(rng.normal(size=(B, Hc, Wc, 3)).astype(np.float32)).to(dev)
    mk = np.ones((B, Hc, Wc), bool)
    for b, (h, w) in enumerate(extents):
        mk[b, :h, :w] = False
    mk = torch.from_numpy(mk).to(dev)
    t_bbox, t_class = L.make_targets(B, seed=3, force_full=False)
    t_bbox, t_class = torch.from_numpy(t_bbox).to(dev), torch.from_numpy(t_class).to(dev)
    for name, inp in (("unmasked", images), ("masked", (images, mk))):
        for _ in range(2):
            training.run_train_step(model, inp, t_bbox, t_class, opt, cfg)
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            training.run_train_step(model, inp, t_bbox, t_class, opt, cfg)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        print(f"bf16 eager training step B{B} {Hc}x{Wc} {name}: {best * 1e3:.2f} ms (forward + loss + backward, no optimiser)")
