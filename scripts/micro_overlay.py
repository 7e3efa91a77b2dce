"""Drawing the detections of one batch onto its frames, at B = 8 frames of 1080 x 1920 with 100 detections each:

  device        one call of detr_hip_overlay (overlay.plan_overlay once, overlay.launch_overlay per call): frames and detections are
                on the device and stay there
  device+heat   the same with a 34 x 60 attention heat map under the boxes
  device+odd    the same as device from a source packed at odd byte offsets (what DeviceInputStage uploads for odd-sized frames)
  copy          a device-to-device copy of the same frame bytes: the kernel reads and writes 3 bytes per pixel, so this is its floor
  host          what a user does without the kernel: frames and detections read back, every box drawn by the NumPy slicing code of
                tests/overlay_ref.py (the restatement the tests compare the kernel with), heat map excluded

The four ALTERNATE step by step inside one process.  A device step is --inner calls between two HIP events on the current stream
(time per call = elapsed / inner); the host path is timed with the host clock round a step that starts from device tensors.  The
figures are medians over --steps steps after --warmup steps; device and host results are compared first, byte for byte.

  python scripts/micro_overlay.py [--steps 50] [--warmup 5] [--inner 10] [--host-steps 3] [--batch 8] [--height 1080] [--width 1920] [--boxes 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "detr-tensorflow_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--boxes", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_overlay.py needs a GPU")
    import overlay_ref as R
    from detr_tf import overlay as O

    B, H, W, K = args.batch, args.height, args.width, args.boxes
    rng = np.random.default_rng(0)
    frames_h = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(B)]
    names = [f"class {i}" for i in range(91)]
    dets = []
    for _ in range(B):                                               # boxes of every size, as a detector's top 100 are
        cx, cy = rng.uniform(0, W, K), rng.uniform(0, H, K)
        w, h = rng.uniform(0.02, 0.5, K) * W, rng.uniform(0.02, 0.5, K) * H
        boxes = np.clip(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1), 0, [W, H, W, H]).astype(np.float32)
        dets.append((torch.from_numpy(boxes).cuda(), torch.from_numpy(rng.integers(0, 91, K)).cuda(), torch.from_numpy(rng.random(K).astype(np.float32)).cuda()))
    packed = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames_h])).cuda()
    frames = O.RaggedFrames(packed, np.arange(B, dtype=np.int64) * (H * W * 3), [(H, W)] * B)
    heat = torch.from_numpy(rng.random((B, 34, 60)).astype(np.float32) ** 4).cuda()
    copy_dst = torch.empty_like(packed)

    plain = O.plan_overlay(frames, dets, names)
    heated = O.plan_overlay(frames, dets, names, heat=heat)
    shifted = torch.empty(packed.numel() + 1, dtype=torch.uint8, device=packed.device)
    shifted[1:] = packed
    odd = O.plan_overlay(O.RaggedFrames(shifted, frames.offsets + 1, frames.sizes), dets, names)

    def host():
        out = []
        font, glyphs = O.font_atlas(), (ord("0") - 32, ord(":") - 32, ord(".") - 32)
        coded = [O.encode_text(n) for n in names]
        palette = O.class_palette(100)
        for img, (bx, lb, sc) in zip(frames.views(), dets):
            out.append(R.draw_image(img.cpu().numpy(), bx.cpu().numpy(), lb.cpu().numpy(), sc.cpu().numpy(), names=coded, colors=palette, atlas=font,
                                    glyphs=glyphs, thickness=2, scale=O.default_scale(H)))
        return out

    O.launch_overlay(plain[0])
    torch.cuda.synchronize()
    want = host()
    O.launch_overlay(odd[0])
    for got, got_odd, ref in zip(plain[2], odd[2], want):
        assert (got.cpu().numpy() == ref).all() and (got_odd.cpu().numpy() == ref).all(), "device and host drawings differ"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.inner              # microseconds per call

    paths = {"device": lambda: O.launch_overlay(plain[0]), "device+heat": lambda: O.launch_overlay(heated[0]),
             "device+odd": lambda: O.launch_overlay(odd[0]), "copy": lambda: copy_dst.copy_(packed)}
    times = {k: [] for k in paths}
    for step in range(args.warmup + args.steps):
        for k, fn in paths.items():
            t = timed(fn)
            if step >= args.warmup:
                times[k].append(t)
    host_t = []
    for _ in range(args.host_steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        host_t.append((time.perf_counter() - t0) * 1e6)
    med = {k: float(np.median(v)) for k, v in times.items()}
    nbytes = 2 * B * H * W * 3
    result = {"shape": {"batch": B, "height": H, "width": W, "boxes": K}, "bytes_read_and_written": nbytes,
              "us": {k: round(v, 1) for k, v in med.items()}, "us_min": {k: round(float(np.min(v)), 1) for k, v in times.items()},
              "us_max": {k: round(float(np.max(v)), 1) for k, v in times.items()},
              "GBps": {k: round(nbytes / v / 1e3, 1) for k, v in med.items()},
              "ratio_to_copy": {k: round(med[k] / med["copy"], 2) for k in ("device", "device+heat", "device+odd")},
              "host_us": round(float(np.median(host_t)), 1), "host_over_device": round(float(np.median(host_t)) / med["device"], 1)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
