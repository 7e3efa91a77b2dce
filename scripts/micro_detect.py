"""Post-processing of one batch of model outputs into sorted, thresholded pixel-space detections, two ways, at B=8, Q=100, C=92:

  device   inference.detect_batched: one launch of detr_hip_detect + the counts read-back (what Detector runs)
  host     inference.get_model_inference_batched (one launch + counts), then per image the boxes / labels / scores copied to
           the host, bbox.np_rescale_bbox_xy_min_xy_max, the score threshold and a stable argsort in NumPy

Both start from the same device tensors and end with the results where their caller uses them (device: sliced device tensors,
counts known on the host; host: NumPy arrays).  The two ALTERNATE call by call inside one process; each call is timed with HIP
events on the current stream (the closing event is recorded after the call's host work) and with the host clock around a call
that ends in a device synchronise.  The figure is the median over --steps calls after --warmup calls; the results of both
paths are compared first.

  python scripts/micro_detect.py [--steps 300] [--warmup 30] [--batch 8] [--queries 100] [--classes 92] [--threshold 0.7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "detr-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--classes", type=int, default=92)
    ap.add_argument("--threshold", type=float, default=0.7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_detect.py needs a GPU")
    from detr_tf import bbox, inference

    B, Q, C = args.batch, args.queries, args.classes
    bg = C - 1
    rng = np.random.default_rng(0)
    logits = rng.normal(0.0, 1.0, (B, Q, C)).astype(np.float32)
    hot = rng.random((B, Q)) < 0.3                                  # ~30 % confident foreground queries, the rest background
    logits[hot, rng.integers(0, bg, int(hot.sum()))] += rng.uniform(4.0, 9.0, int(hot.sum())).astype(np.float32)
    logits[~hot, bg] += 8.0
    out = {"pred_logits": torch.from_numpy(logits).cuda(), "pred_boxes": torch.from_numpy(rng.random((B, Q, 4)).astype(np.float32)).cuda()}
    sizes = np.array([(480, 640), (1333, 800)] * B, np.int32)[:B]
    sizes_d = torch.from_numpy(sizes).cuda()

    def device():
        return inference.detect_batched(out, sizes_d, bg, score_threshold=args.threshold, bbox_format="xyxy")

    def host():
        res = []
        for (boxes, labels, scores), size in zip(inference.get_model_inference_batched(out, bg, "xyxy"), sizes):
            boxes, labels, scores = boxes.cpu().numpy(), labels.cpu().numpy(), scores.cpu().numpy()
            boxes = bbox.np_rescale_bbox_xy_min_xy_max(boxes, size)
            keep = np.nonzero(scores >= np.float32(args.threshold))[0]
            order = keep[np.argsort(-scores[keep], kind="stable")]
            res.append((boxes[order], labels[order], scores[order]))
        return res

    for d, (hb, hl, hs), size in zip(device(), host(), sizes):      # same detections, same order; boxes to fp32 rounding
        assert d.labels.tolist() == hl.tolist() and d.scores.cpu().numpy().tobytes() == hs.tobytes()
        assert np.abs(d.boxes.cpu().numpy() - hb).max(initial=0.0) <= 4 * np.spacing(np.float32(size.max()))
    kept = [int(d.scores.shape[0]) for d in device()]

    paths = {"device": device, "host": host}
    ev_ms = {k: [] for k in paths}
    wall_ms = {k: [] for k in paths}
    for i in range(args.warmup + args.steps):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= args.warmup:
                ev_ms[name].append(e0.elapsed_time(e1))
                wall_ms[name].append((t1 - t0) * 1e3)
    result = {"shape": [B, Q, C], "threshold": args.threshold, "kept_per_image": kept, "steps": args.steps, "warmup": args.warmup,
              "gpu": torch.cuda.get_device_name(0)}
    for name in paths:
        e, w = np.array(ev_ms[name]), np.array(wall_ms[name])
        result[name] = {"events_ms_median": float(np.median(e)), "events_ms_p10": float(np.percentile(e, 10)),
                        "events_ms_p90": float(np.percentile(e, 90)), "wall_ms_median": float(np.median(w))}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
