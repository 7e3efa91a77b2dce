"""The cross-tile merge of sliced inference, two ways, at B=8 images, 3 x 3 tiles + the full view (N = 80 tiles), Q=100, C=92:

  device   inference.merge_tiles: ONE launch of detr_hip_tile_merge for the batch + one read-back (counts and status)
  host     the loop a user writes: get_model_inference_batched over the N tiles (one launch + counts), every tile's boxes / labels /
           scores copied to the host, then per image NumPy mapping to image pixels, the score threshold, a stable argsort and a
           greedy class-wise NMS (vectorised IoU of the current box against the rest) -- B host loops

Both start from the same device tensors (seeded synthetic outputs that leave a few hundred candidates per image).  The two ALTERNATE
call by call inside one process; each call is timed with HIP events on the current stream (the closing event is recorded after the
call's host work) and with the host clock around a call that ends in a device synchronise.  The figure is the median over --steps
calls after --warmup calls; the results of both paths are compared first (reported as paths_agree_to_the_bit).  Also printed: candidates and survivors per image -- the
device walk takes ONE workgroup barrier per survivor.

  python scripts/micro_tiles.py [--steps 200] [--warmup 20] [--batch 8] [--grid 3] [--queries 100] [--classes 92] [--threshold 0.7]
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


def host_nms(boxes, labels, scores, thr, K):
    """Greedy class-wise NMS on the host: boxes float32 [n, 4] xyxy sorted by descending score."""
    alive = np.ones(len(boxes), bool)
    b = boxes.astype(np.float64)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    keep = []
    for i in range(len(b)):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) == K:
            break
        r = slice(i + 1, None)
        iw = np.clip(np.minimum(b[i, 2], b[r, 2]) - np.maximum(b[i, 0], b[r, 0]), 0, None)
        ih = np.clip(np.minimum(b[i, 3], b[r, 3]) - np.maximum(b[i, 1], b[r, 1]), 0, None)
        inter = iw * ih
        den = area[i] + area[r] - inter
        iou = np.divide(inter, den, out=np.zeros_like(inter), where=den != 0)
        alive[r] &= ~((labels[r] == labels[i]) & (iou > thr))
    return np.array(keep, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--grid", type=int, default=3)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--classes", type=int, default=92)
    ap.add_argument("--threshold", type=float, default=0.7)
    ap.add_argument("--nms", type=float, default=0.5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_tiles.py needs a GPU")
    from detr_tf import inference
    from detr_tf.data import transformation as T

    B, Q, C, K = args.batch, args.queries, args.classes, 100
    bg = C - 1
    sizes = np.array([(3000, 4000), (2160, 3840)] * B, np.int32)[:B]
    recs = [T.tile_records(h, w, args.grid, args.grid) for h, w in sizes]
    tile_start = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32)
    windows = np.array([(t.y0, t.x0, t.hc, t.wc) for r in recs for t in r], np.int32)
    N = int(tile_start[-1])
    rng = np.random.default_rng(0)
    logits = rng.normal(0.0, 1.0, (N, Q, C)).astype(np.float32)
    hot = rng.random((N, Q)) < 0.3                                  # ~30 % confident foreground queries, the rest background
    logits[hot, rng.integers(0, 20, int(hot.sum()))] += rng.uniform(4.0, 9.0, int(hot.sum())).astype(np.float32)
    logits[~hot, bg] += 8.0
    boxes = np.concatenate([rng.random((N, Q, 2)), rng.uniform(0.05, 0.5, (N, Q, 2))], -1).astype(np.float32)
    out = {"pred_logits": torch.from_numpy(logits).cuda(), "pred_boxes": torch.from_numpy(boxes).cuda()}
    sizes_d, windows_d = torch.from_numpy(sizes).cuda(), torch.from_numpy(windows).cuda()

    def device():
        return inference.merge_tiles(out, tile_start, windows_d, sizes_d, bg, score_threshold=args.threshold, max_detections=K,
                                     nms_threshold=args.nms)

    def host():
        per_tile = [(b.cpu().numpy(), l.cpu().numpy(), s.cpu().numpy()) for b, l, s in inference.get_model_inference_batched(out, bg, "xy_center")]
        res, cand = [], []
        for i in range(B):
            bs, ls, ss = [], [], []
            for n in range(tile_start[i], tile_start[i + 1]):
                b, l, s = per_tile[n]
                y0, x0, hc, wc = windows[n].astype(np.float32)
                cx, cy, w, h = x0 + b[:, 0] * wc, y0 + b[:, 1] * hc, b[:, 2] * wc, b[:, 3] * hc
                xyxy = np.stack([cx - w * np.float32(0.5), cy - h * np.float32(0.5), cx + w * np.float32(0.5), cy + h * np.float32(0.5)], 1)
                xyxy = np.clip(xyxy, 0, np.array([sizes[i, 1], sizes[i, 0]] * 2, np.float32))
                bs.append(xyxy), ls.append(l), ss.append(s)
            b, l, s = np.concatenate(bs), np.concatenate(ls), np.concatenate(ss)
            sel = np.nonzero(s >= np.float32(args.threshold))[0]
            order = sel[np.argsort(-s[sel], kind="stable")]
            keep = order[host_nms(b[order], l[order], s[order], args.nms, K)]
            res.append((b[keep], l[keep], s[keep]))
            cand.append(len(sel))
        return res, cand

    dev, (hst, cand) = device(), host()
    agree = all(d.labels.tolist() == hl.tolist() and d.scores.cpu().numpy().tobytes() == hs.tobytes() and
                d.boxes.cpu().numpy().tobytes() == hb.tobytes() for d, (hb, hl, hs) in zip(dev, hst))      # same detections, same order
    # survivors of the whole walk (no cap) = barriers an image takes when max_detections does not cut it short
    uncapped = [int(d.scores.shape[0]) for d in inference.merge_tiles(out, tile_start, windows_d, sizes_d, bg, score_threshold=args.threshold,
                                                                      max_detections=2048, nms_threshold=args.nms)]

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
    result = {"shape": [B, N, Q, C], "tiles_per_image": int(tile_start[1]), "threshold": args.threshold, "nms_threshold": args.nms,
              "max_detections": K, "candidates_per_image": cand, "kept_per_image": [int(d.scores.shape[0]) for d in dev],
              "survivors_uncapped_per_image": uncapped, "steps": args.steps, "warmup": args.warmup, "gpu": torch.cuda.get_device_name(0), "paths_agree_to_the_bit": agree}
    for name in paths:
        e, w = np.array(ev_ms[name]), np.array(wall_ms[name])
        result[name] = {"events_ms_median": float(np.median(e)), "events_ms_p10": float(np.percentile(e, 10)),
                        "events_ms_p90": float(np.percentile(e, 90)), "wall_ms_median": float(np.median(w))}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
