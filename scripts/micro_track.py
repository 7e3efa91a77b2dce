"""Tracking a batch of video streams, the device way against the host way it replaces, and the tracker kernel on its own.

Default mode, --streams 8 videos of 720 x 1280 frames through a Detector (100 queries, default canvas, bf16) with random weights,
score_threshold 0 so that every non-background query is a detection, track_threshold at the median score of the first frame:

  call     Detector.__call__                                       (what a frame cost before there was a tracker)
  track    Detector.track: the same + ONE launch of detr_hip_track, one host synchronisation in all
  host     Detector.__call__, every field copied to the host, then per stream the association in NumPy: fp64 IoU matrix of
           tracks x detections, label and threshold masks, the pairs sorted by (descending IoU, id, detection), a greedy walk

The three ALTERNATE frame by frame inside one process, each with its own tracker state over the same frames; a frame is timed with
the host clock around a call that ends in a device synchronise.  Figures: median and p10 - p90 over --steps frames after --warmup.
The ids of `track` and `host` are compared first (reported as ids_agree).

--kernel-only N: no model.  --streams trackers' worth of N objects on a grid, jittered every frame, D = N detections per stream,
--steps launches of detr_hip_track back to back (HIP events around the lot); --cluster puts every box on one spot with one label, so
that every (track, detection) pair is a candidate: the association's worst case.  Run under a kernel trace for the kernel's own time:
  rocprofv3 --kernel-trace --stats -d OUT -o track -- python scripts/micro_track.py --kernel-only 100

  python scripts/micro_track.py [--streams 8] [--steps 40] [--warmup 5] [--kernel-only N [--cluster]]
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

F = np.float32


class HostTracker:
    """The algorithm of detr_hip_track (include/detr_hip.h) for one stream in vectorised NumPy, the way a user would write it."""

    def __init__(self, track_threshold=0.7, new_threshold=None, match_threshold=0.3, low_match_threshold=0.5, max_age=30, min_hits=3,
                 alpha=0.75, beta=0.25):
        self.p = dict(thr=F(track_threshold), new=F(track_threshold if new_threshold is None else new_threshold), match=match_threshold,
                      low=low_match_threshold, max_age=max_age, min_hits=min_hits, alpha=F(alpha), beta=F(beta))
        self.x, self.v = np.zeros((0, 4), F), np.zeros((0, 4), F)
        self.label, self.id = np.zeros(0, np.int64), np.zeros(0, np.int64)
        self.hits, self.miss, self.conf = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool)
        self.next_id = 1

    @staticmethod
    def _iou(a, b):
        a, b = a.astype(np.float64)[:, None, :], b.astype(np.float64)[None, :, :]
        iw = np.clip(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), 0, None)
        ih = np.clip(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), 0, None)
        inter = iw * ih
        den = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter
        return np.divide(inter, den, out=np.zeros_like(inter), where=den != 0)

    def _walk(self, iou, rows, cols, thr, t_det, d_trk):
        ok = np.zeros(iou.shape, bool)
        ok[np.ix_(rows, cols)] = True
        t, d = np.nonzero(ok & (iou > thr))
        for k in np.lexsort((d, self.id[t], -iou[t, d])):
            if t_det[t[k]] < 0 and d_trk[d[k]] < 0:
                t_det[t[k]], d_trk[d[k]] = d[k], t[k]

    def step(self, boxes, labels, scores):
        p, half = self.p, F(0.5)
        pred = self.x + self.v
        pred[:, 2:] = np.where(pred[:, 2:] < 0, F(0), pred[:, 2:])
        corners = np.concatenate([pred[:, :2] - pred[:, 2:] * half, pred[:, :2] + pred[:, 2:] * half], 1)
        z = np.concatenate([(boxes[:, :2] + boxes[:, 2:]) * half, boxes[:, 2:] - boxes[:, :2]], 1)
        high = scores >= p["thr"]
        iou = self._iou(corners, boxes)
        iou[self.label[:, None] != labels[None, :]] = -1.0
        t_det, d_trk = np.full(len(pred), -1), np.full(len(boxes), -1)
        self._walk(iou, np.arange(len(pred)), np.nonzero(high)[0], p["match"], t_det, d_trk)
        self._walk(iou, np.nonzero((t_det < 0) & self.conf & (self.miss == 0))[0], np.nonzero(~high)[0], p["low"], t_det, d_trk)
        m = t_det >= 0
        r = z[t_det[m]] - pred[m]
        self.x, self.v = pred, self.v.copy()
        self.x[m], self.v[m] = pred[m] + p["alpha"] * r, self.v[m] + p["beta"] * r
        self.hits[m] += 1
        self.miss = np.where(m, 0, self.miss + 1)
        self.conf |= self.hits >= p["min_hits"]
        keep = m | (self.conf & (self.miss <= p["max_age"]))
        born = np.nonzero((d_trk < 0) & high & (scores >= p["new"]))[0]
        slot = np.cumsum(keep) - 1                                     # where a kept track lands
        sel = d_trk >= 0
        d_trk[sel] = np.where(keep[d_trk[sel]], slot[d_trk[sel]], -1)
        d_trk[born] = keep.sum() + np.arange(len(born))
        n = len(born)
        self.x, self.v = np.concatenate([self.x[keep], z[born]]), np.concatenate([self.v[keep], np.zeros((n, 4), F)])
        self.label, self.id = np.concatenate([self.label[keep], labels[born]]), np.concatenate([self.id[keep], self.next_id + np.arange(n)])
        self.hits, self.miss = np.concatenate([self.hits[keep], np.ones(n, np.int64)]), np.concatenate([self.miss[keep], np.zeros(n, np.int64)])
        self.conf = np.concatenate([self.conf[keep], np.full(n, p["min_hits"] <= 1)])
        self.next_id += n
        out = np.nonzero(d_trk >= 0)[0]
        out = out[self.conf[d_trk[out]]]
        return out, self.id[d_trk[out]]


def summary(ms):
    a = np.array(ms)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90))}


def kernel_only(args, N):
    from detr_tf.inference import Tracker
    S = args.streams
    rng = np.random.default_rng(0)
    base = np.array([(50.0 * (i % 20), 50.0 * (i // 20), 50.0 * (i % 20) + 40.0, 50.0 * (i // 20) + 40.0) for i in range(N)], F)
    if args.cluster:                                               # the worst case: every box on one spot, one label: every pair is a candidate
        base = np.tile(np.array([[100.0, 100.0, 300.0, 300.0]], F), (N, 1)) + rng.uniform(-10, 10, (N, 4)).astype(F)
    tracker = Tracker(S, min_hits=1)
    labels = torch.from_numpy(np.tile(np.arange(N) % (1 if args.cluster else 4), (S, 1))).cuda()
    scores = torch.full((S, N), 0.9, dtype=torch.float32, device="cuda")
    query = torch.zeros(S, N, dtype=torch.int32, device="cuda")
    counts = torch.full((S,), N, dtype=torch.int32, device="cuda")
    frames = [torch.from_numpy(np.stack([base + rng.uniform(-3, 3, (N, 4)).astype(F) for _ in range(S)])).cuda() for _ in range(8)]
    emitted = tracker.update_rows(torch.from_numpy(np.stack([base] * S)).cuda(), labels, scores, query, counts)       # births
    active = tracker._active(None)
    for i in range(args.warmup):
        tracker._launch(frames[i % 8], labels, scores, query, counts, active)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(args.steps):
        tracker._launch(frames[i % 8], labels, scores, query, counts, active)
    e1.record()
    torch.cuda.synchronize()
    state = tracker.state_dict()
    print(json.dumps({"mode": "kernel-only", "clustered": bool(args.cluster), "streams": S, "tracks": N, "detections": N, "steps": args.steps,
                      "live_tracks_per_stream": (state["id"] > 0).sum(1).tolist(), "ids_issued": int(state["next_id"][0]) - 1,
                      "emitted_first_frame": [int(t.ids.shape[0]) for t in emitted],
                      "events_us_per_call_launch_path_included": e0.elapsed_time(e1) * 1e3 / args.steps, "gpu": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N")
    ap.add_argument("--cluster", action="store_true", help="--kernel-only: all boxes overlap each other (the association's worst case)")
    ap.add_argument("--precision", default="bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_track.py needs a GPU")
    if args.kernel_only:
        return kernel_only(args, args.kernel_only)
    from detr_tf.inference import Detector, Tracker
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.training_config import TrainingConfig

    S = args.streams
    cfg = TrainingConfig()
    cfg.background_class = 91
    model = get_detr_model(cfg, include_top=True, seed=0, dropout=0.0, precision=args.precision)
    det = Detector(model, cfg, score_threshold=0.0, max_detections=100)
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (S, 720, 1280, 3)).astype(np.int16)
    video = [[np.clip(im + rng.integers(-4, 5, im.shape), 0, 255).astype(np.uint8) for im in base] for _ in range(4)]
    first = det(video[0])
    thr = float(np.median(np.concatenate([d.scores.cpu().numpy() for d in first])))
    params = dict(track_threshold=thr, min_hits=2)
    dev_tracker = Tracker(S, **params)
    host_trackers = [HostTracker(**params) for _ in range(S)]
    ids = {"track": [], "host": []}

    def call(frames):
        return det(frames)

    def track(frames):
        ids["track"].append([t.ids.tolist() for t in det.track(frames, dev_tracker)])

    def host(frames):
        row = []
        for d, h in zip(det(frames), host_trackers):
            out, tid = h.step(d.boxes.cpu().numpy(), d.labels.cpu().numpy(), d.scores.cpu().numpy())
            row.append(tid.tolist())
        ids["host"].append(row)

    paths = {"call": call, "track": track, "host": host}
    wall = {k: [] for k in paths}
    for i in range(args.warmup + args.steps):
        frames = video[i % 4]
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(frames)
            torch.cuda.synchronize()
            if i >= args.warmup:
                wall[name].append((time.perf_counter() - t0) * 1e3)
    state = dev_tracker.state_dict()
    result = {"streams": S, "frame": [720, 1280], "queries": 100, "precision": args.precision, "steps": args.steps, "warmup": args.warmup,
              "track_threshold": thr, "detections_per_stream_first_frame": [int(d.scores.shape[0]) for d in first],
              "live_tracks_per_stream": (state["id"] > 0).sum(1).tolist(), "emitted_last_frame": [len(r) for r in ids["track"][-1]],
              "ids_agree": ids["track"] == ids["host"], "gpu": torch.cuda.get_device_name(0)}
    for name in paths:
        result[name] = summary(wall[name])
    result["track_minus_call_ms"] = result["track"]["median_ms"] - result["call"]["median_ms"]
    result["host_minus_call_ms"] = result["host"]["median_ms"] - result["call"]["median_ms"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
