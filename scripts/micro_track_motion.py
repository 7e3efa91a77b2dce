"""Camera-motion compensation (detr_hip_track_motion): its three launches on their own, and what a frame of Detector.track costs with
and without it.

--kernel-only: no model.  --streams videos of --size H W frames (seeded texture, every second frame the scene moved by a few
thumbnail pixels, so that every block votes), frames already on the device; --steps calls of detr_hip_track_motion back to back on
one prebuilt descriptor, HIP events around the lot: thumbnail + block matching + finalise, the ctypes call included.  Run under a
kernel trace for the kernels' own times:
  rocprofv3 --kernel-trace --stats -d OUT -o motion -- python scripts/micro_track_motion.py --kernel-only --size 1080 1920

Default mode: --streams videos of --size frames through a Detector (100 queries, default canvas, bf16, random weights,
score_threshold 0), Detector.track with a plain Tracker and with Tracker(motion=True), alternating frame by frame inside one
process, each with its own tracker over the same frames; a frame is timed with the host clock around a call that ends in a device
synchronise.  Figures: median and p10 - p90 over --steps frames after --warmup.  --plain-only times the plain tracker alone (the
form that also runs on a tree from before the motion launches, for an A/B on the same machine).

  python scripts/micro_track_motion.py [--streams 1] [--size 720 1280] [--radius 8] [--steps 40] [--warmup 5] [--kernel-only] [--plain-only]
"""
import argparse
import json
import os
import sys
import time
from ctypes import byref

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "detr-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def video(streams, h, w, frames, step):
    """frames x streams uint8 [h, w, 3]: crops of one seeded scene of 4 x 4-pixel blocks per stream, moved by `step` pixels in x and y
    on every second frame."""
    out = [[] for _ in range(frames)]
    for s in range(streams):
        rng = np.random.default_rng(s)
        small = rng.integers(0, 256, ((h + step + 3) // 4, (w + step + 3) // 4, 3), dtype=np.uint8)
        big = np.repeat(np.repeat(small, 4, axis=0), 4, axis=1)
        for f in range(frames):
            o = step * (f % 2)
            out[f].append(np.ascontiguousarray(big[o:o + h, o:o + w]))
    return out


def summary(ms):
    a = np.array(ms)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90))}


def kernel_only(args):
    from detr_tf import _hip as hip
    from detr_tf.inference import Tracker
    S, (h, w) = args.streams, args.size
    f = max(1, -(-w // hip.MOTION_SIDE), -(-h // hip.MOTION_SIDE))
    tracker = Tracker(S, motion=True, motion_radius=args.radius, min_hits=1)
    frames = video(S, h, w, 2, 3 * f)
    nbytes = h * w * 3
    bufs = [torch.from_numpy(np.concatenate([im.reshape(-1) for im in fr])).cuda() for fr in frames]
    meta = torch.from_numpy(np.concatenate([(np.arange(S, dtype=np.int64) * nbytes).view(np.uint8),
                                            np.tile(np.array([h, w], np.int32), S).view(np.uint8)])).cuda()
    out = torch.zeros(S + 1, 6, dtype=torch.int32, device="cuda")
    descs = []
    for buf in bufs:
        d = hip.TrackMotionDesc()
        d.S, d.frames, d.frames_bytes, d.offsets, d.sizes = S, buf.data_ptr(), buf.numel(), meta.data_ptr(), meta.data_ptr() + 8 * S
        d.active, d.radius = tracker._all_active.data_ptr(), args.radius
        d.motion_state, d.motion_state_bytes = tracker._motion.data_ptr(), tracker._motion.numel()
        d.state, d.state_bytes = tracker._state.data_ptr(), tracker._state.numel()
        d.workspace, d.workspace_bytes = tracker._votes.data_ptr(), tracker._votes.numel()
        d.out_motion, d.status = out.data_ptr(), out.data_ptr() + 24 * S
        descs.append(d)
    lib, stream = hip.load(), hip._stream()
    for i in range(args.warmup):
        hip._check(lib.detr_hip_track_motion(byref(descs[i % 2]), stream), "detr_hip_track_motion")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(args.warmup, args.warmup + args.steps):
        lib.detr_hip_track_motion(byref(descs[i % 2]), stream)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"mode": "kernel-only", "streams": S, "frame": [h, w], "radius": args.radius, "f": f, "steps": args.steps,
                      "last_out_motion": out[:S].tolist()[:2], "status": int(out[S, 0]),
                      "events_us_per_call_three_launches": e0.elapsed_time(e1) * 1e3 / args.steps, "gpu": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--size", type=int, nargs=2, default=(720, 1280), metavar=("H", "W"))
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--precision", default="bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_track_motion.py needs a GPU")
    if args.kernel_only:
        return kernel_only(args)
    from detr_tf.inference import Detector, Tracker
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.training_config import TrainingConfig

    S, (h, w) = args.streams, args.size
    cfg = TrainingConfig()
    cfg.background_class = 91
    model = get_detr_model(cfg, include_top=True, seed=0, dropout=0.0, precision=args.precision)
    det = Detector(model, cfg, score_threshold=0.0, max_detections=100)
    frames = video(S, h, w, 4, 12)
    first = det(frames[0])
    thr = float(np.median(np.concatenate([d.scores.cpu().numpy() for d in first])))
    trackers = {"plain": Tracker(S, track_threshold=thr, min_hits=2)}
    if not args.plain_only:
        trackers["motion"] = Tracker(S, track_threshold=thr, min_hits=2, motion=True, motion_radius=args.radius)
    wall = {k: [] for k in trackers}
    for i in range(args.warmup + args.steps):
        for name, tracker in trackers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            det.track(frames[i % 4], tracker)
            torch.cuda.synchronize()
            if i >= args.warmup:
                wall[name].append((time.perf_counter() - t0) * 1e3)
    result = {"streams": S, "frame": [h, w], "radius": args.radius, "precision": args.precision, "steps": args.steps, "warmup": args.warmup,
              "gpu": torch.cuda.get_device_name(0)}
    for name, tracker in trackers.items():
        result[name] = summary(wall[name])
        result[name + "_live_tracks"] = (tracker.state_dict()["id"] > 0).sum(1).tolist()
    if "motion" in trackers:
        result["last_motion"] = trackers["motion"].last_motion.tolist()[:2]
        result["motion_minus_plain_ms"] = result["motion"]["median_ms"] - result["plain"]["median_ms"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
