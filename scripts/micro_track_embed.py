"""detr_hip_track_embed (tracking by appearance) against detr_hip_track on the same rows, and against the host way it replaces.

No model: --detections D detections per stream on a grid, jittered every frame, an embedding of --embed-dim per detection (a unit
direction per object times a random length plus noise); --tracks T of the objects are tracked (born in a first frame), the others
score below new_threshold so that the number of live tracks stays T.  With T > D the tracks beyond D coast.  For every (streams,
tracks) pair of --streams x --tracks:

  track        --steps calls of detr_hip_track, back to back, HIP events around the lot; the descriptor is built once (through
               Tracker._launch) and re-issued through ctypes, so the figure is the kernel and the bare call, not torch allocations
  track_embed  the same with detr_hip_track_embed, appearance_weight 0.5, re-identification on; the two ALTERNATE in blocks
  host         what a user does without it: the frame's boxes, labels, scores and embeddings and the bank copied to the host, then
               NumPy: normalise, cosine matrix tracks x detections (host clock around the lot, it ends in the copies' synchronise)

  python scripts/micro_track_embed.py [--streams 1 8] [--tracks 10 200] [--detections 100] [--embed-dim 256] [--steps 200]
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


def captured_call(tracker, name, *rows, **kw):
    """Run tracker._launch once and return a closure that re-issues the same C call (same descriptor, same buffers)."""
    from detr_tf import _hip as hip
    lib, seen = hip.load(), []
    real = getattr(lib, name)

    def spy(dref, stream):
        seen.append(dref)
        return real(dref, stream)

    setattr(lib, name, spy)
    try:
        keep = tracker._launch(*rows, **kw)
    finally:
        setattr(lib, name, real)
    dref, stream = seen[0], hip._stream()

    def again():
        if real(dref, stream) != 0:
            raise RuntimeError(lib.detr_hip_last_error().decode())
    again.keep = keep
    return again


def case(S, T, D, E, steps, warmup):
    from detr_tf.inference import Tracker
    rng = np.random.default_rng(0)
    N = max(T, D)
    base = np.array([(50.0 * (i % 20), 50.0 * (i // 20), 50.0 * (i % 20) + 40.0, 50.0 * (i // 20) + 40.0) for i in range(N)], F)
    look = rng.normal(0, 1, (N, E))
    look /= np.linalg.norm(look, axis=1, keepdims=True)
    params = dict(min_hits=1, new_threshold=0.95, max_age=10 ** 6)
    trackers = {"track": Tracker(S, **params), "track_embed": Tracker(S, embed_dim=E, **params)}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    labels_n = np.tile(np.arange(N) % 4, (S, 1))
    birth = (dev(np.stack([base[:T]] * S)), dev(labels_n[:, :T]), torch.full((S, T), 0.99, device="cuda"), dev(np.tile(np.arange(T, dtype=np.int32), (S, 1))),
             torch.full((S,), T, dtype=torch.int32, device="cuda"))
    birth_emb = dev(np.stack([look[:T].astype(F)] * S))
    trackers["track"].update_rows(*birth)
    trackers["track_embed"].update_rows(*birth, embeddings=birth_emb)
    labels, scores = dev(labels_n[:, :D]), torch.full((S, D), 0.9, device="cuda")
    query = dev(np.tile(np.arange(D, dtype=np.int32), (S, 1)))
    counts = torch.full((S,), D, dtype=torch.int32, device="cuda")
    boxes = dev(np.stack([base[:D] + rng.uniform(-3, 3, (D, 4)).astype(F) for _ in range(S)]))
    emb = dev(np.stack([(rng.uniform(0.5, 4.0, (D, 1)) * (look[:D] + rng.normal(0, 0.1 / np.sqrt(E), (D, E)))).astype(F) for _ in range(S)]))
    calls = {}
    for name, tr in trackers.items():
        kw = dict(embeddings=emb) if name == "track_embed" else {}
        calls[name] = captured_call(tr, "detr_hip_" + name, boxes, labels, scores, query, counts, tr._active(None), **kw)
    times = {name: [] for name in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    block = max(steps // 4, 1)
    for name in calls:
        for _ in range(warmup):
            calls[name]()
    for _ in range(4):                                             # alternate the two in blocks
        for name, fn in calls.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(block):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / block)
    bank = trackers["track_embed"]._bank
    host = []
    for _ in range(max(steps // 10, 5)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b, la, sc, em, bk = boxes.cpu().numpy(), labels.cpu().numpy(), scores.cpu().numpy(), emb.cpu().numpy(), bank.cpu().numpy()
        for s in range(S):
            n = em[s].astype(np.float64)
            n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
            sim = bk[s, :T].astype(np.float64) @ n.T
        host.append((time.perf_counter() - t0) * 1e6)
    state = trackers["track_embed"].state_dict()
    same = all(state[k].tobytes() == v.tobytes() for k, v in trackers["track"].state_dict().items() if k in ("id", "hits", "miss"))
    return {"streams": S, "tracks": T, "detections": D, "embed_dim": E, "calls_per_block": block,
            "live_tracks_per_stream": (state["id"] > 0).sum(1).tolist(), "same_ids_hits_miss_as_track": bool(same),
            "track_us": [round(t, 2) for t in times["track"]], "track_embed_us": [round(t, 2) for t in times["track_embed"]],
            "host_readback_cosine_us_median": round(float(np.median(host)), 1), "sim_shape": list(sim.shape)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--tracks", type=int, nargs="+", default=[10, 200])
    ap.add_argument("--detections", type=int, default=100)
    ap.add_argument("--embed-dim", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_track_embed.py needs a GPU")
    for S in args.streams:
        for T in args.tracks:
            print(json.dumps(dict(case(S, T, args.detections, args.embed_dim, args.steps, args.warmup), gpu=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
