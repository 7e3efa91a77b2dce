"""Hand-worked tracking scenarios shared by tests/test_track_cpu.py (which pins tests/track_ref.py on them) and tests/test_gpu_track.py
(which replays them on the device).  A scenario is (tracker parameters, frames); a frame is a list of (box xyxy, label, score)."""
import numpy as np

import track_ref as R

F = np.float32


def square(x, y=100.0, side=40.0):
    return (x, y, x + side, y + side)


def moving(frames, visible=lambda f: True, score=lambda f: 0.9, step=4.0, label=1):
    """The 40 x 40 box that moves `step` pixels per frame in x."""
    return [[(square(50.0 + step * f), label, score(f))] if visible(f) else [] for f in range(frames)]


GAP = range(20, 25)                                                       # the five frames the box is missing in


def scenarios():
    far = (square(600.0, 400.0), 1, 0.5)                                  # another object, only ever seen at a low score
    both = [(square(50.0), 1, 0.9), (square(50.0), 2, 0.9)]
    out = {
        "steady": ({}, moving(30)),
        "gap": ({}, moving(30, lambda f: f not in GAP)),
        "gap_no_velocity": (dict(beta=0.0), moving(30, lambda f: f not in GAP)),
        "gap_max_age_4": (dict(max_age=4), moving(30, lambda f: f not in GAP)),
        "score_dip": ({}, [fr + [far] for fr in moving(16, score=lambda f: 0.5 if 8 <= f < 12 else 0.9)]),
        "unconfirmed_miss": ({}, moving(8, lambda f: f != 1)),
        "two_labels": ({}, [both if f % 2 == 0 else both[::-1] for f in range(8)]),
        "two_labels_agnostic": (dict(class_agnostic=True), [both if f % 2 == 0 else both[::-1] for f in range(8)]),
        "tie_lower_id": (dict(min_hits=1), [[((0, 0, 40, 40), 1, 0.9), ((16, 0, 56, 40), 1, 0.9)], [((8, 0, 48, 40), 1, 0.9)]]),
        "tie_lower_index": (dict(min_hits=1), [[((0, 0, 40, 40), 1, 0.9)], [((0, 0, 40, 40), 1, 0.9), ((0, 0, 40, 40), 1, 0.9)]]),
        "overflow": (dict(min_hits=1), [[(square(50.0 * (i % 20), 50.0 * (i // 20)), 1, 0.9) for i in range(257)]] * 2),
    }
    return out


def arrays(frame):
    """(boxes float32 [n, 4], labels int64 [n], scores float32 [n]) of a frame."""
    return (np.array([f[0] for f in frame], F).reshape(-1, 4), np.array([f[1] for f in frame], np.int64),
            np.array([f[2] for f in frame], F))


def run_ref(params, frames, tracker=None):
    """-> (tracker, [step results], [state_dict after every frame])"""
    t = R.RefTracker(**params) if tracker is None else tracker
    results, states = [], []
    for frame in frames:
        results.append(t.step(*arrays(frame)))
        states.append(t.state_dict())
    return t, results, states


def random_walk(seed, streams=3, frames=12, max_det=9, labels=4):
    """Seeded objects that drift, appear and vanish; scores on both sides of the thresholds; some frames are empty.
    -> [frame][stream] = (boxes, labels, scores)."""
    rng = np.random.default_rng(seed)
    out = []
    objs = [[] for _ in range(streams)]
    for f in range(frames):
        row = []
        for s in range(streams):
            keep = [o for o in objs[s] if rng.random() > 0.05]                            # deaths
            while len(keep) < max_det and rng.random() < 0.6:                            # births
                keep.append(dict(c=rng.uniform(40, 400, 2), wh=rng.uniform(20, 90, 2), v=rng.uniform(-6, 6, 2), label=int(rng.integers(labels))))
            objs[s] = keep
            boxes, lab, sc = [], [], []
            if rng.random() > 0.08:                                                       # else: a frame without detections
                for o in keep:
                    o["c"] = o["c"] + o["v"] + rng.normal(0, 1.0, 2)
                    if rng.random() < 0.08:
                        continue                                                           # a missed detection
                    wh = o["wh"] * rng.uniform(0.95, 1.05, 2)
                    boxes.append((o["c"][0] - wh[0] / 2, o["c"][1] - wh[1] / 2, o["c"][0] + wh[0] / 2, o["c"][1] + wh[1] / 2))
                    lab.append(o["label"])
                    sc.append(rng.choice([0.95, 0.8, 0.7, 0.6, 0.4], p=[0.35, 0.25, 0.15, 0.15, 0.1]))
            order = np.argsort(-np.array(sc, F), kind="stable") if sc else []
            row.append((np.array(boxes, F).reshape(-1, 4)[order], np.array(lab, np.int64)[order], np.array(sc, F)[order]))
        out.append(row)
    return out
