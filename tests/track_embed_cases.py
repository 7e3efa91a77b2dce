"""Scenarios of tracking by appearance, shared by tests/test_track_embed_cpu.py (which pins tests/track_embed_ref.py on them) and
tests/test_gpu_track_embed.py (which replays them on the device).  A scenario is (tracker parameters incl. embed_dim, frames); a frame
is a list of (box xyxy, label, score, embedding).  A packed frame, what the trackers take, is (boxes, labels, scores, query, embeddings
[R, E]): the embedding of detection d is row query[d]."""
import numpy as np

import track_cases as C
import track_embed_ref as ER

F = np.float32
MARGIN = 1e-6                    # what random_walk leaves between any two numbers a decision hangs on (see there)


def axis(E, k, scale=1.0):
    """scale * the k-th unit vector: orthogonal embeddings with exact arithmetic."""
    v = np.zeros(E, F)
    v[k] = scale
    return v


def arrays(frame, E):
    """(boxes, labels, scores, query, embeddings) of a frame; the embedding rows stand in REVERSE order, so that query matters."""
    n = len(frame)
    emb = np.array([f[3] for f in frame][::-1], F).reshape(n, E)
    return C.arrays(frame) + (np.arange(n, dtype=np.int32)[::-1].copy(), emb)


def run_ref(params, frames, tracker=None):
    """-> (tracker, [step results], [state_dict after every frame])"""
    t = ER.RefEmbedTracker(**params) if tracker is None else tracker
    results, states = [], []
    for frame in frames:
        results.append(t.step(*arrays(frame, t.E)))
        states.append(t.state_dict())
    return t, results, states


A_BOX, B_BOX = (0, 0, 40, 40), (16, 0, 56, 40)


def swap(E=8):
    """Two objects of one label whose detections stand at each other's place in the second frame."""
    a, b = axis(E, 0, 3.0), axis(E, 1, 0.5)
    return [[(A_BOX, 1, 0.9, a), (B_BOX, 1, 0.9, b)], [(A_BOX, 1, 0.9, b), (B_BOX, 1, 0.9, a)]]


def occlusion(E=8, back=None):
    """An object seen for 6 frames, missing for 10, and back 200 px away (with the embedding `back`, its own by default)."""
    own = axis(E, 2, 2.0) + axis(E, 5, 1.0)
    back = own if back is None else back
    seen = [[(C.square(50.0 + 4.0 * f), 1, 0.9, own)] for f in range(6)]
    return seen + [[] for _ in range(10)] + [[(C.square(50.0 + 4.0 * f + 200.0), 1, 0.9, back)] for f in range(16, 20)]


def low_score(E=8):
    """A confirmed track that is carried by stage 2 for two frames, by detections that look different."""
    own, other = axis(E, 0), axis(E, 3)
    return [[(C.square(50.0 + 4.0 * f), 1, 0.5 if f in (4, 5) else 0.9, other if f in (4, 5) else own)] for f in range(8)]


def twins(E=8):
    """Deliberate ties: bit-equal boxes AND embeddings, so every m of a frame is the same number."""
    e = axis(E, 1) + axis(E, 2)
    return [[(A_BOX, 1, 0.9, e)] * 3, [(A_BOX, 1, 0.9, e)] * 4, [(A_BOX, 1, 0.9, e)] * 2]


def scenarios():
    E = 8
    return {
        "swap_w0.5": (dict(embed_dim=E, min_hits=1), swap(E)),
        "swap_w0": (dict(embed_dim=E, min_hits=1, appearance_weight=0.0, reid_threshold=None), swap(E)),
        "swap_w1": (dict(embed_dim=E, min_hits=1, appearance_weight=1.0), swap(E)),
        "occlusion_reid": (dict(embed_dim=E), occlusion(E)),
        "occlusion_reid_off": (dict(embed_dim=E, reid_threshold=None), occlusion(E)),
        "occlusion_other_object": (dict(embed_dim=E), occlusion(E, back=axis(E, 2, 1.0) + axis(E, 6, 2.0))),
        "low_score": (dict(embed_dim=E), low_score(E)),
        "twins": (dict(embed_dim=E, min_hits=1), twins(E)),
        "twins_agnostic_reid": (dict(embed_dim=E, min_hits=1, class_agnostic=True, reid_threshold=0.5), twins(E) + [[]] + twins(E)),
        "overflow": (dict(embed_dim=E, min_hits=1), [[fr + (axis(E, i % E),) for i, fr in enumerate(C.scenarios()["overflow"][1][0])]] * 2),
    }


# the tracker parameters the GPU tests run the random walks with; random_walk holds every one of them to MARGIN
WALK_PARAMS = {
    "defaults": {},
    "agnostic_w0.8": dict(class_agnostic=True, appearance_weight=0.8, reid_threshold=0.6),
    "min_hits1_momentum0": dict(min_hits=1, max_age=3, momentum=0.0, reid_threshold=0.7),
    "w0_reid": dict(appearance_weight=0.0, new_threshold=0.75, min_hits=2),
}
WALK_SEEDS = {4: 20, 32: 20, 68: 20, 256: 20}        # embed_dim -> a seed that random_walk accepts


def random_walk(seed, E, streams=3, frames=12, max_det=9, labels=3):
    """track_cases.random_walk with an appearance: every object draws a direction, and every detection of it is that direction times a
    random length plus small noise; objects also JUMP now and then, further than any IoU gate reaches, which is what re-identification
    is for.  The embedding rows of a frame are shuffled (and two rows belong to nothing), the detections name theirs by query.
    -> [frame][stream] = (boxes, labels, scores, query, embeddings [R, E]).

    The device is compared with the reference bit for bit.  The one assumption behind that which nothing here can check off the device
    is that its fp64 sqrt and division round correctly; should they not, a similarity could differ in its last bits and flip a decision
    that hangs on less than that.  So this generator runs the reference with every WALK_PARAMS and ASSERTS that no two competing m or
    sim values, and no sim and its threshold, are closer than MARGIN -- ten orders of magnitude above an fp64 ulp -- in any walk it
    returns: a seed that fails is not committed."""
    rng = np.random.default_rng(seed)
    out = []
    objs = [[] for _ in range(streams)]
    for f in range(frames):
        row = []
        for s in range(streams):
            keep = [o for o in objs[s] if rng.random() > 0.05]                            # deaths
            while len(keep) < max_det and rng.random() < 0.6:                            # births
                e = rng.normal(0, 1, E)
                keep.append(dict(c=rng.uniform(40, 400, 2), wh=rng.uniform(20, 90, 2), v=rng.uniform(-6, 6, 2), label=int(rng.integers(labels)),
                                 e=e / np.linalg.norm(e)))
            objs[s] = keep
            boxes, lab, sc, emb = [], [], [], []
            if rng.random() > 0.08:                                                       # else: a frame without detections
                for o in keep:
                    o["c"] = o["c"] + o["v"] + rng.normal(0, 1.0, 2)
                    if rng.random() < 0.12:
                        o["c"] = o["c"] + rng.choice([-1.0, 1.0], 2) * rng.uniform(120, 200, 2)      # a jump
                    if rng.random() < 0.08:
                        continue                                                           # a missed detection
                    wh = o["wh"] * rng.uniform(0.95, 1.05, 2)
                    boxes.append((o["c"][0] - wh[0] / 2, o["c"][1] - wh[1] / 2, o["c"][0] + wh[0] / 2, o["c"][1] + wh[1] / 2))
                    lab.append(o["label"])
                    sc.append(rng.choice([0.95, 0.8, 0.7, 0.6, 0.4], p=[0.35, 0.25, 0.15, 0.15, 0.1]))
                    emb.append(rng.uniform(0.5, 8.0) * (o["e"] + rng.normal(0, 0.1 / np.sqrt(E), E)))
            n = len(sc)
            order = np.argsort(-np.array(sc, F), kind="stable") if sc else []
            where = rng.permutation(n + 2)[:n].astype(np.int32)                           # the row of every (sorted) detection
            rows = rng.normal(0, 1, (n + 2, E)).astype(F)
            if n:
                rows[where] = np.array(emb, F)[order]
            row.append((np.array(boxes, F).reshape(-1, 4)[order], np.array(lab, np.int64)[order], np.array(sc, F)[order], where, rows))
        out.append(row)
    for name, params in WALK_PARAMS.items():
        for s in range(streams):
            ref = ER.RefEmbedTracker(embed_dim=E, **params)
            for fr in out:
                ref.step(*fr[s])
            assert not ref.gaps or min(ref.gaps) >= MARGIN, (seed, E, name, s, min(ref.gaps))
    return out
