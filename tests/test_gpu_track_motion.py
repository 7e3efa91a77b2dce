"""detr_hip_track_motion (csrc/track_motion.hip) in front of the trackers against its NumPy restatement (tests/track_motion_ref.py,
pinned by tests/test_track_motion_cpu.py), EXACTLY: after every frame out_motion, the bytes of the motion state (the header and both
thumbnail slots), the bytes of the whole track state and the emitted rows."""
import numpy as np
import pytest
import torch

import track_cases as C
import track_embed_ref as ER
import track_motion_cases as MC
import track_motion_ref as M
import track_ref as R
from test_gpu_detect import _config, _same, model  # noqa: F401  (the tiny model of the detector's tests)
from test_track_motion_cpu import run_ref, scenarios

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


def _tracker(streams=1, **params):
    from detr_tf.inference import Tracker
    return Tracker(streams, DEV, **params)


def _frames_as(images, how):
    """The three forms frames= takes: host arrays, device tensors, a RaggedFrames."""
    from detr_tf.overlay import RaggedFrames
    if how == 0:
        return list(images)
    if how == 1:
        return [torch.from_numpy(np.ascontiguousarray(im)).to(DEV) for im in images]
    sizes = [im.shape[:2] for im in images]
    nbytes = np.array([im.size for im in images], np.int64)
    offsets = np.zeros(len(images), np.int64)
    offsets[1:] = np.cumsum(nbytes + 5)[:-1]                                   # a gap: the frames need no alignment
    buf = np.zeros(int(offsets[-1] + nbytes[-1]), np.uint8)
    for im, o in zip(images, offsets):
        buf[o:o + im.size] = im.reshape(-1)
    return RaggedFrames(torch.from_numpy(buf).to(DEV), offsets, sizes)


def _pack(dets, E=None):
    """dets: per stream (boxes, labels, scores[, embeddings [k, E]]) -> padded device rows, host counts, embeddings or None."""
    S = len(dets)
    counts = np.array([len(d[0]) for d in dets], np.int32)
    D = max(int(counts.max()), 1)
    boxes, labels, scores, query = np.zeros((S, D, 4), F), np.zeros((S, D), np.int64), np.zeros((S, D), F), np.zeros((S, D), np.int32)
    emb = None if E is None else np.zeros((S, D, E), F)
    for s, d in enumerate(dets):
        k = counts[s]
        boxes[s, :k], labels[s, :k], scores[s, :k], query[s, :k] = d[0], d[1], d[2], np.arange(k)
        if E is not None:
            emb[s, :k] = d[3]
    return [torch.from_numpy(a).to(DEV) for a in (boxes, labels, scores, query)], counts, None if E is None else torch.from_numpy(emb).to(DEV)


def _step(tracker, images, dets, active=None, how=0):
    """One frame through the tracker's own launch path -> ([per stream the six emitted arrays], status word, out_motion [S, 6])."""
    rows, n, emb = _pack(dets, tracker.embed_dim)
    out, tail = tracker._launch(*rows, torch.from_numpy(n).to(DEV), tracker._active(active), emb, _frames_as(images, how))
    *k, status = tail.tolist()
    host = [r.cpu().numpy() for r in out]
    for s in range(len(dets)):
        assert all(not r[s, k[s]:].any() for r in host), "the rows behind the count are zero"
    motion = tracker.last_motion.cpu().numpy()
    assert motion.dtype == np.int32 and motion.shape == (len(dets), 6)
    return [tuple(r[s, :k[s]] for r in host) for s in range(len(dets))], status, motion


def _same_rows(got, want):
    for name, g, w in zip(("boxes", "labels", "scores", "query", "ids", "hits"), got, want[:6]):
        w = np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, g, w)


def _same_state(tracker, trackers, motions):
    """The bytes of the whole track state (and of the bank) and of the whole motion state."""
    got = tracker.state_dict()
    embed = tracker.embed_dim is not None
    want = dict((ER if embed else R).stack_states(trackers), **M.stack_motion(motions))
    assert set(got) == set(want) == set(ER.KEYS if embed else R.KEYS) | {"motion_head", "motion_thumb"}
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (k, np.argwhere(g != w)[:5])
    free = got["id"] == 0                                                       # a free slot is zero bytes, whatever moved around it
    assert all(not got[k][free].any() for k in ("x", "v", "label", "hits", "miss", "confirmed", "score"))


class _Side:
    """The reference of one stream: a RefMotion in front of a RefTracker / RefEmbedTracker."""

    def __init__(self, radius, params, embed_dim=None):
        self.mo = M.RefMotion(radius)
        self.tr = R.RefTracker(**params) if embed_dim is None else ER.RefEmbedTracker(embed_dim, **params)

    def step(self, image, det, bad=False):
        out = self.mo.step(image, self.tr.s, bad=bad)
        query = np.arange(len(det[0]), dtype=np.int32)
        return out, self.tr.step(det[0], det[1], det[2], query, *det[3:])


def _replay(radius, params, videos, dets, active=None, embed_dim=None, tracker=None, sides=None):
    """videos[s][f] an image, dets[s][f] = (boxes, labels, scores[, embeddings]); active[f][s] or None.  Device and reference side by
    side, compared after every frame; the frames go in as host arrays, device tensors and RaggedFrames in turn."""
    S = len(videos)
    extra = {} if embed_dim is None else dict(embed_dim=embed_dim)
    tracker = _tracker(S, motion=True, motion_radius=radius, **extra, **params) if tracker is None else tracker
    sides = [_Side(radius, params, embed_dim) for _ in range(S)] if sides is None else sides
    motions = []
    for f in range(len(videos[0])):
        act = None if active is None else active[f]
        got, status, motion = _step(tracker, [v[f] for v in videos], [d[f] for d in dets], act, how=f % 3)
        assert status == 0
        for s in range(S):
            if act is not None and not act[s]:
                assert all(len(g) == 0 for g in got[s]) and not motion[s].any()     # six zeros, nothing emitted
                continue
            want_motion, want = sides[s].step(videos[s][f], dets[s][f])
            assert motion[s].tolist() == want_motion.tolist(), (f, s, motion[s], want_motion)
            assert want[6] == 0
            _same_rows(got[s], want)
        _same_state(tracker, [sd.tr for sd in sides], [sd.mo for sd in sides])
        motions.append(motion)
    return tracker, sides, motions


# ---- every scenario of the CPU tests, replayed -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(scenarios()))
def test_motion_replays_the_cpu_scenarios(hip, name):
    sc = scenarios()[name]
    tracker, sides, motions = _replay(sc["radius"], sc["params"], [sc["frames"]], [[C.arrays(d) for d in sc["dets"]]])
    steps = run_ref(name)                                                      # what the CPU tests pinned, frame by frame
    assert [m[0].tolist() for m in motions] == [s[0].tolist() for s in steps]
    assert sides[0].tr.state_dict()["x"].tobytes() == steps[-1][4]["x"].tobytes()


def test_motion_jitter_keeps_the_id_the_plain_tracker_loses(hip):
    sc = scenarios()["jitter"]
    with_motion, plain = _tracker(motion=True, motion_radius=16), _tracker()
    ids, lost = [], []
    for image, det in zip(sc["frames"], sc["dets"]):
        rows, n, _ = _pack([C.arrays(det)])
        counts = torch.from_numpy(n).to(DEV)
        ids.append(with_motion.update_rows(*rows, counts, frames=[image])[0].ids.tolist())
        lost.append(plain.update_rows(*rows, counts)[0].ids.tolist())
    assert lost == [[]] * 8 and ids == [[], []] + [[1]] * 6
    assert with_motion.last_motion.tolist() == [[1, 32, -32, 100, 100, 2]] and plain.last_motion is None


# ---- several streams, mixed sizes, one of them without a frame ----------------------------------------------------------------------
def test_motion_three_streams_of_mixed_sizes_and_an_inactive_one(hip):
    names = ("b_80x100_r8", "resize", "cut")                                   # 80 x 100, 80 x 100 -> 96 x 100, 80 x 100; three frames each
    sc = [scenarios()[n] for n in names]
    assert {s["radius"] for s in sc} == {8} and {len(s["frames"]) for s in sc} == {3}
    videos = [s["frames"] + s["frames"][::-1] for s in sc]
    videos[2] = [MC.video(3, 401, 778, [(0, 0)])[0]] + videos[2][1:]            # and a frame of f = 3 among them, then a size change
    dets = [[C.arrays(d) for d in s["dets"] + s["dets"][::-1]] for s in sc]
    active = [[1, 1, 1], [1, 0, 1], [0, 1, 1], [1, 1, 0], [1, 1, 1], [1, 0, 1]]
    tracker, sides, motions = _replay(8, dict(min_hits=1), videos, dets, active=active)
    assert [int(sd.mo.m["head"][6]) for sd in sides] == [1, 0, 1]               # the slot flips once per delivered frame: 5, 4, 5 of them
    assert sum(int(m[s][0]) for m in motions for s in range(3)) >= 6            # estimates were made and applied


@pytest.mark.parametrize("radius", [1, 16])
def test_motion_smallest_and_largest_radius(hip, radius):
    shifts = [(0, 0), (radius, -radius), (radius - 1, 0), (0, 0)]
    video = MC.video(20 + radius, 80, 100, shifts)
    dets = [C.arrays(d) for d in MC.follow(shifts)]
    tracker, sides, motions = _replay(radius, dict(min_hits=1), [video], [dets])
    gx, gy = M.geometry(80, 100, radius)[3:]
    assert (gx, gy) == ((6, 4) if radius == 1 else (4, 3))
    assert [m[0].tolist() for m in motions[1:]] == [[1, radius, -radius, gx * gy, gx * gy, 1], [1, -1, radius, gx * gy, gx * gy, 1],
                                                     [1, 1 - radius, 0, gx * gy, gx * gy, 1]]


# ---- the state the shift is applied to -----------------------------------------------------------------------------------------------
def _scattered_state():
    """Live slots among free ones, far apart: the first, a middle one, the last; with velocities, sizes and fractions to round."""
    ref = R.RefTracker(min_hits=1)
    st = ref.state_dict()
    for i, t in enumerate((0, 5, 130, 255)):
        st["id"][t], st["hits"][t], st["confirmed"][t], st["label"][t], st["score"][t] = 7 + i, 2, True, 1 + i % 2, F(0.9)
        st["x"][t] = (F(60.0) + F(0.1) * F(i), F(50.0) + F(1e7) * F(i == 3), 40, 40)        # near 1e7 floats are whole numbers: every half is rounded
        st["v"][t] = (F(0.25), F(-0.5), 0, 0)
    st["next_id"] = np.int32(11)
    return st


def test_motion_moves_live_slots_only_and_leaves_free_ones_zero(hip):
    sc = scenarios()["b_80x100_r8"]
    tracker = _tracker(motion=True, motion_radius=8, min_hits=1)
    fresh = tracker.state_dict()
    tracker.load_state_dict(dict(fresh, **{k: np.asarray(v)[None] for k, v in _scattered_state().items()}))
    side = _Side(8, dict(min_hits=1))
    side.tr.load_state_dict(_scattered_state())
    before = side.tr.state_dict()
    empty = (np.zeros((0, 4), F), np.zeros(0, np.int64), np.zeros(0, F))
    _replay(8, dict(min_hits=1), [sc["frames"][:2]], [[empty, empty]], tracker=tracker, sides=[side])
    after = side.tr.state_dict()
    live = before["id"] >= 1
    assert live.sum() == 4 and (after["id"] == before["id"]).all()               # confirmed: they coast
    # x = (x + v) on frame 0; x = ((x + shift) + v) on frame 1, the shift (5, -7) added first and rounded on its own
    for t in np.flatnonzero(live):
        x0 = before["x"][t, :2] + before["v"][t, :2]
        assert after["x"][t, :2].tobytes() == ((x0 + np.array([5, -7], F)) + before["v"][t, :2]).astype(F).tobytes()
        assert after["x"][t, 2:].tolist() == [40, 40] and after["v"][t].tobytes() == before["v"][t].tobytes()
    assert after["x"][255, 1] == F(1e7) + F(50.0) - F(0.5) - F(7) - F(0.5)


def test_motion_with_appearance_tracking(hip):
    rng = np.random.default_rng(31)
    shifts = [(0, 0), (5, -7), (0, 0), (-6, 3), (-6, 3)]
    video = MC.video(32, 80, 100, shifts)
    emb = rng.normal(size=(2, 8)).astype(F)
    dets = [C.arrays(d) + ((emb + rng.normal(scale=0.05, size=emb.shape)).astype(F),) for d in MC.follow(shifts)]
    params = dict(min_hits=1, appearance_weight=0.5, reid_threshold=0.8, momentum=0.9)
    tracker, sides, motions = _replay(8, params, [video], [dets], embed_dim=8)
    assert [m[0, :3].tolist() for m in motions] == [[0, 0, 0], [1, 5, -7], [1, -5, 7], [1, -6, 3], [1, 0, 0]]
    assert sides[0].tr.state_dict()["hits"][:2].tolist() == [5, 5] and sides[0].tr.bank[:2].any()


def test_motion_resumes_and_reruns_bit_identically(hip):
    shifts = [(0, 0), (3, 1), (-2, 5), (4, 4), (0, -2), (1, 1)]
    video, dets = MC.video(33, 96, 128, shifts), [C.arrays(d) for d in MC.follow(shifts)]
    tracker, sides, _ = _replay(8, {}, [video[:3]], [dets[:3]])
    saved = tracker.state_dict()
    assert saved["motion_head"].shape == (1, 16) and saved["motion_thumb"].shape == (1, 2, 384 * 384)
    runs = []
    for _ in range(2):                                                         # two runs from one loaded state
        other = _tracker(motion=True)
        other.load_state_dict(saved)
        outs = [_step(other, [im], [d]) for im, d in zip(video[3:], dets[3:])]
        runs.append((outs, other.state_dict()))
    (a_out, a_state), (b_out, b_state) = runs
    assert all(x.tobytes() == y.tobytes() for fa, fb in zip(a_out, b_out) for x, y in zip(fa[0][0] + (fa[2],), fb[0][0] + (fb[2],)))
    assert set(a_state) == set(b_state) and all(a_state[k].tobytes() == b_state[k].tobytes() for k in a_state)
    for f in range(3, 6):                                                      # and it equals the uninterrupted run
        sides[0].step(video[f], dets[f])
    _same_state(other, [sides[0].tr], [sides[0].mo])
    assert [o[2][0, :3].tolist() for o in a_out] == [[1, 6, -1], [1, -4, -6], [1, 1, 3]]
    with pytest.raises(ValueError, match="motion_head"):
        other.load_state_dict({k: v for k, v in saved.items() if k != "motion_head"})
    other.reset()                                                              # a reset zeroes the motion state: the next frame has no predecessor
    state = other.state_dict()
    assert not state["motion_head"].any() and not state["motion_thumb"].any()
    assert _step(other, [video[4]], [dets[4]])[2].tolist() == [[0, 0, 0, 0, 0, 1]]


def test_motion_refuses_a_frame_outside_its_buffer(hip):
    from detr_tf.overlay import RaggedFrames
    sc = scenarios()["b_80x100_r8"]
    tracker, side = _tracker(motion=True, min_hits=1), _Side(8, dict(min_hits=1))
    dets = [C.arrays(d) for d in sc["dets"]]
    _replay(8, dict(min_hits=1), [sc["frames"][:1]], [dets[:1]], tracker=tracker, sides=[side])
    short = RaggedFrames(torch.from_numpy(sc["frames"][1].reshape(-1)[:-1].copy()).to(DEV), [0], [(80, 100)])     # one byte is missing
    rows, n, _ = _pack([dets[1]])
    out, tail = tracker._launch(*rows, torch.from_numpy(n).to(DEV), tracker._active(None), None, short)
    assert tail.tolist()[-1] == M.BAD_FRAME and tracker.last_motion.tolist() == [[0, 0, 0, 0, 0, 1]]
    side.step(sc["frames"][1], dets[1], bad=True)                              # run as 0 x 0: no pixel read, no estimate, the header says so
    _same_state(tracker, [side.tr], [side.mo])
    with pytest.raises(ValueError, match="does not lie inside"):
        tracker.update_rows(*rows, torch.from_numpy(n).to(DEV), frames=short)


def test_frames_argument_is_mandatory_with_motion_and_refused_without(hip):
    sc = scenarios()["a_36x36_r2"]
    rows, n, _ = _pack([C.arrays(sc["dets"][0])])
    counts = torch.from_numpy(n).to(DEV)
    with pytest.raises(ValueError, match="mandatory with motion"):
        _tracker(motion=True).update_rows(*rows, counts)
    with pytest.raises(ValueError, match="refused without"):
        _tracker().update_rows(*rows, counts, frames=sc["frames"][:1])
    two = _tracker(2, motion=True)
    both = [t.expand(2, *t.shape[1:]).contiguous() for t in rows]
    with pytest.raises(ValueError, match="1 frames for 2 streams"):
        two.update_rows(*both, counts.expand(2).contiguous(), frames=sc["frames"][:1])
    with pytest.raises(TypeError, match="Tracker: frames"):
        _tracker(motion=True).update_rows(*rows, counts, frames=[sc["frames"][0].astype(np.float32)])


def test_tracker_without_motion_is_the_tracker_it_was(hip):
    params, frames = C.scenarios()["gap"]
    tracker, ref = _tracker(**params), R.RefTracker(**params)
    assert tracker.motion is False and not hasattr(tracker, "_motion")
    for frame in frames:
        rows, n, _ = _pack([C.arrays(frame)])
        out, tail = tracker._launch(*rows, torch.from_numpy(n).to(DEV), tracker._active(None))
        k, status = tail.tolist()
        want = ref.step(*C.arrays(frame), np.arange(len(frame), dtype=np.int32))
        _same_rows([r[0, :k].cpu().numpy() for r in out], want)
        got, state = tracker.state_dict(), R.stack_states([ref])
        assert status == 0 and set(got) == set(R.KEYS) and all(got[key].tobytes() == state[key].tobytes() for key in R.KEYS)
    assert tracker.last_motion is None


# ---- Detector.track -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["plain", "nms", "fixed"])
def test_detector_track_with_motion_equals_detect_then_update_rows(hip, model, path):  # noqa: F811
    from detr_tf.inference import Detector, TrackedDetections
    kw = dict(nms_threshold=0.5) if path == "nms" else dict(resize="fixed") if path == "fixed" else {}
    det = Detector(model, _config(), score_threshold=0.0, max_detections=20, shortest_side=64, max_size=96, canvas=(96, 96), **kw)
    shifts = [(0, 0), (4, -3), (-3, 2), (-3, 2)]
    sizes = ((96, 128), (96, 128)) if path == "fixed" else ((96, 128), (120, 80))
    videos = [MC.video(40 + s, h, w, shifts) for s, (h, w) in enumerate(sizes)]
    params = dict(track_threshold=0.0, min_hits=1, motion=True, motion_radius=8)
    tracker, by_hand = _tracker(2, **params), _tracker(2, **params)
    motions = [M.RefMotion(8) for _ in range(2)]
    emitted = 0
    for f in range(len(shifts)):
        frame = [v[f] for v in videos]
        got = det.track(frame, tracker)
        mine = tracker.last_motion.cpu().numpy()
        dets = det(frame)
        want = by_hand.update(dets, frames=frame)
        assert all(isinstance(g, TrackedDetections) for g in got)
        _same(got, want)
        assert mine.tobytes() == by_hand.last_motion.cpu().numpy().tobytes()
        assert mine.tolist() == [m.step(im).tolist() for m, im in zip(motions, frame)]       # and it is what the frames say
        emitted += sum(len(g.ids) for g in got)
        a, b = tracker.state_dict(), by_hand.state_dict()
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert emitted > 0 and mine[:, :3].tolist() == [[1, 0, 0]] * 2 and tracker.state_dict()["motion_head"][:, 5].tolist() == [1, 1]
    one = _tracker(motion=True)                                                # one array in, one TrackedDetections out
    assert isinstance(det.track(videos[0][0], one), TrackedDetections) and one.last_motion.tolist() == [[0, 0, 0, 0, 0, 1]]
