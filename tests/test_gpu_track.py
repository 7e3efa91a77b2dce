"""detr_hip_track (csrc/track.hip) against its NumPy restatement (tests/track_ref.py, pinned by tests/test_track_cpu.py), EXACTLY:
after every frame the emitted ids, hits, counts and the bytes of boxes, labels, scores and query, plus the bytes of the whole state.
The one exception is stated where it is made: the payload bits of a NaN, which no arithmetic standard fixes."""
import numpy as np
import pytest
import torch

import track_cases as C
import track_ref as R
from test_gpu_detect import _config, _images, _same, model  # noqa: F401  (the tiny model of the detector's tests)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SCENARIOS = C.scenarios()


def _tracker(streams=1, **params):
    from detr_tf.inference import Tracker
    return Tracker(streams, DEV, **params)


def _pack(frames, D=None):
    """frames: per stream (boxes, labels, scores[, query]) -> padded device rows and host counts."""
    S = len(frames)
    counts = np.array([len(f[0]) for f in frames], np.int32)
    D = max(int(counts.max()), 1) if D is None else D
    boxes, labels, scores, query = np.zeros((S, D, 4), F), np.zeros((S, D), np.int64), np.zeros((S, D), F), np.zeros((S, D), np.int32)
    for s, f in enumerate(frames):
        k = counts[s]
        boxes[s, :k], labels[s, :k], scores[s, :k] = f[0], f[1], f[2]
        query[s, :k] = f[3] if len(f) > 3 else np.arange(k)
    return [torch.from_numpy(a).to(DEV) for a in (boxes, labels, scores, query)], counts


def _step(tracker, frames, active=None, counts=None, D=None):
    """One launch through the tracker's own launch path -> ([per stream the six emitted arrays], status word)."""
    rows, n = _pack(frames, D)
    n = n if counts is None else np.asarray(counts, np.int32)
    out, tail = tracker._launch(*rows, torch.from_numpy(n).to(DEV), tracker._active(active))
    *k, status = tail.tolist()
    host = [r.cpu().numpy() for r in out]
    for s in range(len(frames)):
        assert all(not r[s, k[s]:].any() for r in host), "the rows behind the count are zero"
    return [tuple(r[s, :k[s]] for r in host) for s in range(len(frames))], status


def _ref_step(ref, frame):
    query = frame[3] if len(frame) > 3 else np.arange(len(frame[0]), dtype=np.int32)
    return ref.step(frame[0], frame[1], frame[2], query)


def _same_rows(got, want):
    names = ("boxes", "labels", "scores", "query", "ids", "hits")
    for name, g, w in zip(names, got, want[:6]):
        w = np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, g, w)


def _same_state(tracker, refs, nan_ok=False):
    got, want = tracker.state_dict(), R.stack_states(refs)
    assert set(got) == set(R.KEYS)
    for k in R.KEYS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        if nan_ok and k in ("x", "v"):                     # a NaN is a NaN on both sides; which payload bits it carries is not arithmetic
            assert (np.isnan(g) == np.isnan(w)).all(), k
            g, w = np.where(np.isnan(g), F(0), g), np.where(np.isnan(w), F(0), w)
        assert g.tobytes() == w.tobytes(), (k, np.argwhere(g != w)[:5])


def _replay(params, frames_per_stream, active=None, expect_status=0, nan_ok=False):
    """frames_per_stream[f][s] = (boxes, labels, scores); active[f][s] or None.  Device and reference side by side, compared
    after every frame.  -> (tracker, refs, emitted counts per frame)"""
    S = len(frames_per_stream[0])
    tracker, refs = _tracker(S, **params), [R.RefTracker(**params) for _ in range(S)]
    emitted = []
    for f, frames in enumerate(frames_per_stream):
        act = None if active is None else active[f]
        got, status = _step(tracker, frames, act)
        want_status = 0
        for s in range(S):
            if act is not None and not act[s]:
                assert all(len(g) == 0 for g in got[s])
                continue
            want = _ref_step(refs[s], frames[s])
            want_status |= want[6]
            _same_rows(got[s], want)
        assert status == want_status and (expect_status is None or status == expect_status), (f, status, want_status)
        _same_state(tracker, refs, nan_ok)
        emitted.append([len(g[4]) for g in got])
    return tracker, refs, emitted


# ---- the scenarios of the CPU tests, replayed ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_track_replays_the_hand_worked_scenarios(hip, name):
    params, frames = SCENARIOS[name]
    tracker, refs, emitted = _replay(params, [[C.arrays(fr)] for fr in frames], expect_status=R.FULL if name == "overflow" else 0)
    assert sum(map(sum, emitted)) > 0


# ---- seeded random walks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [{}, dict(class_agnostic=True), dict(min_hits=1, max_age=0), dict(new_threshold=0.9, min_hits=2, max_age=2)],
                         ids=["defaults", "agnostic", "min_hits1_max_age0", "new_threshold"])
def test_track_random_walks(hip, params):
    walk = C.random_walk(11)
    assert any(len(fr[s][0]) == 0 for fr in walk for s in range(3)) and max(len(fr[s][0]) for fr in walk for s in range(3)) == 9
    tracker, refs, emitted = _replay(params, walk)
    assert sum(map(sum, emitted)) >= 20                                        # tracks were confirmed and followed ...
    assert all(int(r.s["next_id"]) > 10 for r in refs)                         # ... born ...
    assert all(int(r.s["next_id"]) - 1 > int((r.s["id"] > 0).sum()) for r in refs)          # ... and dropped


def test_track_active_mask_skips_a_stream(hip):
    walk = C.random_walk(11, frames=8)
    active = [[1, f % 2 == 0, 1] for f in range(8)]                            # stream 1 delivers no frame on odd frames
    tracker, refs, emitted = _replay({}, walk, active=active)
    assert [int(r.s["frame"]) for r in refs] == [8, 4, 8] and tracker.state_dict()["frame"].tolist() == [8, 4, 8]
    assert all(emitted[f][1] == 0 for f in range(1, 8, 2)) and sum(e[1] for e in emitted) > 0


# ---- many tracks, many detections: both strided loops pass the thread count, hundreds of rounds ------------------------------------
def _crowd():
    rng = np.random.default_rng(5)
    base = np.array([C.square(50.0 * (i % 20), 50.0 * (i // 20)) for i in range(300)], F)
    labels = np.arange(300) % 4
    frames = [[(base[:250], labels[:250], np.full(250, 0.9, F))]]              # 250 tracks, confirmed at birth (min_hits = 1)
    for f in range(2):
        boxes = base + rng.uniform(-3, 3, (300, 4)).astype(F)
        boxes[7] = boxes[3]                                                    # duplicates: exact IoU ties between detections ...
        boxes[260] = boxes[100]
        scores = rng.choice(np.array([0.95, 0.9, 0.8, 0.6, 0.5], F), 300)
        scores[250:255], scores[255:] = 0.9, 0.5                               # five newcomers; the rest is only ever seen at a low score
        order = np.argsort(-scores, kind="stable")
        frames.append([(boxes[order], labels[order], scores[order])])
    return frames


def test_track_300_detections_against_250_tracks(hip):
    tracker, refs, emitted = _replay(dict(min_hits=1), _crowd())
    assert emitted[0] == [250] and min(e[0] for e in emitted[1:]) > 240
    assert int(refs[0].s["next_id"]) > 251 and int((refs[0].s["id"] > 0).sum()) >= 250      # the newcomers were taken in


def test_track_duplicated_boxes_make_real_ties(hip):
    box = np.array([C.square(50.0)] * 6 + [C.square(200.0)] * 6, F)            # six tracks on one box, six on another
    labels = np.array([1, 1, 1, 2, 2, 1] * 2)
    scores = np.array([0.9, 0.9, 0.8, 0.8, 0.5, 0.5] * 2, F)
    frames = [[(box, labels, scores)], [(box[::-1].copy(), labels[::-1].copy(), scores)], [(box, labels, scores[::-1].copy())]] * 2
    for params in (dict(min_hits=1), dict(min_hits=1, class_agnostic=True), dict(min_hits=2, low_match_threshold=0.3)):
        tracker, refs, emitted = _replay(params, frames)
        assert sum(map(sum, emitted)) > 12


def test_track_overflow_raises_after_the_state_was_updated(hip):
    params, frames = SCENARIOS["overflow"]
    tracker, ref = _tracker(**params), R.RefTracker(**params)
    rows, counts = _pack([C.arrays(frames[0])])
    with pytest.raises(ValueError, match="live tracks"):
        tracker.update_rows(*rows, torch.from_numpy(counts).to(DEV))
    _ref_step(ref, C.arrays(frames[0]))
    _same_state(tracker, [ref])                                                # the state is the updated, valid one
    assert (tracker.state_dict()["id"] > 0).sum() == 256


def test_track_nan_box_matches_nothing_and_corrupts_nothing(hip):
    frames = []
    for f, fr in enumerate(C.moving(8)):
        boxes, labels, scores = C.arrays(fr + [(C.square(300.0), 1, 0.8)])
        bad = np.array([[np.nan, 100, 140, 140], [300, 100, 340, np.nan]], F)   # a NaN corner at a high score, one at a NaN score
        frames.append([(np.concatenate([bad[:1], boxes, bad[1:]]), np.concatenate([[1], labels, [1]]),
                        np.concatenate([[F(0.95)], scores, [F(np.nan)]]).astype(F))])
    tracker, refs, emitted = _replay(dict(min_hits=2), frames, nan_ok=True)
    assert emitted == [[0]] + [[2]] * 7                                        # the two real objects, every frame; the NaN box never
    state = tracker.state_dict()
    assert sorted(state["id"][0][~np.isnan(state["x"][0]).any(1) & (state["id"][0] > 0)].tolist()) == [2, 3]


def test_track_bad_count_is_an_empty_frame(hip):
    walk = C.random_walk(13, frames=5)
    tracker, refs, _ = _replay({}, walk[:4])
    frames = walk[4]
    D = 9
    got, status = _step(tracker, frames, counts=[-1, D + 1, len(frames[2][0])], D=D)
    assert status == R.BAD_COUNT
    empty = (np.zeros((0, 4), F), np.zeros(0, np.int64), np.zeros(0, F))
    for s, frame in enumerate((empty, empty, frames[2])):
        _same_rows(got[s], _ref_step(refs[s], frame))
    _same_state(tracker, refs)
    rows, _ = _pack(frames, D)
    with pytest.raises(ValueError, match="count outside"):
        tracker.update_rows(*rows, torch.tensor([0, D + 1, 0], dtype=torch.int32, device=DEV))


def test_track_resumes_and_reruns_bit_identically(hip):
    walk = C.random_walk(14, frames=10)
    tracker, refs, _ = _replay({}, walk[:6])
    saved = tracker.state_dict()
    runs = []
    for _ in range(2):                                                         # two runs from one loaded state
        other = _tracker(3)
        other.load_state_dict(saved)
        outs = [_step(other, frames) for frames in walk[6:]]
        runs.append((outs, other.state_dict()))
    (a_out, a_state), (b_out, b_state) = runs
    assert all(x.tobytes() == y.tobytes() for fa, fb in zip(a_out, b_out) for sa, sb in zip(fa[0], fb[0]) for x, y in zip(sa, sb))
    assert all(a_state[k].tobytes() == b_state[k].tobytes() for k in R.KEYS)
    for frames in walk[6:]:                                                    # and it equals the uninterrupted run
        for s in range(3):
            _ref_step(refs[s], frames[s])
    _same_state(other, refs)
    other.reset(1)                                                             # reset of one stream: a fresh state there, the others untouched
    refs[1] = R.RefTracker()
    _same_state(other, refs)
    other.reset()
    _same_state(other, [R.RefTracker() for _ in range(3)])


def test_tracker_update_packs_like_update_rows(hip):
    from detr_tf.inference import Detections, TrackedDetections
    walk = C.random_walk(11, frames=6)
    a, b = _tracker(3, min_hits=1), _tracker(3, min_hits=1)
    for frames in walk:
        dets = [Detections(*(torch.from_numpy(x).to(DEV) for x in f), torch.arange(len(f[0]), dtype=torch.int32, device=DEV)) for f in frames]
        got = a.update(dets)
        want, status = _step(b, frames)
        assert status == 0 and all(isinstance(g, TrackedDetections) for g in got)
        for g, w in zip(got, want):
            _same_rows([t.cpu().numpy() for t in g], w)
    with pytest.raises(ValueError, match="streams"):
        a.update(dets[:2])
    one = _tracker(min_hits=1)                                                  # a single triple is the frame of a one-stream tracker
    f = walk[3][0]
    assert one.update(tuple(torch.from_numpy(x) for x in f))[0].ids.tolist() == list(range(1, 1 + int((f[2] >= F(0.7)).sum())))


# ---- Detector.track ---------------------------------------------------------------------------------------------------------------
def _video(n):
    rng = np.random.default_rng(9)
    base = _images()
    return [[np.clip(im.astype(np.int16) + rng.integers(-6, 7, im.shape), 0, 255).astype(np.uint8) for im in base] for _ in range(n)]


def test_detector_track_equals_call_then_the_reference(hip, model):  # noqa: F811
    from detr_tf.inference import Detector, TrackedDetections
    det = Detector(model, _config(), score_threshold=0.0, max_detections=20, shortest_side=64, max_size=96, canvas=(96, 96))
    video = _video(6)
    plain = [det(frame) for frame in video]                                    # what __call__ returns, frame by frame
    scores = np.sort(np.concatenate([d.scores.cpu().numpy() for d in plain[0]]))
    thr = float(scores[len(scores) // 2])                                      # the median: high and low detections both exist
    params = dict(track_threshold=thr, min_hits=2)
    tracker, refs = _tracker(2, **params), [R.RefTracker(**params) for _ in range(2)]
    total = 0
    for frame, dets in zip(video, plain):
        before = det(frame)
        got = det.track(frame, tracker)
        _same(det(frame), before)                                              # __call__ returns the same bits before and after a track call
        _same(before, dets)
        for s in range(2):
            assert isinstance(got[s], TrackedDetections)
            want = refs[s].step(*(t.cpu().numpy() for t in dets[s]))
            _same_rows([t.cpu().numpy() for t in got[s]], want)
            total += len(want[4])
        _same_state(tracker, refs)
    assert total > 0 and max(int(r.s["hits"].max()) for r in refs) >= 3          # something was followed across frames: the comparison is not empty
    single = _tracker(**params)                                                # one array in, one TrackedDetections out
    assert isinstance(det.track(video[0][1], single), TrackedDetections)
    with pytest.raises(ValueError, match="streams"):
        det.track(video[0], single)
    # through the merge (nms_threshold): the same tracker code behind merge_tiles' detections
    nms = Detector(model, _config(), score_threshold=0.0, max_detections=20, shortest_side=64, max_size=96, canvas=(96, 96), nms_threshold=0.5)
    tracker, refs = _tracker(2, **params), [R.RefTracker(**params) for _ in range(2)]
    for frame in video[:3]:
        dets, got = nms(frame), nms.track(frame, tracker)
        for s in range(2):
            _same_rows([t.cpu().numpy() for t in got[s]], refs[s].step(*(t.cpu().numpy() for t in dets[s][:4])))
        _same_state(tracker, refs)
