"""detr_hip_track_embed (csrc/track_embed.hip, csrc/track_core.h) against its NumPy restatement (tests/track_embed_ref.py, pinned by
tests/test_track_embed_cpu.py), EXACTLY: after every frame the emitted ids, hits, counts and the bytes of boxes, labels, scores and
query, plus the bytes of BOTH states, the tracks and the embedding bank.  Then the layers above it: DetrModel return_embeddings,
Tracker(embed_dim=...) and Detector.track."""
import functools
import os

import numpy as np
import pytest
import torch

import track_cases as C
import track_embed_cases as EC
import track_embed_ref as ER
import track_ref as R
from test_gpu_detect import _config, _images  # noqa: F401  (the frames of the detector's tests)
from test_track_embed_cpu import check_track_embed_desc_layout, check_track_embed_rejects_bad_arguments

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SCENARIOS = EC.scenarios()


def _tracker(streams=1, **params):
    from detr_tf.inference import Tracker
    return Tracker(streams, DEV, **params)


def _pack(frames, D=None, query=True):
    """frames: per stream (boxes, labels, scores, query, embeddings [R, E]) -> padded device rows, host counts, embeddings [S, R, E]."""
    S = len(frames)
    counts = np.array([len(f[0]) for f in frames], np.int32)
    D = max(int(counts.max()), 1) if D is None else D
    rows_max, E = max(max(len(f[4]) for f in frames), 1), frames[0][4].shape[1]
    boxes, labels, scores, q = np.zeros((S, D, 4), F), np.zeros((S, D), np.int64), np.zeros((S, D), F), np.zeros((S, D), np.int32)
    emb = np.zeros((S, rows_max, E), F)
    for s, f in enumerate(frames):
        k = counts[s]
        boxes[s, :k], labels[s, :k], scores[s, :k], q[s, :k] = f[0], f[1], f[2], f[3]
        emb[s, :len(f[4])] = f[4]
    rows = [torch.from_numpy(a).to(DEV) for a in (boxes, labels, scores, q)]
    if not query:
        rows[3] = None
    return rows, counts, torch.from_numpy(emb).to(DEV)


def _step(tracker, frames, active=None, counts=None, D=None, query=True):
    """One launch through the tracker's own launch path -> ([per stream the six emitted arrays], status word)."""
    rows, n, emb = _pack(frames, D, query)
    n = n if counts is None else np.asarray(counts, np.int32)
    out, tail = tracker._launch(*rows, torch.from_numpy(n).to(DEV), tracker._active(active), emb if tracker.embed_dim is not None else None)
    *k, status = tail.tolist()
    host = [r.cpu().numpy() for r in out]
    for s in range(len(frames)):
        assert all(not r[s, k[s]:].any() for r in host), "the rows behind the count are zero"
    return [tuple(r[s, :k[s]] for r in host) for s in range(len(frames))], status


def _same_rows(got, want):
    names = ("boxes", "labels", "scores", "query", "ids", "hits")
    for name, g, w in zip(names, got, want[:6]):
        w = np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, g, w)


def _same_state(tracker, refs):
    got, want = tracker.state_dict(), ER.stack_states(refs)
    assert set(got) == set(ER.KEYS)
    for k in ER.KEYS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (k, np.argwhere(g != w)[:5])


def _replay(params, frames_per_stream, active=None, expect_status=0, query=True):
    """frames_per_stream[f][s] = a packed frame; active[f][s] or None.  Device and reference side by side, compared after every
    frame.  -> (tracker, refs, emitted counts per frame)"""
    S = len(frames_per_stream[0])
    tracker, refs = _tracker(S, **params), [ER.RefEmbedTracker(**params) for _ in range(S)]
    emitted = []
    for f, frames in enumerate(frames_per_stream):
        act = None if active is None else active[f]
        got, status = _step(tracker, frames, act, query=query)
        want_status = 0
        for s in range(S):
            if act is not None and not act[s]:
                assert all(len(g) == 0 for g in got[s])
                continue
            fr = frames[s]
            want = refs[s].step(fr[0], fr[1], fr[2], fr[3] if query else None, fr[4])
            want_status |= want[6]
            _same_rows(got[s], want)
        assert status == want_status and (expect_status is None or status == expect_status), (f, status, want_status)
        _same_state(tracker, refs)
        emitted.append([len(g[4]) for g in got])
    return tracker, refs, emitted


@functools.lru_cache(maxsize=None)
def _walk(E, frames=12):
    return EC.random_walk(EC.WALK_SEEDS[E], E, frames=frames)


# ---- the scenarios of the CPU tests, replayed ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_track_embed_replays_the_hand_worked_scenarios(hip, name):
    params, frames = SCENARIOS[name]
    tracker, refs, emitted = _replay(params, [[EC.arrays(fr, params["embed_dim"])] for fr in frames],
                                     expect_status=ER.FULL if name == "overflow" else 0)
    assert sum(map(sum, emitted)) > 0
    if name == "occlusion_reid":
        assert refs[0].n_reid == 1 and emitted[16] == [1]                       # the scenario does what it is named after, on the device too


# ---- seeded random walks: E = 4 and 68 are the lane tails of dot64 ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EC.WALK_PARAMS))
@pytest.mark.parametrize("E", [4, 68, 256])
def test_track_embed_random_walks(hip, E, name):
    tracker, refs, emitted = _replay(dict(embed_dim=E, **EC.WALK_PARAMS[name]), _walk(E))
    assert sum(map(sum, emitted)) >= 20 and all(int(r.s["next_id"]) > 5 for r in refs)
    assert sum(r.n_reid for r in refs) >= 1                                     # tracks were found again by appearance


def test_track_embed_query_none_takes_row_d(hip):
    walk = [[(f[0], f[1], f[2], f[3], f[4][f[3]]) for f in frame] for frame in _walk(68)]       # the rows in the detections' order
    tracker, refs, emitted = _replay(dict(embed_dim=68, min_hits=1), walk, query=False)
    with_query = [ER.RefEmbedTracker(embed_dim=68, min_hits=1) for _ in range(3)]
    for frame in _walk(68):
        for s in range(3):
            with_query[s].step(*frame[s])
    for a, b in zip(refs, with_query):                                         # the same tracking as through query; only the emitted query is 0
        assert all(np.asarray(a.state_dict()[k]).tobytes() == np.asarray(b.state_dict()[k]).tobytes() for k in ER.KEYS)
    assert sum(map(sum, emitted)) >= 20


def test_track_embed_active_mask_keeps_both_states(hip):
    walk = _walk(68)[:8]
    active = [[1, f % 2 == 0, 1] for f in range(8)]                            # stream 1 delivers no frame on odd frames
    tracker, refs, emitted = _replay(dict(embed_dim=68, min_hits=1), walk, active=active)      # the bank of stream 1 is compared after every frame
    assert [int(r.s["frame"]) for r in refs] == [8, 4, 8] and tracker.state_dict()["frame"].tolist() == [8, 4, 8]
    assert all(emitted[f][1] == 0 for f in range(1, 8, 2)) and sum(e[1] for e in emitted) > 0 and refs[1].bank.any()


# ---- many tracks, many detections: every strided loop passes the thread count, the table pass runs five ballots per slot ----------
def _crowd(E=32):
    rng = np.random.default_rng(5)
    base = np.array([C.square(50.0 * (i % 20), 50.0 * (i // 20)) for i in range(300)], F)
    labels = np.arange(300) % 4
    look = rng.normal(0, 1, (300, E))
    look /= np.linalg.norm(look, axis=1, keepdims=True)

    def frame(boxes, scores):
        order = np.argsort(-scores, kind="stable")
        emb = (rng.uniform(0.5, 4.0, (300, 1)) * (look + rng.normal(0, 0.1 / np.sqrt(E), (300, E)))).astype(F)
        return [(boxes[order], labels[order], scores[order], order.astype(np.int32), emb)]

    frames = [[(base[:250], labels[:250], np.full(250, 0.9, F), np.arange(250, dtype=np.int32), look[:250].astype(F))]]
    for f in range(2):
        boxes = base + rng.uniform(-3, 3, (300, 4)).astype(F)
        boxes[7] = boxes[3]                                                    # duplicated boxes: IoU ties that the looks decide
        boxes[260] = boxes[100]
        scores = rng.choice(np.array([0.95, 0.9, 0.8, 0.6, 0.5], F), 300)
        scores[250:255], scores[255:] = 0.9, 0.5                               # five newcomers; the rest is only ever seen at a low score
        if f == 0:
            boxes[20:30] += F(5000.0)                                          # ten objects are gone for a frame ...
            scores[20:30] = 0.5
        else:
            boxes[20:30] += np.array([0, 1000, 0, 1000], F)                    # ... and back far from where they were
            scores[20:30] = 0.9
        frames.append(frame(boxes, scores))
    return frames


def test_track_embed_300_detections_against_250_tracks(hip):
    tracker, refs, emitted = _replay(dict(embed_dim=32, min_hits=1), _crowd())
    assert emitted[0] == [250] and min(e[0] for e in emitted[1:]) > 230
    assert refs[0].n_reid == 10 and int(refs[0].s["next_id"]) == 256            # the ten came back under their ids; five newcomers, no other birth
    assert min(refs[0].gaps) >= EC.MARGIN                                       # (the reference's own numbers: nothing here hangs on a last bit)


def test_track_embed_overflow_raises_after_the_states_were_updated(hip):
    params, frames = SCENARIOS["overflow"]
    tracker, ref = _tracker(**params), ER.RefEmbedTracker(**params)
    packed = EC.arrays(frames[0], params["embed_dim"])
    rows, counts, emb = _pack([packed])
    with pytest.raises(ValueError, match="live tracks"):
        tracker.update_rows(*rows, torch.from_numpy(counts).to(DEV), embeddings=emb)
    ref.step(*packed)
    _same_state(tracker, [ref])
    assert (tracker.state_dict()["id"] > 0).sum() == 256 and tracker.state_dict()["embed"].any(2).all()


# ---- without appearance it IS detr_hip_track --------------------------------------------------------------------------------------
def test_track_embed_weight_0_reid_off_equals_detr_hip_track(hip):
    walk = C.random_walk(11)
    rng = np.random.default_rng(2)
    params = dict(min_hits=2)
    plain, embed = _tracker(3, **params), _tracker(3, embed_dim=256, appearance_weight=0.0, reid_threshold=None, **params)
    for frames in walk:
        packed = [f + (np.arange(len(f[0]), dtype=np.int32), rng.normal(0, 1, (max(len(f[0]), 1), 256)).astype(F)) for f in frames]
        got, status = _step(embed, packed)
        want, want_status = _step(plain, packed)
        assert status == want_status == 0
        for g, w in zip(got, want):
            _same_rows(g, w)
        a, b = embed.state_dict(), plain.state_dict()
        assert set(b) == set(R.KEYS) and all(a[k].tobytes() == b[k].tobytes() for k in R.KEYS)       # TrackState, bit for bit
    assert int(plain.state_dict()["next_id"].min()) > 8 and embed.state_dict()["embed"].any()


# ---- bad embeddings ---------------------------------------------------------------------------------------------------------------
def test_track_embed_bad_rows_set_bit_4_and_corrupt_nothing(hip):
    E = 8
    params = dict(embed_dim=E, min_hits=1)
    tracker, ref = _tracker(**params), ER.RefEmbedTracker(**params)
    boxes, labels, scores = C.arrays([(C.square(50.0 + 150.0 * i), 1, 0.9) for i in range(5)])
    emb = np.stack([EC.axis(E, i, 2.0) for i in range(5)])

    def both(query, emb, want_status):
        got, status = _step(tracker, [(boxes, labels, scores, np.asarray(query, np.int32), emb)])
        want = ref.step(boxes, labels, scores, np.asarray(query, np.int32), emb)
        assert status == want[6] == want_status
        _same_rows(got[0], want)
        _same_state(tracker, [ref])

    both([0, 1, 2, 3, 4], emb, 0)
    guard = tracker.state_dict()["embed"][0, 5:].copy()
    poisoned = emb.copy()
    poisoned[1, 3], poisoned[2, 0] = np.nan, np.inf
    both([0, 1, 2, 3, 4], poisoned, ER.BAD_EMBED)                               # a NaN and an infinity: the zero embedding for those two
    both([0, 5, -1, 2**31 - 1, 4], emb, ER.BAD_EMBED)                           # rows outside [0, R): never read
    both([4, 3, 2, 1, 0], emb, 0)                                               # and the tracker goes on
    state = tracker.state_dict()
    assert np.isfinite(state["embed"]).all() and state["embed"][0, 5:].tobytes() == guard.tobytes()
    assert sorted(state["id"][0][state["id"][0] > 0].tolist()) == [1, 2, 3, 4, 5]
    rows, counts, dev = _pack([(boxes, labels, scores, np.array([0, 1, 2, 3, 9], np.int32), emb)])
    with pytest.raises(ValueError, match="embedding row index"):
        tracker.update_rows(*rows, torch.from_numpy(counts).to(DEV), embeddings=dev)


# ---- resume, rerun, reset ---------------------------------------------------------------------------------------------------------
def test_track_embed_resumes_and_reruns_bit_identically(hip):
    walk, params = _walk(256), dict(embed_dim=256, min_hits=2)
    tracker, refs, _ = _replay(params, walk[:6])
    saved = tracker.state_dict()
    assert saved["embed"].shape == (3, 256, 256) and saved["embed"].dtype == F
    runs = []
    for _ in range(2):                                                         # two runs from one loaded pair of states
        other = _tracker(3, **params)
        other.load_state_dict(saved)
        outs = [_step(other, frames) for frames in walk[6:]]
        runs.append((outs, other.state_dict()))
    (a_out, a_state), (b_out, b_state) = runs
    assert all(x.tobytes() == y.tobytes() for fa, fb in zip(a_out, b_out) for sa, sb in zip(fa[0], fb[0]) for x, y in zip(sa, sb))
    assert all(a_state[k].tobytes() == b_state[k].tobytes() for k in ER.KEYS)
    for frames in walk[6:]:                                                    # and it equals the uninterrupted run
        for s in range(3):
            refs[s].step(*frames[s])
    _same_state(other, refs)
    with pytest.raises(ValueError, match="embed"):
        other.load_state_dict({k: v for k, v in saved.items() if k != "embed"})
    with pytest.raises(ValueError, match="embed"):
        other.load_state_dict(dict(saved, embed=saved["embed"][:, :, :128]))
    other.reset(1)                                                             # reset of one stream: fresh states there, the others untouched
    refs[1] = ER.RefEmbedTracker(**params)
    _same_state(other, refs)
    other.reset()
    _same_state(other, [ER.RefEmbedTracker(**params) for _ in range(3)])


def test_tracker_update_with_embeddings_packs_like_update_rows(hip):
    from detr_tf.inference import Detections, TrackedDetections
    walk, params = _walk(68)[:6], dict(embed_dim=68, min_hits=1)
    a, b = _tracker(3, **params), _tracker(3, **params)
    for frames in walk:
        dets = [Detections(*(torch.from_numpy(x).to(DEV) for x in f[:4])) for f in frames]
        emb = _pack(frames)[2]
        got = a.update(dets, embeddings=emb)
        want, status = _step(b, frames)
        assert status == 0 and all(isinstance(g, TrackedDetections) for g in got)
        for g, w in zip(got, want):
            _same_rows([t.cpu().numpy() for t in g], w)
    with pytest.raises(ValueError, match="mandatory"):
        a.update(dets)
    with pytest.raises(ValueError, match="mandatory"):
        _tracker(3).update(dets, embeddings=emb)                                # a tracker without embed_dim takes none
    for bad in (emb[:, :, :64], emb.double(), emb[:2], emb.cpu(), emb.transpose(1, 2).contiguous().transpose(1, 2)):
        with pytest.raises(ValueError, match="embeddings must be"):
            a.update(dets, embeddings=bad)
    one = _tracker(embed_dim=68, min_hits=1)                                    # a triple has no query: its detections take the rows 0..k-1
    f = next(fr[0] for fr in walk if len(fr[0][0]) >= 3)
    out = one.update(tuple(torch.from_numpy(x) for x in f[:3]), embeddings=torch.from_numpy(f[4][f[3]][None]).to(DEV))
    assert out[0].query.tolist() == list(range(len(out[0].ids))) and len(out[0].ids) == int((f[2] >= F(0.7)).sum())


# ---- the C entry point on this machine ---------------------------------------------------------------------------------------------
def test_track_embed_desc_layout(hip):
    check_track_embed_desc_layout()


def test_track_embed_rejects_bad_arguments(hip):
    check_track_embed_rejects_bad_arguments()
    with pytest.raises(ValueError, match="embed_dim"):
        _tracker(embed_dim=6)
    with pytest.raises(ValueError, match="appearance_weight"):
        _tracker(embed_dim=8, appearance_weight=1.5)
    tracker = _tracker(embed_dim=8)
    assert tracker.reid_threshold == 0.8 and _tracker(embed_dim=8, reid_threshold=None).reid_threshold is None
    assert set(_tracker().state_dict()) == set(R.KEYS)                          # embed_dim=None: today's keys


# ---- the model's embeddings and Detector.track --------------------------------------------------------------------------------------
def _tiny(**kw):
    """The committed tiny model: the configuration and seed of tests/golden/tiny_r50_e1d2_64x96.npz."""
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref as O
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_r50_e1d2_64x96.npz")) as z:
        seed, num_enc, num_dec = (int(v) for v in z["meta"][:3])
        images = z["images"]
    m = get_detr_model(_config(), num_encoder_layers=num_enc, num_decoder_layers=num_dec, dropout=0.0, **kw)
    m.load_weights(O.make_params(seed, num_enc=num_enc, num_dec=num_dec))
    return m, images


@pytest.fixture(scope="module")
def tiny(hip):
    return _tiny(include_top=True)


def test_model_return_embeddings_is_the_headless_hidden_state(hip, tiny):
    model, images = tiny
    headless, _ = _tiny(include_top=False)
    assert headless.headless and model.engine.num_dec == 2
    hs = headless(images)
    assert tuple(hs.shape) == (2, images.shape[0], 100, 256)
    want = hs[-1].cpu().numpy()
    plain = model(images)                                                      # eager: the first sighting of the shape
    keys = set(plain)
    assert "embed" not in keys
    outs = [model(images, return_embeddings=True) for _ in range(3)]           # recorded, then replayed
    assert model._eval_graph is not None
    recorded = model._eval_graph["graph"]
    assert all(set(o) == keys | {"embed"} for o in outs)
    for o in outs:
        e = o["embed"]
        assert e.dtype == torch.float32 and tuple(e.shape) == (images.shape[0], 100, 256) and e.is_contiguous()
        assert e.cpu().numpy().tobytes() == want.tobytes()
        assert o["pred_logits"].cpu().numpy().tobytes() == plain["pred_logits"].cpu().numpy().tobytes()
    assert outs[0]["embed"].data_ptr() != outs[1]["embed"].data_ptr()           # clones: a later call does not overwrite an earlier result
    again = model(images)                                                      # the flag is no part of the graph key: the same graph replays
    assert set(again) == keys and model._eval_graph["graph"] is recorded
    model.eval_graph = False
    try:
        assert model(images, return_embeddings=True)["embed"].cpu().numpy().tobytes() == want.tobytes()      # eager
    finally:
        model.eval_graph = True
    with pytest.raises(NotImplementedError, match="evaluation mode"):
        model(images, training=True, return_embeddings=True)
    with pytest.raises(NotImplementedError, match="headless"):
        headless(images, return_embeddings=True)


def test_detector_track_by_appearance_equals_detect_then_update_rows(hip, tiny):
    from detr_tf.inference import Detector, TrackedDetections, _detect
    model, _ = tiny
    kw = dict(score_threshold=0.0, max_detections=20, shortest_side=64, max_size=96, canvas=(96, 96))
    det = Detector(model, _config(), **kw)
    rng = np.random.default_rng(9)
    video = [[np.clip(im.astype(np.int16) + rng.integers(-6, 7, im.shape), 0, 255).astype(np.uint8) for im in _images()] for _ in range(5)]
    scores = np.sort(np.concatenate([d.scores.cpu().numpy() for d in det(video[0])]))
    params = dict(track_threshold=float(scores[len(scores) // 2]), min_hits=2, embed_dim=256)       # the median: high and low detections both exist
    tracker, hand, refs = _tracker(2, **params), _tracker(2, **params), [ER.RefEmbedTracker(**params) for _ in range(2)]
    sizes = np.array([im.shape[:2] for im in video[0]], np.int32)
    total = 0
    for frame in video:
        got = det.track(frame, tracker)
        out, _ = det._forward(frame, sizes, return_embeddings=True)
        rows = _detect(out["pred_logits"], out["pred_boxes"], sizes, 91, 0.0, 20, "xyxy", True)
        want = hand.update_rows(*rows, embeddings=out["embed"])
        emb = out["embed"].cpu().numpy()
        for s in range(2):
            assert isinstance(got[s], TrackedDetections)
            _same_rows([t.cpu().numpy() for t in got[s]], [t.cpu().numpy() for t in want[s]])
            k = int(rows[4][s])
            ref = refs[s].step(*(r[s, :k].cpu().numpy() for r in rows[:4]), emb[s])
            _same_rows([t.cpu().numpy() for t in got[s]], ref)
            total += len(ref[4])
        a, b = tracker.state_dict(), hand.state_dict()
        assert all(a[k].tobytes() == b[k].tobytes() for k in ER.KEYS)
        _same_state(tracker, refs)
    assert total > 0 and max(int(r.s["hits"].max()) for r in refs) >= 3          # something was followed across frames
    with pytest.raises(ValueError, match="256"):
        det.track(video[0], _tracker(2, embed_dim=128))
    with pytest.raises(NotImplementedError, match="per-tile"):
        Detector(model, _config(), nms_threshold=0.5, **kw).track(video[0], tracker)
    assert isinstance(det.track(video[0], _tracker(2)), list)                   # a tracker without embed_dim: the call of before
