"""csrc/detect.hip on the device: detr_hip_detect against an fp64 NumPy restatement of the reference chain -- get_model_inference
(inference.py:68-83), the score threshold, a stable argsort(-score), the top-k cut, the numpy box helpers (bbox.py:230-294) --,
bit-equality of scores / labels with detr_hip_postprocess, threshold equality, edge cases, clipping, determinism, and the Detector
end to end against the hand-assembled chain (padded and fixed-size input, eager and replayed evaluation graph).

Inputs are built so that the fp64 and the fp32 order cannot legitimately differ, and the oracle asserts it before the kernel runs:
two kept scores come from identical logit rows (exact ties) or differ by >= 1e-3, and no score lies within 1e-4 of the threshold."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 1, 2), (3, 37, 5), (2, 100, 92), (1, 300, 92), (2, 1024, 4)]          # (B, Q, C)
SIZES = [(480, 640), (1333, 800), (1, 1)]                                            # (height, width): landscape, portrait, one pixel
FORMATS = ("xy_center", "xyxy", "yxyx", "xywh")
GRID = np.arange(0.52, 0.98, 0.002)                                                  # target scores: 2e-3 apart
THRESHOLD = float(np.float32(0.701))                                                 # between two grid points
# Box error against fp64, in ulp(fp32) of the image's longest side: one product (cx * W), one halving (w * W, then / 2, exact),
# one add or subtract (the corner) and one clip / corner difference -- one rounding of at most an ulp of max(H, W) each.
N_ROUNDINGS = 1 + 1 + 1 + 1


def box_bound(h, w):
    return N_ROUNDINGS * float(np.spacing(np.float32(max(h, w))))


# ---- inputs and the fp64 oracle ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(B, Q, C):
    """(logits fp32 [B, Q, C], boxes fp32 [B, Q, 4], sizes int32 [B, 2], background, fp64 score [B, Q], label [B, Q]); read-only."""
    rng = np.random.default_rng(1000 * B + Q + C)
    bg = C - 1
    logits = np.zeros((B, Q, C), np.float32)
    for b in range(B):
        others = rng.normal(0.0, 0.3, (Q, C))
        n_fg = max(1, min(int(0.6 * Q), len(GRID) - 30))                             # foreground queries: DISTINCT grid scores
        fg = rng.permutation(Q)[:n_fg]
        is_fg = np.zeros(Q, bool)
        is_fg[fg] = True
        target = rng.choice(GRID, Q)                                                 # background queries: any grid score
        target[fg] = rng.permutation(GRID)[:n_fg]
        label = np.where(is_fg, rng.integers(0, max(bg, 1), Q), bg)
        for q in range(Q):
            o = others[q]
            rest = np.exp(np.delete(o, label[q])).sum()
            o[label[q]] = np.log(target[q] / (1.0 - target[q]) * rest)               # softmax(o)[label] == target
        logits[b] = others.astype(np.float32)
        if Q >= 37:                                                                  # exact ties: a pair and a triple of identical rows
            src = fg[:2]
            spots = rng.permutation(np.setdiff1d(np.arange(Q), src))[:3]
            logits[b, spots[0]] = logits[b, src[0]]
            logits[b, spots[1]] = logits[b, src[1]]
            logits[b, spots[2]] = logits[b, src[1]]
    boxes = rng.random((B, Q, 4)).astype(np.float32)
    sizes = np.array([SIZES[(b + Q) % len(SIZES)] for b in range(B)], np.int32)
    x = logits.astype(np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)                                                 # inference.py:73
    score, label = p.max(-1), p.argmax(-1)                                           # :74-75
    for a in (logits, boxes, sizes, score, label):
        a.setflags(write=False)
    return logits, boxes, sizes, bg, score, label


def convert(boxes, size, fmt, clip):
    """bbox.py:230-294 in fp64: scale (cx, cy, w, h) by (W, H, W, H), then convert; clip the corners to the image."""
    H, W = float(size[0]), float(size[1])
    s = boxes.astype(np.float64) * np.array([W, H, W, H])
    if fmt == "xy_center":
        return s
    xyxy = np.concatenate([s[:, :2] - s[:, 2:] / 2, s[:, :2] + s[:, 2:] / 2], -1)
    if clip:
        xyxy = np.clip(xyxy, 0.0, np.array([W, H, W, H]))
    if fmt == "xyxy":
        return xyxy
    if fmt == "yxyx":
        return xyxy[:, [1, 0, 3, 2]]
    return np.concatenate([xyxy[:, :2], xyxy[:, 2:] - xyxy[:, :2]], -1)


def oracle(B, Q, C, thr, K, fmt, clip, background=None):
    """Per image (query order [k], fp64 boxes [k, 4]); asserts the conditions on the inputs."""
    logits, boxes, sizes, bg, score, label = case(B, Q, C)
    bg = bg if background is None else background
    assert (np.abs(score - thr) > 1e-4).all(), "a score lies within 1e-4 of the threshold"
    out = []
    for b in range(B):
        keep = np.nonzero((label[b] != bg) & (score[b] >= thr))[0]                   # :78-83, then the threshold
        s = score[b, keep]
        gap = np.abs(s[:, None] - s[None, :])
        same = (logits[b, keep][:, None, :] == logits[b, keep][None, :, :]).all(-1)
        assert (same | (gap >= 1e-3)).all(), "two kept scores are neither an exact tie nor 1e-3 apart"
        order = keep[np.argsort(-s, kind="stable")][:K]
        out.append((order, convert(boxes[b, order], sizes[b], fmt, clip)))
    return out


def device_case(B, Q, C, wide=False):
    logits, boxes, sizes, bg, _, _ = case(B, Q, C)
    lg = torch.from_numpy(logits.copy()).to(DEV)
    if wide:                                                                         # a slice of a wider tensor: row stride C + 8
        buf = torch.full((B, Q, C + 8), 50.0, device=DEV)
        buf[:, :, 3:3 + C] = lg
        lg = buf[:, :, 3:3 + C]
        assert not lg.is_contiguous() and lg.stride(-1) == 1
    return {"pred_logits": lg, "pred_boxes": torch.from_numpy(boxes.copy()).to(DEV)}, sizes.copy(), bg


def postprocess_scores(B, Q, C, background=None):
    """What detr_hip_postprocess returns: per image {query: (label, score bits)} of the non-background queries."""
    from detr_tf.inference import get_model_inference_batched
    out, _, bg = device_case(B, Q, C)
    _, _, _, _, score, label = case(B, Q, C)
    bg = bg if background is None else background
    res = []
    for b, (_, labels, scores) in enumerate(get_model_inference_batched(out, bg)):
        queries = np.nonzero(label[b] != bg)[0]                                      # query order is preserved
        assert len(queries) == labels.shape[0]
        res.append(dict(zip(queries.tolist(), zip(labels.tolist(), scores.cpu().numpy().view(np.int32).tolist()))))
    return res


def check(B, Q, C, thr, K, fmt, clip, wide=False):
    from detr_tf.inference import _detect
    want = oracle(B, Q, C, thr, Q if K is None else K, fmt, clip)
    out, sizes, bg = device_case(B, Q, C, wide)
    raw = [t.cpu().numpy() for t in _detect(out["pred_logits"], out["pred_boxes"], sizes, bg, thr, K, fmt, clip)]
    g_boxes, g_labels, g_scores, g_query, g_counts = raw
    post = postprocess_scores(B, Q, C)
    logits, _, _, _, score, label = case(B, Q, C)
    worst = 0.0
    for b, (order, boxes) in enumerate(want):
        k = len(order)
        assert g_counts[b] == k, (b, g_counts[b], k)
        assert g_query[b, :k].tolist() == order.tolist(), b                          # the order, ties in ascending query index
        assert g_labels[b, :k].tolist() == label[b, order].tolist(), b
        for r in range(1, k):
            if (logits[b, order[r]] == logits[b, order[r - 1]]).all():
                assert order[r - 1] < order[r]
        # scores and labels: the bits of detr_hip_postprocess
        assert [post[b][q] for q in order.tolist()] == list(zip(g_labels[b, :k].tolist(), g_scores[b, :k].view(np.int32).tolist())), b
        assert np.abs(g_scores[b, :k] - score[b, order]).max(initial=0.0) < 1e-6
        err = float(np.abs(g_boxes[b, :k].astype(np.float64) - boxes).max(initial=0.0))
        worst = max(worst, err / box_bound(*sizes[b]))
        assert err <= box_bound(*sizes[b]), (b, fmt, err, box_bound(*sizes[b]))
        for t in (g_boxes, g_labels, g_scores, g_query):                             # the tail rows are zero
            assert not t[b, k:].any(), b
    print(f"B={B} Q={Q} C={C} thr={thr:.3f} K={K} {fmt} clip={clip}: counts {g_counts.tolist()}, worst box error {worst:.2f} of the bound")
    return raw


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Q,C", SHAPES)
def test_detect_matches_the_fp64_chain(hip, B, Q, C):
    for fmt in FORMATS:
        check(B, Q, C, THRESHOLD, None, fmt, True)
    check(B, Q, C, 0.0, None, "xyxy", False)                                         # every foreground query, ties included, unclipped
    check(B, Q, C, 0.0, None, "xywh", False)
    check(B, Q, C, 0.0, 1, "yxyx", True)                                             # max_detections = 1
    check(B, Q, C, THRESHOLD, max(1, Q // 7), "xywh", True)                          # a cut inside the kept list
    check(B, Q, C, 0.0, Q, "xy_center", True)                                        # max_detections = Q
    if Q >= 37:
        kept = [len(o) for o, _ in oracle(B, Q, C, 0.0, Q, "xyxy", True)]
        assert min(kept) >= 5 and all(k < Q for k in kept)                           # foreground and background queries are both there
        logits = case(B, Q, C)[0]
        for b, (order, _) in enumerate(oracle(B, Q, C, 0.0, Q, "xyxy", True)):       # ... and so are exact ties, next to each other
            assert sum(bool((logits[b, i] == logits[b, j]).all()) for i, j in zip(order[:-1], order[1:])) >= 2


def test_detect_takes_strided_logits(hip):
    a = check(3, 37, 5, THRESHOLD, None, "xyxy", True, wide=True)
    b = check(3, 37, 5, THRESHOLD, None, "xyxy", True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_detect_threshold_is_inclusive(hip):
    """A score read back from detr_hip_postprocess as the threshold keeps that query (>=); the next float above drops it."""
    from detr_tf.inference import detect_batched
    B, Q, C = 2, 100, 92
    out, sizes, bg = device_case(B, Q, C)
    post = postprocess_scores(B, Q, C)
    for b in range(B):
        q, (_, bits) = sorted(post[b].items())[len(post[b]) // 2]
        s = np.array([bits], np.int32).view(np.float32)[0]
        at = detect_batched(out, sizes, bg, score_threshold=float(s))[b]
        above = detect_batched(out, sizes, bg, score_threshold=float(np.nextafter(s, np.float32(2.0))))[b]
        assert q in at.query.tolist() and q not in above.query.tolist()
        assert at.scores.min().item() == float(s)
        assert len(above.query) < len(at.query) and set(above.query.tolist()) < set(at.query.tolist())


def test_detect_all_background_and_caps(hip):
    from detr_tf.inference import _detect, detect_batched
    B, Q, C = 3, 37, 5
    logits = np.zeros((B, Q, C), np.float32)
    logits[:, :, 2] = 3.0                                                            # every query predicts class 2
    out = {"pred_logits": torch.from_numpy(logits).to(DEV), "pred_boxes": torch.rand(B, Q, 4, device=DEV)}
    sizes = [(48, 64)] * B
    raw = _detect(out["pred_logits"], out["pred_boxes"], sizes, 2, 0.0, None, "xyxy", True)
    assert raw[4].tolist() == [0, 0, 0] and all(not t.any() for t in raw) and raw[0].shape == (B, Q, 4)
    dets = detect_batched(out, sizes, 2)
    assert all(d.boxes.shape == (0, 4) and d.labels.shape == (0,) and d.scores.shape == (0,) and d.query.shape == (0,) for d in dets)
    # the same rows as foreground: Q exact ties, kept in query order; max_detections 1 and Q
    full = detect_batched(out, sizes, 4, max_detections=Q)
    assert all(d.query.tolist() == list(range(Q)) and d.labels.tolist() == [2] * Q for d in full)
    one = detect_batched(out, sizes, 4, max_detections=1)
    assert all(d.query.tolist() == [0] and d.boxes.shape == (1, 4) for d in one)
    assert full[0].labels.dtype == torch.int64 and full[0].query.dtype == torch.int32 and full[0].boxes.dtype == torch.float32
    with pytest.raises(RuntimeError, match="max_detections"):
        detect_batched(out, sizes, 4, max_detections=Q + 1)
    with pytest.raises(RuntimeError, match="sizes"):
        detect_batched(out, sizes[:2], 4)


def test_detect_clip(hip):
    """A box centred at 0.01 with width 0.5 reaches left of the image: clip=0 leaves x0 negative, clip=1 gives 0 and the xywh
    width shrinks to the clipped extent."""
    from detr_tf.inference import detect_batched
    logits = torch.tensor([[[4.0, 0.0, 0.0]]], device=DEV)
    boxes = torch.tensor([[[0.01, 0.5, 0.5, 0.25]]], device=DEV)
    out = {"pred_logits": logits, "pred_boxes": boxes}
    size = [(480, 640)]
    H, W = 480.0, 640.0
    bound = box_bound(480, 640)
    want_x0, want_x1 = 0.01 * W - 0.25 * W, 0.01 * W + 0.25 * W                     # -153.6, 166.4
    free = detect_batched(out, size, 2, bbox_format="xywh", clip=False)[0].boxes[0].tolist()
    assert free[0] < -153.0 and abs(free[0] - want_x0) <= bound and abs(free[2] - 0.5 * W) <= bound
    clipped = detect_batched(out, size, 2, bbox_format="xywh", clip=True)[0].boxes[0].tolist()
    assert clipped[0] == 0.0 and abs(clipped[2] - want_x1) <= bound and clipped[2] < 0.3 * W
    assert abs(clipped[1] - 0.375 * H) <= bound and abs(clipped[3] - 0.25 * H) <= bound
    xyxy = detect_batched(out, size, 2, bbox_format="xyxy", clip=False)[0].boxes[0].tolist()
    assert xyxy[0] < 0.0 and detect_batched(out, size, 2, bbox_format="xyxy", clip=True)[0].boxes[0].tolist()[0] == 0.0
    centre = detect_batched(out, size, 2, bbox_format="xy_center", clip=True)[0].boxes[0].tolist()       # never clipped
    assert np.abs(np.array(centre) - np.array([0.01 * W, 0.5 * H, 0.5 * W, 0.25 * H])).max() <= bound


def test_detect_is_deterministic(hip):
    from detr_tf.inference import _detect
    out, sizes, bg = device_case(2, 1024, 4)
    a = _detect(out["pred_logits"], out["pred_boxes"], sizes, bg, 0.0, None, "xywh", True)
    b = _detect(out["pred_logits"], out["pred_boxes"], sizes, bg, 0.0, None, "xywh", True)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ---- Detector --------------------------------------------------------------------------------------------------------------------
def _config():
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.image_size = (64, 96)
    return cfg


@pytest.fixture(scope="module")
def model(hip):
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref as R
    m = get_detr_model(_config(), include_top=True, num_encoder_layers=1, num_decoder_layers=1, dropout=0.0)
    assert not m.load_weights(R.make_params(2, num_enc=1, num_dec=1))
    return m


def _images():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((96, 128), (120, 80))]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            assert s.dtype == t.dtype and s.shape == t.shape and s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()


def test_detector_equals_the_hand_assembled_padded_chain(hip, model):
    from detr_tf.data import transformation as T
    from detr_tf.data.processing import DeviceInputStage
    from detr_tf.inference import Detections, Detector, detect_batched
    cfg, imgs = _config(), _images()
    canvas = (96, 96)
    det = Detector(model, cfg, score_threshold=0.0, max_detections=20, shortest_side=64, max_size=96, canvas=canvas)
    first = det(imgs)                                                                # eager: the first sighting of the shape
    assert len(first) == 2 and all(isinstance(d, Detections) and 1 <= d.scores.shape[0] <= 20 for d in first)
    # the chain by hand: the same records -> augmented_padded -> model((images, masks)) -> detect_batched with the ORIGINAL sizes
    recs = [T.eval_record(96, 128, 64, 96, T.CUBIC), T.eval_record(120, 80, 64, 96, T.CUBIC)]
    assert [(r.hd, r.wd) for r in recs] == [(64, 85), (96, 64)] and recs == det.records(imgs)
    x, m = DeviceInputStage(cfg).augmented_padded(imgs, recs, canvas=canvas)
    hand = detect_batched(model((x, m), training=False), [(96, 128), (120, 80)], 91, score_threshold=0.0, max_detections=20)
    _same(first, hand)
    assert model._eval_graph is not None                                             # the second forward of the shape was recorded
    recorded = model._eval_graph["graph"]
    _same(det(imgs), first)                                                          # replayed
    _same(det(imgs), first)
    assert model._eval_graph["graph"] is recorded
    # boxes are pixels of each image's own size, whatever the canvas
    for d, (h, w) in zip(first, ((96, 128), (120, 80))):
        b = d.boxes.cpu().numpy()
        assert (b >= 0).all() and (b[:, [0, 2]] <= w).all() and (b[:, [1, 3]] <= h).all()
        s = d.scores.cpu().numpy()
        assert (np.diff(s) <= 0).all() and (d.labels != 91).all()
    _same([det(imgs[1])], det([imgs[1]]))                                            # one array in, one Detections out
    # need_weights is passed through: the maps come back next to the same detections
    dets, maps = det(imgs, need_weights=True)
    _same(dets, first)
    assert len(maps) == 2 and all(v.shape[0] == 2 and v.shape[-2:] == (3, 3) for v in maps.values())


def test_detector_fixed_equals_the_hand_assembled_chain(hip, model):
    from detr_tf.data.processing import DeviceInputStage
    from detr_tf.inference import Detector, detect_batched
    cfg = _config()
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (120, 80, 3)).astype(np.uint8) for _ in range(2)]
    det = Detector(model, cfg, score_threshold=0.0, max_detections=10, bbox_format="xywh", resize="fixed")
    got = det(imgs)
    x = DeviceInputStage(cfg, interpolation="cubic").images(np.stack(imgs))
    assert tuple(x.shape) == (2, 64, 96, 3)
    hand = detect_batched(model(x, training=False), [(120, 80)] * 2, 91, score_threshold=0.0, max_detections=10, bbox_format="xywh")
    _same(got, hand)
    assert all(1 <= d.scores.shape[0] <= 10 for d in got)
    recs = det.to_coco_results(got, [7, 8])
    assert len(recs) == sum(d.scores.shape[0] for d in got) and recs[0]["image_id"] == 7 and recs[-1]["image_id"] == 8
    assert recs[0]["bbox"] == got[0].boxes[0].tolist() and recs[0]["score"] == got[0].scores[0].item()
    with pytest.raises(ValueError, match="ONE size"):
        det([imgs[0], imgs[0][:100]])
