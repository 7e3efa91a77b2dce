"""Multi-label detections on the device: detr_hip_detect_multilabel and detr_hip_postprocess_multilabel against the float64 rule
of tests/multilabel_ref.py -- every row of every output, three images per launch, one regime each --, the bits they share with the
entry points that exist (detr_hip_detect_scored's scores and boxes, detr_hip_postprocess's boxes), the rejections, and the
`multilabel` keyword through Detector and eval_model."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import multilabel_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 2, 0), (1, 2, 1), (5, 65, 64), (100, 92, 91), (100, 130, 0), (300, 92, 91), (1024, 3, 1)]     # (Q, C, background)
KS = (1, 7, 100, 300, 1024)
SIZES = np.array([(96, 128), (120, 80), (64, 64)], np.int32)


def ks_of(Q, C):
    """The K that make a distinct case: every K <= Q * (C - 1), and the first one above it (K > candidates; the rest repeat it)."""
    pairs = Q * (C - 1)
    return [k for k in KS if k <= pairs] + [k for k in KS if k > pairs][:1]


CASES = [(Q, C, bg, K) for Q, C, bg in SHAPES for K in ks_of(Q, C)]
J_KINDS = ("none", "K-1", "K", "K+1")


def case_id(case):
    return "Q%d-C%d-bg%d-K%d" % case


@functools.lru_cache(maxsize=None)
def shared_images(Q, C, bg):
    """Images 0 and 1 and the boxes of a shape, computed once; nobody writes to them."""
    rng = np.random.default_rng(100000 * Q + 100 * C + bg)
    boxes = np.empty((3, Q, 4), np.float32)
    boxes[..., :2] = rng.uniform(0.0, 1.0, (3, Q, 2))                 # centres up to the edge: half of a box may leave the image
    boxes[..., 2:] = rng.uniform(0.02, 0.6, (3, Q, 2))
    out = MR.grid_image(rng, Q, C, bg), MR.equal_image(Q, C), boxes
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def make_case(Q, C, bg, K, thr, j_kind):
    """(logits [3, Q, C], boxes [3, Q, 4], [the reference's (query, label, score) per image])."""
    grid, equal, boxes = shared_images(Q, C, bg)
    pairs = Q * (C - 1)
    j = min(pairs, {"none": 0, "K-1": K - 1, "K": K, "K+1": K + 1}[j_kind])
    counted = MR.counted_image(np.random.default_rng(7 * Q + C + K + j), Q, C, bg, j)
    logits = np.stack([grid, equal, counted])
    want = [reference(Q, C, bg, K, thr, 0), reference(Q, C, bg, K, thr, 1), MR.topk_pairs(counted, bg, thr, K)]
    if thr == MR.MID:
        assert len(want[2][0]) == min(j, K)
    return logits, boxes, want


@functools.lru_cache(maxsize=None)
def reference(Q, C, bg, K, thr, image):
    return MR.topk_pairs(shared_images(Q, C, bg)[image], bg, thr, K)


def g(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: the shared arrays are read-only)


def strided(a, pad):
    """The same values as a view whose row stride is larger than its row."""
    wide = torch.full(a.shape[:-1] + (a.shape[-1] + pad,), 7.0, device=DEV)
    wide[..., :a.shape[-1]] = g(a)
    return wide[..., :a.shape[-1]]


def detect_ml(lg, bx, bg, thr, K, fmt="xyxy", clip=True, sizes=SIZES):
    from detr_tf.inference import _detect
    rows = _detect(lg, bx, sizes, bg, thr, K, fmt, clip, "sigmoid", True)
    torch.cuda.synchronize()
    return [t.cpu() for t in rows]                                    # boxes, labels, scores, query, counts


def post_ml(lg, bx, bg, thr, K, fmt):
    from detr_tf.inference import _post_multilabel
    rows = _post_multilabel(lg, bx, bg, fmt, K, thr)
    torch.cuda.synchronize()
    return [t.cpu() for t in rows]                                    # boxes, labels, scores, counts


def boxes_of_all_queries(bx, Q, C, bg, fmt, clip=True, sizes=SIZES):
    """[B, Q, 4]: the box detr_hip_detect_scored emits for every query -- a call on equal logits keeps all Q queries in query order."""
    from detr_tf.inference import _detect
    flat = torch.zeros(bx.shape[0], Q, C, device=DEV)
    boxes, _, _, query, counts = _detect(flat, bx, sizes, bg, 0.0, None, fmt, clip, "sigmoid")
    assert counts.tolist() == [Q] * bx.shape[0] and query.tolist() == [list(range(Q))] * bx.shape[0]
    return boxes.cpu()


def post_boxes_of_all_queries(bx, Q, C, bg, fmt):
    from detr_tf.inference import _post
    boxes, _, _, counts = _post(torch.zeros(bx.shape[0], Q, C, device=DEV), bx, bg, fmt, "sigmoid")
    assert counts.tolist() == [Q] * bx.shape[0]
    return boxes.cpu()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


def check_case(Q, C, bg, K, thr, j_kind):
    logits, boxes, want = make_case(Q, C, bg, K, thr, j_kind)
    lg, bx = g(logits), g(boxes)
    got = detect_ml(lg, bx, bg, thr, K)
    d_boxes, d_labels, d_scores, d_query, d_counts = got
    assert d_boxes.shape == (3, K, 4) and d_labels.dtype == torch.int64 and d_query.dtype == torch.int32
    all_boxes = boxes_of_all_queries(bx, Q, C, bg, "xyxy")
    worst = 0.0
    for b, (q, c, s) in enumerate(want):
        n = len(q)
        assert int(d_counts[b]) == n, (b, int(d_counts[b]), n)
        assert d_query[b, :n].tolist() == q.tolist(), b
        assert d_labels[b, :n].tolist() == c.tolist(), b
        if n:
            worst = max(worst, float(np.abs(d_scores[b, :n].numpy().astype(np.float64) - s).max()))
            assert same_bytes(d_boxes[b, :n], all_boxes[b, torch.from_numpy(q).long()])           # detr_hip_detect_scored's box of that query
        for rows in (d_boxes, d_labels, d_scores, d_query):                                       # rows past the count are zero
            assert not rows[b, n:].numpy().view(np.uint8).any(), b
    print(f"Q{Q} C{C} bg{bg} K{K} thr{thr:.4f} {j_kind}: counts {d_counts.tolist()}, max score err {worst:.3e}, bound {MR.SCORE_BOUND:.0e}")
    assert worst <= MR.SCORE_BOUND
    # a second launch gives identical bytes, and so does a strided view of the same values
    for again in (detect_ml(lg, bx, bg, thr, K), detect_ml(strided(logits, 5), strided(boxes, 4), bg, thr, K)):
        assert all(same_bytes(a, b) for a, b in zip(again, got))
    # detr_hip_postprocess_multilabel: the same selection; the boxes are detr_hip_postprocess's of those queries
    p_boxes, p_labels, p_scores, p_counts = post_ml(lg, bx, bg, thr, K, "yxyx")
    assert same_bytes(p_counts, d_counts) and same_bytes(p_labels, d_labels) and same_bytes(p_scores, d_scores)
    unit = post_boxes_of_all_queries(bx, Q, C, bg, "yxyx")
    for b in range(3):
        n = int(d_counts[b])
        assert same_bytes(p_boxes[b, :n], unit[b, d_query[b, :n].long()]) and not p_boxes[b, n:].numpy().view(np.uint8).any()
    return want


@pytest.mark.parametrize("j_kind", J_KINDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_three_regimes_at_the_middle_threshold(hip, case, j_kind):
    Q, C, bg, K = case
    want = check_case(Q, C, bg, K, MR.MID, j_kind)
    pairs = Q * (C - 1)
    assert len(want[1][0]) == min(K, pairs)                                      # the image of equal logits: the first K flat indexes
    if pairs >= 9100 and K >= 7:                                                 # the random grid image: ties straddle the cut
        more = reference(Q, C, bg, K + 1, MR.MID, 0)[2]
        assert len(more) == K + 1 and abs(more[K] - more[K - 1]) < MR.SAME


@pytest.mark.parametrize("thr", [MR.THRESHOLDS[0], MR.THRESHOLDS[2]], ids=["thr0", "thr1.5"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_threshold_that_passes_everything_and_the_one_that_passes_nothing(hip, case, thr):
    Q, C, bg, K = case
    want = check_case(Q, C, bg, K, thr, "K")
    if thr > 1:
        assert [len(w[0]) for w in want] == [0, 0, 0]
    elif Q * (C - 1) >= 5:                                                       # the NaN is no candidate, the 0.0 of the -inf is one
        grid = shared_images(Q, C, bg)[0]
        assert np.isnan(grid).sum() == 1 and np.isneginf(grid).sum() == 1
        everything = reference(Q, C, bg, 1024, thr, 0) if Q * (C - 1) <= 1024 else None
        if everything is not None:
            assert len(everything[0]) == Q * (C - 1) - 1 and everything[2][-1] == 0.0


@pytest.mark.parametrize("Q,bg", [(1, 0), (1, 1), (100, 0), (300, 1)])
def test_with_one_real_class_it_is_detect_scored(hip, Q, bg):
    """C = 2: every query has one real class, so the whole output equals detect_batched(scoring="sigmoid") byte for byte."""
    from detr_tf.inference import _detect
    rng = np.random.default_rng(Q + bg)
    logits = rng.choice(MR.GRID, (3, Q, 2)).astype(np.float32)
    logits[0, Q // 2, 1 - bg] = np.nan
    logits[1, Q // 3, 1 - bg] = -np.inf
    logits[2, :, 1 - bg] = 1.25                                                 # all tie
    lg, bx = g(logits), g(shared_images(Q, 2, bg)[2])
    for K in [k for k in KS if k <= Q]:
        for thr in (0.0, MR.MID):
            old = _detect(lg, bx, SIZES, bg, thr, K, "xyxy", True, "sigmoid")
            new = detect_ml(lg, bx, bg, thr, K)
            assert all(same_bytes(a.cpu(), b) for a, b in zip(old, new)), (K, thr)
            assert int(new[4].sum()) > 0 or Q == 1


def test_every_box_format_and_clip(hip):
    from detr_tf.inference import DETECT_FORMATS, BBOX_FORMATS
    Q, C, bg, K = 5, 65, 64, 100
    logits, boxes, _ = make_case(Q, C, bg, K, MR.MID, "K")
    lg, bx = g(logits), g(boxes)
    seen = set()
    for fmt in DETECT_FORMATS:
        for clip in (True, False):
            d_boxes, _, _, d_query, d_counts = detect_ml(lg, bx, bg, MR.MID, K, fmt, clip)
            all_boxes = boxes_of_all_queries(bx, Q, C, bg, fmt, clip)
            for b in range(3):
                n = int(d_counts[b])
                assert n > 0 and same_bytes(d_boxes[b, :n], all_boxes[b, d_query[b, :n].long()]), (fmt, clip, b)
            seen.add(d_boxes.numpy().tobytes())
    assert len(seen) == 7                                                        # xy_center is never clipped; everything else differs
    for fmt in BBOX_FORMATS:
        p_boxes, _, _, p_counts = post_ml(lg, bx, bg, MR.MID, K, fmt)
        unit = post_boxes_of_all_queries(bx, Q, C, bg, fmt)
        for b in range(3):
            n = int(p_counts[b])
            assert n == int(d_counts[b]) and same_bytes(p_boxes[b, :n], unit[b, d_query[b, :n].long()]), (fmt, b)


def test_rejections(hip):
    """Every rejection happens on the host, before a launch, with its message."""
    lib = hip.load()
    keep = [torch.zeros(64, device=DEV) for _ in range(8)]

    def detect_desc(**kw):
        d = hip.DetectDesc()
        d.B, d.Q, d.C, d.background_class, d.bbox_format, d.clip, d.max_detections, d.score_threshold = 1, 4, 3, 2, 1, 1, 4, 0.0
        for fld, t in zip(("logits", "boxes", "sizes", "out_boxes", "out_labels", "out_scores", "out_query", "counts"), keep):
            setattr(d, fld, t.data_ptr())
        d.sL_b, d.sL_q, d.sB_b, d.sB_q = 12, 3, 16, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def post_desc(**kw):
        d = hip.PostprocessDesc()
        d.B, d.Q, d.C, d.background_class, d.bbox_format = 1, 4, 3, 2, 2
        for fld, t in zip(("logits", "boxes", "out_boxes", "out_labels", "out_scores", "counts"), keep):
            setattr(d, fld, t.data_ptr())
        d.sL_b, d.sL_q, d.sB_b, d.sB_q = 12, 3, 16, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(rc, text):
        message = lib.detr_hip_last_error().decode()
        assert rc == -1 and text in message, (rc, message)

    det, post = lib.detr_hip_detect_multilabel, lib.detr_hip_postprocess_multilabel
    assert det(ctypes.byref(detect_desc()), hip._stream()) == 0 and post(ctypes.byref(post_desc()), 4, 0.0, hip._stream()) == 0
    torch.cuda.synchronize()
    for kw, text in ((dict(C=1, background_class=0, sL_q=1), "needs a class beside the background class, C=1"),
                     (dict(background_class=3), "background_class=3 outside [0, C=3)"),
                     (dict(background_class=-1), "background_class=-1 outside [0, C=3)"),
                     (dict(logits=None), "null operand"), (dict(counts=None), "null operand"),
                     (dict(Q=1025), "bad shape"), (dict(sL_q=2), "strides")):
        refused(det(ctypes.byref(detect_desc(**kw)), None), "detect_multilabel: ")
        refused(det(ctypes.byref(detect_desc(**kw)), None), text)
        refused(post(ctypes.byref(post_desc(**kw)), 4, 0.0, None), "postprocess_multilabel: ")
        refused(post(ctypes.byref(post_desc(**kw)), 4, 0.0, None), text)
    for K in (0, 1025, -3):
        refused(det(ctypes.byref(detect_desc(max_detections=K)), None), f"max_detections={K} must be in 1..1024")
        refused(post(ctypes.byref(post_desc()), K, 0.0, None), f"max_detections={K} must be in 1..1024")
    for thr in (float("nan"), float("inf"), float("-inf")):
        refused(det(ctypes.byref(detect_desc(score_threshold=thr)), None), "score_threshold is not finite")
        refused(post(ctypes.byref(post_desc()), 4, thr, None), "score_threshold is not finite")
    refused(det(None, None), "null descriptor")
    refused(post(None, 4, 0.0, None), "null descriptor")
    refused(det(ctypes.byref(detect_desc(out_query=None)), None), "null operand")
    refused(det(ctypes.byref(detect_desc(bbox_format=4)), None), "bbox_format")
    refused(post(ctypes.byref(post_desc(bbox_format=3)), 4, 0.0, None), "bbox_format")
    refused(post(ctypes.byref(post_desc(out_boxes=keep[2].data_ptr() + 4)), 4, 0.0, None), "16-byte aligned")
    # through the Python surface
    from detr_tf.inference import detect_batched
    out = {"pred_logits": torch.zeros(1, 4, 1, device=DEV), "pred_boxes": torch.full((1, 4, 4), 0.5, device=DEV)}
    with pytest.raises(RuntimeError, match="C=1"):
        detect_batched(out, [(8, 8)], 0, scoring="sigmoid", multilabel=True)
    with pytest.raises(ValueError, match="multilabel"):
        detect_batched(out, [(8, 8)], 0, multilabel=True)


# ---- Detector and evaluation: the tiny model of tests/test_gpu_focal.py (one encoder layer, one decoder layer, random weights).
# Its logits are not on a grid, so paths that share the kernel are compared, not the reference.
def _config(criterion="focal"):
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.image_size = (64, 96)
    cfg.class_criterion = criterion
    return cfg


@pytest.fixture(scope="module")
def model(hip):
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref as R
    m = get_detr_model(_config("softmax"), include_top=True, num_encoder_layers=1, num_decoder_layers=1, dropout=0.0)
    assert not m.load_weights(R.make_params(2, num_enc=1, num_dec=1))
    return m


def test_detector_with_multilabel(hip, model):
    from detr_tf.data import transformation as T
    from detr_tf.data.processing import DeviceInputStage
    from detr_tf.inference import Detections, Detector, Tracker, detect_batched
    cfg = _config()
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((96, 128), (120, 80))]
    canvas, K = (96, 96), 150                                                   # K > Q = 100: some query must emit two classes
    kw = dict(score_threshold=0.0, max_detections=K, shortest_side=64, max_size=96, canvas=canvas)
    det = Detector(model, cfg, multilabel=True, **kw)
    assert det.scoring == "sigmoid" and det.multilabel
    got = det(imgs)
    recs = [T.eval_record(96, 128, 64, 96, T.CUBIC), T.eval_record(120, 80, 64, 96, T.CUBIC)]
    x, m = DeviceInputStage(cfg).augmented_padded(imgs, recs, canvas=canvas)
    out = model((x, m), training=False)
    hand = detect_batched(out, [(96, 128), (120, 80)], 91, score_threshold=0.0, max_detections=K, scoring="sigmoid", multilabel=True)
    per_query = detect_batched(out, [(96, 128), (120, 80)], 91, score_threshold=0.0, scoring="sigmoid")
    for d, h, one in zip(got, hand, per_query):
        assert isinstance(d, Detections) and d.scores.shape[0] == K
        assert all(same_bytes(s.cpu(), t.cpu()) for s, t in zip(d, h))
        q = d.query.cpu().numpy()
        assert len(set(q.tolist())) < K and 0 <= q.min() and q.max() < 100       # at least one query repeats
        assert (np.diff(d.scores.cpu().numpy()) <= 0).all() and bool((d.labels != 91).all())
        pairs = (q.astype(np.int64) * 92 + d.labels.cpu().numpy()).tolist()
        assert len(set(pairs)) == K                                              # ... but no (query, class) pair does
        # the best pair overall is the best query's best class: the first row of the per-query rule, bit for bit
        assert all(same_bytes(s[:1].cpu(), t[:1].cpu()) for s, t in zip(d, one))
    # the rows have the layout of the per-query ones: track(), draw() and to_coco_results() take them
    tracker = Tracker(streams=2, track_threshold=0.0, min_hits=1)
    tracked = [det.track(imgs, tracker) for _ in range(2)][-1]
    assert len(tracked) == 2 and all(t.boxes.shape[0] > 0 and t.boxes.shape[0] == t.ids.shape[0] for t in tracked)
    drawn = det.draw(None, got, [f"c{i}" for i in range(92)])
    assert len(drawn) == 2 and tuple(drawn[0].shape) == (96, 128, 3) and drawn[0].dtype == torch.uint8
    coco = Detector(model, cfg, multilabel=True, bbox_format="xywh", **kw)
    records = coco.to_coco_results(coco(imgs), [7, 8])
    assert len(records) == 2 * K and {r["image_id"] for r in records} == {7, 8} and all(len(r["bbox"]) == 4 for r in records)
    # the default is the per-query rule, as before
    plain = Detector(model, cfg, score_threshold=0.0, max_detections=100, shortest_side=64, max_size=96, canvas=canvas)(imgs)
    assert all(same_bytes(s.cpu(), t.cpu()) for d, one in zip(plain, per_query) for s, t in zip(d, one))
    assert all(len(set(d.query.tolist())) == 100 for d in plain)


def _eval_batches(coco):
    from oracle import set_loss_ref as L
    rng = np.random.default_rng(11)
    batches = []
    for i in range(2):
        tb, tc = L.make_targets(2, seed=40 + i, force_full=False)
        batch = (rng.normal(size=(2, 64, 96, 3)).astype(np.float32), tb, tc)
        if coco:
            n = tb[:, 0, 0].astype(np.int64)
            crowd = (rng.random(tb.shape[:2]) < 0.2).astype(np.uint8)
            area = (tb[..., 2] * 96 * tb[..., 3] * 64).astype(np.float32)
            for b in range(2):
                crowd[b, 0] = 0
                crowd[b, 1 + n[b]:] = 0
            batch += ({"crowd": crowd, "area": area, "size": np.array([(64, 96)] * 2, np.int32)},)
        batches.append(batch)
    return batches


@pytest.mark.parametrize("protocol", ["reference", "coco"])
def test_eval_model_with_multilabel(hip, model, protocol):
    from detr_tf.evaluation import eval_model
    from detr_tf.loss.coco_eval import DeviceCOCOAccumulator
    from detr_tf.loss.compute_map import DeviceAPAccumulator
    names = [f"c{i}" for i in range(92)]
    batches = _eval_batches(protocol == "coco")
    focal, softmax = _config(), _config("softmax")
    for K in (100, 150):
        kw = dict(print_result=False, protocol=protocol, scoring="sigmoid", multilabel=True, max_detections=K)
        host = eval_model(model, focal, names, iter(batches), **kw)
        device = eval_model(model, focal, names, iter(batches), accumulate="device", **kw)
        assert host == device
        assert eval_model(model, focal, names, iter(batches), print_result=False, protocol=protocol, multilabel=True, max_detections=K) == host
    # the matcher's row capacity is K
    out = model(batches[0][0], training=False)
    if protocol == "coco":
        acc = DeviceCOCOAccumulator(92, device=out["pred_logits"].device)
        acc.add_batch(out, batches[0][1], batches[0][2], batches[0][3], 91, "sigmoid", 150)
    else:
        acc = DeviceAPAccumulator(92, device=out["pred_logits"].device)
        acc.add_batch(out, batches[0][1], batches[0][2], 91, "sigmoid", 150)
    assert tuple(acc._records[-1].shape[1:]) == (2, 150)
    acc.to_host()
    # the defaults reproduce an evaluation without the keyword, bit for bit, under both scorings
    for cfg in (focal, softmax):
        for how in ("host", "device"):
            before = eval_model(model, cfg, names, iter(batches), print_result=False, protocol=protocol, accumulate=how)
            after = eval_model(model, cfg, names, iter(batches), print_result=False, protocol=protocol, accumulate=how, multilabel=False,
                               max_detections=100)
            assert before == after
    with pytest.raises(ValueError, match="multilabel"):
        eval_model(model, softmax, names, iter(batches), print_result=False, protocol=protocol, multilabel=True)
