"""csrc/fuse_views.hip on the device: detr_hip_fuse_views (inference.fuse_views) against the NumPy restatement of
tests/fuse_views_ref.py -- EXACTLY for hard NMS, linear soft-NMS and weighted box fusion: the kept set, its order, labels, query,
tile, members and counts equal, boxes and scores bit-equal; for Gaussian soft-NMS everything exact but the scores, which may differ
by one fp32 ulp (the device's fp64 exp and NumPy's may differ in the last bit; a kept score is the product of at most n such
factors, a relative difference below 2 n 2^-52, which moves the fp32 rounding only at a rounding boundary) and that only on inputs
whose selections and deaths the reference's gap counters show to be further than 2^-30 from any tie -- and the Detector with views
end to end against the chain assembled by hand.

The inputs are OBJECTS SEEN BY SEVERAL VIEWS, each view reporting each object with jitter, plus clutter; the reference's counters
are asserted on, so that a case that claims to exercise clusters of three, singletons, a candidate between two clusters or a join
that only the moved box allows really does.  Scores and labels come from detr_hip_detect, as in test_gpu_tiles.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fuse_views_ref as R
import tile_merge_ref as M

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
FORMATS = M.FORMATS
METHODS = R.METHODS
ARGS = ("score", "label", "boxes", "view_start", "windows", "flips", "sizes", "bg")  # fuse_views_ref.fuse's positional arguments
GAP = 2.0 ** -30


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def scores_labels(logits, bg):
    """fp32 score / label of every query as the device computes them: one detr_hip_detect launch over the N views, scattered back to
    [N, Q].  Background and NaN queries (which detect drops) come back as background: the fusion drops them too."""
    from detr_tf.inference import _detect
    N, Q, _ = logits.shape
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(DEV)
    _, out_l, out_s, out_q, counts = _detect(lg, torch.zeros(N, Q, 4, device=DEV), np.ones((N, 2), np.int32), bg, -1.0, Q, "xy_center", False)
    out_l, out_s, out_q, counts = out_l.cpu().numpy(), out_s.cpu().numpy(), out_q.cpu().numpy(), counts.cpu().numpy()
    score, label = np.zeros((N, Q), F), np.full((N, Q), bg, np.int64)
    for n in range(N):
        k = counts[n]
        score[n, out_q[n, :k]], label[n, out_q[n, :k]] = out_s[n, :k], out_l[n, :k]
    return score, label


def finish(case):
    case["score"], case["label"] = scores_labels(case["logits"], case["bg"])
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def outputs(case):
    return {"pred_logits": torch.from_numpy(case["logits"].copy()).to(DEV), "pred_boxes": torch.from_numpy(case["boxes"].copy()).to(DEV)}


def run(case, **kw):
    from detr_tf.inference import fuse_views
    return fuse_views(outputs(case), case["view_start"], case["windows"].copy(), case["flips"].copy(), case["sizes"].copy(), case["bg"], **kw)


def ulps(a, b):
    """distance of two arrays of positive float32 in units in the last place"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def same(got, want, method):
    """got: [FusedDetections]; want: fuse_views_ref.fuse's list.  Exact, but for the scores of the Gaussian method: one ulp."""
    assert len(got) == len(want)
    for g, (wb, wl, ws, wq, wt, wm, _) in zip(got, want):
        assert g.query.cpu().numpy().tolist() == wq.tolist() and g.tile.cpu().numpy().tolist() == wt.tolist()
        assert g.labels.dtype == torch.int64 and g.labels.cpu().numpy().tolist() == wl.tolist()
        assert g.members.dtype == torch.int32 and g.members.cpu().numpy().tolist() == wm.tolist()
        gs = g.scores.cpu().numpy()
        if method == "soft_nms_gaussian":
            assert gs.shape == ws.shape and (ulps(gs, ws) <= 1).all()
        else:
            assert gs.tobytes() == ws.tobytes()
        assert g.boxes.dtype == torch.float32 and tuple(g.boxes.shape) == wb.shape and g.boxes.cpu().numpy().tobytes() == wb.tobytes()


def reference(case, **kw):
    want = R.fuse(*(case[k] for k in ARGS), **kw)
    if kw.get("method", "wbf") == "soft_nms_gaussian":                 # no selection and no death may hang on exp's last bit
        assert all(w[6]["select_gap"] > GAP and w[6]["min_gap"] > GAP for w in want), [(w[6]["select_gap"], w[6]["min_gap"]) for w in want]
    return want


def check(case, **kw):
    """fuse_views == the reference; returns the reference's result."""
    want = reference(case, **kw)
    same(run(case, **kw), want, kw.get("method", "wbf"))
    return want


def make_case(seed, views, sizes, Q, C, n_obj, jitter=0.1, seen=0.85, clutter=0.15, spread=1.3, windows=None):
    """Seeded outputs of several views per image.  views: per image a list of flip flags, every view a whole-image window unless
    `windows` says otherwise.  Per image n_obj objects (label, box normalised to the image, sides 0.1 .. 0.35), the first two of one
    label and 0.35 of a width apart -- neighbours a fused box can drift between; query q < n_obj of a view reports object q with
    probability `seen`, every coordinate jittered by up to `jitter` of the side and boxes allowed to leave the image by `spread`;
    the other queries are clutter (a random foreground box) with probability `clutter`, else background.  The logit margins are
    moderate, so the scores spread over (0.3, 1) and equal fp32 scores are rare."""
    rng = np.random.default_rng(seed)
    N, bg = sum(len(v) for v in views), C - 1
    logits = rng.normal(0.0, 1.0, (N, Q, C)).astype(F)
    logits[:, :, bg] += 6.0
    boxes = np.concatenate([rng.random((N, Q, 2)), rng.uniform(0.05, 0.3, (N, Q, 2))], -1).astype(F)
    n = 0
    for b, flips in enumerate(views):
        k = min(n_obj, Q)
        obj = np.concatenate([(rng.random((k, 2)) - 0.5) * spread + 0.5, rng.uniform(0.1, 0.35, (k, 2))], -1)
        lab = rng.integers(0, max(bg, 1), k)
        if k >= 2:
            obj[1] = obj[0] + (0.35 * obj[0, 2], 0.0, 0.0, 0.0)
            lab[1] = lab[0]
        H, W = sizes[b]
        for flip in flips:
            y0, x0, hc, wc = (0, 0, H, W) if windows is None else windows[n]
            for q in range(Q):
                hot = (q < k and rng.random() < seen) or (q >= k and rng.random() < clutter)
                if not hot:
                    continue
                if q < k:
                    cx, cy, w, h = obj[q] + rng.uniform(-jitter, jitter, 4) * obj[q, [2, 3, 2, 3]]
                    px = (1.0 - cx if flip else cx) * W                 # a flipped view sees the mirrored image
                    boxes[n, q] = ((px - x0) / wc, (cy * H - y0) / hc, w * W / wc, h * H / hc)
                logits[n, q, bg] = -20.0
                logits[n, q, lab[q] if q < k else rng.integers(0, max(bg, 1))] += rng.uniform(1.0, 5.0)
            n += 1
    case = dict(logits=logits, boxes=boxes, view_start=np.concatenate([[0], np.cumsum([len(v) for v in views])]).astype(np.int32),
                windows=np.array([(0, 0) + tuple(sizes[b]) for b, v in enumerate(views) for _ in v] if windows is None else windows, np.int32),
                flips=np.array([f for v in views for f in v], np.int32), sizes=np.array(sizes, np.int32).reshape(-1, 2), bg=bg)
    return finish(case)


@functools.lru_cache(maxsize=None)
def two_images():
    """B = 2 with 2 views (flip) and 4 views (flip x two scales: the same windows), Q = 70 (no multiple of 64), C = 5."""
    return make_case(1, [(0, 1), (0, 0, 1, 1)], [(90, 120), (100, 200)], 70, 5, 12)


@functools.lru_cache(maxsize=None)
def six_views():
    """B = 1, 6 views x Q = 100, C = 7, half of the clutter kept too: more than 256 candidates at a low threshold, i.e. more than
    one compaction pass and more than one lane stride of the walk."""
    return make_case(2, [(0, 1, 0, 1, 0, 1)], [(300, 400)], 100, 7, 40, clutter=0.6)


def wbf_counters(want):
    return [w[6] for w in want]


# ---- the seeded inputs are what they claim to be ---------------------------------------------------------------------------------
def test_seeded_inputs_exercise_the_walk(hip):
    multi = moved = 0
    for case, thr in ((two_images(), 0.3), (six_views(), 0.05)):
        counters = wbf_counters(reference(case, method="wbf", score_threshold=thr, max_detections=600))
        sizes = [size for c in counters for size in c["sizes"]]
        assert max(sizes) >= 3 and min(sizes) == 1, counters                          # a cluster of three or more, and a singleton
        multi, moved = multi + sum(c["multi"] for c in counters), moved + sum(c["moved_joins"] for c in counters)
    assert multi >= 1 and moved >= 1                                                   # a candidate between two clusters; a join the moved box allowed
    assert reference(six_views(), method="wbf", score_threshold=0.05)[0][6]["candidates"] > 256


# ---- method 0 is merge_tiles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS[1:])
def test_nms_without_flips_equals_merge_tiles(hip, fmt):
    from detr_tf.inference import merge_tiles
    for case in (two_images(), six_views()):
        kw = dict(score_threshold=0.3, max_detections=80, bbox_format=fmt, match="ios", class_agnostic=True, edge_margin=2.0)
        plain = dict(case, flips=np.zeros_like(case["flips"]))
        want = merge_tiles(outputs(case), case["view_start"], case["windows"].copy(), case["sizes"].copy(), case["bg"], nms_threshold=0.4, **kw)
        got = run(plain, method="nms", threshold=0.4, **kw)
        assert sum(int(w.scores.shape[0]) for w in want) > 10
        for g, w in zip(got, want):
            for a, b in zip(g[:5], w):
                assert a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
            assert g.members.cpu().numpy().tolist() == [1] * int(w.scores.shape[0])


# ---- every option against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("match", ("iou", "ios"))
@pytest.mark.parametrize("agnostic", (False, True))
def test_methods_match_modes_and_class_agnostic(hip, method, match, agnostic):
    want = check(two_images(), method=method, score_threshold=0.3, match=match, class_agnostic=agnostic, max_detections=300)
    assert all(0 < len(w[3]) <= w[6]["candidates"] for w in want)
    if method == "wbf":
        members = np.concatenate([w[5] for w in want])
        assert members.max() >= 3 and members.min() == 1
    assert sorted(set(want[1][4].tolist())) != [0]                                     # results from more than the first view


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("clip", (True, False))
def test_formats_and_clip(hip, fmt, clip):
    case = two_images()
    for method in METHODS:
        want = check(case, method=method, score_threshold=0.3, bbox_format=fmt, clip=clip, max_detections=300)
        if fmt == "xyxy":                                                              # boxes do leave the image, and the clip holds them
            out = np.concatenate([w[0] for w in want])
            W = np.concatenate([[s[1]] * len(w[0]) for w, s in zip(want, case["sizes"])])
            assert (((out[:, 0] < 0) | (out[:, 2] > W)).any()) != clip


def test_six_views_every_method_and_reruns(hip):
    case = six_views()
    for method in METHODS:
        kw = dict(method=method, score_threshold=0.05, max_detections=400)
        want = check(case, **kw)
        assert want[0][6]["candidates"] > 256 and len(want[0][3]) > 100
        first, again = run(case, **kw), run(case, **kw)
        for a, b in zip(first[0], again[0]):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()              # a rerun gives the same bits
    want = check(case, method="wbf", score_threshold=0.05, max_detections=400, min_members=3, expected_views=6)
    assert 0 < len(want[0][3]) and want[0][5].min() >= 3
    want = check(case, method="wbf", score_threshold=0.05, max_detections=400, threshold=0.3, expected_views=2)
    assert want[0][5].max() > 6                                                        # neighbours merged at the looser threshold


def test_empty_single_and_full_images(hip):
    """B = 3: the first image has no candidate, the second exactly one, the third the usual."""
    base = make_case(3, [(0, 1), (0, 1), (0, 1)], [(64, 64), (90, 120), (100, 200)], 70, 5, 12)
    logits = base["logits"].copy()
    logits[:4, :, 4] = 20.0                                                            # images 0 and 1: everything background ...
    logits[3, 5, 4] = -20.0                                                            # ... but one query of image 1's flipped view
    case = finish(dict(base, logits=logits))
    for method in METHODS:
        want = check(case, method=method, score_threshold=0.3)
        assert [w[6]["candidates"] for w in want][:2] == [0, 1] and [len(w[3]) for w in want][:2] == [0, 1] and len(want[2][3]) > 1
        assert want[1][4].tolist() == [1] and want[1][3].tolist() == [5] and want[1][5].tolist() == [1]
    assert [len(w[3]) for w in check(case, method="wbf", score_threshold=0.3, min_members=2)][:2] == [0, 0]


@pytest.mark.parametrize("method", METHODS)
def test_one_query(hip, method):
    logits = np.array([[[2.0, 0.0]], [[1.0, 0.0]]], F)                                 # two views of Q = 1: scores 0.88 and 0.73, label 0
    boxes = np.array([[[0.25, 0.5, 0.25, 0.5]], [[0.75, 0.5, 0.25, 0.5]]], F)          # the second view is flipped: the same box
    case = finish(dict(logits=logits, boxes=boxes, view_start=np.array([0, 2], np.int32), windows=np.array([[0, 0, 8, 16]] * 2, np.int32),
                       flips=np.array([0, 1], np.int32), sizes=np.array([[8, 16]], np.int32), bg=1))
    want = check(case, method=method, score_threshold=0.5)
    assert want[0][0][0].tolist() == [2.0, 2.0, 6.0, 6.0]
    # the Gaussian method only decays the copy: 0.73 * exp(-1 / 0.5) stays above score_min
    assert want[0][5].tolist() == {"wbf": [2], "soft_nms_gaussian": [1, 1]}.get(method, [1])
    assert check(case, method=method, score_threshold=0.8)[0][5].tolist() == [1]


# ---- caps, tails and guard words -------------------------------------------------------------------------------------------------
GUARD = 64


def raw_fuse(case, K, method, **kw):
    """detr_hip_fuse_views called directly on output buffers with GUARD poisoned elements on both sides; asserts the guards are
    intact and returns the outputs, counts and the status word."""
    from detr_tf import _hip
    from detr_tf.inference import DETECT_FORMATS, MATCH_MODES
    lg, bx = torch.from_numpy(case["logits"].copy()).to(DEV), torch.from_numpy(case["boxes"].copy()).to(DEV)
    B, (N, Q, C) = len(case["sizes"]), lg.shape
    start_h = np.ascontiguousarray(case["view_start"], np.int32)
    start_d, win_d, size_d, flip_d = (torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)
                                      for a in (start_h, case["windows"], case["sizes"], case["flips"]))
    spec = dict(boxes=(B * K * 4, torch.float32, 1.5), labels=(B * K, torch.int64, -7), scores=(B * K, torch.float32, 2.5),
                query=(B * K, torch.int32, -7), tile=(B * K, torch.int32, -7), members=(B * K, torch.int32, -7), counts=(B, torch.int32, -7),
                status=(1, torch.int32, -7))
    bufs = {n: torch.full((GUARD + size + GUARD,), poison, dtype=dt, device=DEV) for n, (size, dt, poison) in spec.items()}
    bufs["status"][GUARD] = 0
    d = _hip.TileMergeDesc()
    d.B, d.N, d.Q, d.C = B, N, Q, C
    d.logits, d.sL_b, d.sL_q = lg.data_ptr(), lg.stride(0), lg.stride(1)
    d.boxes, d.sB_b, d.sB_q = bx.data_ptr(), bx.stride(0), bx.stride(1)
    d.tile_start, d.tile_start_host, d.windows, d.sizes = start_d.data_ptr(), start_h.ctypes.data, win_d.data_ptr(), size_d.data_ptr()
    d.background_class, d.score_threshold, d.max_detections = case["bg"], kw.get("score_threshold", 0.0), K
    d.bbox_format, d.clip = DETECT_FORMATS[kw.get("bbox_format", "xyxy")], int(kw.get("clip", True))
    d.match, d.class_agnostic = MATCH_MODES[kw.get("match", "iou")], int(kw.get("class_agnostic", False))
    d.edge_margin, d.nms_threshold = kw.get("edge_margin", 0.0), kw.get("threshold", R.THRESHOLDS[method])
    address = lambda name: bufs[name].data_ptr() + GUARD * bufs[name].element_size()   # noqa: E731
    for field, name in (("out_boxes", "boxes"), ("out_labels", "labels"), ("out_scores", "scores"), ("out_query", "query"), ("out_tile", "tile"),
                        ("counts", "counts"), ("status", "status")):
        setattr(d, field, address(name))
    block = (ctypes.c_double * _hip.FUSE_PARAMS)(_hip.FUSE_METHODS[method], 0.5, 0.001, kw.get("expected_views", 0), kw.get("min_members", 1), 0)
    _hip._check(_hip.load().detr_hip_fuse_views(ctypes.byref(d), flip_d.data_ptr() if kw.get("flips", True) else None, ctypes.byref(block),
                                                address("members"), _hip._stream()), "detr_hip_fuse_views")
    torch.cuda.synchronize()
    out = {}
    for n, (size, dt, poison) in spec.items():
        h = bufs[n].cpu().numpy()
        assert (h[:GUARD] == poison).all() and (h[GUARD + size:] == poison).all(), f"a guard word of {n} was overwritten"
        out[n] = h[GUARD:GUARD + size]
    out["status"] = int(out["status"][0])
    for n in ("labels", "scores", "query", "tile", "members"):
        out[n] = out[n].reshape(B, K)
    out["boxes"] = out["boxes"].reshape(B, K, 4)
    return out


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", (1, 2048))
def test_max_detections_and_zero_tail(hip, method, K):
    case = two_images()
    want = check(case, method=method, score_threshold=0.3, max_detections=K)
    full = reference(case, method=method, score_threshold=0.3, max_detections=2048)
    n = [len(f[3]) for f in full]
    assert all(1 < v < 2048 for v in n) and [len(w[3]) for w in want] == [min(K, v) for v in n]
    assert all(w[3].tolist() == f[3][:K].tolist() and w[4].tolist() == f[4][:K].tolist() for w, f in zip(want, full))
    raw = raw_fuse(case, K, method, score_threshold=0.3)
    assert raw["status"] == 0 and raw["counts"].tolist() == [min(K, v) for v in n]
    for b in range(2):
        for name in ("boxes", "labels", "scores", "query", "tile", "members"):
            assert not raw[name][b, min(K, n[b]):].any(), name                         # rows past the count are zero
        assert raw["members"][b, :min(K, n[b])].tolist() == want[b][5].tolist()
    null = raw_fuse(dict(case, flips=np.zeros_like(case["flips"])), K, method, score_threshold=0.3, flips=False)   # NULL = none flipped
    zero = raw_fuse(dict(case, flips=np.zeros_like(case["flips"])), K, method, score_threshold=0.3)
    assert all(null[name].tobytes() == zero[name].tobytes() for name in ("boxes", "labels", "scores", "query", "tile", "members", "counts"))


def clutter_case(seed, n_views, sizes=((600, 800),), before=(), after=()):
    """One image of n_views x 100 foreground queries with small random boxes (so nearly every box is its own cluster), optionally
    between two ordinary images."""
    views = [tuple([0, 1] * 8)[:len(v)] for v in before] + [tuple([0, 1] * 16)[:n_views]] + [tuple([0, 1] * 8)[:len(v)] for v in after]
    all_sizes = [(90, 120)] * len(before) + list(sizes) + [(100, 200)] * len(after)
    return make_case(seed, views, all_sizes, 100, 92, 12, seen=1.1, clutter=1.1)


def test_over_the_candidate_cap(hip):
    """Three images, the middle one with 21 views x 100 foreground queries = 2100 candidates > 2048."""
    from detr_tf import _hip
    assert _hip.TILE_MAX_CAND == 2048
    case = clutter_case(11, 21, before=[(0, 1)], after=[(0, 1, 0)])
    assert (case["label"][2:23] != case["bg"]).sum() == 2100
    K = 150
    for method in ("nms", "wbf"):
        with pytest.raises(ValueError, match="2048"):
            run(case, method=method, score_threshold=0.0, max_detections=K)
        raw = raw_fuse(case, K, method, score_threshold=0.0)
        assert raw["status"] == 1 and raw["counts"][1] == 0                            # DETR_TILE_OVER_CAP
        for name in ("boxes", "labels", "scores", "query", "tile", "members"):
            assert not raw[name][1].any(), name                                        # the image over the cap: no detections, zero rows
        want = [R.fuse_image(case["score"][a:b], case["label"][a:b], case["boxes"][a:b], case["windows"][a:b], case["flips"][a:b], case["sizes"][i],
                             case["bg"], method=method, score_threshold=0.0, max_detections=K) for i, (a, b) in ((0, (0, 2)), (2, (23, 26)))]
        for b, (wb, wl, ws, wq, wt, wm, _) in zip((0, 2), want):                       # its neighbours: as if it were not there
            k = len(wq)
            assert raw["counts"][b] == k and raw["query"][b, :k].tolist() == wq.tolist() and raw["tile"][b, :k].tolist() == wt.tolist()
            assert raw["members"][b, :k].tolist() == wm.tolist() and raw["scores"][b, :k].tobytes() == ws.tobytes()
            assert raw["boxes"][b, :k].tobytes() == wb.tobytes() and not raw["boxes"][b, k:].any()


def test_over_the_cluster_cap(hip):
    """11 views x 100 small random boxes: 1100 candidates, under the candidate cap, but nearly as many clusters > 1024."""
    from detr_tf import _hip
    assert _hip.FUSE_MAX_CLUSTERS == 1024
    case = clutter_case(12, 11)
    want = reference(case, method="wbf", score_threshold=0.0, max_detections=50)
    assert want[0][6]["candidates"] == 1100 and sum(want[0][6]["sizes"].values()) > 1024
    with pytest.raises(ValueError, match="1024 clusters"):
        run(case, method="wbf", score_threshold=0.0, max_detections=50)
    raw = raw_fuse(case, 50, "wbf", score_threshold=0.0)
    assert raw["status"] == 4 and raw["counts"].tolist() == [0] and not raw["boxes"].any() and not raw["members"].any()
    for method in ("nms", "soft_nms"):                                                 # the other methods have no such cap
        check(case, method=method, score_threshold=0.0, max_detections=50)
    fewer = clutter_case(12, 10)                                                       # 1000 candidates: every one may found a cluster
    want = check(fewer, method="wbf", score_threshold=0.0, max_detections=50)
    assert 900 < sum(want[0][6]["sizes"].values()) <= 1000


# ---- the mirror ------------------------------------------------------------------------------------------------------------------
def test_a_flipped_view_fuses_with_the_plain_view(hip):
    """Hand-built, exact coordinates: W = 256, H = 128; three objects, the flipped view reports their mirror images."""
    objects = [(32, 16, 96, 80), (128, 32, 192, 96), (200, 8, 248, 40)]
    H, W = 128, 256
    logits = np.full((2, 4, 3), 0.0, F)
    logits[:, :, 2] = 20.0
    boxes = np.zeros((2, 4, 4), F)
    for v in range(2):
        for q, (x0, y0, x1, y1) in enumerate(objects):
            if v:
                x0, x1 = W - x1, W - x0
            boxes[v, q] = ((x0 + x1) / 2 / W, (y0 + y1) / 2 / H, (x1 - x0) / W, (y1 - y0) / H)
            logits[v, q] = (3.0 - q - 0.5 * v, 0.0, 0.0)
    case = finish(dict(logits=logits, boxes=boxes, view_start=np.array([0, 2], np.int32), windows=np.array([[0, 0, H, W]] * 2, np.int32),
                       flips=np.array([0, 1], np.int32), sizes=np.array([[H, W]], np.int32), bg=2))
    for method in METHODS:
        want = check(case, method=method, score_threshold=0.2)
        got = run(case, method=method, score_threshold=0.2)[0]
        kept = got.boxes.cpu().numpy()
        assert len(kept) == (6 if method == "soft_nms_gaussian" else 3)
        for box in kept[:3] if method != "soft_nms_gaussian" else kept:
            nearest = min(objects, key=lambda o: abs(o[0] - box[0]))
            assert np.allclose(box, nearest, rtol=2.0 ** -23, atol=0)                   # within one fp32 rounding of the original
        if method == "wbf":
            assert got.members.cpu().numpy().tolist() == [2, 2, 2] and want[0][4].tolist() == [0, 0, 0]
    unflipped = run(dict(case, flips=np.zeros(2, np.int32)), method="wbf", score_threshold=0.2)[0]
    assert unflipped.members.cpu().numpy().tolist().count(1) >= 4                       # without the mirror the views disagree


def test_the_edge_rule_on_a_flipped_tile(hip):
    """A 100 x 200 image, the whole image plus its two halves, plain and flipped.  A flipped tile's window lies in the MIRRORED
    image: its left half covers the image's right half, and the rule must test the edges of that frame."""
    size, tiles = (100, 200), [(0, 0, 100, 200), (0, 0, 100, 111), (0, 89, 100, 111)]
    case = make_case(5, [(0, 0, 0, 1, 1, 1)], [size], 70, 5, 12, windows=tiles + tiles)
    for method in ("nms", "wbf"):
        plain = check(case, method=method, score_threshold=0.3, clip=False, max_detections=600)
        edged = check(case, method=method, score_threshold=0.3, clip=False, max_detections=600, edge_margin=4.0)
        assert edged[0][6]["candidates"] < plain[0][6]["candidates"]
    # by hand: a box at the right edge of the flipped LEFT tile (mirrored x 91 .. 111 of a window 0 .. 111, interior edge at 111) is
    # dropped; the same numbers in the flipped RIGHT tile (window 89 .. 200: mirrored x 180 .. 200, the image border) are kept and
    # come back as x 0 .. 20 of the image
    logits = np.array([[[3.0, 0.0]], [[3.0, 0.0]]], F)
    boxes = np.array([[[101 / 111, 0.5, 20 / 111, 0.5]]] * 2, F)
    hand = finish(dict(logits=logits, boxes=boxes, view_start=np.array([0, 2], np.int32), windows=np.array(tiles[1:], np.int32),
                       flips=np.array([1, 1], np.int32), sizes=np.array([size], np.int32), bg=1))
    want = check(hand, method="nms", score_threshold=0.5, edge_margin=4.0)
    assert want[0][4].tolist() == [1] and np.allclose(want[0][0], [[0, 25, 20, 75]], atol=1e-4)
    assert len(check(hand, method="nms", score_threshold=0.5, threshold=1.0)[0][3]) == 2


# ---- the Detector ----------------------------------------------------------------------------------------------------------------
def _config():
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.image_size = (64, 96)
    return cfg


@pytest.fixture(scope="module")
def model(hip):
    """The committed tiny model: the configuration and seed of tests/golden/tiny_r50_e1d2_64x96.npz."""
    import os
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_r50_e1d2_64x96.npz")) as z:
        seed, num_enc, num_dec = (int(v) for v in z["meta"][:3])
    m = get_detr_model(_config(), include_top=True, num_encoder_layers=num_enc, num_decoder_layers=num_dec, dropout=0.0)
    m.load_weights(detr_ref.make_params(seed, num_enc=num_enc, num_dec=num_dec))
    return m


def _images():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((96, 128), (80, 150))]


def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert type(x) is type(y)
        for s, t in zip(x, y):
            assert s.dtype == t.dtype and s.shape == t.shape and s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()


def test_detector_with_views_equals_the_hand_assembled_chain(hip, model):
    from detr_tf.data import transformation as T
    from detr_tf.data.processing import DeviceInputStage
    from detr_tf.inference import Detector, FusedDetections, TrackedDetections, Tracker
    cfg, imgs = _config(), _images()
    canvas = (96, 128)
    kw = dict(score_threshold=0.0, max_detections=40)
    det = Detector(model, cfg, shortest_side=64, max_size=96, canvas=canvas, flip=True, scales=(64, 48), merge="wbf", **kw)
    first = det(imgs)
    assert len(first) == 2 and all(isinstance(d, FusedDetections) for d in first)
    # the chain by hand: view_records -> augmented_tiles -> model -> the reference fusion on the device's scores
    recs = [T.view_records(im.shape[0], im.shape[1], (64, 48), 96, True, T.CUBIC) for im in imgs]
    assert recs == det.view_records(imgs) and [len(r) for r in recs] == [4, 4]
    x, m, view_start = DeviceInputStage(cfg).augmented_tiles(imgs, recs, canvas=canvas)
    assert tuple(x.shape) == (8, 96, 128, 3) and view_start.tolist() == [0, 4, 8]
    out = model((x, m), training=False)
    logits, boxes = out["pred_logits"].float().cpu().numpy(), out["pred_boxes"].float().cpu().numpy()
    score, label = scores_labels(logits, 91)
    windows = np.array([(t.y0, t.x0, t.hc, t.wc) for r in recs for t in r], np.int32)
    flips = np.array([t.flip for r in recs for t in r], np.int32)
    sizes = np.array([im.shape[:2] for im in imgs], np.int32)
    want = R.fuse(score, label, boxes, view_start, windows, flips, sizes, 91, method="wbf", expected_views=4, **kw)
    assert all(w[6]["candidates"] >= len(w[3]) >= 1 for w in want)
    same(first, want, "wbf")
    _same_lists(det(imgs), first)                                                      # a second call: the same bits
    # chunks of views smaller than their number, a single image, another rule
    chunked = Detector(model, cfg, shortest_side=64, max_size=96, canvas=canvas, flip=True, scales=(64, 48), merge="wbf", tile_batch=3, **kw)
    got = chunked(imgs)
    assert len(got) == 2 and all(isinstance(g, FusedDetections) and 1 <= g.scores.shape[0] <= 40 for g in got)
    one = det(imgs[1])
    assert isinstance(one, FusedDetections)
    soft = Detector(model, cfg, shortest_side=64, max_size=96, canvas=canvas, flip=True, merge="soft_nms", nms_threshold=0.4, **kw)(imgs)
    want = R.fuse(score[[0, 2, 4, 6]], label[[0, 2, 4, 6]], boxes[[0, 2, 4, 6]], np.array([0, 2, 4]), windows[[0, 2, 4, 6]], flips[[0, 2, 4, 6]], sizes, 91,
                  method="soft_nms", threshold=0.4, **kw)
    same(soft, want, "soft_nms")
    with pytest.raises(ValueError, match="does not fit"):                              # a fixed canvas must fit the largest view
        Detector(model, cfg, shortest_side=64, max_size=200, canvas=canvas, scales=(64, 128), max_detections=40)(imgs)
    with pytest.raises(NotImplementedError):
        det(imgs, need_weights=True)
    # track, draw and to_coco_results accept the result
    tracked = det.track(imgs, Tracker(streams=2, min_hits=1, track_threshold=0.0))
    assert len(tracked) == 2 and all(isinstance(t, TrackedDetections) and t.ids.shape[0] >= 1 for t in tracked)
    with pytest.raises(NotImplementedError, match="appearance"):
        det.track(imgs, Tracker(streams=2, embed_dim=256))
    drawn = det.draw(None, first, [str(i) for i in range(92)])
    assert len(drawn) == 2 and tuple(drawn[0].shape) == (96, 128, 3) and drawn[0].dtype == torch.uint8
    coco = Detector(model, cfg, shortest_side=64, max_size=96, canvas=canvas, flip=True, merge="wbf", bbox_format="xywh", **kw)
    records = coco.to_coco_results(coco(imgs), [7, 9])
    assert len(records) == sum(int(d.scores.shape[0]) for d in coco(imgs)) and {r["image_id"] for r in records} == {7, 9}
