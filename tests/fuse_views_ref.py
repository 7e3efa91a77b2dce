"""The fusion of views (csrc/fuse_views.hip) restated in plain NumPy, step by step, from its specification (include/detr_hip.h:
detr_hip_fuse_views).  A test helper, not product code: it is sequential and slow on purpose.

Mapping, edge rule and match measure are tile_merge_ref's own functions (the kernel shares that code too); the mirror and the
centre form are np.float32 operations, one rounding each; soft-NMS and weighted box fusion are Python floats, i.e. IEEE fp64 with one
rounding per operation and no fused multiply-add.  Scores and labels are an INPUT (the tests take them from detr_hip_detect).

Besides the result every call returns COUNTERS, so that a test can assert that its input really exercises what it claims to:
  candidates     after the edge rule
  sizes          {members: number of clusters} (wbf; before min_members)
  multi          walk steps at which the candidate exceeded the threshold against two or more clusters (wbf)
  moved_joins    joins that would not have happened against the cluster's founder alone (wbf)
  moved_refusals foundings although some same-label cluster's founder alone would have accepted the candidate (wbf)
  select_gap     the smallest relative gap between a selected score and the runner-up's (soft-NMS; inf when there never was one)
  min_gap        the smallest relative gap between a decayed score and score_min (soft-NMS; inf with score_min = 0)"""
import math

import numpy as np

from tile_merge_ref import FORMATS, edge_drop, map_box, measure

F = np.float32
METHODS = ("nms", "soft_nms", "soft_nms_gaussian", "wbf")
THRESHOLDS = {"nms": 0.5, "soft_nms": 0.5, "soft_nms_gaussian": 0.5, "wbf": 0.55}


def candidates(scores, labels, boxes, windows, flips, size, background, score_threshold, clip, edge_margin):
    """Steps 1..3: [(score, label, view, query, corners)] in (view, query) order."""
    H, W = F(int(size[0])), F(int(size[1]))
    cand = []
    for t in range(len(windows)):
        for q in range(scores.shape[1]):
            s = F(scores[t, q])
            if int(labels[t, q]) == background or not s >= F(score_threshold):  # NaN fails the comparison
                continue
            _, corners = map_box(boxes[t, q], windows[t])                       # in the view's own frame, mirrored for a flipped view
            if edge_drop(corners, windows[t], size, edge_margin):
                continue
            x0, y0, x1, y1 = corners
            if flips[t]:
                x0, x1 = W - x1, W - x0                                         # one fp32 rounding each
            if clip:
                x0, y0, x1, y1 = min(max(x0, F(0)), W), min(max(y0, F(0)), H), min(max(x1, F(0)), W), min(max(y1, F(0)), H)
            cand.append((s, int(labels[t, q]), t, q, (F(x0), F(y0), F(x1), F(y1))))
    return cand


def emit(corners, bbox_format):
    x0, y0, x1, y1 = (F(v) for v in corners)
    if bbox_format == "xy_center":
        return ((x0 + x1) * F(0.5), (y0 + y1) * F(0.5), x1 - x0, y1 - y0)
    if bbox_format == "xyxy":
        return (x0, y0, x1, y1)
    if bbox_format == "yxyx":
        return (y0, x0, y1, x1)
    return (x0, y0, x1 - x0, y1 - y0)


def _nms(cand, order, thr, match, agnostic, K):
    kept = []
    for i in order:
        if len(kept) == K:
            break
        if any((agnostic or cand[k][1] == cand[i][1]) and measure(cand[k][4], cand[i][4], match) > thr for k in kept):
            continue
        kept.append(i)
    return [(cand[i][4], cand[i][1], cand[i][0], cand[i][3], cand[i][2], 1) for i in kept]


def _soft_nms(cand, gaussian, thr, match, agnostic, K, sigma, score_min, counters):
    cur = [float(c[0]) for c in cand]
    alive = [True] * len(cand)
    out = []
    while len(out) < K:
        best, sel, second = -math.inf, None, -math.inf
        for j in range(len(cand)):
            if not alive[j]:
                continue
            if cur[j] > best:                                                   # ties: the lower position stays; NaN never wins
                best, sel, second = cur[j], j, best
            elif cur[j] > second:
                second = cur[j]
        if sel is None:
            break
        if second > -math.inf and best > 0:
            counters["select_gap"] = min(counters["select_gap"], (best - second) / best)
        out.append((cand[sel][4], cand[sel][1], F(best), cand[sel][3], cand[sel][2], 1))
        alive[sel] = False
        for j in range(len(cand)):
            if not alive[j] or not (agnostic or cand[j][1] == cand[sel][1]):
                continue
            m = measure(cand[sel][4], cand[j][4], match)
            if gaussian:
                cur[j] = cur[j] * float(np.exp(-(m * m) / sigma))
            elif m > thr:
                cur[j] = cur[j] * (1.0 - m)
            if score_min > 0:
                counters["min_gap"] = min(counters["min_gap"], abs(cur[j] - score_min) / score_min)
            if cur[j] < score_min:
                alive[j] = False
    return out


def _wbf(cand, order, thr, match, agnostic, K, expected_views, min_members, counters):
    clusters = []                                                               # dicts, in creation order
    for i in order:
        s, label, view, query, box = cand[i]
        s = float(s)
        best, at, over, founder_ok = -math.inf, None, 0, False
        for k, c in enumerate(clusters):
            if not (agnostic or c["label"] == label):
                continue
            m = measure(c["fused"], box, match)
            over += m > thr
            founder_ok = founder_ok or measure(c["first_box"], box, match) > thr
            if m > best:                                                        # ties: the lower cluster stays; NaN never wins
                best, at = m, k
        counters["multi"] += over >= 2
        if at is not None and best > thr:
            c = clusters[at]
            counters["moved_joins"] += not measure(c["first_box"], box, match) > thr
            c["sw"] = c["sw"] + s
            c["sx"] = [a + s * float(x) for a, x in zip(c["sx"], box)]
            c["cnt"] += 1
            c["fused"] = tuple(F(a / c["sw"]) for a in c["sx"])
        else:
            counters["moved_refusals"] += founder_ok
            clusters.append(dict(label=label, sw=s, sx=[s * float(x) for x in box], cnt=1, fused=box, first_box=box, first=(view, query)))
    rows = []
    for k, c in enumerate(clusters):
        counters["sizes"][c["cnt"]] = counters["sizes"].get(c["cnt"], 0) + 1
        conf = c["sw"] / float(c["cnt"])
        if expected_views:
            conf = conf * float(min(c["cnt"], expected_views)) / float(expected_views)
        if c["cnt"] >= min_members:
            rows.append((c["fused"], c["label"], F(conf), c["first"][1], c["first"][0], c["cnt"], k))
    rows.sort(key=lambda r: (-float(r[2]), r[6]))
    return [r[:6] for r in rows[:K]]


def fuse_image(scores, labels, boxes, windows, flips, size, background, *, method="wbf", threshold=None, score_threshold=0.0, max_detections=100,
               bbox_format="xyxy", clip=True, match="iou", class_agnostic=False, edge_margin=0.0, sigma=0.5, score_min=0.001,
               expected_views=None, min_members=1):
    """One image: scores float32 [V, Q], labels [V, Q], boxes float32 [V, Q, 4], windows [V, 4] (y0, x0, hc, wc), flips [V], size (H, W).
    Returns (boxes float32 [k, 4], labels int64 [k], scores float32 [k], query int32 [k], tile int32 [k], members int32 [k], counters)."""
    assert bbox_format in FORMATS and match in ("iou", "ios") and method in METHODS
    thr = float(THRESHOLDS[method] if threshold is None else threshold)
    cand = candidates(scores, labels, boxes, windows, flips, size, background, score_threshold, clip, edge_margin)
    counters = dict(candidates=len(cand), sizes={}, multi=0, moved_joins=0, moved_refusals=0, select_gap=math.inf, min_gap=math.inf)
    order = sorted(range(len(cand)), key=lambda i: (-float(cand[i][0]), i))     # stable: ties by (view, query)
    if method == "nms":
        rows = _nms(cand, order, thr, match, class_agnostic, max_detections)
    elif method == "wbf":
        rows = _wbf(cand, order, thr, match, class_agnostic, max_detections, expected_views, int(min_members), counters)
    else:
        rows = _soft_nms(cand, method == "soft_nms_gaussian", thr, match, class_agnostic, max_detections, float(sigma), float(score_min), counters)
    out = np.zeros((len(rows), 4), F)
    for r, row in enumerate(rows):
        out[r] = emit(row[0], bbox_format)
    col = lambda i, dtype: np.array([row[i] for row in rows], dtype)            # noqa: E731
    return out, col(1, np.int64), col(2, F), col(3, np.int32), col(4, np.int32), col(5, np.int32), counters


def fuse(scores, labels, boxes, view_start, windows, flips, sizes, background, **kw):
    """All images: scores / labels [N, Q], boxes [N, Q, 4], view_start [B + 1], windows [N, 4], flips [N], sizes [B, 2]."""
    return [fuse_image(scores[a:b], labels[a:b], boxes[a:b], windows[a:b], flips[a:b], sizes[i], background, **kw)
            for i, (a, b) in enumerate(zip(view_start[:-1], view_start[1:]))]
