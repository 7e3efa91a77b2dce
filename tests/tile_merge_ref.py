"""The cross-tile merge of sliced inference (csrc/tile_merge.hip) restated in plain NumPy, step by step, from its specification
(include/detr_hip.h: detr_tile_merge_desc).  A test helper, not product code: it is sequential and slow on purpose.

The mapping mirrors the kernel's fp32 arithmetic with np.float32 operations -- every product, sum and difference is rounded once,
there is no fused multiply-add in NumPy --, the match measure is float64 on the float32 corners.  Scores and labels are an INPUT here
(the tests take them from detr_hip_postprocess / detect, whose bits the merge kernel shares by construction, or from
`scores_labels`, an fp32 restatement that is exact only where the tests make it so)."""
import numpy as np

F = np.float32
FORMATS = ("xy_center", "xyxy", "yxyx", "xywh")


def scores_labels(logits):
    """fp64 softmax -> (score fp64 [.., Q], label [.., Q]): for ORDER decisions on inputs whose scores are exact ties or far apart."""
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    return p.max(-1), p.argmax(-1)


def measure(p, g, match):
    """fp64 IoU ("iou") or intersection over the smaller area ("ios") of two (x0, y0, x1, y1) float32 boxes; 0 for a zero denominator."""
    p, g = [float(v) for v in p], [float(v) for v in g]
    ix = min(p[2], g[2]) - max(p[0], g[0])
    iy = min(p[3], g[3]) - max(p[1], g[1])
    inter = max(0.0, ix) * max(0.0, iy)
    ap, ag = (p[2] - p[0]) * (p[3] - p[1]), (g[2] - g[0]) * (g[3] - g[1])
    den = ap + ag - inter if match == "iou" else min(ap, ag)
    if den == 0.0:
        return 0.0
    return inter / den


def map_box(box, window):
    """Tile-normalised (cx, cy, w, h) float32 -> ((cx, cy, w, h), unclipped (x0, y0, x1, y1)) in image pixels, float32 roundings."""
    y0, x0, hc, wc = (F(int(v)) for v in window)
    bx = np.asarray(box, F)
    cx, cy, w, h = x0 + bx[0] * wc, y0 + bx[1] * hc, bx[2] * wc, bx[3] * hc
    half = F(0.5)
    return (cx, cy, w, h), (cx - w * half, cy - h * half, cx + w * half, cy + h * half)


def edge_drop(corners, window, size, margin):
    """Step 3: is a corner within `margin` pixels of (or beyond) a window edge that is interior to the image?"""
    y0, x0, hc, wc = (int(v) for v in window)
    H, W = int(size[0]), int(size[1])
    if not margin > 0 or (x0 == 0 and y0 == 0 and wc == W and hc == H):
        return False
    m = F(margin)
    bx0, by0, bx1, by1 = corners
    return bool((x0 > 0 and bx0 - F(x0) <= m) or (x0 + wc < W and F(x0 + wc) - bx1 <= m) or
                (y0 > 0 and by0 - F(y0) <= m) or (y0 + hc < H and F(y0 + hc) - by1 <= m))


def merge_image(scores, labels, boxes, windows, size, background, *, score_threshold=0.0, max_detections=100, bbox_format="xyxy",
                clip=True, nms_threshold=0.5, match="iou", class_agnostic=False, edge_margin=0.0):
    """One image: scores float32 [T, Q], labels [T, Q], boxes float32 [T, Q, 4], windows [T, 4] (y0, x0, hc, wc), size (H, W).
    Returns (boxes float32 [k, 4], labels int64 [k], scores float32 [k], query int32 [k], tile int32 [k], n_candidates)."""
    assert bbox_format in FORMATS and match in ("iou", "ios")
    H, W = F(int(size[0])), F(int(size[1]))
    cand = []                                                                   # (score, label, tile, query, corners, centre form)
    for t in range(len(windows)):
        for q in range(scores.shape[1]):
            s = F(scores[t, q])
            if int(labels[t, q]) == background or not s >= F(score_threshold):  # NaN fails the comparison
                continue
            centre, corners = map_box(boxes[t, q], windows[t])
            if edge_drop(corners, windows[t], size, edge_margin):
                continue
            if clip:
                x0, y0, x1, y1 = corners
                corners = (min(max(x0, F(0)), W), min(max(y0, F(0)), H), min(max(x1, F(0)), W), min(max(y1, F(0)), H))
            cand.append((s, int(labels[t, q]), t, q, corners, centre))
    order = sorted(range(len(cand)), key=lambda i: (-float(cand[i][0]), i))     # stable: ties by (tile, query)
    kept = []
    for i in order:
        if len(kept) == max_detections:
            break
        if any((class_agnostic or cand[k][1] == cand[i][1]) and measure(cand[k][4], cand[i][4], match) > nms_threshold for k in kept):
            continue
        kept.append(i)
    out = np.zeros((len(kept), 4), F)
    for r, i in enumerate(kept):
        x0, y0, x1, y1 = cand[i][4]
        if bbox_format == "xy_center":
            out[r] = cand[i][5]
        elif bbox_format == "xyxy":
            out[r] = (x0, y0, x1, y1)
        elif bbox_format == "yxyx":
            out[r] = (y0, x0, y1, x1)
        else:
            out[r] = (x0, y0, x1 - x0, y1 - y0)
    return (out, np.array([cand[i][1] for i in kept], np.int64), np.array([cand[i][0] for i in kept], F),
            np.array([cand[i][3] for i in kept], np.int32), np.array([cand[i][2] for i in kept], np.int32), len(cand))


def merge(scores, labels, boxes, tile_start, windows, sizes, background, **kw):
    """All images: scores / labels [N, Q], boxes [N, Q, 4], tile_start [B + 1], windows [N, 4], sizes [B, 2] -> [merge_image(...)]."""
    return [merge_image(scores[a:b], labels[a:b], boxes[a:b], windows[a:b], sizes[i], background, **kw)
            for i, (a, b) in enumerate(zip(tile_start[:-1], tile_start[1:]))]
