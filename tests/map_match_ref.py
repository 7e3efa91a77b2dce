"""NumPy restatement of the record format of csrc/map_match.hip (detr_hip_map_match), written as plain loops over one image
-- independent of both the kernel and the vectorised APAccumulator -- plus the inputs the CPU and GPU tests share:
seeded random batches in the post-processed layout, with the corner cases the matching rules are about planted in them, and
the golden fixture refpy_map.npz repacked into that layout."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THRESHOLDS = [x / 100.0 for x in range(50, 100, 5)]
BAD_LABEL, BAD_TARGET_CLASS, BAD_HEADER, BAD_COUNT = 1, 2, 4, 8
R_PAD = 100                                   # rows of the padded targets, header included (data/processing.py)


def targets_to_yxyx(t):
    """bbox.xcycwh_to_yx_min_yx_max in fp32: [n, 4] cx, cy, w, h -> y1, x1, y2, x2 clipped to [0, 1]."""
    t = np.asarray(t, np.float32).reshape(-1, 4)
    half_w, half_h = t[:, 2] / np.float32(2), t[:, 3] / np.float32(2)
    out = np.stack([t[:, 1] - half_h, t[:, 0] - half_w, t[:, 1] + half_h, t[:, 0] + half_w], 1).astype(np.float32)
    return np.clip(out, np.float32(0), np.float32(1))


def _iou(p, g):
    """compute_overlaps for one pair of [y1, x1, y2, x2] boxes, fp64, same operation order."""
    p, g = [np.float64(v) for v in p], [np.float64(v) for v in g]
    area1 = (p[2] - p[0]) * (p[3] - p[1])
    area2 = (g[2] - g[0]) * (g[3] - g[1])
    y1, y2, x1, x2 = max(p[0], g[0]), min(p[2], g[2]), max(p[1], g[1]), min(p[3], g[3])
    inter = max(x2 - x1, np.float64(0)) * max(y2 - y1, np.float64(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area1 + area2 - inter)


def map_match_ref(boxes, labels, scores, counts, t_bbox, t_class, nb_class, thresholds=None):
    """What detr_hip_map_match writes: (rec_score [B, Q] fp32, rec_class [B, Q] int32, rec_flags [B, Q] uint32,
    num_gt [nb_class] int64, status)."""
    thresholds = THRESHOLDS if thresholds is None else list(thresholds)
    boxes, scores = np.asarray(boxes, np.float32), np.asarray(scores, np.float32)
    labels, counts = np.asarray(labels, np.int64), np.asarray(counts, np.int32)
    t_bbox, t_class = np.asarray(t_bbox, np.float32), np.asarray(t_class, np.int64).reshape(t_bbox.shape[0], -1)
    B, Q = labels.shape
    R = t_bbox.shape[1]
    rec_score, rec_class = np.zeros((B, Q), np.float32), np.full((B, Q), -1, np.int32)
    rec_flags, num_gt, status = np.zeros((B, Q), np.uint32), np.zeros(nb_class, np.int64), 0
    for b in range(B):
        n = int(counts[b])
        if not 0 <= n <= Q:
            status |= BAD_COUNT
            n = min(max(n, 0), Q)
        head = t_bbox[b, 0, 0]
        G = 0
        if head > -1 and head < R:
            G = int(head)
        else:
            status |= BAD_HEADER
        gt = targets_to_yxyx(t_bbox[b, 1:1 + G])
        gcls = []
        for j in range(G):
            c = int(t_class[b, 1 + j])
            if 0 <= c < nb_class:
                num_gt[c] += 1
                gcls.append(c)
            else:
                status |= BAD_TARGET_CLASS
                gcls.append(-1)
        used = [[False] * len(thresholds) for _ in range(G)]
        order = np.argsort(-scores[b, :n].astype(np.float64), kind="stable")
        for r, i in enumerate(order):
            c = int(labels[b, i])
            rec_score[b, r] = scores[b, i]
            if not 0 <= c < nb_class:
                status |= BAD_LABEL
                continue
            rec_class[b, r] = c
            ious = [_iou(boxes[b, i], gt[j]) if gcls[j] == c else None for j in range(G)]
            word = 0
            for t, thr in enumerate(thresholds):
                best, best_j = None, -1
                for j in range(G):
                    if ious[j] is not None and not used[j][t] and ious[j] > thr and (best_j < 0 or ious[j] > best):
                        best, best_j = ious[j], j
                if best_j >= 0:
                    used[best_j][t] = True
                    word |= 1 << t
            rec_flags[b, r] = word
    return rec_score, rec_class, rec_flags, num_gt, status


def host_accumulate(acc, boxes, labels, scores, counts, t_bbox, t_class):
    """The host path of evaluation.eval_model on one batch in the post-processed layout: APAccumulator.add_image per image."""
    import torch
    from detr_tf import bbox
    tb = torch.as_tensor(np.asarray(t_bbox)).float()
    tc = np.asarray(t_class).reshape(len(tb), -1)
    for b in range(len(tb)):
        k, n = int(counts[b]), int(tb[b, 0, 0])
        acc.add_image(boxes[b, :k], labels[b, :k], scores[b, :k], bbox.xcycwh_to_yx_min_yx_max(tb[b, 1:1 + n]).numpy(), tc[b, 1:1 + n])


def assert_same_accumulator(got, want):
    """scores lists, concatenated flags and num_gt, compared with == (no tolerance)."""
    nt = len(want.thresholds)
    assert got.nb_class == want.nb_class and list(got.thresholds) == list(want.thresholds)
    assert np.array_equal(np.asarray(got.num_gt), np.asarray(want.num_gt)) and np.asarray(got.num_gt).dtype == np.int64
    for c in range(want.nb_class):
        assert got.scores[c] == want.scores[c], c
        fg = np.concatenate(got.flags[c], 0) if got.flags[c] else np.zeros((0, nt), bool)
        fw = np.concatenate(want.flags[c], 0) if want.flags[c] else np.zeros((0, nt), bool)
        assert fg.dtype == bool and fg.shape == fw.shape and np.array_equal(fg, fw), c


# ---- the golden fixture in the post-processed layout ----------------------------------------------------------------------
def _yxyx_to_target(box):
    """cx, cy, w, h (fp32) of a [y1, x1, y2, x2] fp32 box such that targets_to_yxyx gives the box back, bit for bit where a
    few steps of the last place can arrange it (the caller checks what the round trip does to the flags)."""
    box = np.asarray(box, np.float32)
    out = np.zeros(4, np.float32)
    for lo, hi, ic, iw in ((box[1], box[3], 0, 2), (box[0], box[2], 1, 3)):
        c0 = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        w0 = np.float32(np.float64(hi) - np.float64(lo))
        cands_c, cands_w = [c0], [w0]
        for base, cands in ((c0, cands_c), (w0, cands_w)):
            up = down = base
            for _ in range(3):
                up, down = np.nextafter(up, np.float32(2)), np.nextafter(down, np.float32(-1))
                cands += [up, down]
        best = (c0, w0)
        for c in cands_c:
            hit = [w for w in cands_w if np.float32(c - w / np.float32(2)) == lo and np.float32(c + w / np.float32(2)) == hi]
            if hit:
                best = (c, hit[0])
                break
        out[ic], out[iw] = best
    return out


def golden_case(ci):
    """Case ci of refpy_map.npz as one batch: (nb_class, boxes [B, Q, 4], labels, scores, counts, t_bbox [B, R, 4], t_class
    [B, R, 1], per-image originals).  The fixture stores its ground truths as [y1, x1, y2, x2]; the device path takes the
    loaders' cx, cy, w, h with a header row, so they are converted back (_yxyx_to_target)."""
    with np.load(os.path.join(GOLD, "refpy_map.npz"), allow_pickle=False) as z:
        fx = {k: z[k] for k in z.files}
    nb, B = int(fx[f"m{ci}_nb_class"]), int(fx[f"m{ci}_n_images"])
    Q = max(1, max(len(fx[f"m{ci}_{i}_p_cls"]) for i in range(B)))
    boxes, labels, scores = np.zeros((B, Q, 4), np.float32), np.zeros((B, Q), np.int64), np.zeros((B, Q), np.float32)
    counts, t_bbox, t_class = np.zeros(B, np.int32), np.zeros((B, R_PAD, 4), np.float32), np.zeros((B, R_PAD, 1), np.int64)
    images = []
    for i in range(B):
        pb, pc, ps = fx[f"m{ci}_{i}_p_bbox"], fx[f"m{ci}_{i}_p_cls"], fx[f"m{ci}_{i}_p_score"]
        tb, tc = fx[f"m{ci}_{i}_t_bbox"], fx[f"m{ci}_{i}_t_cls"]
        assert pb.dtype == np.float32 and ps.dtype == np.float32 and tb.dtype == np.float32
        k, n = len(pc), len(tc)
        boxes[i, :k], labels[i, :k], scores[i, :k], counts[i] = pb.reshape(-1, 4), pc, ps, k
        t_bbox[i, 0, 0] = n
        for j in range(n):
            t_bbox[i, 1 + j] = _yxyx_to_target(tb[j])
        t_class[i, 1:1 + n, 0] = tc
        images.append((pb, pc, ps, tb, tc))
    return nb, boxes, labels, scores, counts, t_bbox, t_class, images, fx


# ---- seeded random batches ------------------------------------------------------------------------------------------------
RANDOM_SHAPES = [(1, 100, 92), (5, 100, 92), (8, 300, 92), (3, 7, 3)]


def n_batches(B):
    return max(3, -(-4 // B))                 # at least 3 batches and at least 4 images (the four planted image kinds)


def random_batches(B, Q, C, seed):
    """[(boxes, labels, scores, counts, t_bbox, t_class)] * n_batches(B) in the post-processed layout, nb_class = C.  Image g
    (counted over the batches) is
      g = 0: a duplicated prediction on one ground truth (the second is a false positive), a duplicated ground truth under two
             identical predictions with EQUAL scores (both match; the tie goes to the lowest index), then exact and jittered
             copies of further ground truths;
      g = 1: the pair [0,0,1,1] / [0,0,.5,1] of IoU exactly 0.5, a zero-area prediction on a zero-area ground truth (NaN);
      g = 2: no detection, 99 ground truths;
      g = 3: detections, no ground truth;
      else : random ground truths (few classes, so that several share one), exact / jittered copies and random boxes, scores
             rounded to two decimals (ties)."""
    rng = np.random.default_rng(seed)
    fill_cls = C - 1

    def rand_targets(n, classes):
        t = np.concatenate([rng.uniform(0.1, 0.9, (n, 2)), rng.uniform(0.05, 0.5, (n, 2))], 1).astype(np.float32)
        return t, rng.choice(classes, n).astype(np.int64)

    def copies(t, tcls, room, jitter=True):
        """predictions made from ground truths: exact copies (IoU 1) and copies scaled by up to 30 % (IoU 0.5 .. 1)"""
        dets = []
        for j in rng.permutation(len(tcls))[:room]:
            box = targets_to_yxyx(t[j:j + 1])[0]
            if jitter and rng.random() < 0.7:
                s = np.float32(rng.uniform(0.7, 1.0))
                cy, cx, h, w = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2, (box[2] - box[0]) * s, (box[3] - box[1]) * s
                box = np.clip(np.array([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], np.float32), 0, 1)
            dets.append((box, int(tcls[j]), np.float32(round(float(rng.uniform(0.05, 0.99)), 2))))
        return dets

    out, g = [], 0
    for _ in range(n_batches(B)):
        boxes, labels, scores = np.zeros((B, Q, 4), np.float32), np.zeros((B, Q), np.int64), np.zeros((B, Q), np.float32)
        counts, t_bbox, t_class = np.zeros(B, np.int32), np.zeros((B, R_PAD, 4), np.float32), np.zeros((B, R_PAD, 1), np.int64)
        for b in range(B):
            if g == 0:
                t = np.array([[0.3, 0.3, 0.2, 0.2], [0.7, 0.7, 0.2, 0.3], [0.7, 0.7, 0.2, 0.3]], np.float32)
                tcls = np.array([0, 1, 1], np.int64)
                p0, p1 = targets_to_yxyx(t[0:1])[0], targets_to_yxyx(t[1:2])[0]
                dets = [(p0, 0, np.float32(0.9)), (p0, 0, np.float32(0.8)), (p1, 1, np.float32(0.6)), (p1, 1, np.float32(0.6))]
                ft, fc = rand_targets(3, [fill_cls])
                dets += copies(ft[:1], fc[:1], 1, jitter=False) + copies(ft[1:], fc[1:], Q - 5)
                t, tcls = np.concatenate([t, ft]), np.concatenate([tcls, fc])
            elif g == 1:
                t = np.array([[0.5, 0.25, 1.0, 0.5], [0.4, 0.6, 0.0, 0.0]], np.float32)       # yxyx [0,0,.5,1]; a point
                tcls = np.array([0, 1], np.int64)
                point = targets_to_yxyx(t[1:2])[0]
                dets = [(np.array([0, 0, 1, 1], np.float32), 0, np.float32(0.7)), (point, 1, np.float32(0.5))]
                ft, fc = rand_targets(3, [fill_cls])
                dets += copies(ft, fc, Q - 2)
                t, tcls = np.concatenate([t, ft]), np.concatenate([tcls, fc])
            elif g == 2:
                t, tcls = rand_targets(R_PAD - 1, np.arange(C))
                dets = []
            elif g == 3:
                t, tcls = np.zeros((0, 4), np.float32), np.zeros(0, np.int64)
                dets = [(np.sort(rng.uniform(0, 1, (2, 2)), 0).reshape(4).astype(np.float32), int(rng.integers(C)),
                         np.float32(round(float(rng.uniform(0.05, 0.99)), 2))) for _ in range(min(Q, 20))]
            else:
                classes = rng.choice(C, min(C, 4), replace=False)
                t, tcls = rand_targets(int(rng.integers(1, 30)), classes)
                dets = copies(t, tcls, Q // 2)
                dets += [(np.sort(rng.uniform(0, 1, (2, 2)), 0).reshape(4).astype(np.float32), int(rng.choice(classes)),
                          np.float32(round(float(rng.uniform(0.05, 0.99)), 2))) for _ in range(int(rng.integers(0, Q - len(dets) + 1)))]
            perm = rng.permutation(len(dets)) if g > 1 else np.arange(len(dets))      # query order is not score order
            for k, i in enumerate(perm):
                boxes[b, k], labels[b, k], scores[b, k] = dets[i]
            counts[b] = len(dets)
            t_bbox[b, 0, 0] = len(tcls)
            t_bbox[b, 1:1 + len(tcls)], t_class[b, 1:1 + len(tcls), 0] = t, tcls
            g += 1
        out.append((boxes, labels, scores, counts, t_bbox, t_class))
    return out


def dense_batch(B, Q, C, seed):
    """One batch with every slot used: Q detections per image (scaled copies of the 99 ground truths and random boxes, scores
    rounded to two decimals) over C classes -- the largest work one workgroup of the kernel can get."""
    rng = np.random.default_rng(seed)
    boxes, labels = np.zeros((B, Q, 4), np.float32), rng.integers(0, C, (B, Q)).astype(np.int64)
    scores = np.round(rng.uniform(0.01, 0.99, (B, Q)), 2).astype(np.float32)
    t_bbox, t_class = np.zeros((B, R_PAD, 4), np.float32), np.zeros((B, R_PAD, 1), np.int64)
    n = R_PAD - 1
    t_bbox[:, 0, 0] = n
    t_bbox[:, 1:, :2], t_bbox[:, 1:, 2:] = rng.uniform(0.1, 0.9, (B, n, 2)), rng.uniform(0.05, 0.5, (B, n, 2))
    t_class[:, 1:, 0] = rng.integers(0, C, (B, n))
    for b in range(B):
        gt = targets_to_yxyx(t_bbox[b, 1:])
        for q in range(Q):
            if rng.random() < 0.6:
                j = int(rng.integers(n))
                s = np.float32(1.0 if rng.random() < 0.3 else rng.uniform(0.6, 1.0))
                cy, cx, h, w = (gt[j, 0] + gt[j, 2]) / 2, (gt[j, 1] + gt[j, 3]) / 2, (gt[j, 2] - gt[j, 0]) * s, (gt[j, 3] - gt[j, 1]) * s
                boxes[b, q] = gt[j] if s == 1.0 else np.clip(np.array([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], np.float32), 0, 1)
                labels[b, q] = t_class[b, 1 + j, 0]
            else:
                boxes[b, q] = np.sort(rng.uniform(0, 1, (2, 2)), 0).reshape(4)
    return boxes, labels, scores, np.full(B, Q, np.int32), t_bbox, t_class


def assert_planted_cases_occur(batches, C):
    """Every corner case random_batches plants is really there -- checked on the HOST result (compute_overlaps, APAccumulator),
    so that an equality test on these inputs cannot pass vacuously."""
    from detr_tf.loss.compute_map import APAccumulator, compute_overlaps
    seen = dict.fromkeys(["equal_scores", "dup_pred_fp", "dup_gt_tie", "iou_half", "zero_area_nan", "no_det", "no_target",
                          "full_targets"], False)
    total = APAccumulator(C)
    for boxes, labels, scores, counts, t_bbox, t_class in batches:
        host_accumulate(total, boxes, labels, scores, counts, t_bbox, t_class)
        for b in range(len(counts)):
            k, n = int(counts[b]), int(t_bbox[b, 0, 0])
            seen["no_det"] |= k == 0
            seen["no_target"] |= n == 0 and k > 0
            seen["full_targets"] |= n == t_bbox.shape[1] - 1 == 99
            one = APAccumulator(C)
            host_accumulate(one, boxes[b:b + 1], labels[b:b + 1], scores[b:b + 1], counts[b:b + 1], t_bbox[b:b + 1], t_class[b:b + 1])
            pb, pl, ps = boxes[b, :k], labels[b, :k], scores[b, :k]
            gt, gc = targets_to_yxyx(t_bbox[b, 1:1 + n]), t_class[b, 1:1 + n, 0]
            iou = compute_overlaps(pb, gt) if k and n else np.zeros((k, n))
            same = pl[:, None] == gc[None, :]
            seen["zero_area_nan"] |= bool((np.isnan(iou) & same).any())
            for c in range(C):
                det = np.argsort(-ps.astype(float), kind="stable")
                det = det[pl[det] == c]
                if len(det) == 0:
                    continue
                fl = one.flags[c][0]                                  # [n_det, 10] in the visiting order `det`
                seen["equal_scores"] |= len(set(ps[det].tolist())) < len(det)
                for u in range(len(det)):
                    at_half = (iou[det[u]] == 0.5) & same[det[u]]
                    if at_half.any() and not (iou[det[u]][same[det[u]]] > 0.5).any():
                        assert not fl[u, 0]                           # IoU exactly 0.5 is not a match at .50
                        seen["iou_half"] = True
                    for v in range(u + 1, len(det)):
                        if np.array_equal(pb[det[u]], pb[det[v]]):
                            tie = np.nonzero(same[det[u]] & (iou[det[u]] == np.nanmax(np.where(same[det[u]], iou[det[u]], np.nan))))[0] \
                                if same[det[u]].any() and not np.all(np.isnan(iou[det[u]][same[det[u]]])) else []
                            if len(tie) == 1 and fl[u, 0] and not fl[v, 0]:
                                seen["dup_pred_fp"] = True
                            if len(tie) >= 2 and np.array_equal(gt[tie[0]], gt[tie[1]]) and fl[u, 0] and fl[v, 0]:
                                seen["dup_gt_tie"] = True
    missing = [k for k, v in seen.items() if not v]
    assert not missing, missing
    flags = np.concatenate([np.concatenate(f, 0) for f in total.flags if f], 0)
    assert flags.any(0).all() and (~flags).any(0).all(), "a true and a false positive at every threshold"
    zero_area = any(((bx[..., 2] - bx[..., 0]) * (bx[..., 3] - bx[..., 1]) == 0)[np.arange(bx.shape[1])[None, :] < ct[:, None]].any()
                    for bx, _, _, ct, _, _ in batches)
    assert zero_area, "a zero-area prediction"
    return total
