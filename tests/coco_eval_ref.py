"""Oracle of the COCO evaluation protocol for boxes, written from the protocol (COCOeval's bbIou / evaluateImg / accumulate /
summarize as include/detr_hip.h: detr_hip_coco_match and the issue restate them) as plain Python loops in fp64 over one image,
class, area range and threshold at a time -- independent of the vectorised detr_tf/loss/coco_eval.py and of the kernel.  It
writes the record format of csrc/coco_match.hip, and holds the seeded inputs the CPU and GPU tests share."""
import functools
import math

import numpy as np

from map_match_ref import targets_to_yxyx

THRESHOLDS = [float(v) for v in np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1)]
AREA_RANGES = [[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]]
MAX_DETS = (1, 10, 100)
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
BAD_LABEL, BAD_TARGET_CLASS, BAD_HEADER, BAD_COUNT, BAD_SIZE = 1, 2, 4, 8, 16


def iou_ref(d, g, crowd):
    """bbIou of one [y1, x1, y2, x2] detection and ground truth (fp32 values, fp64 arithmetic)."""
    dy1, dx1, dy2, dx2 = [float(v) for v in d]
    gy1, gx1, gy2, gx2 = [float(v) for v in g]
    w = (dx2 if dx2 < gx2 else gx2) - (dx1 if dx1 > gx1 else gx1)
    h = (dy2 if dy2 < gy2 else gy2) - (dy1 if dy1 > gy1 else gy1)
    if not (w > 0 and h > 0):
        return 0.0
    i = w * h
    area_d = (dx2 - dx1) * (dy2 - dy1)
    u = area_d if crowd else area_d + (gx2 - gx1) * (gy2 - gy1) - i
    return float(np.float64(i) / np.float64(u))               # (numpy: IEEE division by zero instead of an exception)


def comes_before(sa, ia, sb, ib):
    """np.argsort(-scores, kind="stable"): descending, ties by position, NaN last."""
    na, nb = math.isnan(sa), math.isnan(sb)
    if na or nb:
        return ia < ib if na == nb else nb
    return sa > sb or (sa == sb and ia < ib)


def coco_match_ref(boxes, labels, scores, counts, t_bbox, t_class, t_crowd, t_area, sizes, nb_class, thresholds=None, area_ranges=None,
                   taken=None):
    """What detr_hip_coco_match writes: (rec_score [B, Q] fp32, rec_class [B, Q] int32, rec_rank [B, Q] int32,
    rec_flags [n_area, B, Q] uint32, npig [nb_class, n_area] int64, status).  `taken`: a list that receives, per image, the set of
    ground-truth indices some detection matched at some (area range, threshold) -- for tests that must know WHERE matches fell."""
    thresholds = THRESHOLDS if thresholds is None else [float(t) for t in thresholds]
    area_ranges = AREA_RANGES if area_ranges is None else [[float(lo), float(hi)] for lo, hi in area_ranges]
    boxes, scores = np.asarray(boxes, np.float32), np.asarray(scores, np.float32)
    labels, counts = np.asarray(labels, np.int64), np.asarray(counts, np.int32)
    t_bbox, t_class = np.asarray(t_bbox, np.float32), np.asarray(t_class, np.int64).reshape(t_bbox.shape[0], -1)
    t_crowd, t_area, sizes = np.asarray(t_crowd, np.uint8), np.asarray(t_area, np.float32), np.asarray(sizes, np.int32)
    B, Q = labels.shape
    R, nt, na = t_bbox.shape[1], len(thresholds), len(area_ranges)
    rec_score, rec_class, rec_rank = np.zeros((B, Q), np.float32), np.full((B, Q), -1, np.int32), np.zeros((B, Q), np.int32)
    rec_flags, npig, status = np.zeros((na, B, Q), np.uint32), np.zeros((nb_class, na), np.int64), 0
    for b in range(B):
        n = int(counts[b])
        if not 0 <= n <= Q:
            status |= BAD_COUNT
            n = min(max(n, 0), Q)
        head, G = t_bbox[b, 0, 0], 0
        if head > -1 and head < R:
            G = int(head)
        else:
            status |= BAD_HEADER
        H, W = int(sizes[b, 0]), int(sizes[b, 1])
        if H <= 0 or W <= 0:
            status |= BAD_SIZE
        gt = targets_to_yxyx(t_bbox[b, 1:1 + G])
        gcls, crowd, garea = [], [], []
        for j in range(G):
            c = int(t_class[b, 1 + j])
            crowd.append(bool(t_crowd[b, 1 + j]))
            garea.append(float(t_area[b, 1 + j]))
            if 0 <= c < nb_class:
                gcls.append(c)
            else:
                status |= BAD_TARGET_CLASS
                gcls.append(-1)

        def ignore(j, a):
            return crowd[j] or garea[j] < area_ranges[a][0] or garea[j] > area_ranges[a][1]

        for j in range(G):
            for a in range(na):
                if gcls[j] >= 0 and not ignore(j, a):
                    npig[gcls[j], a] += 1
        order = sorted(range(n), key=functools.cmp_to_key(
            lambda i, j: -1 if comes_before(float(scores[b, i]), i, float(scores[b, j]), j) else 1))
        matched_at = [[[False] * nt for _ in range(na)] for _ in range(G)]
        seen = {}
        if taken is not None:
            taken.append(set())
        for r, i in enumerate(order):
            c = int(labels[b, i])
            rec_score[b, r] = scores[b, i]
            if not 0 <= c < nb_class:
                status |= BAD_LABEL
                continue
            rec_class[b, r] = c
            rec_rank[b, r] = seen.get(c, 0)
            seen[c] = seen.get(c, 0) + 1
            dy1, dx1, dy2, dx2 = [float(v) for v in boxes[b, i]]
            pix = ((dy2 - dy1) * float(H)) * ((dx2 - dx1) * float(W))
            ious = [iou_ref(boxes[b, i], gt[j], crowd[j]) if gcls[j] == c else None for j in range(G)]
            for a in range(na):
                word = 0
                for t in range(nt):
                    cur, m = min(thresholds[t], 1 - 1e-10), -1
                    for j in range(G):                                     # phase 1: the ground truths the range keeps
                        if ious[j] is None or ignore(j, a) or matched_at[j][a][t]:
                            continue
                        if ious[j] >= cur:
                            cur, m = ious[j], j
                    if m < 0:
                        for j in range(G):                                 # phase 2: the ignored ones; a crowd may be taken again
                            if ious[j] is None or not ignore(j, a) or (matched_at[j][a][t] and not crowd[j]):
                                continue
                            if ious[j] >= cur:
                                cur, m = ious[j], j
                    if m >= 0:
                        matched_at[m][a][t] = True
                        word |= 1 << t
                        if taken is not None:
                            taken[-1].add(m)
                        ignored = ignore(m, a)
                    else:
                        ignored = pix < area_ranges[a][0] or pix > area_ranges[a][1]
                    if ignored:
                        word |= 1 << (16 + t)
                rec_flags[a, b, r] = word
    return rec_score, rec_class, rec_rank, rec_flags, npig, status


def summarize_ref(records, npig, nb_class, thresholds=None, area_ranges=None, max_dets=MAX_DETS):
    """COCOeval.accumulate + summarize in loops.  records: list of (rec_score, rec_class, rec_rank, rec_flags) as coco_match_ref
    returns them, in push order.  Returns ({stat name: value}, per-class AP list, precision, recall)."""
    thresholds = THRESHOLDS if thresholds is None else list(thresholds)
    area_ranges = AREA_RANGES if area_ranges is None else area_ranges
    nt, na, nm = len(thresholds), len(area_ranges), len(max_dets)
    rec_thrs = [float(v) for v in np.linspace(0.0, 1.0, 101)]
    per_class = [[] for _ in range(nb_class)]                  # (score, rank, [word per area]) in push order
    for rs, rc, rr, rf in records:
        rs, rc, rr, rf = rs.reshape(-1), rc.reshape(-1), rr.reshape(-1), rf.reshape(na, -1)
        for i in range(len(rc)):
            if rc[i] >= 0:
                per_class[int(rc[i])].append((float(rs[i]), int(rr[i]), [int(rf[a, i]) for a in range(na)]))
    precision = -np.ones((nt, 101, nb_class, na, nm))
    recall = -np.ones((nt, nb_class, na, nm))
    eps = float(np.spacing(1))
    for k in range(nb_class):
        for mi, max_det in enumerate(max_dets):
            dets = [d for d in per_class[k] if d[1] < max_det]
            dets = sorted(dets, key=lambda d: (math.isnan(d[0]), -d[0] if not math.isnan(d[0]) else 0.0))      # stable
            for a in range(na):
                n_pos = int(npig[k, a])
                if n_pos == 0:
                    continue
                for t in range(nt):
                    tp = fp = 0
                    rc_l, pr_l = [], []
                    for _s, _r, words in dets:
                        matched, ignored = (words[a] >> t) & 1, (words[a] >> (16 + t)) & 1
                        if matched and not ignored:
                            tp += 1
                        if not matched and not ignored:
                            fp += 1
                        rc_l.append(tp / n_pos)
                        pr_l.append(tp / (fp + tp + eps))
                    recall[t, k, a, mi] = rc_l[-1] if dets else 0.0
                    for i in range(len(pr_l) - 1, 0, -1):
                        if pr_l[i] > pr_l[i - 1]:
                            pr_l[i - 1] = pr_l[i]
                    for ri, thr in enumerate(rec_thrs):
                        pi = 0
                        while pi < len(rc_l) and rc_l[pi] < thr:           # searchsorted(rc, thr, side="left")
                            pi += 1
                        precision[t, ri, k, a, mi] = pr_l[pi] if pi < len(pr_l) else 0.0

    def mean(values):
        values = [v for v in values if v > -1]
        return sum(values) / len(values) if values else -1.0

    def t_of(v):
        hit = [t for t, th in enumerate(thresholds) if abs(th - v) < 1e-9]
        return hit[0] if hit else None

    def ap(a, t=None):
        if a >= na or (t is not None and t_of(t) is None):
            return -1.0
        ts = range(nt) if t is None else [t_of(t)]
        return mean([precision[tt, ri, k, a, nm - 1] for tt in ts for ri in range(101) for k in range(nb_class)])

    def ar(a, mi):
        if a >= na or mi >= nm:
            return -1.0
        return mean([recall[tt, k, a, mi] for tt in range(nt) for k in range(nb_class)])

    stats = dict(AP=ap(0), AP50=ap(0, 0.5), AP75=ap(0, 0.75), APs=ap(1), APm=ap(2), APl=ap(3), AR1=ar(0, 0), AR10=ar(0, 1), AR100=ar(0, 2),
                 ARs=ar(1, nm - 1), ARm=ar(2, nm - 1), ARl=ar(3, nm - 1))
    per_class_ap = [mean([precision[tt, ri, k, 0, nm - 1] for tt in range(nt) for ri in range(101)]) for k in range(nb_class)]
    return stats, per_class_ap, precision, recall


# ---- seeded batches --------------------------------------------------------------------------------------------------------------
def _yxyx(t):
    return targets_to_yxyx(np.asarray(t, np.float32).reshape(-1, 4))


def empty_batch(B, Q, R):
    return dict(boxes=np.zeros((B, Q, 4), np.float32), labels=np.zeros((B, Q), np.int64), scores=np.zeros((B, Q), np.float32),
                counts=np.zeros(B, np.int32), t_bbox=np.zeros((B, R, 4), np.float32), t_class=np.zeros((B, R, 1), np.int64),
                t_crowd=np.zeros((B, R), np.uint8), t_area=np.zeros((B, R), np.float32), sizes=np.zeros((B, 2), np.int32))


KEYS = ("boxes", "labels", "scores", "counts", "t_bbox", "t_class", "t_crowd", "t_area", "sizes")


def as_args(bt):
    return tuple(bt[k] for k in KEYS)


def fill_image(bt, b, dets, t, tcls, crowd, area, size, perm=None):
    """dets: [(yxyx box, class, score)]; t: [n, 4] cx cy w h; writes image b of the batch."""
    order = np.arange(len(dets)) if perm is None else perm
    for k, i in enumerate(order):
        bt["boxes"][b, k], bt["labels"][b, k], bt["scores"][b, k] = dets[i]
    bt["counts"][b] = len(dets)
    n = len(tcls)
    bt["t_bbox"][b, 0, 0] = n
    bt["t_bbox"][b, 1:1 + n], bt["t_class"][b, 1:1 + n, 0] = np.asarray(t, np.float32).reshape(-1, 4), tcls
    bt["t_crowd"][b, 1:1 + n], bt["t_area"][b, 1:1 + n] = crowd, area
    bt["sizes"][b] = size


def random_batches(B, Q, R, C, seed, n_batches=2):
    """Batches in the post-processed layout with every rule planted.  Image g (counted over the batches) is
      g = 0: two identical ground truths under two identical detections (the first takes the LATER index); a crowd of the same class
             with three detections inside it (all absorbed); a detection over a regular AND a crowd ground truth (takes the regular);
             an unmatched tiny detection (ignored outside `small`, a false positive in `all`); a NaN score; a zero-area pair;
      g = 1: no detection, R - 1 ground truths;      g = 2: only crowd ground truths, detections inside them;
      g = 3: detections, no ground truth;
      else : random ground truths over few classes with areas in every range and ~15 % crowds, exact / shrunk copies and random
             boxes as detections, scores rounded to two decimals (ties)."""
    rng = np.random.default_rng(seed)
    fc = C - 1

    def rand_targets(n, classes, p_crowd=0.15):
        t = np.concatenate([rng.uniform(0.1, 0.9, (n, 2)), rng.uniform(0.02, 0.5, (n, 2))], 1).astype(np.float32)
        return t, rng.choice(classes, n).astype(np.int64), (rng.random(n) < p_crowd).astype(np.uint8)

    def areas(t, size, exact=False):
        box = _yxyx(t)
        px = (box[:, 2] - box[:, 0]).astype(np.float64) * size[0] * (box[:, 3] - box[:, 1]) * size[1]
        return (px * (1.0 if exact else rng.uniform(0.4, 1.0, len(t)))).astype(np.float32)      # a mask's area is below its box's

    def score():
        return np.float32(round(float(rng.uniform(0.05, 0.99)), 2))

    def copies(t, tcls, room):
        dets = []
        for j in rng.permutation(len(tcls))[:max(room, 0)]:
            box = _yxyx(t[j:j + 1])[0]
            if rng.random() < 0.7:
                s = np.float32(rng.uniform(0.6, 1.0))
                cy, cx, h, w = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2, (box[2] - box[0]) * s, (box[3] - box[1]) * s
                box = np.clip(np.array([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], np.float32), 0, 1)
            dets.append((box, int(tcls[j]), score()))
        return dets

    def rand_box():
        return np.sort(rng.uniform(0, 1, (2, 2)), 0).reshape(4).astype(np.float32)

    out, g = [], 0
    for _ in range(n_batches):
        bt = empty_batch(B, Q, R)
        for b in range(B):
            size = (int(rng.integers(60, 700)), int(rng.integers(60, 700)))
            perm = None
            if g == 0 and R >= 9 and Q >= 12:
                size = (480, 640)
                t = np.array([[0.2, 0.2, 0.2, 0.2], [0.2, 0.2, 0.2, 0.2],          # 0, 1: identical, class 0
                              [0.7, 0.3, 0.5, 0.5],                                   # 2: crowd, class 1
                              [0.6, 0.3, 0.1, 0.1],                                   # 3: regular inside the crowd, class 1
                              [0.3, 0.8, 0.0, 0.1],                                   # 4: zero area, class 0
                              [0.5, 0.8, 0.05, 0.04]], np.float32)                    # 5: small regular, class 0
                tcls = np.array([0, 0, 1, 1, 0, 0], np.int64)
                crowd = np.array([0, 0, 1, 0, 0, 0], np.uint8)
                area = areas(t, size, exact=True)
                y = _yxyx(t)
                inside = [np.array([0.1, 0.5, 0.2, 0.6], np.float32), np.array([0.3, 0.55, 0.45, 0.8], np.float32),
                          np.array([0.12, 0.7, 0.3, 0.9], np.float32)]
                dets = [(y[0], 0, np.float32(0.9)), (y[0], 0, np.float32(0.9)),       # both match; the first takes index 1
                        (y[3], 1, np.float32(0.8))] + [(bx, 1, np.float32(0.7)) for bx in inside] + \
                       [(np.array([0.9, 0.9, 0.91, 0.915], np.float32), 0, np.float32(0.95)),    # tiny and unmatched
                        (y[4], 0, np.float32(0.5)), (y[5], 0, np.float32("nan"))]
                ft, fcl, fcr = rand_targets(2, [fc], 0.0)
                dets += copies(ft, fcl, min(2, Q - len(dets)))
                t, tcls, crowd, area = np.concatenate([t, ft]), np.concatenate([tcls, fcl]), np.concatenate([crowd, fcr]), \
                    np.concatenate([area, areas(ft, size)])
            elif g == 1:
                t, tcls, crowd = rand_targets(R - 1, np.arange(C))
                area, dets = areas(t, size), []
            elif g == 2:
                n = min(3, R - 1)
                t, tcls, _ = rand_targets(n, np.arange(min(C, 2)))
                crowd, area = np.ones(n, np.uint8), areas(t, size)
                dets = (copies(t, tcls, n) + copies(t, tcls, n))[:Q]
            elif g == 3:
                t, tcls, crowd, area = np.zeros((0, 4), np.float32), np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.float32)
                dets = [(rand_box(), int(rng.integers(C)), score()) for _ in range(min(Q, 20))]
            else:
                classes = rng.choice(C, min(C, 4), replace=False)
                t, tcls, crowd = rand_targets(int(rng.integers(1, min(30, R))), classes)
                area = areas(t, size)
                dets = copies(t, tcls, Q // 2)
                dets += [(rand_box(), int(rng.choice(classes)), score()) for _ in range(int(rng.integers(0, Q - len(dets) + 1)))]
                perm = rng.permutation(len(dets))
            fill_image(bt, b, dets, t, tcls, crowd, area, size, perm)
            g += 1
        out.append(bt)
    return out


def dense_batch(B=2, Q=128, R=256, C=3, seed=11):
    """Every image has R - 1 ground truths over C classes (~15 % crowds, areas in every range) and Q detections that are exact or
    shrunk copies of ground truths drawn from EVERY quarter of the index range (so with R = 256 the matching runs on ground truths
    0..63, 64..127, 128..191 and 192..254), two-decimal scores (ties), plus, per image: a ground truth duplicated at the LAST index
    under two identical detections (a tie between index 70 and index R - 2: the later one is taken first), three detections inside
    a crowd placed at index 130, and a few random boxes."""
    rng = np.random.default_rng(seed)
    n = R - 1
    bt = empty_batch(B, Q, R)
    for b in range(B):
        size = (int(rng.integers(300, 700)), int(rng.integers(300, 700)))
        t = np.concatenate([rng.uniform(0.1, 0.9, (n, 2)), rng.uniform(0.03, 0.4, (n, 2))], 1).astype(np.float32)
        tcls = rng.integers(0, C, n).astype(np.int64)
        crowd = (rng.random(n) < 0.15).astype(np.uint8)
        if n > 140:
            t[n - 1], tcls[n - 1], crowd[n - 1], crowd[70] = t[70], tcls[70], 0, 0               # identical boxes at 70 and n - 1
            t[130], crowd[130] = (0.5, 0.5, 0.6, 0.6), 1                                          # a large crowd
        box = _yxyx(t)
        area = ((box[:, 2] - box[:, 0]).astype(np.float64) * size[0] * (box[:, 3] - box[:, 1]) * size[1] * rng.uniform(0.4, 1.0, n)).astype(np.float32)
        dets = []
        if n > 140:
            dets += [(box[70], int(tcls[70]), np.float32(0.97)), (box[70], int(tcls[70]), np.float32(0.97))]
            dets += [(np.array([0.3 + 0.1 * i, 0.3, 0.4 + 0.1 * i, 0.45], np.float32), int(tcls[130]), np.float32(0.6)) for i in range(3)]
        quarters = np.array_split(rng.permutation(n), 4)
        room = Q - len(dets) - 6
        for k in range(room):
            j = int(quarters[k % 4][(k // 4) % len(quarters[k % 4])])
            bx = box[j]
            if rng.random() < 0.6:
                s = np.float32(rng.uniform(0.6, 1.0))
                cy, cx, h, w = (bx[0] + bx[2]) / 2, (bx[1] + bx[3]) / 2, (bx[2] - bx[0]) * s, (bx[3] - bx[1]) * s
                bx = np.clip(np.array([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], np.float32), 0, 1)
            dets.append((bx, int(tcls[j]), np.float32(round(float(rng.uniform(0.05, 0.95)), 2))))
        dets += [(np.sort(rng.uniform(0, 1, (2, 2)), 0).reshape(4).astype(np.float32), int(rng.integers(C)),
                  np.float32(round(float(rng.uniform(0.05, 0.95)), 2))) for _ in range(6)]
        fill_image(bt, b, dets, t, tcls, crowd, area, size, rng.permutation(len(dets)))
    return bt


@functools.lru_cache(maxsize=None)
def dense_case(C=3):
    """(batch, oracle result, per-image sets of matched ground-truth indices) of dense_batch(), computed once per process."""
    bt, taken = dense_batch(C=C), []
    want = coco_match_ref(*as_args(bt), C, taken=taken)
    return bt, want, taken


def assert_every_chunk_matched(taken, R=256):
    """Some detection matched a ground truth in each 64-wide chunk of the index range, in every image; the duplicated ground
    truth at the last index was taken (the later index wins the tie) and so was the crowd at 130."""
    for hit in taken:
        for k in range((R - 1 + 63) // 64):
            assert any(k * 64 <= g < (k + 1) * 64 for g in hit), (k, sorted(hit))
        assert R - 2 in hit and 70 in hit and 130 in hit and max(hit) >= 192
