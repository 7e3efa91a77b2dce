"""COCO-protocol box evaluation: AP / AP50 / AP75 / APs / APm / APl / AR1 / AR10 / AR100 / ARs / ARm / ARl.

compute_map.py keeps the reference's YOLACT-style cal_map.  This module restates the protocol DETR results are quoted in --
COCOeval's bbIou / evaluateImg (per image) and accumulate / summarize (per evaluation) -- for boxes:
  * crowd regions: IoU against a crowd is intersection over the DETECTION's area, and a crowd absorbs any number of detections;
  * area ranges: a ground truth outside the range (or a crowd) is `ignored`: it does not count as a positive, and a detection
    matched to it, or an unmatched detection whose own pixel area is outside the range, counts neither as true nor as false positive;
  * maxDets: only the `maxDet` best detections of a class in an image are counted (1, 10, 100);
  * recall next to precision.
The per-image half has the semantics of csrc/coco_match.hip (include/detr_hip.h: detr_hip_coco_match), bit for bit: COCOAccumulator
runs it in NumPy on the host, DeviceCOCOAccumulator as one launch per batch on the device.  Three deviations from running
pycocotools on the annotation file: boxes are clipped to the image before matching, IoU is taken on per-image-normalised fp32
boxes rather than on JSON doubles, and parity with pycocotools itself is not pinned by a test.
"""
from collections import OrderedDict
from ctypes import byref

import numpy as np
import torch

from .. import _hip as hip
from .compute_map import _DeviceAccumulator

IOU_THRESHOLDS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1)
RECALL_THRESHOLDS = np.linspace(0.0, 1.0, 101)
AREA_RANGES = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
AREA_NAMES = ("all", "small", "medium", "large")
MAX_DETS = (1, 10, 100)
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


def box_iou(p_bbox, t_bbox, t_crowd):
    """bbIou on [y1, x1, y2, x2] boxes, fp64: [len(p_bbox), len(t_bbox)].  Against a crowd the union is the detection's area."""
    p = np.asarray(p_bbox, np.float64).reshape(-1, 4)[:, None, :]
    g = np.asarray(t_bbox, np.float64).reshape(-1, 4)[None, :, :]
    crowd = np.asarray(t_crowd, bool).reshape(1, -1)
    w = np.where(p[..., 3] < g[..., 3], p[..., 3], g[..., 3]) - np.where(p[..., 1] > g[..., 1], p[..., 1], g[..., 1])
    h = np.where(p[..., 2] < g[..., 2], p[..., 2], g[..., 2]) - np.where(p[..., 0] > g[..., 0], p[..., 0], g[..., 0])
    inter = w * h
    area_p = (p[..., 3] - p[..., 1]) * (p[..., 2] - p[..., 0])
    area_g = (g[..., 3] - g[..., 1]) * (g[..., 2] - g[..., 0])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        union = np.where(crowd, np.broadcast_to(area_p, inter.shape), area_p + area_g - inter)
        return np.where((w > 0) & (h > 0), inter / union, 0.0)


def _last_best(eligible, v):
    """Along the last axis: (any eligible, index of the LAST eligible entry of largest v) -- what a walk in index order with
    `>=` against a bound that rises to every taken value ends on."""
    val = np.where(eligible, v, -np.inf)
    n = val.shape[-1]
    return eligible.any(-1), n - 1 - np.argmax(val[..., ::-1], axis=-1)


class COCOAccumulator:
    """Host path.  Holds the per-detection records (score, class, in-class rank, one flag word per area range: bit t = matched at
    thresholds[t], bit 16 + t = ignored) in push order and npig[class][area range], the number of non-ignored ground truths."""

    def __init__(self, nb_class, iou_thresholds=None, area_ranges=None, max_dets=MAX_DETS):
        self.thresholds = [float(t) for t in (IOU_THRESHOLDS if iou_thresholds is None else iou_thresholds)]
        self.area_ranges = [[float(lo), float(hi)] for lo, hi in (AREA_RANGES if area_ranges is None else area_ranges)]
        self.max_dets = tuple(int(m) for m in max_dets)
        self.nb_class = int(nb_class)
        if not 1 <= len(self.thresholds) <= hip.COCO_MAX_THR:
            raise ValueError(f"COCOAccumulator: {len(self.thresholds)} thresholds, 1..{hip.COCO_MAX_THR} are supported")
        if not 1 <= len(self.area_ranges) <= hip.COCO_MAX_AREA:
            raise ValueError(f"COCOAccumulator: {len(self.area_ranges)} area ranges, 1..{hip.COCO_MAX_AREA} are supported")
        if self.nb_class <= 0:
            raise ValueError("COCOAccumulator: nb_class must be positive")
        self.npig = np.zeros((self.nb_class, len(self.area_ranges)), np.int64)
        self._rec = []                                   # (score fp32 [n], class int32 [n], rank int32 [n], flags uint32 [n, n_area])

    def add_records(self, score, cls, rank, flags):
        """Records as detr_hip_coco_match writes them (flat, push order; flags [n_area, n]); class -1 slots are dropped."""
        score, cls = np.ascontiguousarray(score, np.float32).reshape(-1), np.ascontiguousarray(cls, np.int32).reshape(-1)
        rank = np.ascontiguousarray(rank, np.int32).reshape(-1)
        flags = np.ascontiguousarray(flags, np.uint32).reshape(len(self.area_ranges), -1)
        if cls.size and int(cls.max()) >= self.nb_class:
            raise ValueError(f"COCOAccumulator: class {int(cls.max())} in the records, nb_class is {self.nb_class}")
        keep = cls >= 0
        self._rec.append((score[keep], cls[keep], rank[keep], np.ascontiguousarray(flags[:, keep].T)))

    def records(self):
        """(score fp32 [N], class int32 [N], rank int32 [N], flags uint32 [N, n_area]) of everything pushed so far."""
        if not self._rec:
            return np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, len(self.area_ranges)), np.uint32)
        return tuple(np.concatenate(x, 0) for x in zip(*self._rec))

    def add_image(self, p_bbox, p_labels, p_scores, t_bbox, t_labels, t_crowd, t_area, size):
        """evaluateImg for one image.  Boxes [y1, x1, y2, x2] normalised to the image (fp32 values); t_area in pixels^2 of the
        original image; size = its (height, width)."""
        pb = np.asarray(p_bbox, np.float32).reshape(-1, 4).astype(np.float64)
        gt = np.asarray(t_bbox, np.float32).reshape(-1, 4).astype(np.float64)
        scores = np.asarray(p_scores, np.float32).reshape(-1)
        classes = np.asarray(p_labels).astype(np.int64).reshape(-1)
        gcls = np.asarray(t_labels).astype(np.int64).reshape(-1)
        crowd = np.asarray(t_crowd).reshape(-1) != 0
        garea = np.asarray(t_area, np.float32).reshape(-1).astype(np.float64)
        for what, c in (("label", classes), ("target class", gcls)):
            if c.size and (c.min() < 0 or c.max() >= self.nb_class):
                raise ValueError(f"COCOAccumulator.add_image: a {what} outside [0, {self.nb_class})")
        H, W = float(int(size[0])), float(int(size[1]))
        if H <= 0 or W <= 0:
            raise ValueError("COCOAccumulator.add_image: a non-positive image size")
        nd, na, nt = len(classes), len(self.area_ranges), len(self.thresholds)
        lo, hi = np.array(self.area_ranges)[:, 0:1], np.array(self.area_ranges)[:, 1:2]
        ig = crowd[None, :] | (garea[None, :] < lo) | (garea[None, :] > hi)                    # [na, ng]
        np.add.at(self.npig, (np.repeat(gcls, na), np.tile(np.arange(na), len(gcls))), (~ig).T.reshape(-1).astype(np.int64))
        if nd == 0:
            return
        pix = ((pb[:, 2] - pb[:, 0]) * H) * ((pb[:, 3] - pb[:, 1]) * W)
        det_out = (pix[None, :] < lo) | (pix[None, :] > hi)                                      # [na, nd]
        iou = box_iou(pb, gt, crowd)
        cur0 = np.minimum(np.array(self.thresholds), 1 - 1e-10)
        order = np.argsort(-scores.astype(np.float64), kind="stable")
        where = np.empty(nd, np.int64)
        where[order] = np.arange(nd)                                                             # slot of a detection in visiting order
        rank = np.zeros(nd, np.int32)
        words = np.zeros((nd, na), np.uint32)
        bit_m = (np.uint32(1) << np.arange(nt, dtype=np.uint32))[None, :]
        bit_i = (np.uint32(1) << (16 + np.arange(nt, dtype=np.uint32)))[None, :]
        for c in np.unique(classes):
            det = order[classes[order] == c]
            gidx = np.nonzero(gcls == c)[0]
            rank[where[det]] = np.arange(len(det))
            ig_c, crowd_c = ig[:, gidx][:, None, :], crowd[gidx][None, None, :]
            used = np.zeros((na, nt, len(gidx)), bool)
            a_idx, t_idx = np.nonzero(np.ones((na, nt), bool))
            for d in det:                                          # sequential: a ground truth is consumed once per (a, t)
                matched = np.zeros((na, nt), bool)
                ignored = np.broadcast_to(det_out[:, d:d + 1], (na, nt))
                if len(gidx):
                    v = iou[d, gidx][None, None, :]
                    ge = v >= cur0[None, :, None]
                    has1, j1 = _last_best(~ig_c & ~used & ge, v)
                    has2, j2 = _last_best(ig_c & (~used | crowd_c) & ge, v)
                    matched = has1 | has2
                    m = np.where(has1, j1, j2)
                    ignored = np.where(matched, ig[:, gidx][a_idx, m.reshape(-1)].reshape(na, nt), ignored)
                    used[a_idx[matched.reshape(-1)], t_idx[matched.reshape(-1)], m[matched]] = True
                words[where[d]] = (np.where(matched, bit_m, 0).sum(1) + np.where(ignored, bit_i, 0).sum(1)).astype(np.uint32)
        self._rec.append((scores[order], classes[order].astype(np.int32), rank, words))

    def evaluate(self):
        """COCOeval.accumulate: (precision [T, 101, K, A, M], recall [T, K, A, M]); -1 where the class has no non-ignored ground truth."""
        score, cls, rank, flags = self.records()
        nt, na, nm, K = len(self.thresholds), len(self.area_ranges), len(self.max_dets), self.nb_class
        precision = -np.ones((nt, len(RECALL_THRESHOLDS), K, na, nm))
        recall = -np.ones((nt, K, na, nm))
        by_class = np.argsort(cls, kind="stable")
        bounds = np.searchsorted(cls[by_class], np.arange(K + 1))
        tbits = np.arange(nt, dtype=np.uint32)[:, None]
        for k in range(K):
            if not self.npig[k].any():
                continue
            idx_k = by_class[bounds[k]:bounds[k + 1]]
            for mi, max_det in enumerate(self.max_dets):
                idx = idx_k[rank[idx_k] < max_det]
                idx = idx[np.argsort(-score[idx].astype(np.float64), kind="mergesort")]
                nd = len(idx)
                for a in range(na):
                    npig = int(self.npig[k, a])
                    if npig == 0:
                        continue
                    word = flags[idx, a][None, :]
                    matched, ignored = ((word >> tbits) & 1).astype(bool), ((word >> (tbits + np.uint32(16))) & 1).astype(bool)
                    tp = np.cumsum(matched & ~ignored, axis=1).astype(np.float64)
                    fp = np.cumsum(~matched & ~ignored, axis=1).astype(np.float64)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[:, k, a, mi] = rc[:, -1] if nd else 0.0
                    pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]               # right-to-left running maximum
                    for t in range(nt):
                        inds = np.searchsorted(rc[t], RECALL_THRESHOLDS, side="left")
                        precision[t, :, k, a, mi] = np.where(inds < nd, pr[t][np.minimum(inds, max(nd - 1, 0))], 0.0) if nd else 0.0
        return precision, recall

    def _summaries(self, precision, recall):
        """COCOeval.summarize's twelve (name, ap, iou threshold or None, area index, maxDet index) rows -> values."""
        def find(seq, value):
            hit = [i for i, v in enumerate(seq) if np.isclose(v, value)]
            return hit[0] if hit else None

        m_last = len(self.max_dets) - 1
        rows = [("AP", 1, None, 0, m_last), ("AP50", 1, 0.5, 0, m_last), ("AP75", 1, 0.75, 0, m_last), ("APs", 1, None, 1, m_last),
                ("APm", 1, None, 2, m_last), ("APl", 1, None, 3, m_last), ("AR1", 0, None, 0, 0), ("AR10", 0, None, 0, 1),
                ("AR100", 0, None, 0, 2), ("ARs", 0, None, 1, m_last), ("ARm", 0, None, 2, m_last), ("ARl", 0, None, 3, m_last)]
        out = []
        for name, ap, iou_thr, a, m in rows:
            t = None if iou_thr is None else find(self.thresholds, iou_thr)
            if a >= len(self.area_ranges) or m >= len(self.max_dets) or (iou_thr is not None and t is None):
                out.append((name, ap, iou_thr, a, m, -1.0))
                continue
            s = (precision[:, :, :, a, m] if ap else recall[:, :, a, m])
            s = s if t is None else s[t:t + 1]
            s = s[s > -1]
            out.append((name, ap, iou_thr, a, m, float(np.mean(s)) if s.size else -1.0))
        return out

    def result(self, class_names=None, print_result=False):
        """COCOeval.accumulate + summarize: OrderedDict of the twelve statistics (-1 = no cell to average) plus "per_class_AP",
        the AP @[.50:.95 | all | last maxDet] of every class (-1 for a class without non-ignored ground truths)."""
        precision, recall = self.evaluate()
        rows = self._summaries(precision, recall)
        out = OrderedDict((name, value) for name, *_, value in rows)
        n_cls = self.nb_class if class_names is None else min(len(class_names), self.nb_class)
        per_class = []
        for k in range(n_cls):
            s = precision[:, :, k, 0, len(self.max_dets) - 1]
            s = s[s > -1]
            per_class.append(float(np.mean(s)) if s.size else -1.0)
        out["per_class_AP"] = per_class
        if print_result:
            print_summary(rows, self.thresholds, self.max_dets)
        return out


def print_summary(rows, thresholds, max_dets):
    """COCOeval.summarize's twelve lines."""
    fmt = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
    for _name, ap, iou_thr, a, m, value in rows:
        iou = "{:0.2f}:{:0.2f}".format(thresholds[0], thresholds[-1]) if iou_thr is None else "{:0.2f}".format(iou_thr)
        print(fmt.format("Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou,
                         AREA_NAMES[a] if a < len(AREA_NAMES) else str(a), max_dets[m] if m < len(max_dets) else -1, value))


META_KEYS = ("crowd", "area", "size", "image_id")


def check_meta(meta, who):
    if not isinstance(meta, dict) or any(k not in meta for k in META_KEYS[:3]):
        raise TypeError(f"{who}: meta must be the dict of a with_meta=True loader (crowd [B, R], area [B, R], size [B, 2], image_id [B])")
    return meta


class DeviceCOCOAccumulator(_DeviceAccumulator):
    """COCOAccumulator whose per-image work runs on the device: one detr_hip_coco_match launch per batch (after the one of
    detr_hip_postprocess), no host synchronisation until `to_host()`.  Records and counts are the host path's exactly."""
    BAD = hip.COCO_BAD

    def __init__(self, nb_class, iou_thresholds=None, area_ranges=None, max_dets=MAX_DETS, device=None):
        self._host = COCOAccumulator(nb_class, iou_thresholds, area_ranges, max_dets)       # (validates; never filled)
        self.thresholds, self.area_ranges, self.max_dets = self._host.thresholds, self._host.area_ranges, self._host.max_dets
        self.nb_class = self._host.nb_class
        self._open(device, "COCOAccumulator")    # records per batch: int32 [3 + n_area, B, Q] = score bits, class, rank, flag words
        self._npig = torch.zeros(self.nb_class * len(self.area_ranges), dtype=torch.int64, device=self.device)

    def add_detections(self, boxes, labels, scores, counts, t_bbox, t_class, t_crowd, t_area, sizes):
        """Device tensors: what detr_hip_postprocess wrote in "yxyx" format (boxes [B, Q, 4] fp32, labels [B, Q] int64, scores
        [B, Q] fp32, counts [B] int32), the padded targets t_bbox [B, R, 4] fp32 (header row 0), t_class [B, R, 1] int64, and the
        loader's metadata t_crowd [B, R] uint8, t_area [B, R] fp32, sizes [B, 2] int32."""
        self._check_tensors((("boxes", boxes, torch.float32, 3), ("labels", labels, torch.int64, 2), ("scores", scores, torch.float32, 2),
                             ("counts", counts, torch.int32, 1), ("t_bbox", t_bbox, torch.float32, 3), ("t_class", t_class, torch.int64, None),
                             ("t_crowd", t_crowd, torch.uint8, 2), ("t_area", t_area, torch.float32, 2), ("sizes", sizes, torch.int32, 2)))
        B, Q = labels.shape
        R = t_bbox.shape[1]
        if tuple(boxes.shape) != (B, Q, 4) or tuple(scores.shape) != (B, Q) or tuple(counts.shape) != (B,) or \
                tuple(t_bbox.shape) != (B, R, 4) or tuple(t_class.shape) not in ((B, R, 1), (B, R)) or \
                tuple(t_crowd.shape) != (B, R) or tuple(t_area.shape) != (B, R) or tuple(sizes.shape) != (B, 2):
            raise ValueError("add_detections: shapes must be boxes [B, Q, 4], labels / scores [B, Q], counts [B], t_bbox [B, R, 4], "
                             "t_class [B, R, 1], t_crowd / t_area [B, R], sizes [B, 2]")
        boxes, labels, scores, counts = boxes.contiguous(), labels.contiguous(), scores.contiguous(), counts.contiguous()
        t_bbox, t_class, t_crowd, t_area, sizes = t_bbox.contiguous(), t_class.contiguous(), t_crowd.contiguous(), t_area.contiguous(), sizes.contiguous()
        na = len(self.area_ranges)
        rec = torch.empty(3 + na, B, Q, dtype=torch.int32, device=self.device)
        d = hip.CocoMatchDesc()
        d.B, d.Q, d.R, d.nb_class, d.n_thr, d.n_area = B, Q, R, self.nb_class, len(self.thresholds), na
        d.boxes, d.labels, d.scores, d.counts, d.sD_b = boxes.data_ptr(), labels.data_ptr(), scores.data_ptr(), counts.data_ptr(), Q
        d.t_bbox, d.sT_b, d.t_class, d.sC_b = t_bbox.data_ptr(), R * 4, t_class.data_ptr(), R
        d.t_crowd, d.t_area, d.sM_b, d.sizes = t_crowd.data_ptr(), t_area.data_ptr(), R, sizes.data_ptr()
        for t, th in enumerate(self.thresholds):
            d.thresholds[t] = th
        for a, (lo, hi) in enumerate(self.area_ranges):
            d.area_ranges[2 * a], d.area_ranges[2 * a + 1] = lo, hi
        d.rec_score, d.rec_class, d.rec_rank, d.rec_flags = rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr(), rec[3].data_ptr()
        d.npig, d.status = self._npig.data_ptr(), self._status.data_ptr()
        hip._check(hip.load().detr_hip_coco_match(byref(d), hip._stream()), "detr_hip_coco_match")
        self._records.append(rec)

    def add_batch(self, m_outputs, t_bbox, t_class, meta, background_class, scoring="softmax", multilabel=None):
        """The post-processing launch plus the match launch for one batch of model outputs; host / NumPy targets and metadata are
        uploaded asynchronously.  No host synchronisation.  scoring: get_model_inference_batched's.  multilabel = K: the rows are
        the K best (query, class) pairs of every image (detr_hip_postprocess_multilabel, sigmoid scoring) and K is the matcher's row capacity."""
        from ..inference import _post, _post_multilabel
        meta = check_meta(meta, "DeviceCOCOAccumulator.add_batch")
        if multilabel is None:
            out_b, out_l, out_s, counts = _post(m_outputs["pred_logits"], m_outputs["pred_boxes"], background_class, "yxyx", scoring)
        else:
            out_b, out_l, out_s, counts = _post_multilabel(m_outputs["pred_logits"], m_outputs["pred_boxes"], background_class, "yxyx", multilabel)
        self.add_detections(out_b, out_l, out_s, counts, self._device(t_bbox, torch.float32), self._device(t_class, torch.int64),
                            self._device(meta["crowd"], torch.uint8), self._device(meta["area"], torch.float32),
                            self._device(meta["size"], torch.int32))

    def to_host(self):
        """One synchronisation, one device-to-host copy -> the COCOAccumulator the host path would hold.  ValueError when the kernel
        flagged an input."""
        npig, recs = self._unpack(self._npig)
        acc = COCOAccumulator(self.nb_class, self.thresholds, self.area_ranges, self.max_dets)
        for rec in recs:
            acc.add_records(rec[0].view(np.float32), rec[1], rec[2], rec[3:].view(np.uint32))
        acc.npig = npig.reshape(self.nb_class, len(self.area_ranges)).astype(np.int64)
        return acc
