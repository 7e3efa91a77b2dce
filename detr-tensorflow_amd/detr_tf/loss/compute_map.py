"""COCO-style box mAP accumulator -- the arithmetic of the reference's detr_tf/loss/compute_map.py (:17-83 APDataObject,
:124-139 compute_overlaps, :141-168 calc_map, :183-272 cal_map), vectorised with NumPy.

The reference walks predictions x ground truths x classes x 10 IoU thresholds in pure Python for every image.  Here the
IoU matrix is one broadcast, the greedy matching of an image runs for all ten thresholds at once (the only sequential
dimension left is the detections of ONE class in score order, because a ground truth is consumed by the first detection
that claims it), and the AP integration is cummax + searchsorted.  Semantics kept exactly:
  * boxes are [y1, x1, y2, x2]; a detection matches the unused same-class ground truth of LARGEST IoU strictly above the
    threshold, the lowest index on ties (cal_map :233-247);
  * detections are visited by descending score, stable (:207); the data points of a class are sorted by descending
    score, stable, before the precision / recall sweep (:40);
  * AP = mean of the 101-point interpolated precision envelope (:61-83); classes with neither detections nor ground
    truths are left out of the mean (:149-150); `all` = mean over the ten thresholds (:160);
  * the reference also accumulates a 'mask' metric on all-zero dummy masks (eval.py:54): every detection is a false
    positive there, so every non-empty class has mask AP 0; `result()` reports exactly that.
"""
from collections import OrderedDict
from ctypes import byref

import numpy as np
import torch

from .. import _hip as hip

IOU_THRESHOLDS = [x / 100.0 for x in range(50, 100, 5)]          # eval.py:33


def compute_overlaps(boxes1, boxes2):
    """IoU matrix [len(boxes1), len(boxes2)] of [y1, x1, y2, x2] boxes (compute_map.py:103-139)."""
    b1, b2 = np.asarray(boxes1, np.float64).reshape(-1, 4), np.asarray(boxes2, np.float64).reshape(-1, 4)
    area1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    area2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    y1 = np.maximum(b1[:, None, 0], b2[None, :, 0])
    y2 = np.minimum(b1[:, None, 2], b2[None, :, 2])
    x1 = np.maximum(b1[:, None, 1], b2[None, :, 1])
    x2 = np.minimum(b1[:, None, 3], b2[None, :, 3])
    inter = np.maximum(x2 - x1, 0) * np.maximum(y2 - y1, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area1[:, None] + area2[None, :] - inter)


def average_precision(scores, is_true, num_gt_positives):
    """APDataObject.get_ap (:37-83) for one (class, threshold): arrays in push order."""
    if num_gt_positives == 0:
        return 0
    order = np.argsort(-np.asarray(scores, np.float64), kind="stable")
    tp = np.asarray(is_true, bool)[order]
    if tp.size == 0:
        return 0.0
    num_true = np.cumsum(tp)
    precisions = num_true / np.arange(1, tp.size + 1)
    recalls = num_true / num_gt_positives
    precisions = np.maximum.accumulate(precisions[::-1])[::-1]            # right-to-left running maximum (:61-63)
    idx = np.searchsorted(recalls, np.arange(101) / 100.0, side="left")
    y = np.where(idx < tp.size, precisions[np.minimum(idx, tp.size - 1)], 0.0)
    return float(y.sum() / 101)


class APAccumulator:
    """ap_data of eval.py:34-37 / WandbSender.init_ap_data, box metric, all thresholds."""

    def __init__(self, nb_class, iou_thresholds=None):
        self.thresholds = list(IOU_THRESHOLDS if iou_thresholds is None else iou_thresholds)
        self.nb_class = int(nb_class)
        nt = len(self.thresholds)
        self.scores = [[] for _ in range(self.nb_class)]                 # per class: detection scores in push order
        self.flags = [[] for _ in range(self.nb_class)]                  # per class: [n_det, nt] true-positive flags
        self.num_gt = np.zeros(self.nb_class, np.int64)
        self._nt = nt

    def add_image(self, p_bbox, p_labels, p_scores, t_bbox, t_labels):
        """cal_map (:183-272) for one image; boxes [y1, x1, y2, x2]."""
        p_bbox = np.asarray(p_bbox, np.float64).reshape(-1, 4)
        t_bbox = np.asarray(t_bbox, np.float64).reshape(-1, 4)
        classes = np.asarray(p_labels).astype(int).reshape(-1)
        scores = np.asarray(p_scores).astype(float).reshape(-1)
        gt_classes = np.asarray(t_labels).astype(int).reshape(-1)
        iou = compute_overlaps(p_bbox, t_bbox) if len(classes) and len(gt_classes) else np.zeros((len(classes), len(gt_classes)))
        order = np.argsort(-scores, kind="stable")
        thr = np.asarray(self.thresholds)[:, None]
        for c in sorted(set(classes.tolist()) | set(gt_classes.tolist())):
            gt_idx = np.nonzero(gt_classes == c)[0]
            self.num_gt[c] += len(gt_idx)
            det = order[classes[order] == c]
            if len(det) == 0:
                continue
            flags = np.zeros((len(det), self._nt), bool)
            if len(gt_idx):
                used = np.zeros((self._nt, len(gt_idx)), bool)
                sub = iou[np.ix_(det, gt_idx)]
                for k in range(len(det)):                                  # sequential: a ground truth is consumed once
                    cand = np.where(used | ~(sub[k][None, :] > thr), -np.inf, sub[k][None, :])
                    j = np.argmax(cand, axis=1)                            # first index of the largest IoU (ties: lowest j)
                    hit = cand[np.arange(self._nt), j] > -np.inf
                    used[np.nonzero(hit)[0], j[hit]] = True
                    flags[k] = hit
            self.scores[c].extend(scores[det].tolist())
            self.flags[c].append(flags)

    def result(self, class_names=None, print_result=False):
        """calc_map (:141-168): {'box': {'all', 50, 55, ..., 95}, 'mask': {...}} rounded to 2 decimals."""
        n_cls = self.nb_class if class_names is None else len(class_names)
        aps = [[] for _ in self.thresholds]
        n_nonempty = 0
        for c in range(n_cls):
            n_det = len(self.scores[c])
            if n_det == 0 and self.num_gt[c] == 0:
                continue                                                   # is_empty()
            n_nonempty += 1
            flags = np.concatenate(self.flags[c], 0) if n_det else np.zeros((0, self._nt), bool)
            for t in range(self._nt):
                aps[t].append(average_precision(self.scores[c], flags[:, t], int(self.num_gt[c])))
        all_maps = {"box": OrderedDict(), "mask": OrderedDict()}
        for kind in ("box", "mask"):
            all_maps[kind]["all"] = 0
            for t, th in enumerate(self.thresholds):
                vals = aps[t] if kind == "box" else [0.0] * n_nonempty    # dummy zero masks: every detection is a false positive
                all_maps[kind][int(th * 100)] = sum(vals) / len(vals) * 100 if len(vals) > 0 else 0
            all_maps[kind]["all"] = sum(all_maps[kind].values()) / (len(all_maps[kind].values()) - 1)
        if print_result:
            print_maps(all_maps)
        return {k: {j: round(u, 2) for j, u in v.items()} for k, v in all_maps.items()}


def group_records(rec_score, rec_class, rec_flags, nb_class, n_thr):
    """Records of detr_hip_map_match -> (scores, flags) as APAccumulator holds them.  The records are flat arrays in push order
    (image after image, inside an image by descending score): rec_score fp32, rec_class int32 (-1 = empty slot or skipped
    detection), rec_flags uint32 with bit t = true positive at threshold t.  scores[c] is the list of class c's scores in that
    order; flags[c] is [] or one [n_det, n_thr] bool array (APAccumulator keeps one array per image; only their concatenation
    is ever read)."""
    score = np.ascontiguousarray(rec_score, np.float32).reshape(-1)
    cls = np.ascontiguousarray(rec_class, np.int32).reshape(-1)
    word = np.ascontiguousarray(rec_flags, np.uint32).reshape(-1)
    if cls.size and int(cls.max()) >= nb_class:
        raise ValueError(f"group_records: class {int(cls.max())} in the records, nb_class is {nb_class}")
    keep = cls >= 0
    score, cls, word = score[keep].astype(np.float64), cls[keep], word[keep]
    bits = ((word[:, None] >> np.arange(n_thr, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(bool)
    order = np.argsort(cls, kind="stable")
    bounds = np.searchsorted(cls[order], np.arange(nb_class + 1))
    scores, flags = [], []
    for c in range(nb_class):
        idx = order[bounds[c]:bounds[c + 1]]
        scores.append(score[idx].tolist())
        flags.append([bits[idx]] if len(idx) else [])
    return scores, flags


class _DeviceAccumulator:
    """What DeviceAPAccumulator and coco_eval.DeviceCOCOAccumulator share: the device and its status word, the upload and the checks of
    the tensors a batch brings, and the one copy that brings status, counters and records back.  A subclass sets BAD (status bit ->
    text), fills its descriptor in add_detections and appends one int32 [width, B, Q] record block per batch to self._records."""
    BAD = {}

    def _open(self, device, host_class):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}: the matching is a HIP kernel; there is no CPU fallback (use {host_class})")
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._records = []

    def _device(self, x, dtype):
        if torch.is_tensor(x) and x.is_cuda:
            return x.to(device=self.device, dtype=dtype)
        t = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(dtype)
        return t.pin_memory().to(self.device, non_blocking=True)      # pinned + asynchronous: the upload does not block the host

    def _check_tensors(self, want):
        """want: (name, tensor, dtype, number of dimensions or None) of every argument of add_detections."""
        for name, t, dt, nd in want:
            if not (torch.is_tensor(t) and t.is_cuda and t.device == self.device and t.dtype == dt and (nd is None or t.dim() == nd)):
                raise TypeError(f"add_detections: {name} must be a {dt} tensor on {self.device}" + (f" with {nd} dimensions" if nd else ""))

    def _unpack(self, counters):
        """One synchronisation, one device-to-host copy (status word, the int64 counters and every batch's records in one buffer)
        -> (counters, [records int32 [width, B * Q] per batch]).  ValueError when the kernel flagged an input."""
        shapes = [tuple(r.shape) for r in self._records]
        buf = torch.cat([self._status, counters.view(torch.int32)] + [r.reshape(-1) for r in self._records]).cpu().numpy()
        status, off = int(buf[0]), 1 + 2 * counters.numel()
        if status:
            raise ValueError(f"{type(self).__name__}: " + "; ".join(text for bit, text in self.BAD.items() if status & bit))
        recs = []
        for width, B, Q in shapes:
            recs.append(np.ascontiguousarray(buf[off:off + width * B * Q].reshape(width, B * Q)))
            off += width * B * Q
        return buf[1:1 + 2 * counters.numel()].copy().view(np.int64), recs

    def result(self, class_names=None, print_result=False):
        return self.to_host().result(class_names, print_result=print_result)


class DeviceAPAccumulator(_DeviceAccumulator):
    """APAccumulator whose per-image work runs on the device: one detr_hip_map_match launch per batch (after the one of
    detr_hip_postprocess), no host synchronisation until `to_host()`.  The flags, scores and ground-truth counts are the host
    path's exactly (same fp64 IoU arithmetic, same visiting order, same tie rules)."""
    BAD = hip.MAP_BAD

    def __init__(self, nb_class, iou_thresholds=None, device=None):
        self.thresholds = list(IOU_THRESHOLDS if iou_thresholds is None else iou_thresholds)
        self.nb_class = int(nb_class)
        if not 1 <= len(self.thresholds) <= hip.MAP_MAX_THR:
            raise ValueError(f"DeviceAPAccumulator: {len(self.thresholds)} thresholds, 1..{hip.MAP_MAX_THR} are supported")
        if self.nb_class <= 0:
            raise ValueError("DeviceAPAccumulator: nb_class must be positive")
        self._open(device, "APAccumulator")                # records per batch: int32 [3, B, Q] = score bits, class, flag word
        self._num_gt = torch.zeros(self.nb_class, dtype=torch.int64, device=self.device)

    def add_detections(self, boxes, labels, scores, counts, t_bbox, t_class):
        """Device tensors: what detr_hip_postprocess wrote in "yxyx" format (boxes [B, Q, 4] fp32, labels [B, Q] int64, scores
        [B, Q] fp32, counts [B] int32) and the padded targets t_bbox [B, R, 4] fp32 (header row 0), t_class [B, R, 1] int64."""
        self._check_tensors((("boxes", boxes, torch.float32, 3), ("labels", labels, torch.int64, 2), ("scores", scores, torch.float32, 2),
                             ("counts", counts, torch.int32, 1), ("t_bbox", t_bbox, torch.float32, 3), ("t_class", t_class, torch.int64, None)))
        B, Q = labels.shape
        R = t_bbox.shape[1]
        if tuple(boxes.shape) != (B, Q, 4) or tuple(scores.shape) != (B, Q) or tuple(counts.shape) != (B,) or \
                tuple(t_bbox.shape) != (B, R, 4) or tuple(t_class.shape) not in ((B, R, 1), (B, R)):
            raise ValueError("add_detections: shapes must be boxes [B, Q, 4], labels / scores [B, Q], counts [B], t_bbox [B, R, 4], "
                             "t_class [B, R, 1]")
        boxes, labels, scores, counts = boxes.contiguous(), labels.contiguous(), scores.contiguous(), counts.contiguous()
        t_bbox, t_class = t_bbox.contiguous(), t_class.contiguous()
        rec = torch.empty(3, B, Q, dtype=torch.int32, device=self.device)
        d = hip.MapMatchDesc()
        d.B, d.Q, d.R, d.nb_class, d.n_thr = B, Q, R, self.nb_class, len(self.thresholds)
        d.boxes, d.labels, d.scores, d.counts, d.sD_b = boxes.data_ptr(), labels.data_ptr(), scores.data_ptr(), counts.data_ptr(), Q
        d.t_bbox, d.sT_b, d.t_class, d.sC_b = t_bbox.data_ptr(), R * 4, t_class.data_ptr(), R
        for t, th in enumerate(self.thresholds):
            d.thresholds[t] = float(th)
        d.rec_score, d.rec_class, d.rec_flags = rec[0].data_ptr(), rec[1].data_ptr(), rec[2].data_ptr()
        d.num_gt, d.status = self._num_gt.data_ptr(), self._status.data_ptr()
        hip._check(hip.load().detr_hip_map_match(byref(d), hip._stream()), "detr_hip_map_match")
        self._records.append(rec)

    def add_batch(self, m_outputs, t_bbox, t_class, background_class, scoring="softmax", multilabel=None):
        """The post-processing launch plus the match launch for one batch of model outputs; host / NumPy targets are uploaded
        asynchronously.  No host synchronisation.  scoring: get_model_inference_batched's.  multilabel = K: the rows are
        the K best (query, class) pairs of every image (detr_hip_postprocess_multilabel, sigmoid scoring) and K is the matcher's row capacity."""
        from ..inference import _post, _post_multilabel
        if multilabel is None:
            out_b, out_l, out_s, counts = _post(m_outputs["pred_logits"], m_outputs["pred_boxes"], background_class, "yxyx", scoring)
        else:
            out_b, out_l, out_s, counts = _post_multilabel(m_outputs["pred_logits"], m_outputs["pred_boxes"], background_class, "yxyx", multilabel)
        self.add_detections(out_b, out_l, out_s, counts, self._device(t_bbox, torch.float32), self._device(t_class, torch.int64))

    def to_host(self):
        """One synchronisation, one device-to-host copy -> the APAccumulator the host path would hold.  ValueError when the kernel
        flagged an input."""
        num_gt, parts = self._unpack(self._num_gt)
        rec = np.concatenate(parts, 1) if parts else np.zeros((3, 0), np.int32)
        acc = APAccumulator(self.nb_class, self.thresholds)
        acc.scores, acc.flags = group_records(np.ascontiguousarray(rec[0]).view(np.float32), rec[1], np.ascontiguousarray(rec[2]).view(np.uint32),
                                              self.nb_class, len(self.thresholds))
        acc.num_gt = num_gt.astype(np.int64)
        return acc


def print_maps(all_maps):
    """The table of compute_map.py:170-181."""
    def make_row(vals):
        return (" %5s |" * len(vals)) % tuple(vals)

    def make_sep(n):
        return "-------+" * n

    print()
    print(make_row([""] + [(".%d " % x if isinstance(x, int) else x + " ") for x in all_maps["box"].keys()]))
    print(make_sep(len(all_maps["box"]) + 1))
    for kind in ("box", "mask"):
        print(make_row([kind] + ["%.2f" % x if x < 100 else "%.1f" % x for x in all_maps[kind].values()]))
    print(make_sep(len(all_maps["box"]) + 1))
    print()
