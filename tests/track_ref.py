"""The tracker (csrc/track.hip) restated in plain NumPy, step by step, from its specification (include/detr_hip.h: detr_track_desc).
A test helper, not product code: it is sequential and slow on purpose.

Every fp32 operation is an np.float32 scalar operation -- one rounding each, there is no fused multiply-add in NumPy --, the IoU is
Python floats (fp64) on the float32 corners, with the comparisons written as the kernel's ternaries so that a NaN takes the same
side.  The association sorts ALL candidate pairs by (descending IoU, lower id, lower detection) and walks them."""
import numpy as np

F = np.float32
TRACK_MAX = 256
FULL, BAD_COUNT = 1, 2
KEYS = ("x", "v", "label", "id", "hits", "miss", "confirmed", "score", "frame", "next_id")
DEFAULTS = dict(track_threshold=0.7, new_threshold=None, match_threshold=0.3, low_match_threshold=0.5, max_age=30, min_hits=3,
                alpha=0.75, beta=0.25, class_agnostic=False)


def iou(p, g):
    """fp64 IoU of two (x0, y0, x1, y1) float32 boxes: detections.h match_measure with match 0; 0 for a zero denominator."""
    px0, py0, px1, py1 = (float(v) for v in p)
    gx0, gy0, gx1, gy1 = (float(v) for v in g)
    ix = (px1 if px1 < gx1 else gx1) - (px0 if px0 > gx0 else gx0)
    iy = (py1 if py1 < gy1 else gy1) - (py0 if py0 > gy0 else gy0)
    inter = (ix if ix > 0.0 else 0.0) * (iy if iy > 0.0 else 0.0)
    ap, ag = (px1 - px0) * (py1 - py0), (gx1 - gx0) * (gy1 - gy0)
    den = ap + ag - inter
    if den == 0.0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.float64(inter) / np.float64(den))           # IEEE division: inf and NaN come out as the device gives them


def fresh_state():
    return {"x": np.zeros((TRACK_MAX, 4), F), "v": np.zeros((TRACK_MAX, 4), F), "label": np.zeros(TRACK_MAX, np.int64),
            "id": np.zeros(TRACK_MAX, np.int32), "hits": np.zeros(TRACK_MAX, np.int32), "miss": np.zeros(TRACK_MAX, np.int32),
            "confirmed": np.zeros(TRACK_MAX, bool), "score": np.zeros(TRACK_MAX, F), "frame": np.int32(0), "next_id": np.int32(1)}


def to_z(b):
    half = F(0.5)
    return np.array([(b[0] + b[2]) * half, (b[1] + b[3]) * half, b[2] - b[0], b[3] - b[1]], F)


class RefTracker:
    """One stream.  step(boxes [n, 4] xyxy float32, labels [n], scores [n] float32, query [n] or None) ->
    (boxes, labels, scores, query, ids, hits, status) of the emitted detections."""

    def __init__(self, **kw):
        unknown = set(kw) - set(DEFAULTS)
        assert not unknown, unknown
        self.p = dict(DEFAULTS, **kw)
        if self.p["new_threshold"] is None:
            self.p["new_threshold"] = self.p["track_threshold"]
        self.s = fresh_state()

    def state_dict(self):
        return {k: np.array(v, copy=True) for k, v in self.s.items()}

    def load_state_dict(self, state):
        self.s = {k: np.array(state[k], copy=True) for k in KEYS}
        self.s["frame"], self.s["next_id"] = np.int32(self.s["frame"]), np.int32(self.s["next_id"])

    def _walk(self, slots, dets, pred_corners, boxes, labels, thr, slot_det, det_slot):
        s, p = self.s, self.p
        pairs = []
        for t in slots:
            for d in dets:
                if not p["class_agnostic"] and int(labels[d]) != int(s["label"][t]):
                    continue
                m = iou(pred_corners[t], boxes[d])
                if m > thr:                                         # strict; NaN is no pair
                    pairs.append((-m, int(s["id"][t]), d, t))
        for _, _, d, t in sorted(pairs):
            if t not in slot_det and d not in det_slot:
                slot_det[t], det_slot[d] = d, t

    def step(self, boxes, labels, scores, query=None):
        s, p = self.s, self.p
        boxes = np.asarray(boxes, F).reshape(-1, 4)
        labels = np.asarray(labels, np.int64).reshape(-1)
        scores = np.asarray(scores, F).reshape(-1)
        n = len(boxes)
        query = np.zeros(n, np.int32) if query is None else np.asarray(query, np.int32).reshape(-1)
        alpha, beta, half, zero = F(p["alpha"]), F(p["beta"]), F(0.5), F(0)
        thr_t, thr_n = F(p["track_threshold"]), F(p["new_threshold"])
        live = [t for t in range(TRACK_MAX) if s["id"][t] >= 1]
        with np.errstate(all="ignore"):
            # 1. predict
            pred, corners = {}, {}
            for t in live:
                q = s["x"][t] + s["v"][t]
                q[2] = zero if q[2] < zero else q[2]
                q[3] = zero if q[3] < zero else q[3]
                pred[t] = q
                corners[t] = (q[0] - q[2] * half, q[1] - q[3] * half, q[0] + q[2] * half, q[1] + q[3] * half)
            # 2. detections
            z = [to_z(b) for b in boxes]
            high = [bool(scores[d] >= thr_t) for d in range(n)]
            # 3, 4. the two stages
            slot_det, det_slot = {}, {}
            self._walk(live, [d for d in range(n) if high[d]], corners, boxes, labels, p["match_threshold"], slot_det, det_slot)
            second = [t for t in live if t not in slot_det and s["confirmed"][t] and s["miss"][t] == 0]
            self._walk(second, [d for d in range(n) if not high[d]], corners, boxes, labels, p["low_match_threshold"], slot_det, det_slot)
            # 5, 6. update or coast
            for t in live:
                if t in slot_det:
                    d = slot_det[t]
                    r = z[d] - pred[t]
                    s["x"][t] = pred[t] + alpha * r
                    s["v"][t] = s["v"][t] + beta * r
                    s["hits"][t] += 1
                    s["miss"][t] = 0
                    s["score"][t] = scores[d]
                    s["confirmed"][t] = bool(s["confirmed"][t]) or int(s["hits"][t]) >= p["min_hits"]
                else:
                    s["x"][t] = pred[t]
                    s["miss"][t] += 1
                    if not s["confirmed"][t] or int(s["miss"][t]) > p["max_age"]:
                        for k in ("x", "v", "label", "id", "hits", "miss", "confirmed", "score"):
                            s[k][t] = 0
            # 7. spawn
            status = 0
            for d in range(n):
                if d in det_slot or not high[d] or not scores[d] >= thr_n:
                    continue
                free = [t for t in range(TRACK_MAX) if s["id"][t] == 0]
                if not free:
                    status |= FULL
                    continue
                t = free[0]
                s["id"][t] = s["next_id"]
                s["next_id"] = np.int32(s["next_id"] + 1)
                s["x"][t], s["v"][t] = z[d], 0
                s["label"][t], s["score"][t] = labels[d], scores[d]
                s["hits"][t], s["miss"][t], s["confirmed"][t] = 1, 0, p["min_hits"] <= 1
                det_slot[d] = t
        # 8. emit
        out = [d for d in range(n) if d in det_slot and s["confirmed"][det_slot[d]]]
        s["frame"] = np.int32(s["frame"] + 1)
        return (boxes[out], labels[out], scores[out], query[out], np.array([s["id"][det_slot[d]] for d in out], np.int32),
                np.array([s["hits"][det_slot[d]] for d in out], np.int32), status)


def stack_states(trackers):
    """The state_dict of a Tracker with one stream per reference tracker."""
    states = [t.state_dict() for t in trackers]
    return {k: np.stack([np.asarray(st[k]) for st in states]) for k in KEYS}
