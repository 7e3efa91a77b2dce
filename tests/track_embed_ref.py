"""Tracking by appearance (csrc/track_embed.hip, csrc/track_core.h) restated in plain NumPy on top of tests/track_ref.py, from its
specification (include/detr_hip.h: detr_track_embed_desc).  A test helper, not product code: sequential and slow on purpose.

What track_ref says about roundings holds here too.  dot64 is written as the header writes it: 64 lane partials, then
p = p + p[lane ^ o]; the blend m and the similarities are Python floats (fp64), the bank update float32 arrays (one rounding per
NumPy operation).  The tracker also keeps what the scenario generators need to know about a run: `gaps` and `n_reid`."""
import numpy as np

import track_ref as R

F = np.float32
TRACK_MAX = R.TRACK_MAX
FULL, BAD_COUNT, BAD_EMBED = R.FULL, R.BAD_COUNT, 4
KEYS = R.KEYS + ("embed",)
EMBED_DEFAULTS = dict(appearance_weight=0.5, reid_threshold=0.8, momentum=0.9)
_LANES = np.arange(64)


def dot64(a, b):
    a, b = np.asarray(a, F).astype(np.float64), np.asarray(b, F).astype(np.float64)
    p = np.zeros(64, np.float64)
    with np.errstate(all="ignore"):
        for j in range(0, len(a), 64):
            k = min(64, len(a) - j)
            p[:k] = p[:k] + a[j:j + k] * b[j:j + k]
        for o in (32, 16, 8, 4, 2, 1):
            p = p + p[_LANES ^ o]
    return float(p[0])


def unit(f):
    """-> (the unit embedding of the raw row f, float32; is f non-finite)"""
    f = np.asarray(f, F)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(np.float64(dot64(f, f)))
        if not np.isfinite(nrm):
            return np.zeros(len(f), F), True
        if not nrm > 0.0:
            return np.zeros(len(f), F), False
        return (f.astype(np.float64) / nrm).astype(F), False


class RefEmbedTracker(R.RefTracker):
    """One stream.  step(boxes, labels, scores, query or None, embeddings [R, E]) -> RefTracker.step's tuple."""

    def __init__(self, embed_dim, appearance_weight=0.5, reid_threshold=0.8, momentum=0.9, **kw):
        super().__init__(**kw)
        self.E, self.w, self.thr_reid, self.momentum = int(embed_dim), float(appearance_weight), reid_threshold, F(momentum)
        self.bank = np.zeros((TRACK_MAX, self.E), F)
        self.gaps = []          # distances that decide something and hang on a similarity: between two competing pairs, or to reid_threshold
        self.n_reid = 0         # tracks found again by appearance so far

    def state_dict(self):
        return dict(super().state_dict(), embed=self.bank.copy())

    def load_state_dict(self, state):
        super().load_state_dict(state)
        self.bank = np.array(state["embed"], F, copy=True)

    def _walk_pairs(self, pairs, slot_det, det_slot):
        """pairs: (m, id, detection, slot); walked by descending m, lower id, lower detection.  A NaN m is no pair."""
        pairs = [q for q in pairs if q[0] == q[0]]
        for i, a in enumerate(pairs):
            self.gaps += [abs(a[0] - b[0]) for b in pairs[i + 1:] if (a[2] == b[2]) != (a[3] == b[3])]     # they compete for a slot or a detection
        for m, _, d, t in sorted(pairs, key=lambda q: (-q[0], q[1], q[2])):
            if t not in slot_det and d not in det_slot:
                slot_det[t], det_slot[d] = d, t

    def step(self, boxes, labels, scores, query=None, embeddings=None):
        s, p = self.s, self.p
        boxes = np.asarray(boxes, F).reshape(-1, 4)
        labels = np.asarray(labels, np.int64).reshape(-1)
        scores = np.asarray(scores, F).reshape(-1)
        n = len(boxes)
        rows = np.arange(n) if query is None else np.asarray(query, np.int32).reshape(-1)
        query = np.zeros(n, np.int32) if query is None else np.asarray(query, np.int32).reshape(-1)
        embeddings = np.asarray(embeddings, F).reshape(-1, self.E)
        alpha, beta, half, zero = F(p["alpha"]), F(p["beta"]), F(0.5), F(0)
        thr_t, thr_n = F(p["track_threshold"]), F(p["new_threshold"])
        live = [t for t in range(TRACK_MAX) if s["id"][t] >= 1]
        status = 0
        units = []
        for d in range(n):
            if not 0 <= int(rows[d]) < len(embeddings):
                status |= BAD_EMBED
                units.append(np.zeros(self.E, F))
                continue
            u, bad = unit(embeddings[int(rows[d])])
            status |= BAD_EMBED if bad else 0
            units.append(u)
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
            z = [R.to_z(b) for b in boxes]
            high = [bool(scores[d] >= thr_t) for d in range(n)]
            same = lambda t, d: p["class_agnostic"] or int(labels[d]) == int(s["label"][t])       # noqa: E731
            # 3. stage 1: the IoU gate, walked by the blend
            slot_det, det_slot = {}, {}
            pairs, w = [], self.w
            for t in live:
                for d in range(n):
                    if not high[d] or not same(t, d):
                        continue
                    i = R.iou(corners[t], boxes[d])
                    if i > p["match_threshold"]:
                        pairs.append((i if w == 0.0 else (1.0 - w) * i + w * dot64(self.bank[t], units[d]), int(s["id"][t]), d, t))
            n_gaps = len(self.gaps)
            self._walk_pairs(pairs, slot_det, det_slot)
            if w == 0.0:
                del self.gaps[n_gaps:]               # IoU alone: the same bits on both sides, nothing hangs on a similarity
            first = dict(slot_det)
            # 4. stage 2, unchanged
            second = [t for t in live if t not in slot_det and s["confirmed"][t] and s["miss"][t] == 0]
            self._walk(second, [d for d in range(n) if not high[d]], corners, boxes, labels, p["low_match_threshold"], slot_det, det_slot)
            # 4b. re-identification
            found = {}
            if self.thr_reid is not None:
                pairs = []
                for t in live:
                    if t in slot_det or not s["confirmed"][t] or s["miss"][t] < 1:
                        continue
                    for d in range(n):
                        if d in det_slot or not high[d] or not scores[d] >= thr_n or not same(t, d):
                            continue
                        sim = dot64(self.bank[t], units[d])
                        self.gaps.append(abs(sim - float(self.thr_reid)))
                        if sim > float(self.thr_reid):
                            pairs.append((sim, int(s["id"][t]), d, t))
                self._walk_pairs(pairs, found, det_slot)
                self.n_reid += len(found)
            # 5, 6. update, restart or coast
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
                elif t in found:
                    d = found[t]
                    s["x"][t], s["v"][t] = z[d], 0
                    s["hits"][t] += 1
                    s["miss"][t] = 0
                    s["score"][t] = scores[d]
                else:
                    s["x"][t] = pred[t]
                    s["miss"][t] += 1
                    if not s["confirmed"][t] or int(s["miss"][t]) > p["max_age"]:
                        for k in ("x", "v", "label", "id", "hits", "miss", "confirmed", "score"):
                            s[k][t] = 0
                        self.bank[t] = 0
            # the bank of the slots matched by appearance
            for t, d in list(first.items()) + list(found.items()):
                u = self.momentum * self.bank[t] + (F(1) - self.momentum) * units[d]
                nu = np.sqrt(np.float64(dot64(u, u)))
                self.bank[t] = (u.astype(np.float64) / nu).astype(F) if nu > 0.0 and np.isfinite(nu) else 0
            # 7. spawn
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
                self.bank[t] = units[d]
                det_slot[d] = t
        # 8. emit
        out = [d for d in range(n) if d in det_slot and s["confirmed"][det_slot[d]]]
        s["frame"] = np.int32(s["frame"] + 1)
        return (boxes[out], labels[out], scores[out], query[out], np.array([s["id"][det_slot[d]] for d in out], np.int32),
                np.array([s["hits"][det_slot[d]] for d in out], np.int32), status)


def stack_states(trackers):
    """The state_dict of a Tracker(embed_dim=E) with one stream per reference tracker."""
    states = [t.state_dict() for t in trackers]
    return {k: np.stack([np.asarray(st[k]) for st in states]) for k in KEYS}
