"""Reference of the configurable set criterion (tests/test_criterion_cpu.py proves its cases admissible, tests/test_gpu_criterion.py
runs them on csrc/setloss.hip): the softmax criterion with run-time matcher cost weights, loss coefficients, weight of unmatched
queries, per-class weights of the matched targets and the optional clamp of the box count, in torch on the CPU and in the dtype of
its inputs, so that autograd gives the gradients.  It is put together from the pieces of oracle/set_loss_ref.py the way
setloss_cases.oracle_losses is; at the default weights it gives that function's numbers."""
import os
import sys
import zlib
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import setloss_cases as SC                 # noqa: E402

QUANTUM = 1.0 / 64.0                       # class weights are multiples of this in [0, 16]

Weights = namedtuple("Weights", "cost_class cost_bbox cost_giou class_coef bbox_coef giou_coef eos min_one class_weights")
DEFAULTS = Weights(1.0, 5.0, 2.0, 1.0, 5.0, 2.0, 0.1, False, None)
CONFIG_NAMES = ("set_cost_class", "set_cost_bbox", "set_cost_giou", "class_loss_coef", "bbox_loss_coef", "giou_loss_coef", "eos_coef",
                "num_boxes_min_one", "class_weights")      # the TrainingConfig attribute behind each field of Weights

WEIGHT_SETS = ("A", "B", "C", "Z")


def draw_class_weights(C, tag="C"):
    """C class weights, multiples of 1/64 drawn uniformly from [0.25, 4]."""
    rng = np.random.default_rng(zlib.crc32(f"class-weights-{tag}-{C}".encode()))
    return tuple((rng.integers(16, 257, size=C) * QUANTUM).tolist())


def weight_set(name, C):
    """A: the defaults (run through the run-time path); B: other cost / loss weights and eos; C: B + class weights + clamped box
    count; Z: no class term in the cost, no GIoU term in the loss."""
    if name == "A":
        return DEFAULTS
    b = DEFAULTS._replace(cost_class=2.0, cost_bbox=3.0, cost_giou=1.5, class_coef=1.5, bbox_coef=4.0, giou_coef=0.75, eos=0.25)
    if name == "B":
        return b
    if name == "C":
        return b._replace(min_one=True, class_weights=draw_class_weights(C))
    assert name == "Z"
    return DEFAULTS._replace(cost_class=0.0, giou_coef=0.0)


def config_of(w, **extra):
    """A config object (attributes only) that asks for these weights."""
    from types import SimpleNamespace
    return SimpleNamespace(**dict(zip(CONFIG_NAMES, w)), **extra)


def host_block(w):
    """The DETR_CRITERION_FLOATS floats of the _crit_ entry points."""
    import ctypes
    return (ctypes.c_float * 8)(*[float(v) for v in w[:8]])


CONTIGUOUS = [c for c in SC.LOSS_CASES if c[-1] == "contiguous"]
STRIDED_FOR_C = next(c for c in SC.LOSS_CASES if c[-1] == "strided" and c[4] == 65)        # Lv 3, Q 17, C 65: two lane strides of classes
# (weight set, case name) -> seed of setloss_cases.loss_inputs, where seed 0 leaves the float32 and the float64 reference with
# different matchings (tests/test_criterion_cpu.py: test_matching_is_precision_independent)
SEEDS = {}
PAIRS = [(ws, case) for ws in WEIGHT_SETS for case in CONTIGUOUS] + [("C", STRIDED_FOR_C)]
PAIR_IDS = [f"{ws}-{case[0]}" for ws, case in PAIRS]

# d_logits: where the float32 reference itself misses the float64 one by more than the relative bound of the GPU test (2e-5 of the
# largest entry), 4x its measured error is the case's absolute bound, as setloss_cases.D_LOGITS_ATOL.  Keys: (weight set, case
# name without the layout).  Measured by tests/test_criterion_cpu.py::test_recorded_float32_reference_errors, loss_scale 0.5.
# Q = 1 with its one query matched to a +8 logit (setloss_cases.D_LOGITS_F32_ORACLE_ERR explains the cancellation); B and C scale
# the label term by class_loss_coef = 1.5 (C's class weight cancels against the normaliser of the single matched query).
D_LOGITS_F32_REF_ERR = {("A", "Lv1-B1-Q1-C2-bg1-R2"): 3.238e-8, ("B", "Lv1-B1-Q1-C2-bg1-R2"): 4.856e-8,
                        ("C", "Lv1-B1-Q1-C2-bg1-R2"): 4.856e-8, ("Z", "Lv1-B1-Q1-C2-bg1-R2"): 3.238e-8}
D_LOGITS_ATOL = {k: 4 * v for k, v in D_LOGITS_F32_REF_ERR.items()}


# the problem of the get_losses tests (that of tests/test_gpu_setloss_edges.py) and the weights they put into the config
API_CASE = ("api", 2, 2, 9, 5, 0, 6, [5, 2], "contiguous")


def api_weights():
    C = API_CASE[4]
    return [DEFAULTS, DEFAULTS._replace(eos=0.25), weight_set("C", C), weight_set("C", C)._replace(class_weights=draw_class_weights(C, "other"))]


def inputs(ws, case):
    return SC.loss_inputs(case, seed=SEEDS.get((ws, case[0]), 0))


def cost_matrix(tb, tc, p_bbox, p_class, w):
    """oracle cost_matrix with the weights of `w`, operands in its order; a label outside [0, C) has class probability 0."""
    import torch
    from oracle import set_loss_ref as L
    C = p_class.shape[-1]
    valid = (tc >= 0) & (tc < C)
    p_xy = L.xcycwh_to_xy_min_xy_max(p_bbox)
    t_xy = L.xcycwh_to_xy_min_xy_max(tb)
    softmax = torch.softmax(p_class, dim=-1)
    cost_class = -softmax[:, torch.where(valid, tc, torch.zeros_like(tc)).long()]
    if not bool(valid.all()):
        cost_class = cost_class * valid.to(softmax.dtype)[None, :]
    cost_bbox = (p_bbox[:, None, :] - tb[None, :, :]).abs().sum(-1)
    cost_giou = -L.giou_matrix(p_xy, t_xy)
    return w.cost_bbox * cost_bbox + w.cost_class * cost_class + w.cost_giou * cost_giou


def match_from_cost(cost_fn, t_bbox, t_class, Lv, B, Q):
    """setloss_cases.oracle_match with the cost of problem (level, image) supplied by cost_fn(lv, b, tb, tc) -> numpy [Q, n]."""
    import torch
    from oracle import set_loss_ref as L
    out = []
    for lv in range(Lv):
        tbs, tcs, tis, pis, sels = [], [], [], [], []
        t_off = 0
        for b in range(B):
            tb, tc = L.strip_header(t_bbox[b], t_class[b])
            rows, cols, sel = L.lsap(cost_fn(lv, b, tb, tc))
            tis.append(torch.from_numpy(cols) + t_off)
            pis.append(torch.from_numpy(rows) + b * Q)
            sels.append(torch.from_numpy(sel))
            tbs.append(tb)
            tcs.append(tc)
            t_off += tb.shape[0]
        out.append((torch.cat(tbs), torch.cat(tcs), torch.cat(tis), torch.cat(pis), torch.cat(sels)))
    return out


def criterion_match(logits, boxes, t_bbox, t_class, w):
    Lv, B, Q, _ = logits.shape
    return match_from_cost(lambda lv, b, tb, tc: cost_matrix(tb, tc, boxes[lv, b], logits[lv, b], w).detach().numpy(),
                           t_bbox, t_class, Lv, B, Q)


def loss_labels(p_class, t_class, t_indices, p_indices, p_selector, bg, w):
    """oracle loss_labels with weight eos on the unmatched queries and class_weights[class] (1 without) on the matched ones."""
    import torch
    from oracle import set_loss_ref as L
    _, true_neg, true_pos, pos_accuracy = L.loss_labels(p_class, t_class, t_indices, p_indices, p_selector, bg)
    neg_p = p_class[~p_selector]
    neg_t = torch.full((neg_p.shape[0],), bg, dtype=torch.int64)
    pos_p = p_class[p_indices]
    pos_t = t_class[t_indices].long()
    if w.class_weights is None:
        pos_w = torch.full((t_indices.shape[0],), 1.0, dtype=p_class.dtype)
    else:
        pos_w = torch.tensor(w.class_weights, dtype=p_class.dtype)[pos_t]
    weights = torch.cat([torch.full((neg_p.shape[0],), w.eos, dtype=p_class.dtype), pos_w])
    targets = torch.cat([neg_t, pos_t])
    preds = torch.cat([neg_p, pos_p])
    ce = torch.logsumexp(preds, -1) - preds.gather(1, targets[:, None])[:, 0]
    return (ce * weights).sum() / weights.sum(), true_neg, true_pos, pos_accuracy


def loss_boxes(p_bbox, t_bbox, t_indices, p_indices, w):
    """oracle loss_boxes with the divisor max(n, 1) under min_one."""
    import torch
    from oracle import set_loss_ref as L
    pb = p_bbox[p_indices]
    tb = t_bbox[t_indices]
    n = max(pb.shape[0], 1) if w.min_one else pb.shape[0]
    p_xy = L.xcycwh_to_xy_min_xy_max(pb)
    t_xy = L.xcycwh_to_xy_min_xy_max(tb)
    l1 = (pb - tb).abs().sum() / n
    giou = torch.diagonal(L.giou_matrix(p_xy, t_xy))
    return (1 - giou).sum() / n, l1


def criterion_losses(logits, boxes, t_bbox, t_class, bg, w=DEFAULTS, match=None):
    """(total, {name + suffix: unweighted value}, match) of levels [aux 0 .. aux Lv-2, main]; the total adds class_coef * label_cost +
    giou_coef * giou_loss + bbox_coef * l1_loss level by level, main level first."""
    Lv, B, Q, C = logits.shape
    match = criterion_match(logits, boxes, t_bbox, t_class, w) if match is None else match
    losses = {}
    total = 0
    for lv in [Lv - 1] + list(range(Lv - 1)):
        suffix = "" if lv == Lv - 1 else f"_{lv}"
        tb, tc, ti, pi, sel = match[lv]
        vals = loss_labels(logits[lv].reshape(-1, C), tc, ti, pi, sel, bg, w) + loss_boxes(boxes[lv].reshape(-1, 4), tb, ti, pi, w)
        for name, v in zip(SC.LOSS_NAMES, vals):
            losses[name + suffix] = v
        total = total + vals[0] * w.class_coef
        total = total + vals[4] * w.giou_coef
        total = total + vals[5] * w.bbox_coef
    return total, losses, match
