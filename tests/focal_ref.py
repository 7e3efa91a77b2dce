"""Reference of the sigmoid focal class criterion (tests/test_focal_cpu.py checks it and measures its float32 error, tests/test_gpu_focal.py
runs its cases on csrc/setloss.hip, csrc/postprocess.hip and csrc/detect.hip): the focal class term, the matcher's focal class cost and
the logged metrics, in torch on the CPU and in the dtype of its inputs, so that autograd gives the gradients.  It is put together from
tests/criterion_ref.py (match_from_cost, loss_boxes, the cases) and tests/setloss_cases.py the way criterion_ref is put together from the
oracle.  `scores_labels` is the float64 NumPy statement of scoring="sigmoid".

Semantics (include/detr_hip.h states them for the kernels): with sp(z) = max(z, 0) + log1p(exp(-|z|)) an element of the class loss is
    t = 1:  alpha * exp(-gamma * sp(x)) * sp(-x)        t = 0:  (1 - alpha) * exp(-gamma * sp(-x)) * sp(x)
a matched query is one-hot on its target's class, an unmatched one all zero; label_cost = sum of all elements / max(matched, 1);
class cost of the matcher = element(t = 1) - element(t = 0) at the target's class, 0 for a label outside [0, C)."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criterion_ref as CR                 # noqa: E402
import setloss_cases as SC                 # noqa: E402

Focal = namedtuple("Focal", "alpha gamma")
FOCAL_DEFAULTS = Focal(0.25, 2.0)

PARAM_SETS = ("F0", "F1", "F2", "Z")


def param_set(name):
    """(Weights, Focal).  F0: the defaults with set_cost_class 2 (the published matcher weight); F1: gamma 0, alpha 0.5 (half of the
    binary cross-entropy); F2: gamma 1.5, alpha 0.75, other cost / loss coefficients and the clamped box count; Z: no class term in
    the cost.  eos and class_weights of Weights are not read."""
    if name == "F0":
        return CR.DEFAULTS._replace(cost_class=2.0), FOCAL_DEFAULTS
    if name == "F1":
        return CR.DEFAULTS, Focal(0.5, 0.0)
    if name == "F2":
        return (CR.DEFAULTS._replace(cost_class=2.0, cost_bbox=3.0, cost_giou=1.5, class_coef=1.5, bbox_coef=4.0, giou_coef=0.75, min_one=True),
                Focal(0.75, 1.5))
    assert name == "Z"
    return CR.DEFAULTS._replace(cost_class=0.0), FOCAL_DEFAULTS


def config_of(w, f, **extra):
    """A config object (attributes only) that asks for the focal criterion with these values."""
    return CR.config_of(w, class_criterion="focal", focal_alpha=f.alpha, focal_gamma=f.gamma, **extra)


def focal_block(f):
    """The DETR_FOCAL_FLOATS floats of the _focal_ entry points."""
    import ctypes
    return (ctypes.c_float * 2)(float(f.alpha), float(f.gamma))


CASES = list(CR.CONTIGUOUS) + [CR.STRIDED_FOR_C]
PAIRS = [(ps, case) for ps in PARAM_SETS for case in CASES]
PAIR_IDS = [f"{ps}-{case[0]}" for ps, case in PAIRS]


def inputs(case):
    return SC.loss_inputs(case)


# Where the float32 reference itself misses the float64 one by more than the bound of the GPU test, 4x its measured error is that
# pair's absolute bound (the rule of setloss_cases.D_LOGITS_ATOL and criterion_ref.D_LOGITS_ATOL; never derived from the
# kernel's output).  Keys: (parameter set, case name without the layout).  Measured, and measured again, by
# tests/test_focal_cpu.py::test_recorded_float32_reference_errors: the cost against 2e-6 * max(1, cost weights), d_logits (loss_scale
# 0.5) against 2e-5 of the largest float64 entry, d_boxes against 5e-5 of it.  As measured, no pair needs an entry: the float32
# reference stays within every bound (the cost by a factor 3, the gradients by a factor 20 and more).
COST_F32_REF_ERR = {}
D_LOGITS_F32_REF_ERR = {}
D_BOXES_F32_REF_ERR = {}


def _atol(table, key):
    return 4 * table[key] if key in table else None


def cost_atol(key):
    return _atol(COST_F32_REF_ERR, key)


def d_logits_atol(key):
    return _atol(D_LOGITS_F32_REF_ERR, key)


def d_boxes_atol(key):
    return _atol(D_BOXES_F32_REF_ERR, key)


# ------------------------------------------------------------------------------------------
# the class term
# ------------------------------------------------------------------------------------------
def softplus(z):
    """max(z, 0) + log1p(exp(-|z|)): finite for every finite z."""
    import torch
    return torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))


def element_pos(x, f):
    import torch
    return f.alpha * torch.exp(-f.gamma * softplus(x)) * softplus(-x)


def element_neg(x, f):
    import torch
    return (1 - f.alpha) * torch.exp(-f.gamma * softplus(-x)) * softplus(x)


def elements(x, t, f):
    """The loss elements of logits x under the 0 / 1 targets t (same shape)."""
    import torch
    return torch.where(t > 0, element_pos(x, f), element_neg(x, f))


def elements_textbook(x, t, f):
    """sigmoid_focal_loss as published: alpha_t * (1 - p_t)^gamma * BCE.  Not finite where p or 1 - p rounds to 0."""
    import torch
    p = torch.sigmoid(x)
    ce = -(t * torch.log(p) + (1 - t) * torch.log(1 - p))
    p_t = p * t + (1 - p) * (1 - t)
    return (f.alpha * t + (1 - f.alpha) * (1 - t)) * (1 - p_t) ** f.gamma * ce


def d_elements(x, t, f):
    """Closed form of d elements / dx (what the gradient kernel evaluates): with p = exp(-sp(-x)), 1 - p = exp(-sp(x)),
    t = 1: -alpha * exp(-gamma * sp(x)) * (gamma * p * sp(-x) + 1 - p);  t = 0: (1 - alpha) * exp(-gamma * sp(-x)) * (gamma * (1 - p) * sp(x) + p)."""
    import torch
    sx, snx = softplus(x), softplus(-x)
    p, q = torch.exp(-snx), torch.exp(-sx)
    pos = -f.alpha * torch.exp(-f.gamma * sx) * (f.gamma * p * snx + q)
    neg = (1 - f.alpha) * torch.exp(-f.gamma * snx) * (f.gamma * q * sx + p)
    return torch.where(t > 0, pos, neg)


def class_cost(x, f):
    return element_pos(x, f) - element_neg(x, f)


# ------------------------------------------------------------------------------------------
# matcher cost, metrics, losses
# ------------------------------------------------------------------------------------------
def cost_matrix(tb, tc, p_bbox, p_class, w, f):
    """criterion_ref.cost_matrix with the focal class cost; a label outside [0, C) costs 0 in the class term."""
    import torch
    from oracle import set_loss_ref as L
    C = p_class.shape[-1]
    valid = (tc >= 0) & (tc < C)
    p_xy = L.xcycwh_to_xy_min_xy_max(p_bbox)
    t_xy = L.xcycwh_to_xy_min_xy_max(tb)
    cost_class = class_cost(p_class[:, torch.where(valid, tc, torch.zeros_like(tc)).long()], f)
    if not bool(valid.all()):
        cost_class = cost_class * valid.to(p_class.dtype)[None, :]
    cost_bbox = (p_bbox[:, None, :] - tb[None, :, :]).abs().sum(-1)
    cost_giou = -L.giou_matrix(p_xy, t_xy)
    return w.cost_bbox * cost_bbox + w.cost_class * cost_class + w.cost_giou * cost_giou


def focal_match(logits, boxes, t_bbox, t_class, w, f):
    Lv, B, Q, _ = logits.shape
    return CR.match_from_cost(lambda lv, b, tb, tc: cost_matrix(tb, tc, boxes[lv, b], logits[lv, b], w, f).detach().numpy(),
                              t_bbox, t_class, Lv, B, Q)


def predicted_class(p_class, bg):
    """Per row: the background class when the largest non-background logit is <= 0 (or there is none), else the first arg-max over
    c != bg.  A NaN logit never wins a comparison."""
    import torch
    x = p_class.detach().clone()
    x[:, bg] = float("-inf")
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    mx, am = x.max(-1) if x.shape[0] else (x.new_zeros(0), torch.zeros(0, dtype=torch.int64))
    first = (x == mx[:, None]).to(torch.int64).argmax(-1) if x.shape[0] else am           # first occurrence, whatever max() returns
    return torch.where(mx > 0, first, torch.full_like(first, bg))


def loss_labels(p_class, t_class, t_indices, p_indices, p_selector, bg, f, nan_invalid=True):
    """(label_cost, true_neg, true_pos, pos_accuracy) of one level over the flattened batch [B * Q, C].  A matched label outside
    [0, C) leaves its row without a positive class (it still counts as matched) and turns label_cost NaN; nan_invalid=False keeps
    the finite value, whose gradient is the one the kernel writes."""
    import torch
    C = p_class.shape[-1]
    pos_t = t_class[t_indices].long()
    onehot = torch.zeros_like(p_class)
    ok = (pos_t >= 0) & (pos_t < C)
    onehot[p_indices[ok], pos_t[ok]] = 1
    label = elements(p_class, onehot, f).sum() / max(int(t_indices.shape[0]), 1)
    if nan_invalid and not bool(ok.all()):
        label = label * float("nan")                                 # an invalid matched label: NaN, as the softmax criterion
    pred = predicted_class(p_class, bg)
    neg, pos = pred[~p_selector], pred[p_indices]
    dt = p_class.dtype
    true_neg = (neg == bg).to(dt).mean()
    true_pos = (pos != bg).to(dt).mean()
    pos_accuracy = (pos == pos_t).to(dt).mean()
    return label, true_neg, true_pos, pos_accuracy


def focal_losses(logits, boxes, t_bbox, t_class, bg, w, f, match=None, nan_invalid=True):
    """criterion_ref.criterion_losses with the focal class term: (total, {name + suffix: unweighted value}, match)."""
    Lv, B, Q, C = logits.shape
    match = focal_match(logits, boxes, t_bbox, t_class, w, f) if match is None else match
    losses = {}
    total = 0
    for lv in [Lv - 1] + list(range(Lv - 1)):
        suffix = "" if lv == Lv - 1 else f"_{lv}"
        tb, tc, ti, pi, sel = match[lv]
        vals = loss_labels(logits[lv].reshape(-1, C), tc, ti, pi, sel, bg, f, nan_invalid) + CR.loss_boxes(boxes[lv].reshape(-1, 4), tb, ti, pi, w)
        for name, v in zip(SC.LOSS_NAMES, vals):
            losses[name + suffix] = v
        total = total + vals[0] * w.class_coef
        total = total + vals[4] * w.giou_coef
        total = total + vals[5] * w.bbox_coef
    return total, losses, match


# ------------------------------------------------------------------------------------------
# scoring
# ------------------------------------------------------------------------------------------
def scores_labels(logits, bg):
    """scoring="sigmoid" in float64 NumPy: logits [..., C] -> (scores [...], labels [...] int64).  label = first arg-max over c != bg,
    score = sigmoid of that logit; a NaN among the non-background logits makes the score NaN and is skipped by the arg-max (all NaN, or
    all -inf: the first non-background class)."""
    x = np.asarray(logits, np.float64).copy()
    C = x.shape[-1]
    assert C >= 2 and 0 <= bg < C
    keep = np.arange(C) != bg
    sub = x[..., keep]
    nan = np.isnan(sub).any(-1)
    sub = np.where(np.isnan(sub), -np.inf, sub)
    arg = sub.argmax(-1)                                             # first occurrence
    labels = np.arange(C)[keep][arg]
    best = np.take_along_axis(sub, arg[..., None], -1)[..., 0]
    with np.errstate(over="ignore"):
        scores = 1.0 / (1.0 + np.exp(-best))
    return np.where(nan, np.nan, scores), labels.astype(np.int64)
