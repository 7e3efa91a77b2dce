"""DETR set loss on the device (drop-in for detr_tf/loss/loss.py:6-179).

`get_losses(m_outputs, t_bbox, t_class, config)` keeps the reference signature (plus one optional argument, `before_assign`: a
callable run once between the matcher's cost and assignment launches) and returns
`(total_loss, log_dict)` with the same 36 keys (label_cost, true_neg, true_pos, pos_accuracy,
giou_loss, l1_loss, + suffixes _0.._4) and the 1/2/5 weighting of `get_total_losss`.
The criterion -- matcher cost weights, loss coefficients, the weight of unmatched queries, per-class weights, the clamp of
the box count, and the class term itself (softmax cross-entropy or sigmoid focal loss) -- is read from the config at every call
(`criterion_of`) into a `Criterion`, a plain twelve-field record; `Criterion.entry(kind)` is the one place that maps it to an entry
point and its argument blocks: at the reference's values the four entry points that have them compiled in, otherwise the `_crit_`
ones (the same kernel bodies on run-time values), and with class_criterion = "focal" the `_focal_` ones (the same kernel bodies
with the focal class-term policy; include/detr_hip.h states its semantics).
All arithmetic runs in csrc/setloss.hip: cost matrix (K12), exact assignment (K13), loss sums /
finalisation / gradients (K14).  Under data parallelism the per-level normalisers (sum of CE
weights, number of matched boxes) are all-reduced between the "sums" and "finalize" kernels, so
a B x world step has the reference's single-device whole-batch semantics (loss.py:66-67,82,94).
"""
import math
from collections import namedtuple
from ctypes import byref, c_float

import torch

from .. import _hip as hip
from .hungarian_matching import Matcher, make_desc

LOSS_NAMES = ("label_cost", "true_neg", "true_pos", "pos_accuracy", "giou_loss", "l1_loss")


CRITERION_FIELDS = ("set_cost_class", "set_cost_bbox", "set_cost_giou", "class_loss_coef", "bbox_loss_coef", "giou_loss_coef",
                    "eos_coef", "num_boxes_min_one")                  # the order of DETR_CRITERION_FLOATS (include/detr_hip.h)
CRITERION_DEFAULTS = (1.0, 5.0, 2.0, 1.0, 5.0, 2.0, 0.1, False)       # the reference's literals (loss.py:6-19,60-67, hungarian_matching.py:163)
WEIGHT_QUANTUM, WEIGHT_MAX = 1.0 / 64.0, 16.0                         # class weights: multiples of 1/64 in [0, 16] ...
WEIGHT_MAX_TERMS = 16384                                              # ... and at most this many added: every partial sum < 2^24 quanta


CLASS_CRITERIA = ("softmax", "focal")
CLASS_TERM_FIELDS = ("class_criterion", "focal_alpha", "focal_gamma")
CLASS_TERM_DEFAULTS = ("softmax", 0.25, 2.0)                          # alpha, gamma: the published values (Lin et al.; Deformable DETR)
FOCAL_GAMMA_MAX = 8.0
ENTRY_LEAD = {"match_cost": 1, "set_loss_sums": 1, "set_loss_finalize": 2, "set_loss_grad": 1}    # arguments in front of the criterion's blocks
ENTRY_WEIGHTED = ("set_loss_sums", "set_loss_grad")                   # the kinds whose run-time entry point takes class weights


class Criterion(namedtuple("Criterion", CRITERION_FIELDS + ("class_weights",) + CLASS_TERM_FIELDS, defaults=CLASS_TERM_DEFAULTS)):
    """The set criterion as an immutable, hashable record of twelve fields: seven floats, a bool, the class weights as a tuple of
    multiples of 1/64 (or None), and the class term -- class_criterion ("softmax" or "focal"), focal_alpha and focal_gamma, which
    default to the reference's.  `criterion_of` builds one with normalised types."""
    __slots__ = ()

    @property
    def is_default(self):
        return tuple(self[:8]) == CRITERION_DEFAULTS and self.class_weights is None and not self.is_focal

    @property
    def is_focal(self):
        return self.class_criterion == "focal"

    def floats(self):
        """The host block of the _crit_ and _focal_ entry points."""
        return (c_float * hip.CRITERION_FLOATS)(*[float(v) for v in self[:8]])

    def focal_floats(self):
        """The second host block of the _focal_ entry points."""
        return (c_float * hip.FOCAL_FLOATS)(self.focal_alpha, self.focal_gamma)

    def entry(self, kind, class_weights=None):
        """The one place that maps a criterion to the entry point of a launch -- kind is "match_cost", "set_loss_sums",
        "set_loss_finalize" or "set_loss_grad" -- and to the argument blocks of its own that the call takes behind the leading
        ENTRY_LEAD[kind] arguments: none at the reference's values, floats() on the run-time criterion (then the device pointer
        class_weights, or None, where the kind reads class weights), floats() and focal_floats() under the focal class term."""
        if self.is_focal:
            return f"detr_hip_{kind}_focal_f32", (self.floats(), self.focal_floats())
        if self.is_default:
            return f"detr_hip_{kind}_f32", ()
        return f"detr_hip_{kind}_crit_f32", (self.floats(),) + ((class_weights,) if kind in ENTRY_WEIGHTED else ())

    def call(self, kind, *args, class_weights=None):
        """hip.call of the criterion's `kind` entry point on the kind's own arguments."""
        name, blocks = self.entry(kind, class_weights)
        lead = ENTRY_LEAD[kind]
        hip.call(name, *args[:lead], *blocks, *args[lead:])


def round_class_weights(weights, nb_class=None):
    """A sequence of class weights -> tuple of the nearest multiples of 1/64; ValueError outside [0, 16], on a non-finite
    entry or a length other than nb_class."""
    w = [float(v) for v in (weights.tolist() if hasattr(weights, "tolist") else weights)]
    if nb_class is not None and len(w) != int(nb_class):
        raise ValueError(f"class_weights has {len(w)} entries, the class head has {int(nb_class)}")
    for c, v in enumerate(w):
        if not math.isfinite(v) or v < 0.0 or v > WEIGHT_MAX:
            raise ValueError(f"class_weights[{c}] = {v}: expected a finite value in [0, {WEIGHT_MAX:g}]")
    return tuple(round(v / WEIGHT_QUANTUM) * WEIGHT_QUANTUM for v in w)


def criterion_of(config, nb_class=None):
    """The criterion a config asks for (attributes it lacks read as the defaults).  nb_class: the length class_weights must have,
    where the caller knows it."""
    vals = []
    for name, default in zip(CRITERION_FIELDS[:7], CRITERION_DEFAULTS[:7]):
        v = float(getattr(config, name, default))
        if not math.isfinite(v) or v < 0.0:
            raise ValueError(f"{name} = {v}: expected a finite value >= 0")
        vals.append(v)
    vals.append(bool(getattr(config, "num_boxes_min_one", False)))
    cw = getattr(config, "class_weights", None)
    kind = getattr(config, "class_criterion", "softmax")
    if kind not in CLASS_CRITERIA:
        raise ValueError(f"class_criterion = {kind!r}: expected one of {CLASS_CRITERIA}")
    alpha, gamma = float(getattr(config, "focal_alpha", CLASS_TERM_DEFAULTS[1])), float(getattr(config, "focal_gamma", CLASS_TERM_DEFAULTS[2]))
    if not (math.isfinite(alpha) and 0.0 < alpha < 1.0):
        raise ValueError(f"focal_alpha = {alpha}: expected a finite value inside (0, 1)")
    if not (math.isfinite(gamma) and 0.0 <= gamma <= FOCAL_GAMMA_MAX):
        raise ValueError(f"focal_gamma = {gamma}: expected a finite value in [0, {FOCAL_GAMMA_MAX:g}]")
    if kind == "focal" and cw is not None:
        raise ValueError("class_weights with class_criterion = 'focal': the focal class term has no per-class weights")
    return Criterion(*vals, None if cw is None else round_class_weights(cw, nb_class), str(kind), alpha, gamma)


DEFAULT_CRITERION = Criterion(*CRITERION_DEFAULTS, None)


def get_total_losss(losses, config=None):
    """loss.py:6-19: sum of 1*label_cost + 2*giou_loss + 5*l1_loss over every (suffixed) key; with a config, its
    class_loss_coef / giou_loss_coef / bbox_loss_coef instead."""
    weights = {"label_cost": 1, "giou_loss": 2, "l1_loss": 5}
    if config is not None:
        crit = criterion_of(config)
        weights = {"label_cost": crit.class_loss_coef, "giou_loss": crit.giou_loss_coef, "l1_loss": crit.bbox_loss_coef}
    total = 0
    for key, value in losses.items():
        hit = [w for n, w in weights.items() if n in key]
        if len(hit) == 1:
            total = total + value * hit[0]
    return total


class SetLoss:
    """Device state of the set loss for one (levels, B, Q, C, R) shape."""

    _cache = {}

    @classmethod
    def get(cls, levels, B, Q, C, R, device):
        key = (levels, B, Q, C, R, str(device))
        if key not in cls._cache:
            cls._cache[key] = cls(levels, B, Q, C, R, device)
        return cls._cache[key]

    def __init__(self, levels, B, Q, C, R, device):
        self.levels, self.B, self.Q, self.C, self.R = levels, B, Q, C, R
        self.matcher = Matcher(levels, B, Q, R, device)
        self.sums = torch.zeros(levels * 10, dtype=torch.float32, device=device)
        self.losses = torch.zeros(levels, 6, dtype=torch.float32, device=device)
        self.total = torch.zeros(1, dtype=torch.float32, device=device)
        self.d_logits = torch.zeros(levels, B, Q, C, dtype=torch.float32, device=device)
        self.d_boxes = torch.zeros(levels, B, Q, 4, dtype=torch.float32, device=device)
        self.desc = None
        self.reduce_sums = None          # hook: callable(tensor) doing the data-parallel all-reduce
        self.criterion = DEFAULT_CRITERION
        self._weights = (None, None)     # (tuple, device tensor) of the class weights last used

    def _class_weights(self, crit, world):
        """Device pointer of the criterion's class weights (None without): one tensor, rebuilt when the vector changes."""
        if crit.class_weights is None:
            return None
        if len(crit.class_weights) != self.C:
            raise ValueError(f"class_weights has {len(crit.class_weights)} entries, the class head has {self.C}")
        if world * self.B * (self.R - 1) > WEIGHT_MAX_TERMS:
            raise ValueError(f"class_weights: world * B * (R - 1) = {world * self.B * (self.R - 1)} matched targets could exceed "
                             f"{WEIGHT_MAX_TERMS}, past which the sum of their weights is no longer exact in float32")
        if self._weights[0] != crit.class_weights:
            self._weights = (crit.class_weights, torch.tensor(crit.class_weights, dtype=torch.float32, device=self.sums.device))
        return self._weights[1].data_ptr()

    def forward(self, logits, boxes, t_bbox, t_class, background_class, criterion=DEFAULT_CRITERION, world=1, before_assign=None):
        """criterion: a `Criterion` (criterion_of).  world: data-parallel ranks whose sums the reduce_sums hook adds up.
        before_assign: see Matcher.run."""
        wptr = self._class_weights(criterion, max(1, int(world)))
        self.criterion = criterion
        self.desc = make_desc(logits, boxes, t_bbox, t_class, background_class)
        self._keep = (logits, boxes, t_bbox, t_class)
        tfp = self.matcher.run(self.desc, t_bbox, criterion, before_assign)
        hip.zero_(self.sums)
        criterion.call("set_loss_sums", byref(self.desc), tfp.data_ptr(), self.sums.data_ptr(), class_weights=wptr)
        if self.reduce_sums is not None:
            self.reduce_sums(self.sums)
        self.finalize()
        return self.total, self.losses

    def finalize(self):
        """losses / total of self.sums under the criterion of the last forward."""
        self.criterion.call("set_loss_finalize", self.sums.data_ptr(), self.levels, self.losses.data_ptr(), self.total.data_ptr())

    def grad(self, loss_scale=1.0):
        """Gradients of loss_scale * total w.r.t. logits / boxes, laid out [Lv,B,Q,*] contiguous."""
        # the gradient tensors use the same (level, image, query) strides as contiguous [Lv,B,Q,*]
        assert self._keep[0].is_contiguous() and self._keep[1].is_contiguous(), "set-loss gradients need contiguous head outputs"
        wptr = None if self.criterion.class_weights is None else self._weights[1].data_ptr()
        self.criterion.call("set_loss_grad", byref(self.desc), self.matcher.tgt_for_pred.data_ptr(), self.sums.data_ptr(), c_float(loss_scale),
                            self.d_logits.data_ptr(), self.d_boxes.data_ptr(), class_weights=wptr)
        return self.d_logits, self.d_boxes


def _stack_levels(m_outputs):
    """[aux_0 .. aux_{n-1}, main] -> contiguous [Lv,B,Q,*] (main is the LAST level, detr.py:190-202)."""
    if hasattr(m_outputs, "levels_logits"):
        return m_outputs.levels_logits, m_outputs.levels_boxes
    aux = m_outputs.get("aux", [])
    lg = torch.stack([a["pred_logits"] for a in aux] + [m_outputs["pred_logits"]]).contiguous().float()
    bx = torch.stack([a["pred_boxes"] for a in aux] + [m_outputs["pred_boxes"]]).contiguous().float()
    return lg, bx


def _prep_targets(t_bbox, t_class, device):
    tb = torch.as_tensor(t_bbox).to(device=device, dtype=torch.float32).contiguous()
    tc = torch.as_tensor(t_class).to(device=device, dtype=torch.int64)
    tc = tc.reshape(tb.shape[0], tb.shape[1]).contiguous()
    return tb, tc


def log_from_losses(vals):
    """The reference's log dict (loss.py:23-30: main level first, then aux 0..n-1 with suffixes) as 0-d views of ONE
    [levels, 6] tensor -- the caller passes a fresh clone, so a step's log never aliases the next step's."""
    Lv = vals.shape[0]
    log = {}
    for lv in [Lv - 1] + list(range(Lv - 1)):
        suffix = "" if lv == Lv - 1 else f"_{lv}"
        for k, name in enumerate(LOSS_NAMES):
            log[name + suffix] = vals[lv, k]
    return log


def get_losses(m_outputs, t_bbox, t_class, config, before_assign=None):
    """loss.py:22-34.  Returns (total_loss 0-d tensor, dict name -> 0-d tensor).  before_assign: an optional callable, called once
    between the matcher's cost and assignment launches (Matcher.run)."""
    lg, bx = _stack_levels(m_outputs)
    tb, tc = _prep_targets(t_bbox, t_class, lg.device)
    Lv, B, Q, C = lg.shape
    sl = SetLoss.get(Lv, B, Q, C, tb.shape[1], lg.device)
    hook = getattr(m_outputs, "reduce_sums", None)
    sl.reduce_sums = hook
    dp = getattr(getattr(m_outputs, "model", None), "dp", None)
    world = getattr(dp, "world", 1) if hook is not None else 1
    total, losses = sl.forward(lg, bx, tb, tc, config.background_class, criterion_of(config, C), world, before_assign)
    if getattr(config, "check_matching", False):
        # opt-in (it synchronises): the reference's SciPy call raises ValueError on NaN / inf / infeasible cost matrices
        # (hungarian_matching.py:29); the device matcher records a status per problem instead of stopping the step
        if bool((sl.matcher.status != 0).any()):
            raise ValueError("cost matrix is infeasible or contains invalid numeric entries")
        model = getattr(m_outputs, "model", None)
        if model is not None:
            model.engine.check_mask_status()    # a padded batch's device mask: an image without a valid feature position
    log = log_from_losses(losses.clone())
    total_loss = total.clone()[0]
    if hasattr(m_outputs, "set_loss"):
        m_outputs.set_loss = sl
    return total_loss, log
