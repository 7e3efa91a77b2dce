"""CPU side (no GPU) of the configurable set criterion: the reference of tests/criterion_ref.py against the oracle at the defaults,
the admissibility of every (weight set, case) that tests/test_gpu_criterion.py runs, the configuration surface (attributes, flags,
criterion_of, rounding of class weights), the four appended entry points and their host-side argument checks."""
import ctypes
import math
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criterion_ref as CR                 # noqa: E402
import setloss_cases as SC                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRIT_SYMBOLS = ("detr_hip_match_cost_crit_f32", "detr_hip_set_loss_sums_crit_f32", "detr_hip_set_loss_finalize_crit_f32",
                "detr_hip_set_loss_grad_crit_f32")


def _torch_inputs(ws, case, dtype):
    logits, boxes, t_bbox, t_class, _ = CR.inputs(ws, case)
    return (torch.from_numpy(logits).to(dtype), torch.from_numpy(boxes).to(dtype), torch.from_numpy(t_bbox).to(dtype),
            torch.from_numpy(t_class))


# ------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------
def _same(a, b, tol=1e-12):
    """Within tol (relative above 1), NaN where the other is NaN (a level without an unmatched query has no true_neg)."""
    a, b = float(a.detach()), float(b.detach())
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol * max(1.0, abs(a))


@pytest.mark.parametrize("case", CR.CONTIGUOUS, ids=[c[0] for c in CR.CONTIGUOUS])
def test_reference_at_the_defaults_is_the_oracle(case):
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    grads = []
    outs = []
    for fn in (lambda *a: SC.oracle_losses(*a), lambda *a: CR.criterion_losses(*a, CR.DEFAULTS)):
        lg, bx, tb, tc = _torch_inputs("A", case, torch.float64)
        lg.requires_grad_(True)
        bx.requires_grad_(True)
        total, losses, match = fn(lg, bx, tb, tc, bg)
        total.backward()
        outs.append((total, losses, match))
        grads.append((lg.grad, bx.grad))
    (t0, l0, m0), (t1, l1, m1) = outs
    assert list(l0) == list(l1) and len(l1) == 6 * Lv
    assert _same(t0, t1)
    for k in l0:
        assert _same(l0[k], l1[k]), k
    for lv in range(Lv):
        assert all(torch.equal(x, y) for x, y in zip(m0[lv], m1[lv]))
    for g0, g1 in zip(grads[0], grads[1]):
        assert float((g0 - g1).abs().max()) <= 1e-12


def test_weight_sets_are_the_issue_s():
    a, b, c, z = (CR.weight_set(n, 7) for n in CR.WEIGHT_SETS)
    assert a == CR.DEFAULTS == (1.0, 5.0, 2.0, 1.0, 5.0, 2.0, 0.1, False, None)
    assert b[:8] == (2.0, 3.0, 1.5, 1.5, 4.0, 0.75, 0.25, False) and b.class_weights is None
    assert c[:7] == b[:7] and c.min_one is True and len(c.class_weights) == 7
    assert all(0.25 <= v <= 4.0 and v * 64 == round(v * 64) for v in c.class_weights) and len(set(c.class_weights)) > 1
    assert z == CR.DEFAULTS._replace(cost_class=0.0, giou_coef=0.0)
    assert [p[1] for p in CR.PAIRS[:-1]] == CR.CONTIGUOUS * 4 and CR.PAIRS[-1][0] == "C" and CR.PAIRS[-1][1][-1] == "strided"


@pytest.mark.parametrize("ws,case", CR.PAIRS, ids=CR.PAIR_IDS)
def test_matching_is_precision_independent(ws, case):
    """Admissibility: the float32 and the float64 reference choose the same matching, so no GPU comparison hinges on a near-tie."""
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    w = CR.weight_set(ws, C)
    lg32, bx32, tb32, tc = _torch_inputs(ws, case, torch.float32)
    lg64, bx64, tb64, _ = _torch_inputs(ws, case, torch.float64)
    m32 = CR.criterion_match(lg32, bx32, tb32, tc, w)
    m64 = CR.criterion_match(lg64, bx64, tb64, tc, w)
    for lv in range(Lv):
        for x, y in zip(m32[lv][2:], m64[lv][2:]):
            assert torch.equal(x, y), f"{ws}-{name}: float32 and float64 references match differently at level {lv}: give it a seed"
        assert m64[lv][2].numel() == sum(min(n, Q) for n in n_list)


def test_api_problem_matching_is_precision_independent():
    """The same for the problem and the weights of the get_losses tests."""
    Lv = CR.API_CASE[1]
    logits, boxes, t_bbox, t_class, _ = SC.loss_inputs(CR.API_CASE)
    tc = torch.from_numpy(t_class)
    for w in CR.api_weights():
        m = [CR.criterion_match(torch.from_numpy(logits).to(dt), torch.from_numpy(boxes).to(dt), torch.from_numpy(t_bbox).to(dt), tc, w)
             for dt in (torch.float32, torch.float64)]
        assert all(torch.equal(x, y) for lv in range(Lv) for x, y in zip(m[0][lv][2:], m[1][lv][2:]))


def test_recorded_float32_reference_errors():
    """criterion_ref.D_LOGITS_ATOL is 4x the float32 reference's own d_logits error on the pairs listed there, measured here again;
    every other pair meets the relative bound of the GPU test with a factor 4 to spare."""
    for ws, case in CR.PAIRS:
        name, Lv, B, Q, C, bg, R, n_list, layout = case
        w = CR.weight_set(ws, C)
        grads = {}
        for dtype in (torch.float32, torch.float64):
            lg, bx, tb, tc = _torch_inputs(ws, case, dtype)
            lg.requires_grad_(True)
            total, _, _ = CR.criterion_losses(lg, bx, tb, tc, bg, w)
            total.backward()
            grads[dtype] = 0.5 * lg.grad.double()              # loss_scale of the GPU test
        err = float((grads[torch.float32] - grads[torch.float64]).abs().max())
        rel_bound = 2e-5 * float(grads[torch.float64].abs().max())
        key = (ws, name.rsplit("-", 1)[0])
        print(f"{ws}-{name}: float32 reference d_logits err {err:.3e}, relative bound {rel_bound:.3e}")
        if key in CR.D_LOGITS_F32_REF_ERR:
            rec = CR.D_LOGITS_F32_REF_ERR[key]
            assert 4 * err > rel_bound and 0.5 * rec <= err <= rec * 1.001, (key, err)
        else:
            assert 4 * err <= rel_bound, (key, err, rel_bound)


def test_class_weights_count_for_matched_background_targets_only():
    """A matched target is weighted by its class even where that is the background class; eos weighs the unmatched queries alone."""
    lg = torch.tensor([[0.3, -0.2, 0.1], [1.0, 0.5, -0.5], [0.0, 0.2, 0.4]], dtype=torch.float64)
    tc = torch.tensor([0, 2])                                       # target 0 carries the background class 0
    ti, pi = torch.tensor([0, 1]), torch.tensor([2, 0])
    sel = torch.tensor([True, False, True])
    w = CR.DEFAULTS._replace(eos=0.25, class_weights=(3.0, 1.0, 0.5))
    got = CR.loss_labels(lg, tc, ti, pi, sel, 0, w)[0]
    ce = lambda q, c: float(torch.logsumexp(lg[q], -1) - lg[q, c])
    want = (0.25 * ce(1, 0) + 3.0 * ce(2, 0) + 0.5 * ce(0, 2)) / (0.25 + 3.0 + 0.5)
    assert abs(float(got) - want) <= 1e-14


# ------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------
def test_config_defaults_flags_and_empty_command_line():
    from detr_tf.loss.loss import criterion_of
    from detr_tf.training_config import TrainingConfig, training_config_parser
    want = dict(set_cost_class=1.0, set_cost_bbox=5.0, set_cost_giou=2.0, class_loss_coef=1.0, bbox_loss_coef=5.0, giou_loss_coef=2.0,
                eos_coef=0.1)
    cfg = TrainingConfig()
    for k, v in want.items():
        assert getattr(cfg, k) == v and isinstance(getattr(cfg, k), float), k
    assert cfg.num_boxes_min_one is False and cfg.class_weights is None
    assert criterion_of(cfg).is_default
    cfg.update_from_args(training_config_parser().parse_args([]))
    for k, v in want.items():
        assert getattr(cfg, k) == v and isinstance(getattr(cfg, k), float), k
    assert cfg.num_boxes_min_one is False and cfg.class_weights is None and criterion_of(cfg).is_default
    cfg.update_from_args(training_config_parser().parse_args(
        ["--set_cost_class", "2", "--set_cost_bbox", "3", "--set_cost_giou", "1.5", "--class_loss_coef", "1.5", "--bbox_loss_coef", "4",
         "--giou_loss_coef", "0.75", "--eos_coef", "0.25", "--num_boxes_min_one"]))
    crit = criterion_of(cfg)
    assert tuple(crit) == (2.0, 3.0, 1.5, 1.5, 4.0, 0.75, 0.25, True, None, "softmax", 0.25, 2.0) and not crit.is_default
    assert tuple(crit)[:8] == tuple(CR.weight_set("C", 3))[:8]
    assert not hasattr(training_config_parser().parse_args([]), "class_weights")       # an attribute without a flag


def test_criterion_of_reads_missing_attributes_as_defaults_and_is_immutable():
    from detr_tf.loss.loss import DEFAULT_CRITERION, criterion_of
    crit = criterion_of(SimpleNamespace(background_class=3))
    assert crit == DEFAULT_CRITERION and crit.is_default and crit.class_weights is None
    assert tuple(crit)[:8] == (1.0, 5.0, 2.0, 1.0, 5.0, 2.0, 0.1, False)
    with pytest.raises(AttributeError):
        crit.eos_coef = 0.5
    hash(crit)
    assert list(crit.floats()) == [np.float32(v) for v in (1, 5, 2, 1, 5, 2, 0.1, 0)]
    one = criterion_of(SimpleNamespace(eos_coef=0.25))
    assert not one.is_default and one.eos_coef == 0.25 and one != crit
    # all-one class weights are still the run-time path: the default record has none
    assert not criterion_of(SimpleNamespace(class_weights=[1.0, 1.0])).is_default


DISPATCH_FAMILIES = {"default": (SimpleNamespace(), ""), "crit": (SimpleNamespace(eos_coef=0.25), "_crit"),
                     "crit_class_weights": (SimpleNamespace(class_weights=[1.0, 2.0, 0.5]), "_crit"),
                     "focal": (SimpleNamespace(class_criterion="focal"), "_focal")}
# the arguments of a kind that are not the criterion's: (descriptor | sums, levels), then the operands
DISPATCH_KINDS = {"match_cost": 2, "set_loss_sums": 3, "set_loss_finalize": 4, "set_loss_grad": 6}


@pytest.mark.parametrize("kind", DISPATCH_KINDS)
@pytest.mark.parametrize("family", DISPATCH_FAMILIES)
def test_one_dispatch_names_a_declared_entry_point_with_its_blocks(family, kind):
    from detr_tf import _hip
    from detr_tf.loss.loss import ENTRY_LEAD, criterion_of
    config, suffix = DISPATCH_FAMILIES[family]
    crit = criterion_of(config)
    weights = ctypes.c_void_p(64) if crit.class_weights is not None else None
    name, blocks = crit.entry(kind, weights)
    assert name == f"detr_hip_{kind}{suffix}_f32" and name in _hip._SIGNATURES
    sig = _hip._SIGNATURES[name]
    assert len(blocks) + DISPATCH_KINDS[kind] + 1 == len(sig)                  # + the stream
    lead = ENTRY_LEAD[kind]
    want = {"default": [], "focal": [crit.floats(), crit.focal_floats()]}.get(family, [crit.floats()])
    for k, block in enumerate(want):                                           # host blocks of floats, in the order of the C signature
        assert sig[lead + k] is ctypes.POINTER(ctypes.c_float) and list(blocks[k]) == list(block)
    if suffix == "_crit" and kind in ("set_loss_sums", "set_loss_grad"):       # class weights: a device pointer (or None) behind the block
        assert len(blocks) == 2 and blocks[1] is weights and sig[lead + 1] is _hip.f32p
    else:
        assert len(blocks) == len(want)
    assert all(t is not ctypes.POINTER(ctypes.c_float) for t in sig[:lead] + sig[lead + len(want):])


def test_criterion_is_a_plain_record_and_the_matcher_has_no_global_hook():
    from detr_tf.loss import hungarian_matching
    from detr_tf.loss.loss import CLASS_TERM_DEFAULTS, CRITERION_DEFAULTS, DEFAULT_CRITERION, Criterion
    assert not hasattr(DEFAULT_CRITERION, "__dict__") and not hasattr(DEFAULT_CRITERION, "_class_term")
    assert tuple(DEFAULT_CRITERION) == CRITERION_DEFAULTS + (None,) + CLASS_TERM_DEFAULTS
    for name in ("__new__", "__eq__", "__ne__", "__hash__", "__repr__", "_replace", "__setattr__"):
        assert name not in vars(Criterion), name
    focal = DEFAULT_CRITERION._replace(class_criterion="focal")
    assert focal.is_focal and focal != DEFAULT_CRITERION and hash(focal) != hash(DEFAULT_CRITERION) and "focal" in repr(focal)
    assert not hasattr(hungarian_matching, "before_assign")


@pytest.mark.parametrize("name", ["set_cost_class", "set_cost_bbox", "set_cost_giou", "class_loss_coef", "bbox_loss_coef", "giou_loss_coef",
                                  "eos_coef"])
def test_criterion_of_refuses_bad_values(name):
    from detr_tf.loss.loss import criterion_of
    for bad in (float("nan"), float("inf"), -0.5):
        with pytest.raises(ValueError, match=name):
            criterion_of(SimpleNamespace(**{name: bad}))
    assert getattr(criterion_of(SimpleNamespace(**{name: 0.0})), name) == 0.0


def test_class_weights_are_rounded_to_64ths_and_checked():
    from detr_tf.loss.loss import criterion_of
    crit = criterion_of(SimpleNamespace(class_weights=np.array([0.0, 1.0, 0.3, 2.0 / 3.0, 16.0, 1.0 / 128.0 + 1e-9])), nb_class=6)
    assert crit.class_weights == (0.0, 1.0, 19 / 64, 43 / 64, 16.0, 1 / 64) and isinstance(crit.class_weights, tuple)
    assert all(v * 64 == round(v * 64) for v in crit.class_weights)
    for bad in ([1.0, -0.01], [1.0, 16.5], [float("nan"), 1.0], [float("inf"), 1.0]):
        with pytest.raises(ValueError, match="class_weights"):
            criterion_of(SimpleNamespace(class_weights=bad))
    with pytest.raises(ValueError, match="class_weights"):
        criterion_of(SimpleNamespace(class_weights=[1.0, 2.0, 3.0]), nb_class=4)


def test_class_weights_are_refused_where_their_sum_could_leave_float32():
    """world * B * (R - 1) matched targets at most: past 16384 a sum of 1/64 quanta up to 16 could pass 2^24 quanta."""
    from detr_tf.loss.loss import SetLoss, criterion_of
    sl = SetLoss(1, 200, 2, 3, 42, "cpu")                          # 200 * 41 = 8200 targets per rank
    crit = criterion_of(SimpleNamespace(class_weights=[1.0, 2.0, 0.5]), nb_class=3)
    with pytest.raises(ValueError, match="16384"):
        sl._class_weights(crit, 2)                                 # two ranks: 16400
    assert sl._class_weights(criterion_of(SimpleNamespace()), 2) is None
    with pytest.raises(ValueError, match="class_weights"):
        sl._class_weights(criterion_of(SimpleNamespace(class_weights=[1.0, 2.0])), 1)
    assert 16384 * 16 * 64 == 2 ** 24


def test_get_total_losss_with_and_without_a_config():
    from detr_tf.loss.loss import get_total_losss
    losses = {"label_cost": 1.0, "true_neg": 100.0, "giou_loss": 10.0, "l1_loss": 0.5, "label_cost_0": 2.0, "giou_loss_0": 1.0, "l1_loss_0": 4.0}
    assert get_total_losss(losses) == 1 * 3.0 + 2 * 11.0 + 5 * 4.5
    assert get_total_losss(losses, SimpleNamespace()) == get_total_losss(losses)
    cfg = CR.config_of(CR.weight_set("B", 2))
    assert get_total_losss(losses, cfg) == 1.5 * 3.0 + 0.75 * 11.0 + 4.0 * 4.5


def test_graphed_step_signature_carries_the_criterion():
    """A changed criterion value changes the signature of the recorded step (it re-records); class weights enter as a tuple."""
    from detr_tf.training import GraphedTrainStep
    cfg = CR.config_of(CR.DEFAULTS, train_backbone=False, train_transformers=True, train_nlayers=True, background_class=0,
                       gradient_norm_clipping=0.1, global_clipnorm=None, weight_decay=0.0)
    eng = SimpleNamespace(compute=0, dropout_p=0.0, dilate=(False, False, False))
    step = GraphedTrainStep(SimpleNamespace(engine=eng), {}, cfg)
    args = (torch.zeros(2, 8, 8, 3), torch.zeros(2, 4, 4), torch.zeros(2, 4, 1))
    s0 = step._signature(*args)
    assert step._signature(*args) == s0
    cfg.giou_loss_coef = 1.0
    s1 = step._signature(*args)
    assert s1 != s0
    cfg.class_weights = [1.0, 0.5, 2.0]
    s2 = step._signature(*args)
    assert s2 != s1 and (1.0, 0.5, 2.0) in [getattr(x, "class_weights", None) for x in s2]
    hash(s2)


# ------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------
def test_crit_entry_points_are_declared_mirrored_and_exported():
    from detr_tf import _hip
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    lib = _hip.load()
    for name in CRIT_SYMBOLS:
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and name in _hip._SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define\s+DETR_CRITERION_FLOATS\s+8\b", hdr) and _hip.CRITERION_FLOATS == 8
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9
    assert "#define DETR_HIP_ABI_VERSION 9" in hdr
    # no new descriptor struct, mirror or layout id came with them
    assert len(re.findall(r"\}\s*detr_[a-z0-9_]+_desc\s*;", hdr)) == len(_hip.LAYOUT_STRUCTS) == 18
    assert ctypes.sizeof(_hip.SetLossDesc) == 112


def _desc(_hip, fake):
    d = _hip.SetLossDesc()
    d.levels, d.B, d.Q, d.C, d.R = 2, 2, 9, 5, 6
    d.logits = d.boxes = d.t_bbox = d.t_class = fake
    d.sL_l, d.sL_b, d.sL_q = 90, 45, 5
    d.sB_l, d.sB_b, d.sB_q = 72, 36, 4
    d.background_class = 4
    return d


def test_crit_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument checks run on the host before anything touches device memory: negative code + last_error."""
    from detr_tf import _hip
    lib = _hip.load()
    fake = 4096                                   # never dereferenced: every call below fails its checks first
    d = _desc(_hip, fake)
    block = lambda *v: (ctypes.c_float * 8)(*v)
    good = (1.0, 5.0, 2.0, 1.0, 5.0, 2.0, 0.1, 0.0)

    def with_desc(crit, desc):
        """The three entry points that take a descriptor (only ever called here with one that fails fill_args)."""
        dp = None if desc is None else ctypes.byref(desc)
        return [lib.detr_hip_match_cost_crit_f32(dp, crit, fake, None),
                lib.detr_hip_set_loss_sums_crit_f32(dp, crit, None, fake, fake, None),
                lib.detr_hip_set_loss_grad_crit_f32(dp, crit, None, fake, fake, ctypes.c_float(1.0), fake, fake, None)]

    def refused(crit, needle):
        dp = ctypes.byref(d)
        for name, call in zip(CRIT_SYMBOLS, (
                lambda: lib.detr_hip_match_cost_crit_f32(dp, crit, fake, None),
                lambda: lib.detr_hip_set_loss_sums_crit_f32(dp, crit, None, fake, fake, None),
                lambda: lib.detr_hip_set_loss_finalize_crit_f32(fake, 2, crit, fake, fake, None),
                lambda: lib.detr_hip_set_loss_grad_crit_f32(dp, crit, None, fake, fake, ctypes.c_float(1.0), fake, fake, None))):
            rc = call()
            msg = lib.detr_hip_last_error().decode()
            assert rc < 0 and needle in msg, (name, rc, msg)

    refused(None, "null criterion")
    for i in range(8):
        for bad, needle in ((float("nan"), f"criterion[{i}]"), (float("inf"), f"criterion[{i}]"), (-1.0, f"criterion[{i}]")):
            v = list(good)
            v[i] = bad
            refused(block(*v), needle)
    v = list(good)
    v[7] = 2.0
    refused(block(*v), "criterion[7]")
    v[7] = 0.5
    refused(block(*v), "criterion[7]")
    # with a valid criterion the shape checks of the descriptor are the next gate (the three entry points that take one)
    crit = block(*good)
    bad = _desc(_hip, fake)
    bad.background_class = 5
    assert all(rc < 0 for rc in with_desc(crit, bad)) and "background_class" in lib.detr_hip_last_error().decode()
    assert all(rc < 0 for rc in with_desc(crit, None)) and "null descriptor" in lib.detr_hip_last_error().decode()
    bad = _desc(_hip, fake)
    bad.Q = 513
    assert all(rc < 0 for rc in with_desc(crit, bad)) and "Q=513" in lib.detr_hip_last_error().decode()
    assert lib.detr_hip_set_loss_finalize_crit_f32(fake, 0, crit, fake, fake, None) < 0
    assert lib.detr_hip_match_cost_crit_f32(ctypes.byref(d), crit, None, None) < 0 and "null cost" in lib.detr_hip_last_error().decode()


def test_hungarian_matching_honours_its_cost_weights_up_to_the_launch():
    """The assert on (1, 5, 2) is gone: other weights reach the cost kernel's run-time entry point (which needs a GPU: here the
    call is followed up to the library and stopped there), bad ones are a ValueError."""
    from detr_tf import _hip
    from detr_tf.loss import hungarian_matching as HM
    seen = []
    real = _hip.call

    def spy(name, *args):
        seen.append((name, args))
        raise _Stop()

    class _Stop(Exception):
        pass

    t_bbox = torch.zeros(4, 4)
    t_bbox[0, 0] = 2
    t_class = torch.zeros(4, 1, dtype=torch.int64)
    p_bbox, p_class = torch.rand(5, 4), torch.rand(5, 3)
    _hip.call = spy
    try:
        with pytest.raises(_Stop):
            HM.hungarian_matching(t_bbox, t_class, p_bbox, p_class, 2, 3, 1.5)
        with pytest.raises(_Stop):
            HM.hungarian_matching(t_bbox, t_class, p_bbox, p_class)
        with pytest.raises(ValueError, match="set_cost_giou"):
            HM.hungarian_matching(t_bbox, t_class, p_bbox, p_class, 1, 5, -2)
    finally:
        _hip.call = real
    assert [s[0] for s in seen] == ["detr_hip_match_cost_crit_f32", "detr_hip_match_cost_f32"]
    assert list(seen[0][1][1])[:3] == [2.0, 3.0, 1.5]            # [0] class [1] bbox [2] giou
    assert "compiled into" not in open(HM.__file__).read()
