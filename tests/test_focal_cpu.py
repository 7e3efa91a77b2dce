"""CPU side (no GPU) of the sigmoid focal class criterion: the reference of tests/focal_ref.py against torch's binary cross-entropy,
autograd and the published form; the configuration surface (criterion_of, flags); the appended prototypes; and the float32
reference measured against the float64 one on every (parameter set, case) tests/test_gpu_focal.py runs, which fixes that test's
bounds."""
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
import focal_ref as FR                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOCAL_SYMBOLS = ("detr_hip_match_cost_focal_f32", "detr_hip_set_loss_sums_focal_f32", "detr_hip_set_loss_finalize_focal_f32",
                 "detr_hip_set_loss_grad_focal_f32", "detr_hip_postprocess_scored", "detr_hip_detect_scored")
LOSS_SCALE = 0.5


def _logits(seed=0, n=4096, scale=6.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g, dtype=torch.float64) * scale
    t = (torch.rand(n, generator=g) < 0.3).double()
    return x, t


# ------------------------------------------------------------------------------------------
# the class term
# ------------------------------------------------------------------------------------------
def test_gamma_zero_alpha_half_is_half_the_binary_cross_entropy():
    x, t = _logits()
    got = FR.elements(x, t, FR.Focal(0.5, 0.0))
    want = 0.5 * torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())


@pytest.mark.parametrize("f", [FR.FOCAL_DEFAULTS, FR.Focal(0.5, 0.0), FR.Focal(0.75, 1.5), FR.Focal(0.1, 8.0)], ids=str)
def test_closed_form_gradient_is_autograd(f):
    x, t = _logits(1)
    x.requires_grad_(True)
    FR.elements(x, t, f).sum().backward()
    want = x.grad
    got = FR.d_elements(x.detach(), t, f)
    assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("f", [FR.FOCAL_DEFAULTS, FR.Focal(0.75, 1.5)], ids=str)
def test_stable_form_is_the_textbook_form_where_that_is_finite(f):
    x, t = _logits(2, scale=4.0)
    got, want = FR.elements(x, t, f), FR.elements_textbook(x, t, f)
    ok = torch.isfinite(want)
    assert int(ok.sum()) > 4000
    assert float(((got - want)[ok].abs() / want[ok].abs().clamp(min=1e-300)).max()) <= 1e-9
    # the stable form stays finite where the published one does not: float32 logits of +-120
    big = torch.tensor([-120.0, 120.0, -120.0, 120.0], dtype=torch.float32)
    tt = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=torch.float32)
    assert not bool(torch.isfinite(FR.elements_textbook(big, tt, f)).all())
    e = FR.elements(big, tt, f)
    assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(FR.d_elements(big, tt, f)).all())
    assert float(e[0]) == 0.0 and float(e[3]) == 0.0 and abs(float(e[1]) - (1 - f.alpha) * 120) <= 1e-4 and abs(float(e[2]) - f.alpha * 120) <= 1e-4


def test_class_cost_is_the_published_one_away_from_saturation():
    """-alpha (1-p)^g log(p + 1e-8) + (1-alpha) p^g log(1 - p + 1e-8), the published matcher cost: its 1e-8 moves a logarithm by
    1e-8 / p (or / (1 - p)), so the two agree to 1e-2 while p and 1 - p are above 1e-6 and to 1e-5 above 1e-3."""
    f = FR.FOCAL_DEFAULTS
    x = torch.linspace(-13.0, 13.0, 2001, dtype=torch.float64)
    p = torch.sigmoid(x)
    pub = f.alpha * (1 - p) ** f.gamma * -(p + 1e-8).log() - (1 - f.alpha) * p ** f.gamma * -(1 - p + 1e-8).log()
    dev = (FR.class_cost(x, f) - pub).abs()
    for lim, tol in ((1e-6, 1e-2), (1e-3, 1e-5)):
        mid = (p > lim) & (p < 1 - lim)
        assert int(mid.sum()) > 1000 and float(dev[mid].max()) <= tol


def test_metrics_follow_the_largest_non_background_logit():
    lg = torch.tensor([[5.0, -1.0, -2.0],        # bg = 0 large, others <= 0: background
                       [-3.0, 0.0, 0.0],         # the largest is exactly 0: background
                       [9.0, 0.5, 0.5],          # tie above 0: the first, class 1
                       [0.0, -1.0, 2.0]], dtype=torch.float64)
    assert FR.predicted_class(lg, 0).tolist() == [0, 0, 1, 2]
    assert FR.predicted_class(lg, 2).tolist() == [0, 2, 0, 2]


# ------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------
def test_criterion_of_carries_and_validates_the_class_criterion():
    from detr_tf.loss.loss import DEFAULT_CRITERION, Criterion, criterion_of
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    crit = criterion_of(cfg)
    assert crit.is_default and not crit.is_focal and crit == DEFAULT_CRITERION
    assert (cfg.class_criterion, cfg.focal_alpha, cfg.focal_gamma) == ("softmax", 0.25, 2.0)
    assert Criterion(1.0, 5.0, 2.0, 1.0, 5.0, 2.0, 0.1, False, None).is_default            # positional construction as before
    assert criterion_of(SimpleNamespace()).is_default                                      # attributes it lacks read as the defaults
    cfg.class_criterion, cfg.focal_alpha, cfg.focal_gamma = "focal", 0.3, 1.0
    crit = criterion_of(cfg)
    assert crit.is_focal and not crit.is_default and (crit.focal_alpha, crit.focal_gamma) == (0.3, 1.0)
    assert crit != criterion_of(TrainingConfig()) and hash(crit) != hash(DEFAULT_CRITERION)      # the graph key changes
    assert list(crit.focal_floats()) == [pytest.approx(0.3), 1.0] and len(crit.floats()) == 8
    for name, bad in (("class_criterion", "sigmoid"), ("focal_alpha", 0.0), ("focal_alpha", 1.0), ("focal_alpha", float("nan")),
                      ("focal_gamma", -0.5), ("focal_gamma", 8.5), ("focal_gamma", float("inf"))):
        c = TrainingConfig()
        c.class_criterion = "focal"
        setattr(c, name, bad)
        with pytest.raises(ValueError, match=name):
            criterion_of(c)
    c = TrainingConfig()
    c.focal_gamma = 9.0                              # validated under softmax too
    with pytest.raises(ValueError, match="focal_gamma"):
        criterion_of(c)
    c = TrainingConfig()
    c.class_criterion, c.class_weights = "focal", [1.0] * 5
    with pytest.raises(ValueError, match="class_weights"):
        criterion_of(c, 5)


def test_flags():
    from detr_tf.loss.loss import criterion_of
    from detr_tf.training_config import TrainingConfig, training_config_parser
    cfg = TrainingConfig()
    cfg.update_from_args(training_config_parser().parse_args([]))
    assert criterion_of(cfg).is_default
    cfg.update_from_args(training_config_parser().parse_args(["--class_criterion", "focal", "--focal_alpha", "0.4", "--focal_gamma", "1.5"]))
    crit = criterion_of(cfg)
    assert crit.is_focal and (crit.focal_alpha, crit.focal_gamma) == (0.4, 1.5)


def test_scoring_names():
    from detr_tf import _hip
    from detr_tf.inference import _scoring, scoring_of
    assert _hip.SCORINGS == {"softmax": 0, "sigmoid": 1}
    assert scoring_of(SimpleNamespace()) == "softmax" and scoring_of(SimpleNamespace(class_criterion="focal")) == "sigmoid"
    with pytest.raises(ValueError, match="scoring"):
        _scoring("logistic")


# ------------------------------------------------------------------------------------------
# the C surface
# ------------------------------------------------------------------------------------------
def test_header_declares_the_appended_entry_points():
    from detr_tf import _hip
    header = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    for name in FOCAL_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _hip._SIGNATURES and name in _hip.EXPORTED_SYMBOLS
    assert re.search(r"#define DETR_FOCAL_FLOATS 2\b", header) and _hip.FOCAL_FLOATS == 2
    assert re.search(r"#define DETR_CRITERION_FLOATS 8\b", header) and _hip.CRITERION_FLOATS == 8
    assert re.search(r"#define DETR_HIP_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9
    # the _crit_ signatures plus the focal block, without class weights
    for kind in ("match_cost", "set_loss_sums", "set_loss_finalize", "set_loss_grad"):
        crit, focal = _hip._SIGNATURES[f"detr_hip_{kind}_crit_f32"], _hip._SIGNATURES[f"detr_hip_{kind}_focal_f32"]
        assert len(focal) == len(crit) + (1 if kind in ("match_cost", "set_loss_finalize") else 0)


def test_library_exports_them_and_checks_arguments_on_the_host():
    """Every rejection happens before a launch: no GPU is touched (null descriptors / blocks out of range)."""
    import ctypes
    from detr_tf import _hip
    lib = _hip.load()
    for name in FOCAL_SYMBOLS:
        assert hasattr(lib, name), name
    crit = CR.host_block(CR.DEFAULTS)
    sums = (ctypes.c_float * 10)()
    out = (ctypes.c_float * 6)()
    tot = (ctypes.c_float * 1)()
    fin = lib.detr_hip_set_loss_finalize_focal_f32
    for bad in ((0.0, 2.0), (1.0, 2.0), (float("nan"), 2.0), (0.25, -1.0), (0.25, 8.5), (0.25, float("inf"))):
        rc = fin(ctypes.cast(sums, _hip.f32p), 1, crit, FR.focal_block(FR.Focal(*bad)), ctypes.cast(out, _hip.f32p), ctypes.cast(tot, _hip.f32p), None)
        assert rc == -1, bad
        assert "focal[" in lib.detr_hip_last_error().decode(), lib.detr_hip_last_error().decode()
    assert fin(ctypes.cast(sums, _hip.f32p), 1, crit, None, ctypes.cast(out, _hip.f32p), ctypes.cast(tot, _hip.f32p), None) == -1
    assert "null focal block" in lib.detr_hip_last_error().decode()
    # scoring outside {0, 1}, and a null descriptor
    assert lib.detr_hip_postprocess_scored(None, 2, None) == -1 and "scoring=2" in lib.detr_hip_last_error().decode()
    assert lib.detr_hip_detect_scored(None, -1, None) == -1 and "scoring=-1" in lib.detr_hip_last_error().decode()
    assert lib.detr_hip_postprocess_scored(None, 1, None) == -1 and lib.detr_hip_detect_scored(None, 1, None) == -1
    # C == 1 with sigmoid scoring: refused by the shape checks before the launch
    d = _hip.PostprocessDesc()
    d.B, d.Q, d.C, d.background_class, d.bbox_format = 1, 4, 1, 0, 0
    buf = (ctypes.c_float * 64)()
    for fld in ("logits", "boxes", "out_boxes", "out_labels", "out_scores", "counts"):
        setattr(d, fld, ctypes.addressof(buf))
    d.sL_b, d.sL_q, d.sB_b, d.sB_q = 4, 1, 16, 4
    assert lib.detr_hip_postprocess_scored(ctypes.byref(d), 1, None) == -1 and "C=1" in lib.detr_hip_last_error().decode()
    dd = _hip.DetectDesc()
    dd.B, dd.Q, dd.C, dd.background_class, dd.bbox_format, dd.clip, dd.max_detections, dd.score_threshold = 1, 4, 1, 0, 1, 1, 4, 0.0
    for fld in ("logits", "boxes", "sizes", "out_boxes", "out_labels", "out_scores", "out_query", "counts"):
        setattr(dd, fld, ctypes.addressof(buf) // 16 * 16 + 16)
    dd.sL_b, dd.sL_q, dd.sB_b, dd.sB_q = 4, 1, 16, 4
    assert lib.detr_hip_detect_scored(ctypes.byref(dd), 1, None) == -1 and "C=1" in lib.detr_hip_last_error().decode()


# ------------------------------------------------------------------------------------------
# the reference itself: float32 against float64 on every pair of the GPU test
# ------------------------------------------------------------------------------------------
def _torch_inputs(case, dtype):
    logits, boxes, t_bbox, t_class, _ = FR.inputs(case)
    return (torch.from_numpy(logits).to(dtype), torch.from_numpy(boxes).to(dtype), torch.from_numpy(t_bbox).to(dtype),
            torch.from_numpy(t_class))


def measure(ps, case):
    """(cost err, cost bound, d_logits err, bound, d_boxes err, bound) of the float32 reference against the float64 one, both on the
    float64 reference's matching, gradients at the loss_scale of the GPU test."""
    from oracle import set_loss_ref as L
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    w, f = FR.param_set(ps)
    lg64, bx64, tb64, tc = _torch_inputs(case, torch.float64)
    match = FR.focal_match(lg64, bx64, tb64, tc, w, f)
    cost_err = 0.0
    lg32, bx32, tb32, _ = _torch_inputs(case, torch.float32)
    for lv in range(Lv):
        for b in range(B):
            t64, c64 = L.strip_header(tb64[b], tc[b])
            t32, c32 = L.strip_header(tb32[b], tc[b])
            if t64.shape[0]:
                c_64 = FR.cost_matrix(t64, c64, bx64[lv, b], lg64[lv, b], w, f)
                c_32 = FR.cost_matrix(t32, c32, bx32[lv, b], lg32[lv, b], w, f)
                cost_err = max(cost_err, float((c_32.double() - c_64).abs().max()))
    grads = {}
    for dtype in (torch.float32, torch.float64):
        lg, bx, tb, _ = _torch_inputs(case, dtype)
        lg.requires_grad_(True)
        bx.requires_grad_(True)
        m = [tuple(x.to(dtype) if x.is_floating_point() else x for x in lvl) for lvl in match]
        total, _, _ = FR.focal_losses(lg, bx, tb, tc, bg, w, f, match=m)
        total.backward()
        grads[dtype] = (LOSS_SCALE * lg.grad.double(), LOSS_SCALE * bx.grad.double())
    dl_err = float((grads[torch.float32][0] - grads[torch.float64][0]).abs().max())
    db_err = float((grads[torch.float32][1] - grads[torch.float64][1]).abs().max())
    cost_bound = 2e-6 * max(1.0, w.cost_class, w.cost_bbox, w.cost_giou)
    return (cost_err, cost_bound, dl_err, 2e-5 * float(grads[torch.float64][0].abs().max()), db_err,
            5e-5 * float(grads[torch.float64][1].abs().max()))


@pytest.mark.parametrize("ps", FR.PARAM_SETS)
def test_recorded_float32_reference_errors(ps):
    """focal_ref's three tables hold exactly the pairs on which the float32 reference misses the float64 one by more than the GPU
    test's bound, with its error as measured here; on every other pair it stays within that bound."""
    for case in FR.CASES:
        if case[-1] != "contiguous" and ps != "F2":
            continue                                              # both layouts share their values: measured once
        key = (ps, case[0].rsplit("-", 1)[0])
        ce, cb, le, lb, be, bb = measure(ps, case)
        print(f"{ps}-{case[0]}: cost {ce:.3e} / {cb:.1e}  d_logits {le:.3e} / {lb:.3e}  d_boxes {be:.3e} / {bb:.3e}")
        for table, err, bound in ((FR.COST_F32_REF_ERR, ce, cb), (FR.D_LOGITS_F32_REF_ERR, le, lb), (FR.D_BOXES_F32_REF_ERR, be, bb)):
            if key in table:
                assert err > bound and 0.5 * table[key] <= err <= table[key] * 1.001, (key, err, bound, table[key])
            else:
                assert err <= bound, (key, err, bound)


def test_scores_labels_reference():
    lg = np.array([[0.0, 2.0, 2.0, -1.0],            # tie: the first
                   [9.0, -3.0, -5.0, -4.0],          # the background logit does not count
                   [1.0, np.nan, 0.5, 0.25],         # NaN: score NaN, label from the others
                   [np.nan, 1.0, 0.0, 0.0]])         # NaN in the background column only: ignored
    s, l = FR.scores_labels(lg, 0)
    assert l.tolist() == [1, 1, 2, 1]
    assert s[0] == 1 / (1 + math.exp(-2.0)) and s[1] == 1 / (1 + math.exp(3.0)) and math.isnan(s[2]) and s[3] == 1 / (1 + math.exp(-1.0))
    s, l = FR.scores_labels(lg[:2], 3)
    assert l.tolist() == [1, 0]
