"""Multi-label detections, host side (no GPU): the float64 reference of tests/multilabel_ref.py on hand-worked cases, the
argument checks of the `multilabel` keyword that are raised before the device is touched, and the two C entry points: declared in
the header beside detr_hip_detect_scored and exported by the built library."""
import os
import re

import numpy as np
import pytest
import torch

import abi_header
import multilabel_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("detr_hip_detect_multilabel", "detr_hip_postprocess_multilabel")


class _Cfg:
    normalized_method, image_size, background_class, class_criterion = "torch_resnet", (64, 96), 3, "focal"


# ---- the reference -----------------------------------------------------------------------------------------------------------
def test_grid_scores_are_far_apart_and_the_special_values_are_what_they_claim():
    s = MR.sigmoid64(MR.GRID)
    gaps = np.diff(s)
    assert gaps.min() > 1.59e-4 and gaps.argmin() in (0, len(gaps) - 1)              # the minimum is at the ends of the grid
    assert MR.GRID.astype(np.float32).astype(np.float64).tolist() == MR.GRID.tolist()
    one = np.float32(1) / (np.float32(1) + np.exp(-np.array(MR.ONES, np.float32)))
    assert one.dtype == np.float32 and one.tolist() == [1.0, 1.0, 1.0]
    assert MR.sigmoid64(-np.inf) == 0.0 and np.isnan(MR.sigmoid64(np.nan))
    lo, hi = MR.sigmoid64(-1.0), MR.sigmoid64(-15 / 16)
    assert lo + 1e-3 < MR.MID < hi - 1e-3 and MR.THRESHOLDS == (0.0, MR.MID, 1.5)


def test_ties_straddling_the_cut_take_the_lowest_flat_indexes():
    # C = 3, background 1 (its 9.0 would win everything).  Logits: one 2.0, five 1.0 (flat 0, 3, 8, 9, 11), two 0.0 (flat 2, 6).
    lg = np.array([[1.0, 9.0, 0.0],
                   [1.0, 9.0, 2.0],
                   [0.0, 9.0, 1.0],
                   [1.0, 9.0, 1.0]], np.float32)
    q, c, s = MR.topk_pairs(lg, 1, 0.0, 3)
    assert q.tolist() == [1, 0, 1] and c.tolist() == [2, 0, 0]                       # the 2.0, then the b's at flat 0 and 3
    assert s.tolist() == [MR.sigmoid64(2.0), MR.sigmoid64(1.0), MR.sigmoid64(1.0)]
    q, c, _ = MR.topk_pairs(lg, 1, 0.0, 5)
    assert (q * 3 + c).tolist() == [5, 0, 3, 8, 9]                                   # K = 3 and K = 5 both cut through the 1.0s
    q, c, _ = MR.topk_pairs(lg, 1, 0.0, 100)
    assert len(q) == 8 and (q * 3 + c).tolist() == [5, 0, 3, 8, 9, 11, 2, 6]         # K > candidates: all of them


def test_background_is_skipped_nan_is_excluded_and_zero_is_a_candidate():
    lg = np.array([[40.0, 3.0, np.nan],
                   [-np.inf, np.inf, 20.0]], np.float32)
    q, c, s = MR.topk_pairs(lg, 0, 0.0, 10)                                          # the 40 and the -inf are background
    assert (q * 3 + c).tolist() == [4, 5, 1] and s[2] == MR.sigmoid64(3.0)           # inf and 20 tie at one: flat order
    q, c, s = MR.topk_pairs(lg, 1, 0.0, 10)
    assert (q * 3 + c).tolist() == [0, 5, 3] and s[2] == 0.0                         # 0.0 passes a threshold of 0; the NaN never
    assert len(MR.topk_pairs(lg, 1, 1.5, 10)[0]) == 0
    q, c, _ = MR.topk_pairs(lg, 1, MR.MID, 10)
    assert (q * 3 + c).tolist() == [0, 5]


def test_the_reference_refuses_inputs_a_last_bit_could_reorder():
    with pytest.raises(AssertionError, match="closer"):
        MR.topk_pairs(np.array([[0.0, 1.0, 1.0 + 2e-5]]), 0, 0.0, 2)
    with pytest.raises(AssertionError, match="threshold"):
        MR.topk_pairs(np.array([[0.0, 1.0, 2.0]]), 0, float(MR.sigmoid64(1.0)) + 1e-6, 2)


def test_the_regimes_are_what_they_claim():
    rng = np.random.default_rng(0)
    lg = MR.grid_image(rng, 5, 65, 64)
    assert int(np.isnan(lg).sum()) == 1 and int(np.isneginf(lg).sum()) == 1 and not np.isnan(lg[:, 64]).any()
    assert sorted(lg[np.isin(lg, MR.ONES)].tolist()) == sorted(MR.ONES)
    q, c, s = MR.topk_pairs(lg, 64, 0.0, 7)
    assert s[:3].tolist() == pytest.approx([1.0] * 3, abs=1e-8) and s[3] < 0.999
    assert len(MR.topk_pairs(lg, 64, 0.0, 1024)[0]) == 5 * 64 - 1                    # all but the NaN
    q, c, _ = MR.topk_pairs(MR.equal_image(3, 4), 1, 0.0, 5)
    assert (q * 4 + c).tolist() == [0, 2, 3, 4, 6]                                   # stepping over the background column
    for j in (0, 6, 7, 8):
        assert len(MR.topk_pairs(MR.counted_image(rng, 5, 65, 64, j), 64, MR.MID, 1024)[0]) == j


# ---- the keyword -------------------------------------------------------------------------------------------------------------
def test_multilabel_needs_sigmoid_scoring_before_the_device_is_touched():
    from detr_tf import _hip
    from detr_tf.evaluation import eval_model
    from detr_tf.inference import Detector, detect_batched
    out = {"pred_logits": torch.zeros(1, 4, 5), "pred_boxes": torch.full((1, 4, 4), 0.5)}          # host tensors
    with pytest.raises(ValueError, match="multilabel=True needs scoring='sigmoid'"):
        detect_batched(out, [(8, 8)], 4, scoring="softmax", multilabel=True)
    with pytest.raises(ValueError, match="multilabel=True needs scoring='sigmoid'"):
        detect_batched(out, [(8, 8)], 4, multilabel=True)                            # the default scoring is softmax
    with pytest.raises(ValueError, match="multilabel"):
        Detector(None, _Cfg(), scoring="softmax", multilabel=True)
    with pytest.raises(ValueError, match="multilabel"):
        eval_model(None, None, ["a"], [], multilabel=True)                           # config None: softmax
    with pytest.raises(RuntimeError, match=r"max_detections=1025 must be in 1\.\.1024 with multilabel"):
        detect_batched(out, [(8, 8)], 4, scoring="sigmoid", multilabel=True, max_detections=1025)
    with pytest.raises(RuntimeError, match="max_detections=0"):
        Detector(None, _Cfg(), multilabel=True, max_detections=0)
    with pytest.raises(RuntimeError, match="must live on the GPU"):                  # K > Q passes the argument checks
        detect_batched(out, [(8, 8)], 4, scoring="sigmoid", multilabel=True, max_detections=7)
    assert _hip.SCORINGS == {"softmax": 0, "sigmoid": 1} and _hip.MULTILABEL_MAX == 1024


def test_detector_keeps_rejecting_what_sigmoid_scoring_rejects():
    from detr_tf.inference import Detector
    for extra in (dict(tiles=(1, 2)), dict(nms_threshold=0.5), dict(flip=True), dict(scales=(64, 80)), dict(merge="wbf")):
        for multilabel in (False, True):
            with pytest.raises(NotImplementedError, match="scoring"):
                Detector(None, _Cfg(), multilabel=multilabel, **extra)
    det = Detector(None, _Cfg(), multilabel=True, max_detections=300)                # K may exceed the model's Q
    assert det.multilabel and det.scoring == "sigmoid" and det.max_detections == 300
    assert Detector(None, _Cfg()).multilabel is False
    empty = dict(print_result=False, scoring="sigmoid", multilabel=True, max_detections=7)
    from detr_tf.evaluation import eval_model
    assert eval_model(None, None, ["a", "b"], [], **empty) == eval_model(None, None, ["a", "b"], [], print_result=False)
    assert eval_model.__kwdefaults__ == {"protocol": "reference"}


# ---- the C entry points ------------------------------------------------------------------------------------------------------
def test_multilabel_symbols_declared_exported_appended():
    _hip, lib = abi_header.hip_lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "int detr_hip_detect_multilabel(const detr_detect_desc *d, void *stream);" in hdr
    assert ("int detr_hip_postprocess_multilabel(const detr_postprocess_desc *d, int32_t max_detections, float score_threshold, "
            "void *stream);") in hdr
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9 and "#define DETR_HIP_ABI_VERSION 9" in hdr
    # new entry points on the descriptors that exist: declared beside detr_hip_detect_scored, whose descriptor and sigmoid they share
    assert hdr.index("int detr_hip_detect_multilabel(") > hdr.index("int detr_hip_detect_scored(")
    assert list(_hip._SIGNATURES)[-2:] == list(NEW_SYMBOLS)
    assert len(_hip.LAYOUT_STRUCTS) == 18                                            # no new struct: the layout registry is untouched
    mk = open(os.path.join(ROOT, "detr-tensorflow_amd", "Makefile")).read()
    assert "csrc/detect_multilabel.hip" in mk
