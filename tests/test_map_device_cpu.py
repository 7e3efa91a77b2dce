"""Device mAP accumulation, host side: the C entry point detr_hip_map_match (symbol, struct layout, every argument check --
no GPU), and the record format: the NumPy restatement tests/map_match_ref.py plus compute_map.group_records reproduce
APAccumulator's scores / flags / num_gt exactly, on the seeded random batches the GPU test uses and on refpy_map.npz."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abi_header  # noqa: E402
import map_match_ref as MR  # noqa: E402


_lib = abi_header.hip_lib


def test_map_match_symbol_declared_exported_mirrored():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    name = "detr_hip_map_match"
    assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "detr_map_match_desc" in hdr
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9


def test_map_match_struct_layout_is_appended_and_matches():
    _hip, lib = _lib()
    assert _hip.LAYOUT_STRUCTS[9] is _hip.MapMatchDesc and _hip.LAYOUT_STRUCTS[8] is _hip.PostprocessDesc
    assert max(w for w in _hip.LAYOUT_STRUCTS if w < 100) == 9             # the last descriptor of ABI 9 (its layout: test_abi_layout_cpu.py)
    assert ctypes.sizeof(_hip.MapMatchDesc().thresholds) == 8 * _hip.MAP_MAX_THR == 128

def test_map_match_rejects_bad_arguments_without_a_gpu():
    _hip, lib = _lib()
    fake = 4096                                   # never dereferenced: every call below fails its checks first
    ptrs = ("boxes", "labels", "scores", "counts", "t_bbox", "t_class", "rec_score", "rec_class", "rec_flags", "num_gt", "status")

    def desc(**kw):
        d = _hip.MapMatchDesc()
        d.B, d.Q, d.R, d.nb_class, d.n_thr = 4, 100, 100, 92, 10
        for n in ptrs:
            setattr(d, n, fake)
        d.sD_b, d.sT_b, d.sC_b = 100, 400, 100
        for t, th in enumerate(MR.THRESHOLDS):
            d.thresholds[t] = th
        for n, v in kw.items():
            setattr(d, n, v)
        return d

    def rejected(d, text):
        rc = lib.detr_hip_map_match(ctypes.byref(d) if d is not None else None, None)
        msg = lib.detr_hip_last_error().decode()
        assert rc < 0 and text in msg, (rc, msg, text)

    rejected(None, "null descriptor")
    for n in ptrs:
        rejected(desc(**{n: None}), "null operand")
    for kw in (dict(B=0), dict(B=-3), dict(Q=0), dict(Q=-1), dict(Q=1025), dict(R=0), dict(R=-1), dict(R=257)):
        rejected(desc(**kw), "bad shape")
    for c in (0, -5):
        rejected(desc(nb_class=c), "nb_class")
    for t in (0, -1, 17):
        rejected(desc(n_thr=t), "thresholds")
    d = desc()
    d.thresholds[3] = float("nan")
    rejected(d, "not finite")
    d = desc()
    d.thresholds[9] = float("inf")
    rejected(d, "not finite")
    for kw in (dict(sD_b=99), dict(sT_b=399), dict(sC_b=99), dict(sD_b=-100)):
        rejected(desc(**kw), "batch strides")
    rejected(desc(boxes=fake + 4), "16-byte aligned")


def _restated_accumulator(batches, nb_class, thresholds=None):
    """map_match_ref per batch -> group_records -> an APAccumulator, the way DeviceAPAccumulator.to_host builds it."""
    from detr_tf.loss.compute_map import APAccumulator, group_records
    thresholds = MR.THRESHOLDS if thresholds is None else thresholds
    recs, num_gt = [], np.zeros(nb_class, np.int64)
    for boxes, labels, scores, counts, t_bbox, t_class in batches:
        rs, rc, rf, ng, status = MR.map_match_ref(boxes, labels, scores, counts, t_bbox, t_class, nb_class, thresholds)
        assert status == 0
        assert rs.dtype == np.float32 and rc.dtype == np.int32 and rf.dtype == np.uint32
        recs.append((rs.reshape(-1), rc.reshape(-1), rf.reshape(-1)))
        num_gt += ng
    acc = APAccumulator(nb_class, thresholds)
    acc.scores, acc.flags = group_records(*[np.concatenate(x) for x in zip(*recs)], nb_class, len(thresholds))
    acc.num_gt = num_gt
    return acc


@pytest.mark.parametrize("B,Q,C", MR.RANDOM_SHAPES)
def test_restatement_and_grouping_equal_the_host_accumulator_on_random_batches(B, Q, C):
    batches = MR.random_batches(B, Q, C, seed=1000 * B + Q + C)
    assert len(batches) >= 3
    want = MR.assert_planted_cases_occur(batches, C)          # (also accumulates the host result)
    MR.assert_same_accumulator(_restated_accumulator(batches, C), want)
    assert want.result() == _restated_accumulator(batches, C).result()


def test_restatement_and_grouping_equal_the_host_accumulator_on_the_golden_fixture():
    from detr_tf.loss.compute_map import APAccumulator
    for ci in range(3):
        nb, boxes, labels, scores, counts, t_bbox, t_class, images, fx = MR.golden_case(ci)
        want = APAccumulator(nb)
        for pb, pc, ps, tb, tc in images:                     # the fixture's own [y1, x1, y2, x2] ground truths
            want.add_image(pb, pc, ps, tb, tc)
        got = _restated_accumulator([(boxes, labels, scores, counts, t_bbox, t_class)], nb)
        MR.assert_same_accumulator(got, want)
        assert list(got.result()["box"].values()) == list(fx[f"m{ci}_box_vals"])


def test_restatement_with_other_thresholds_and_status_word():
    from detr_tf.loss.compute_map import APAccumulator
    batches = MR.random_batches(2, 20, 5, seed=3)
    thr = [0.3, 0.9, 0.5]                                     # unsorted, three of them
    want = APAccumulator(5, thr)
    for bt in batches:
        MR.host_accumulate(want, *bt)
    MR.assert_same_accumulator(_restated_accumulator(batches, 5, thr), want)
    boxes, labels, scores, counts, t_bbox, t_class = [x.copy() for x in batches[2]]
    clean = MR.map_match_ref(boxes, labels, scores, counts, t_bbox, t_class, 5)
    labels[0, 0], t_class[0, 1, 0], t_bbox[1, 0, 0] = 5, -1, 100.0
    rs, rc, rf, ng, status = MR.map_match_ref(boxes, labels, scores, counts, t_bbox, t_class, 5)
    assert status == MR.BAD_LABEL | MR.BAD_TARGET_CLASS | MR.BAD_HEADER
    assert (rc[0] == -1).sum() == (clean[1][0] == -1).sum() + 1 and ng.sum() < clean[3].sum()


def test_group_records_properties():
    from detr_tf.loss.compute_map import group_records
    score = np.array([0.9, 0.5, 0.0, 0.7, 0.7, 0.2], np.float32)
    cls = np.array([2, 0, -1, 2, 0, 2], np.int32)
    word = np.array([0b101, 0b000, 0b111, 0b010, 0b111, 0b001], np.uint32)
    scores, flags = group_records(score, cls, word, 4, 3)
    assert scores == [[0.5, float(np.float32(0.7))], [], [float(np.float32(0.9)), float(np.float32(0.7)), float(np.float32(0.2))], []]
    assert flags[1] == [] and flags[3] == []
    assert flags[0][0].tolist() == [[False, False, False], [True, True, True]]
    assert flags[2][0].tolist() == [[True, False, True], [False, True, False], [True, False, False]]
    empty = group_records(np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint32), 2, 10)
    assert empty == ([[], []], [[], []])
    with pytest.raises(ValueError):
        group_records(score, cls, word, 2, 3)


def test_device_accumulator_and_eval_model_reject_without_a_gpu():
    import torch
    from detr_tf.evaluation import eval_model
    from detr_tf.loss.compute_map import DeviceAPAccumulator
    with pytest.raises(ValueError):
        eval_model(None, None, ["a"], [], accumulate="gpu")
    with pytest.raises(RuntimeError):
        DeviceAPAccumulator(3, device="cpu")
    with pytest.raises(ValueError):
        DeviceAPAccumulator(3, iou_thresholds=[0.5] * 17, device="cpu")
    assert "accumulate" in eval_model.__code__.co_varnames and eval_model.__defaults__[-1] == "host"
    assert torch is not None
