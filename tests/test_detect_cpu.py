"""Detector, host side (no GPU): the numpy box helpers against hand-computed values, the COCO result records, every argument
error of Detector / detect_batched that is raised before the device is touched, and the C entry point detr_hip_detect: symbol,
descriptor layout against the header, rejection paths."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_lib = abi_header.hip_lib


class _Cfg:
    normalized_method, image_size, background_class = "torch_resnet", (64, 96), 4


# ---- bbox.np_* ---------------------------------------------------------------------------------------------------------------
def test_np_xcycwh_to_xy_min_xy_max_hand_values():
    from detr_tf import bbox
    got = bbox.np_xcycwh_to_xy_min_xy_max(np.array([[0.5, 0.5, 0.5, 0.25], [0.125, 0.75, 0.5, 1.0]]))
    # the second box leaves the image on the left and at the bottom: the numpy helper does not clip (bbox.py:230-240)
    assert got.tolist() == [[0.25, 0.375, 0.75, 0.625], [-0.125, 0.25, 0.375, 1.25]]
    assert got.shape == (2, 4)


def test_np_rescale_helpers_hand_values():
    from detr_tf import bbox
    size = (480, 640)                                               # (height, width)
    assert bbox.np_rescale_bbox_xcycwh([[0.5, 0.25, 0.125, 1.0]], size).tolist() == [[320.0, 120.0, 80.0, 480.0]]
    assert bbox.np_rescale_bbox_xy_min_xy_max([[0.25, 0.5, 0.75, 1.0]], size).tolist() == [[160.0, 240.0, 480.0, 480.0]]
    assert bbox.np_rescale_bbox_yx_min_yx_max([[0.25, 0.5, 0.75, 1.0]], size).tolist() == [[120.0, 320.0, 360.0, 640.0]]
    # lists and float32 arrays are taken; the input is not modified
    src = np.array([[0.5, 0.5, 1.0, 1.0]], np.float32)
    out = bbox.np_rescale_bbox_xcycwh(src, (3, 5))
    assert out.tolist() == [[2.5, 1.5, 5.0, 3.0]] and src.tolist() == [[0.5, 0.5, 1.0, 1.0]]
    # the chain the reference's callers run: convert, then rescale
    px = bbox.np_rescale_bbox_xy_min_xy_max(bbox.np_xcycwh_to_xy_min_xy_max(np.array([[0.5, 0.5, 0.5, 0.5]])), (100, 200))
    assert px.tolist() == [[50.0, 25.0, 150.0, 75.0]]


# ---- Detector.to_coco_results -------------------------------------------------------------------------------------------------
def _detections():
    from detr_tf.inference import Detections
    a = Detections(torch.tensor([[10.0, 20.0, 30.5, 40.0], [0.0, 0.0, 5.0, 6.0]]), torch.tensor([3, 1]), torch.tensor([0.875, 0.75]),
                   torch.tensor([7, 2], dtype=torch.int32))
    b = Detections(torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64), torch.zeros(0), torch.zeros(0, dtype=torch.int32))
    c = Detections(torch.tensor([[1.0, 2.0, 3.0, 4.0]]), torch.tensor([0]), torch.tensor([0.5]), torch.tensor([0], dtype=torch.int32))
    return [a, b, c]


def test_to_coco_results_records_and_id_map():
    from detr_tf.inference import Detector
    det = Detector(None, _Cfg(), bbox_format="xywh")
    recs = det.to_coco_results(_detections(), [11, 12, "img13"])
    assert recs == [{"image_id": 11, "category_id": 3, "bbox": [10.0, 20.0, 30.5, 40.0], "score": 0.875},
                    {"image_id": 11, "category_id": 1, "bbox": [0.0, 0.0, 5.0, 6.0], "score": 0.75},
                    {"image_id": "img13", "category_id": 0, "bbox": [1.0, 2.0, 3.0, 4.0], "score": 0.5}]
    for r in recs:
        assert set(r) == {"image_id", "category_id", "bbox", "score"}
        assert type(r["score"]) is float and type(r["category_id"]) is int and all(type(v) is float for v in r["bbox"])
    mapped = det.to_coco_results(_detections(), [11, 12, 13], category_ids={0: 1, 1: 2, 3: 4})
    assert [r["category_id"] for r in mapped] == [4, 2, 1]
    listed = det.to_coco_results(_detections(), [11, 12, 13], category_ids=[1, 2, 3, 5])
    assert [r["category_id"] for r in listed] == [5, 2, 1]
    one = det.to_coco_results(_detections()[2], 99)                            # one image's Detections with its id
    assert one == [{"image_id": 99, "category_id": 0, "bbox": [1.0, 2.0, 3.0, 4.0], "score": 0.5}]
    assert det.to_coco_results([], []) == []
    with pytest.raises(ValueError, match="image ids"):
        det.to_coco_results(_detections(), [1, 2])


def test_to_coco_results_needs_xywh():
    from detr_tf.inference import Detector
    for fmt in ("xyxy", "yxyx", "xy_center"):
        with pytest.raises(ValueError, match="xywh"):
            Detector(None, _Cfg(), bbox_format=fmt).to_coco_results(_detections(), [1, 2, 3])


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def _outputs(B=2, Q=5, C=4):
    return {"pred_logits": torch.zeros(B, Q, C), "pred_boxes": torch.zeros(B, Q, 4)}


def test_detect_batched_argument_errors():
    from detr_tf.inference import detect_batched
    sizes = [(4, 4), (4, 4)]
    with pytest.raises(RuntimeError, match="GPU"):
        detect_batched(_outputs(), sizes, 3)                                   # CPU tensors: no eager fallback
    with pytest.raises(RuntimeError, match="max_detections"):
        detect_batched(_outputs(Q=5), sizes, 3, max_detections=6)
    with pytest.raises(RuntimeError, match="max_detections"):
        detect_batched(_outputs(), sizes, 3, max_detections=0)
    with pytest.raises(RuntimeError, match="bbox_format"):
        detect_batched(_outputs(), sizes, 3, bbox_format="cxcywh")
    for bad in (float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="finite"):
            detect_batched(_outputs(), sizes, 3, score_threshold=bad)
    with pytest.raises(RuntimeError, match="pred_boxes"):
        detect_batched({"pred_logits": torch.zeros(2, 5, 4), "pred_boxes": torch.zeros(2, 6, 4)}, sizes, 3)


def test_detector_argument_errors():
    from detr_tf.inference import Detector
    cfg = _Cfg()
    assert Detector(None, cfg).background_class == 4                           # config.background_class
    assert Detector(None, cfg, background_class=7).background_class == 7
    d = Detector(None, cfg)
    assert (d.score_threshold, d.max_detections, d.bbox_format, d.resize, d.shortest_side, d.max_size, d.canvas) == \
        (0.7, 100, "xyxy", "shortest_side", 800, 1333, None)
    with pytest.raises(RuntimeError, match="bbox_format"):
        Detector(None, cfg, bbox_format="corners")
    with pytest.raises(RuntimeError, match="max_detections"):
        Detector(None, cfg, max_detections=0)
    with pytest.raises(RuntimeError, match="finite"):
        Detector(None, cfg, score_threshold=float("nan"))
    with pytest.raises(ValueError, match="resize"):
        Detector(None, cfg, resize="stretch")
    with pytest.raises(ValueError, match="interpolation"):
        Detector(None, cfg, interpolation="lanczos")
    with pytest.raises(ValueError, match="interpolation"):
        Detector(None, cfg, resize="fixed", interpolation="area")              # the fixed-size input stage has no area filter

    class NoBackground:
        normalized_method, image_size = "torch_resnet", (64, 96)
    with pytest.raises(ValueError, match="background_class"):
        Detector(None, NoBackground())

    fixed = Detector(None, cfg, resize="fixed")
    a, b = np.zeros((48, 64, 3), np.uint8), np.zeros((64, 48, 3), np.uint8)
    with pytest.raises(ValueError, match="ONE size"):
        fixed([a, b])                                                          # raised before the device is touched
    for bad in ([], np.zeros((48, 64, 3), np.float32), [np.zeros((48, 64), np.uint8)], [np.zeros((48, 64, 4), np.uint8)]):
        with pytest.raises(TypeError, match="uint8"):
            fixed(bad)


def test_detector_records_are_the_loaders_evaluation_records():
    """resize="shortest_side" draws transformation.eval_record, the record of the loaders' "shortest_side" mode."""
    from detr_tf.data import transformation as T
    from detr_tf.inference import Detector
    det = Detector(None, _Cfg(), shortest_side=64, max_size=96, interpolation="linear")
    imgs = [np.zeros((96, 128, 3), np.uint8), np.zeros((120, 80, 3), np.uint8), np.zeros((50, 300, 3), np.uint8)]
    recs = det.records(imgs)
    assert recs == [T.eval_record(96, 128, 64, 96), T.eval_record(120, 80, 64, 96), T.eval_record(50, 300, 64, 96)]
    assert [(r.hd, r.wd) for r in recs] == [(64, 85), (96, 64), (16, 96)]
    assert Detector(None, _Cfg(), shortest_side=64, max_size=96).records(imgs[:1])[0].interp == T.CUBIC


# ---- the C entry point ---------------------------------------------------------------------------------------------------------
def test_detect_symbol_declared_exported_appended():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    name = "detr_hip_detect"
    assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9 and "#define DETR_HIP_ABI_VERSION 9" in hdr
    assert hdr.index("detr_detect_desc;") > hdr.index("detr_hip_conv3x3_dilated(")          # appended, behind the newest entry


def test_detect_desc_layout_matches_the_header():
    _hip, lib = _lib()
    assert abi_header.header_structs()["detr_detect_desc"] == list(_hip.DetectDesc._fields_)    # names, order and types of the C declaration
    assert {w: S for w, S in _hip.LAYOUT_STRUCTS.items() if 100 <= w < 200} == {100: _hip.DetectDesc}
    _hip.check_struct_layouts(lib)                     # the load-time check covers it; library, unknown ids, drift: test_abi_layout_cpu.py


def test_detect_rejects_bad_arguments_without_a_gpu():
    _hip, lib = _lib()
    fake = 4096                                   # never dereferenced: every call below fails its checks first
    ptrs = ("logits", "boxes", "sizes", "out_boxes", "out_labels", "out_scores", "out_query", "counts")

    def desc(**kw):
        d = _hip.DetectDesc()
        d.B, d.Q, d.C = 2, 100, 92
        for n in ptrs:
            setattr(d, n, fake)
        d.sL_b, d.sL_q, d.sB_b, d.sB_q = 9200, 92, 400, 4
        d.background_class, d.score_threshold, d.max_detections, d.bbox_format, d.clip = 91, 0.7, 100, 1, 1
        for n, v in kw.items():
            setattr(d, n, v)
        return d

    def rejected(d, text):
        rc = lib.detr_hip_detect(ctypes.byref(d) if d is not None else None, None)
        msg = lib.detr_hip_last_error().decode()
        assert rc < 0 and text in msg, (rc, msg, text)

    rejected(None, "null descriptor")
    for n in ptrs:
        rejected(desc(**{n: None}), "null operand")
    for kw in (dict(B=0), dict(B=-1), dict(Q=0), dict(Q=1025), dict(C=0), dict(C=-2)):
        rejected(desc(**kw), "bad shape")
    for kw in (dict(sL_q=91), dict(sB_q=3), dict(sL_b=-1), dict(sB_b=-400)):
        rejected(desc(**kw), "strides")
    for k in (0, -1, 101):
        rejected(desc(max_detections=k), "max_detections")
    for f in (-1, 4):
        rejected(desc(bbox_format=f), "bbox_format")
    for c in (-1, 2):
        rejected(desc(clip=c), "clip")
    for t in (float("nan"), float("inf"), float("-inf")):
        rejected(desc(score_threshold=t), "not finite")
    rejected(desc(out_boxes=fake + 4), "16-byte aligned")
