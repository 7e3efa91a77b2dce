"""COCO-protocol evaluation, host side (no GPU): the C entry point detr_hip_coco_match (symbol, the descriptor's array sizes against the
header, every argument check), COCOAccumulator against the loop oracle tests/coco_eval_ref.py, the
hand-computed answers that pin the COCO semantics, and the loader's keep_crowd / with_meta / shuffle / drop_remainder."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abi_header  # noqa: E402
import coco_eval_ref as CR  # noqa: E402
from map_match_ref import targets_to_yxyx  # noqa: E402


_lib = abi_header.hip_lib


# ---- the C entry point -----------------------------------------------------------------------------------------------------------
def test_coco_match_symbol_declared_exported_appended():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    name = "detr_hip_coco_match"
    assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9 and "#define DETR_HIP_ABI_VERSION 9" in hdr
    assert hdr.index("detr_coco_match_desc;") > hdr.index("int detr_hip_detect(")               # appended, behind the newest entry
    assert hdr.index("int detr_hip_coco_match(") > hdr.index("detr_coco_match_desc;")
    order = list(_hip._SIGNATURES)                                          # appended in this order
    assert order.index("detr_hip_detect") < order.index(name) < order.index("detr_hip_overlay")
    assert (_hip.COCO_MAX_THR, _hip.COCO_MAX_AREA) == (10, 4) and "#define DETR_COCO_MAX_THR 10" in hdr and "#define DETR_COCO_MAX_AREA 4" in hdr
    assert set(_hip.COCO_BAD) == {1, 2, 4, 8, 16} and "#define DETR_COCO_BAD_SIZE 16" in hdr


def test_coco_match_desc_layout_matches_the_header():
    _hip, _ = _lib()
    assert _hip.LAYOUT_STRUCTS[800] is _hip.CocoMatchDesc                      # sizeof / offsetof through gcc, for every struct: test_abi_layout_cpu.py
    fields = dict(abi_header.header_structs()["detr_coco_match_desc"])        # the header's arrays, DETR_COCO_MAX_* resolved
    thr_bytes, area_bytes = ctypes.sizeof(fields["thresholds"]), ctypes.sizeof(fields["area_ranges"])
    assert thr_bytes == 80 == ctypes.sizeof(_hip.CocoMatchDesc().thresholds) and area_bytes == 64 == ctypes.sizeof(_hip.CocoMatchDesc().area_ranges)


def test_coco_match_rejects_bad_arguments_without_a_gpu():
    _hip, lib = _lib()
    fake = 4096                                   # never dereferenced: every call below fails its checks first
    ins = ("boxes", "labels", "scores", "counts", "t_bbox", "t_class", "t_crowd", "t_area", "sizes")
    outs = ("rec_score", "rec_class", "rec_rank", "rec_flags", "npig", "status")

    def desc(**kw):
        d = _hip.CocoMatchDesc()
        d.B, d.Q, d.R, d.nb_class, d.n_thr, d.n_area = 4, 100, 100, 92, 10, 4
        for n in ins + outs:
            setattr(d, n, fake)
        d.sD_b, d.sT_b, d.sC_b, d.sM_b = 100, 400, 100, 100
        for t, th in enumerate(CR.THRESHOLDS):
            d.thresholds[t] = th
        for a, (lo, hi) in enumerate(CR.AREA_RANGES):
            d.area_ranges[2 * a], d.area_ranges[2 * a + 1] = lo, hi
        for n, v in kw.items():
            setattr(d, n, v)
        return d

    def rejected(d, text):
        rc = lib.detr_hip_coco_match(ctypes.byref(d) if d is not None else None, None)
        msg = lib.detr_hip_last_error().decode()
        assert rc < 0 and text in msg and msg.startswith("coco_match:"), (rc, msg, text)

    rejected(None, "null descriptor")
    for n in ins:
        rejected(desc(**{n: None}), "null operand (boxes")
    for n in outs:
        rejected(desc(**{n: None}), "null operand (rec_score")
    for kw in (dict(B=0), dict(B=-3), dict(B=65536), dict(Q=0), dict(Q=-1), dict(Q=1025), dict(R=0), dict(R=-1), dict(R=257)):
        rejected(desc(**kw), "bad shape")
    for c in (0, -5):
        rejected(desc(nb_class=c), "nb_class")
    for t in (0, -1, 11):
        rejected(desc(n_thr=t), "thresholds")
    for a in (0, -1, 5):
        rejected(desc(n_area=a), "area ranges")
    for i, v in ((3, float("nan")), (9, float("inf")), (0, float("-inf"))):
        d = desc()
        d.thresholds[i] = v
        rejected(d, "not finite")
    for i, v in ((0, float("nan")), (3, float("inf")), (5, 10.0)):             # range 2 becomes [1024, 10]: lo > hi
        d = desc()
        d.area_ranges[i] = v
        rejected(d, "area range")
    for kw in (dict(sD_b=99), dict(sT_b=399), dict(sC_b=99), dict(sM_b=99), dict(sD_b=-100)):
        rejected(desc(**kw), "batch strides")
    rejected(desc(boxes=fake + 4), "16-byte aligned")


# ---- accumulator against the oracle ----------------------------------------------------------------------------------------------
def _host_accumulate(acc, bt):
    for b in range(len(bt["counts"])):
        k, n = int(bt["counts"][b]), int(bt["t_bbox"][b, 0, 0])
        acc.add_image(bt["boxes"][b, :k], bt["labels"][b, :k], bt["scores"][b, :k], targets_to_yxyx(bt["t_bbox"][b, 1:1 + n]),
                      bt["t_class"][b, 1:1 + n, 0], bt["t_crowd"][b, 1:1 + n], bt["t_area"][b, 1:1 + n], bt["sizes"][b])


def _flat(recs, na):
    keep = np.concatenate([r[1].reshape(-1) for r in recs]) >= 0
    return (np.concatenate([r[0].reshape(-1) for r in recs])[keep], np.concatenate([r[1].reshape(-1) for r in recs])[keep],
            np.concatenate([r[2].reshape(-1) for r in recs])[keep], np.concatenate([r[3].reshape(na, -1) for r in recs], 1)[:, keep].T)


@pytest.mark.parametrize("B,Q,R,C", [(4, 100, 100, 92), (5, 40, 30, 6), (2, 12, 9, 3)])
def test_accumulator_equals_the_oracle_on_random_batches(B, Q, R, C):
    from detr_tf.loss.coco_eval import COCOAccumulator
    batches = CR.random_batches(B, Q, R, C, seed=100 * B + Q + C)
    acc, recs, npig = COCOAccumulator(C), [], np.zeros((C, 4), np.int64)
    for bt in batches:
        rs, rc, rr, rf, ng, status = CR.coco_match_ref(*CR.as_args(bt), C)
        assert status == 0 and rs.dtype == np.float32 and rc.dtype == np.int32 and rr.dtype == np.int32 and rf.dtype == np.uint32
        recs.append((rs, rc, rr, rf))
        npig += ng
        _host_accumulate(acc, bt)
    for got, want in zip(acc.records(), _flat(recs, 4)):                       # flags and counts: exactly equal
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got,
                                                          want.view(np.uint32) if want.dtype == np.float32 else want)
    assert np.array_equal(acc.npig, npig) and acc.npig.dtype == np.int64
    flags = acc.records()[3]
    assert (flags & 0x3FF).any() and (flags >> 16).any() and (acc.records()[2] > 0).any()      # matches, ignores and ranks occur
    stats, per_class, _, _ = CR.summarize_ref(recs, npig, C)
    res = acc.result()
    assert list(res)[:12] == list(CR.STAT_NAMES) and list(res)[12:] == ["per_class_AP"]
    for k in CR.STAT_NAMES:
        assert abs(res[k] - stats[k]) <= 1e-9, (k, res[k], stats[k])
    assert np.abs(np.array(res["per_class_AP"]) - np.array(per_class)).max() <= 1e-9
    assert 0 < res["AP"] < 1 and res["AR1"] <= res["AR10"] <= res["AR100"]
    # the same records pushed the device way (add_records) give the same result
    again = COCOAccumulator(C)
    for rs, rc, rr, rf in recs:
        again.add_records(rs, rc, rr, rf)
    again.npig = npig
    assert again.result() == res


def test_accumulator_equals_the_oracle_with_255_matched_ground_truths():
    """255 ground truths per image with detections on every quarter of the index range (the GPU test's dense case)."""
    from detr_tf.loss.coco_eval import COCOAccumulator
    bt, want, taken = CR.dense_case()
    CR.assert_every_chunk_matched(taken)
    acc = COCOAccumulator(3)
    _host_accumulate(acc, bt)
    for got, w in zip(acc.records(), _flat([want[:4]], 4)):
        assert got.dtype == w.dtype and np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got,
                                                       w.view(np.uint32) if w.dtype == np.float32 else w)
    assert np.array_equal(acc.npig, want[4])
    stats = CR.summarize_ref([want[:4]], want[4], 3)[0]
    res = acc.result()
    for k in CR.STAT_NAMES:
        assert abs(res[k] - stats[k]) <= 1e-9, (k, res[k], stats[k])
    assert 0 < res["AP"] < 1 and min(res[k] for k in CR.STAT_NAMES) > -1


def test_accumulator_other_thresholds_and_ranges():
    from detr_tf.loss.coco_eval import COCOAccumulator
    thr, rng_a = [0.3, 0.75], [[0, 1e10], [0, 5000]]
    bt = CR.random_batches(3, 30, 20, 4, seed=8)[1]
    acc = COCOAccumulator(4, thr, rng_a)
    _host_accumulate(acc, bt)
    rs, rc, rr, rf, ng, _ = CR.coco_match_ref(*CR.as_args(bt), 4, thr, rng_a)
    assert np.array_equal(acc.records()[3], _flat([(rs, rc, rr, rf)], 2)[3]) and np.array_equal(acc.npig, ng)
    stats = CR.summarize_ref([(rs, rc, rr, rf)], ng, 4, thr, rng_a)[0]
    res = acc.result()
    for k in CR.STAT_NAMES:
        assert abs(res[k] - stats[k]) <= 1e-9, k
    assert res["AP50"] == -1 and res["APm"] == -1 and res["AP75"] > -1          # no 0.5 threshold, no third range
    for bad in (dict(iou_thresholds=[0.5] * 11), dict(area_ranges=[[0, 1]] * 5), dict(iou_thresholds=[])):
        with pytest.raises(ValueError):
            COCOAccumulator(4, **bad)


# ---- hand-computed answers -------------------------------------------------------------------------------------------------------
SIZE = (100, 100)


def _acc(images, nb_class=3):
    """images: [(dets [(yxyx, class, score)], gts [(yxyx, class, crowd, area)])] on 100 x 100 images -> (COCOAccumulator, result)."""
    from detr_tf.loss.coco_eval import COCOAccumulator
    acc = COCOAccumulator(nb_class)
    for dets, gts in images:
        acc.add_image(np.array([d[0] for d in dets], np.float32).reshape(-1, 4), [d[1] for d in dets], [d[2] for d in dets],
                      np.array([g[0] for g in gts], np.float32).reshape(-1, 4), [g[1] for g in gts], [g[2] for g in gts],
                      [g[3] for g in gts], SIZE)
    return acc, acc.result()


def _close(res, **want):
    for k, v in want.items():
        assert abs(res[k] - v) <= 1e-9, (k, res[k], v)


BOX = [0.125, 0.125, 0.625, 0.625]                    # 50 x 50 pixels = 2500: `medium`


def test_hand_a_one_perfect_detection():
    _, res = _acc([([(BOX, 1, 0.9)], [(BOX, 1, 0, 2500.0)])])
    _close(res, AP=1, AP50=1, AP75=1, APm=1, AR1=1, AR10=1, AR100=1, ARm=1, APs=-1, APl=-1, ARs=-1, ARl=-1)
    assert res["per_class_AP"][0] == -1 and abs(res["per_class_AP"][1] - 1) <= 1e-9 and res["per_class_AP"][2] == -1


def test_hand_b_detections_inside_a_crowd_are_ignored():
    crowd = [0.5, 0.0, 1.0, 1.0]
    dets = [(BOX, 1, 0.5), ([0.75, 0.125, 0.875, 0.375], 1, 0.9), ([0.625, 0.5, 0.875, 0.75], 1, 0.8)]     # the crowd's score higher
    acc, res = _acc([(dets, [(BOX, 1, 0, 2500.0), (crowd, 1, 1, 5000.0)])])
    _close(res, AP=1, AR100=1)
    score, cls, rank, flags = acc.records()
    assert score.tolist() == [np.float32(0.9), np.float32(0.8), 0.5] and rank.tolist() == [0, 1, 2]
    assert flags[0, 0] == flags[1, 0] == 0x03FF03FF and flags[2, 0] == 0x000003FF            # matched + ignored twice; a plain match
    assert acc.npig[1].tolist() == [1, 0, 1, 0]                                              # the crowd is no positive


def test_hand_c_false_positive_above_the_true_positive():
    _, res = _acc([([([0.75, 0.75, 0.875, 0.875], 1, 0.9), (BOX, 1, 0.8)], [(BOX, 1, 0, 2500.0)])])
    _close(res, AP=0.5, AP50=0.5, AR100=1)


def test_hand_d_maxdets_cuts_per_class_and_image():
    other = [0.75, 0.75, 1.0, 1.0]
    _, res = _acc([([(BOX, 1, 0.9), (other, 1, 0.8)], [(BOX, 1, 0, 2500.0), (other, 1, 0, 625.0)])])
    _close(res, AR1=0.5, AR10=1, AR100=1, AP=1)


def test_hand_e_the_later_ground_truth_wins_a_tie():
    """Two identical ground truths are interchangeable, so which one a detection took cannot be seen.  Two ground truths of exactly
    equal IoU can tell: a detection between them (IoU 0.1875 / 0.3125 with both, exact binary fractions) takes the LATER index at
    threshold 0.5, so the second detection -- a copy of the later ground truth -- finds it used and has only IoU 1/3 with the other."""
    left, right, mid = [0.25, 0.125, 0.75, 0.625], [0.25, 0.375, 0.75, 0.875], [0.25, 0.25, 0.75, 0.75]
    acc, _ = _acc([([(mid, 1, 0.9), (right, 1, 0.8)], [(left, 1, 0, 2500.0), (right, 1, 0, 2500.0)])])
    flags = acc.records()[3]
    assert flags[0, 0] & 1 and not flags[1, 0] & 1
    acc, _ = _acc([([(mid, 1, 0.9), (left, 1, 0.8)], [(left, 1, 0, 2500.0), (right, 1, 0, 2500.0)])])
    flags = acc.records()[3]
    assert flags[0, 0] & 1 and flags[1, 0] & 1                                               # the earlier one was left free
    acc, res = _acc([([(BOX, 1, 0.9), (BOX, 1, 0.9)], [(BOX, 1, 0, 2500.0), (BOX, 1, 0, 2500.0)])])      # identical: both match
    assert acc.records()[3][:, 0].tolist() == [0x3FF, 0x3FF] and abs(res["AP"] - 1) <= 1e-9


def test_hand_f_a_regular_ground_truth_is_preferred_to_a_crowd():
    det, crowd = [0.25, 0.25, 0.75, 0.75], [0.0, 0.0, 1.0, 1.0]                              # IoU 1 with the crowd (inside it)
    regular = [0.25, 0.125, 0.75, 0.625]                                                     # IoU 0.6, listed AFTER the crowd
    acc, res = _acc([([(det, 1, 0.9)], [(crowd, 1, 1, 9000.0), (regular, 1, 0, 2500.0)])])
    word = int(acc.records()[3][0, 0])
    assert word & 0x3FF == 0x3FF                                                             # matched at every threshold:
    assert word & 0b11 == 0b11 and not (word >> 16) & 0b11                                   # the regular one at 0.5 and 0.55 ...
    assert (word >> 16) & 0x3F8 == 0x3F8                                                     # ... from 0.65 on only the crowd is left
    _close(res, AP50=1)


def test_hand_g_an_unmatched_detection_outside_a_range():
    big = [0.0, 0.0, 1.0, 1.0]                                                               # 10000 pixels: `large`
    acc, res = _acc([([(big, 1, 0.9), (BOX, 1, 0.8)], [(BOX, 1, 0, 2500.0)])])
    flags = acc.records()[3]
    assert flags[0].tolist() == [0, 0x03FF0000, 0x03FF0000, 0]                               # ignored in small / medium only
    _close(res, AP=0.5, APm=1)                                                               # a false positive in `all`


# ---- loader --------------------------------------------------------------------------------------------------------------------
class _Cfg:
    image_size = (48, 64)
    normalized_method = "torch_resnet"
    background_class = 0

    class data:
        data_dir = None


def _make_coco(tmp_path):
    """Five images: 0 two boxes, 1 a box and a crowd, 2 no annotation, 3 a box, a degenerate (zero-width) box and a third box
    without an `area` field, 4 one box."""
    from PIL import Image
    img_dir = tmp_path / "images"
    img_dir.mkdir()
    rng = np.random.default_rng(0)
    images, anns = [], []
    boxes = {0: [([5, 6, 20, 10], 0, 150.0), ([30, 8, 12, 30], 0, 300.5)], 1: [([4, 4, 10, 10], 0, 80.0), ([20, 10, 40, 30], 1, 1000.0)], 2: [],
             3: [([2, 3, 30, 20], 0, 500.0), ([10, 10, 0, 15], 0, 7.0), ([40, 20, 8, 16], 0, None)], 4: [([1, 1, 50, 40], 0, 1800.0)]}
    for i in range(5):
        h, w = 48 + 6 * i, 64 + 8 * i
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8), "RGB").save(img_dir / f"{i}.png")
        images.append({"id": 500 + i, "file_name": f"{i}.png", "height": h, "width": w})
        for k, (bb, crowd, area) in enumerate(boxes[i]):
            a = {"id": 10 * i + k, "image_id": 500 + i, "category_id": [1, 3, 7][(i + k) % 3], "iscrowd": crowd, "bbox": [float(v) for v in bb]}
            if area is not None:
                a["area"] = area
            anns.append(a)
    cats = [{"id": 1, "name": "person"}, {"id": 3, "name": "car"}, {"id": 7, "name": "train"}]
    ann_file = tmp_path / "ann.json"
    ann_file.write_text(json.dumps({"images": images, "annotations": anns, "categories": cats}))
    return str(ann_file), str(img_dir)


def test_loader_defaults_are_unchanged(tmp_path):
    import inspect
    from detr_tf.data import load_coco_dataset
    from detr_tf.data.coco import coco_samples
    from detr_tf.data.loader import DetectionDataset, Sample
    ann_file, img_dir = _make_coco(tmp_path)
    samples, names, background = coco_samples(ann_file, img_dir)
    assert [os.path.basename(s.path) for s in samples] == ["0.png", "3.png", "4.png"] and background == 8      # crowd and empty image left out
    old = Sample("p", np.zeros((1, 4), np.float32), np.zeros((1, 1), np.int64))                                  # built the old way
    assert old.crowd is None and old.area is None and old.image_id is None and old.size is None and len(old[:3]) == 3
    for fn, names_ in ((coco_samples, ["keep_crowd"]), (load_coco_dataset, ["keep_crowd", "with_meta", "shuffle", "drop_remainder"]),
                       (DetectionDataset.__init__, ["with_meta", "shuffle", "drop_remainder"])):
        sig = inspect.signature(fn).parameters
        assert [sig[n].default for n in names_] == [{"keep_crowd": False, "with_meta": False, "shuffle": True, "drop_remainder": True}[n] for n in names_]
    ds, _ = load_coco_dataset(_Cfg(), 2, augmentation=False, ann_file=ann_file, img_dir=img_dir, seed=3)
    plain = DetectionDataset([Sample(s.path, s.boxes, s.classes) for s in samples], _Cfg(), 2, False, seed=3)
    a, b = list(ds.host_batches()), list(plain.host_batches())
    assert len(ds) == 1 and len(a) == len(b) == 1 and len(a[0]) == 2
    for x, y in zip(a[0], b[0]):
        assert len(x) == len(y) == 4 and np.array_equal(x[0], y[0]) and x[1] == y[1] and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])
    order = np.random.default_rng(3).permutation(3)[:2]                                     # still one shuffled epoch, remainder dropped
    assert [x[0].shape for x in a[0]] == [(48 + 6 * i, 64 + 8 * i, 3) for i in np.array([0, 3, 4])[order]]


def test_loader_keep_crowd_meta_order_and_short_batch(tmp_path):
    import torch
    from detr_tf.data import load_coco_dataset
    from detr_tf.data.coco import coco_samples
    from detr_tf.data.loader import DetectionDataset
    ann_file, img_dir = _make_coco(tmp_path)
    samples, _, _ = coco_samples(ann_file, img_dir, keep_crowd=True)
    assert [s.image_id for s in samples] == [500, 501, 503, 504]                            # the crowd image kept, the empty one not
    s1, s3 = samples[1], samples[2]
    assert s1.crowd.dtype == np.uint8 and s1.crowd.tolist() == [0, 1] and s1.area.dtype == np.float32 and s1.area.tolist() == [80.0, 1000.0]
    assert s1.size == (54, 72) and s3.size == (66, 88)
    assert s3.area.tolist() == [500.0, 7.0, 128.0]                                          # w * h where the file has no area
    for mode in (False, None, "shortest_side"):
        ds, _ = load_coco_dataset(_Cfg(), 3, augmentation=mode, ann_file=ann_file, img_dir=img_dir, keep_crowd=True, with_meta=True,
                                  shuffle=False, drop_remainder=False, scales=(48,), max_size=96)
        assert len(ds) == 2
        batches = list(ds.host_batches())
        assert [len(b) for b in batches] == [3, 1]                                          # the short last batch
        assert [e[6] for b in batches for e in b] == [500, 501, 503, 504]                   # file order
        assert [e[7] for b in batches for e in b] == [(48, 64), (54, 72), (66, 88), (72, 96)]
        e3 = batches[0][2]                                                                  # image 3: the degenerate box
        if mode is None:
            assert len(e3[2]) == 3 and e3[4].tolist() == [0, 0, 0] and e3[5].tolist() == [500.0, 7.0, 128.0]
        else:                                                                               # is dropped; the metadata follows
            assert len(e3[2]) == 2 and e3[5].tolist() == [500.0, 128.0] and e3[3].reshape(-1).tolist() == s3.classes.reshape(-1)[[0, 2]].tolist()
        for b in batches:                                                                   # rows line up with the padded targets
            t_bbox = torch.zeros(len(b), 100, 4)
            for i, e in enumerate(b):
                t_bbox[i, 0, 0] = len(e[2])
                t_bbox[i, 1:1 + len(e[2])] = torch.from_numpy(e[2])
            meta = DetectionDataset._meta(b, t_bbox)
            assert meta["crowd"].dtype == torch.uint8 and tuple(meta["crowd"].shape) == (len(b), 100)
            assert meta["area"].dtype == torch.float32 and tuple(meta["area"].shape) == (len(b), 100)
            assert meta["size"].dtype == torch.int32 and meta["size"].tolist() == [list(e[7]) for e in b]
            assert meta["image_id"].dtype == torch.int64 and meta["image_id"].tolist() == [e[6] for e in b]
            for i, e in enumerate(b):
                n = int(t_bbox[i, 0, 0])
                assert meta["area"][i, 1:1 + n].tolist() == e[5].tolist() and meta["crowd"][i, 1:1 + n].tolist() == e[4].tolist()
                assert not meta["area"][i, 0] and not meta["area"][i, 1 + n:].any() and not meta["crowd"][i, 1 + n:].any()
        e1 = batches[0][1]
        assert e1[4].tolist() == [0, 1] and e1[5].tolist() == [80.0, 1000.0]


def test_loader_metadata_follows_a_transform_that_drops_and_reorders(tmp_path, monkeypatch):
    from detr_tf.data import transformation as T
    from detr_tf.data.coco import coco_samples
    from detr_tf.data.loader import DetectionDataset
    ann_file, img_dir = _make_coco(tmp_path)
    samples, _, _ = coco_samples(ann_file, img_dir, keep_crowd=True)
    real = T.transform_boxes

    def reversing(b, c, h0, w0, rec, size):                                                 # keeps what the real one keeps, reversed
        boxes, cls = real(b, c, h0, w0, rec, size)
        return boxes[::-1].copy(), np.asarray(cls)[::-1].copy()

    monkeypatch.setattr(T, "transform_boxes", reversing)
    ds = DetectionDataset(samples, _Cfg(), 4, False, with_meta=True, shuffle=False, drop_remainder=False)
    (batch,) = list(ds.host_batches())
    e3 = batch[2]
    assert e3[5].tolist() == [128.0, 500.0] and e3[3].reshape(-1).tolist() == samples[2].classes.reshape(-1)[[2, 0]].tolist()
    assert batch[1][4].tolist() == [1, 0] and batch[1][5].tolist() == [1000.0, 80.0]


def test_loader_with_meta_keeps_an_image_that_loses_all_its_boxes(tmp_path):
    """Its detections are false positives of the evaluation; the training / reference path still skips such an image."""
    from detr_tf.data.coco import coco_samples
    from detr_tf.data.loader import DetectionDataset
    ann_file, img_dir = _make_coco(tmp_path)
    samples, _, _ = coco_samples(ann_file, img_dir, keep_crowd=True)
    flat = samples[3]._replace(boxes=np.array([[0.5, 0.5, 0.0, 0.2]], np.float32))        # image 504: one zero-width box
    samples = samples[:3] + [flat]
    kept = list(DetectionDataset(samples, _Cfg(), 4, False, with_meta=True, shuffle=False, drop_remainder=False).host_batches())
    assert [e[6] for e in kept[0]] == [500, 501, 503, 504]
    last = kept[0][3]
    assert last[2].shape == (0, 4) and len(last[3]) == 0 and len(last[4]) == 0 and len(last[5]) == 0 and last[7] == (72, 96)
    skipped = list(DetectionDataset(samples, _Cfg(), 3, False, shuffle=False).host_batches())
    assert len(skipped) == 1 and len(skipped[0]) == 3 and all(len(e) == 4 and len(e[2]) > 0 for e in skipped[0])


def test_loader_value_errors(tmp_path):
    from detr_tf.data import load_coco_dataset
    from detr_tf.data.coco import coco_samples
    from detr_tf.data.loader import DetectionDataset, Sample
    ann_file, img_dir = _make_coco(tmp_path)
    kw = dict(ann_file=ann_file, img_dir=img_dir)
    for mode in (True, "multiscale"):
        with pytest.raises(ValueError, match="keep_crowd"):
            load_coco_dataset(_Cfg(), 2, augmentation=mode, keep_crowd=True, **kw)
        with pytest.raises(ValueError, match="with_meta"):
            load_coco_dataset(_Cfg(), 2, augmentation=mode, with_meta=True, **kw)
        with pytest.raises(ValueError, match="crowd"):
            DetectionDataset(coco_samples(ann_file, img_dir, keep_crowd=True)[0], _Cfg(), 2, mode)
        load_coco_dataset(_Cfg(), 2, augmentation=mode, **kw)                               # the training path itself is untouched
    with pytest.raises(ValueError, match="with_meta"):
        DetectionDataset([Sample("p", np.zeros((1, 4), np.float32), np.zeros((1, 1), np.int64))], _Cfg(), 1, False, with_meta=True)


def test_eval_model_protocol_argument_without_a_gpu():
    from detr_tf.evaluation import eval_model
    from detr_tf.loss.coco_eval import DeviceCOCOAccumulator
    with pytest.raises(ValueError, match="protocol"):
        eval_model(None, None, ["a"], [], protocol="voc")
    with pytest.raises(TypeError, match="with_meta"):
        eval_model(None, None, ["a"], [(1, 2, 3)], protocol="coco")
    with pytest.raises(TypeError, match="meta"):
        eval_model(None, None, ["a"], [(1, 2, 3, None)], protocol="coco")
    with pytest.raises(RuntimeError):
        DeviceCOCOAccumulator(3, device="cpu")
    empty = eval_model(None, None, ["a", "b"], [], protocol="coco", print_result=False)
    assert [empty[k] for k in CR.STAT_NAMES] == [-1.0] * 12 and empty["per_class_AP"] == [-1.0, -1.0]
    assert eval_model.__kwdefaults__ == {"protocol": "reference"} and eval_model.__defaults__[-1] == "host"


def test_summary_lines(capsys):
    from detr_tf.loss.coco_eval import COCOAccumulator
    acc = COCOAccumulator(2)
    acc.add_image(np.array([BOX], np.float32), [1], [0.9], np.array([BOX], np.float32), [1], [0], [2500.0], SIZE)
    acc.result(print_result=True)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 1.000"
    assert lines[3] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = -1.000"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 1.000"
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000"
