"""Sliced inference without a GPU: the window rule of transformation.tile_records, the NumPy restatement of the merge on hand-worked
cases (tests/tile_merge_ref.py is the reference the GPU tests compare detr_hip_tile_merge with, so it is pinned here first), the
C entry point's declaration / export / descriptor layout / argument checks, and the Detector's argument validation."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import abi_header
import tile_merge_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


_lib = abi_header.hip_lib


# ---- tile_records --------------------------------------------------------------------------------------------------------------
IMAGES = [(1, 1), (7, 5), (96, 128), (480, 640), (3000, 4000), (333, 1999)]
GRIDS = [(1, 1), (1, 2), (2, 2), (3, 4)]
OVERLAPS = [0, 0.2, 0.5]


@pytest.mark.parametrize("h0,w0", IMAGES)
@pytest.mark.parametrize("rows,cols", GRIDS)
@pytest.mark.parametrize("overlap", OVERLAPS)
def test_tile_records_properties(h0, w0, rows, cols, overlap):
    from detr_tf.data import transformation as T
    if rows > h0 or cols > w0:
        with pytest.raises(ValueError, match="does not fit"):
            T.tile_records(h0, w0, rows, cols, overlap)
        return
    recs = T.tile_records(h0, w0, rows, cols, overlap, short=64, max_size=96, interp=T.CUBIC)
    assert recs[0] == T.eval_record(h0, w0, 64, 96, T.CUBIC)                       # include_full: record 0 is the whole image
    tiles = recs[1:]
    assert tiles == T.tile_records(h0, w0, rows, cols, overlap, short=64, max_size=96, interp=T.CUBIC, include_full=False)
    assert len(tiles) == rows * cols
    for t in tiles:
        T.check_padded_record(t)
        assert (t.h0, t.w0, t.flip, t.interp) == (h0, w0, False, T.CUBIC)
    hc, wc = tiles[0].hc, tiles[0].wc
    assert {(t.hc, t.wc) for t in tiles} == {(hc, wc)}                              # one window size ...
    assert {(t.hd, t.wd) for t in tiles} == {T.target_size(hc, wc, 64, 96)}         # ... so one destination size
    ys = [tiles[r * cols].y0 for r in range(rows)]
    xs = [tiles[c].x0 for c in range(cols)]
    assert [(t.y0, t.x0) for t in tiles] == [(y, x) for y in ys for x in xs]        # a grid, row-major
    frac = Fraction(repr(float(overlap)))
    for origins, size, length, n in ((ys, hc, h0, rows), (xs, wc, w0, cols)):
        assert origins[0] == 0 and origins[-1] + size == length                     # coverage: from 0 to exactly the far edge
        steps = np.diff(origins)
        assert (steps >= 0).all()
        if n > 1:
            assert steps.max() - steps.min() <= 1                                   # evenly spaced up to integer rounding
            shared = size - steps.max()
            assert shared >= frac.numerator * size // frac.denominator and shared >= math.floor(overlap * size) and shared >= 0
            if size > -(-length // n):                                              # the smallest such window: one pixel less fails
                s = size - 1
                assert s - -(-(length - s) // (n - 1)) < frac.numerator * s // frac.denominator


def test_tile_records_one_by_one_is_the_eval_record():
    from detr_tf.data import transformation as T
    for h0, w0 in IMAGES:
        assert T.tile_records(h0, w0, 1, 1, include_full=False) == [T.eval_record(h0, w0)]
        assert T.tile_records(h0, w0, 1, 1, 0.5, 480, 640, T.CUBIC, False) == [T.eval_record(h0, w0, 480, 640, T.CUBIC)]
        assert T.tile_records(h0, w0, 1, 1) == [T.eval_record(h0, w0)] * 2


def test_tile_records_rejects_bad_arguments():
    from detr_tf.data import transformation as T
    for rows, cols in ((8, 1), (1, 6), (0, 1), (1, 0), (-1, 2)):
        with pytest.raises(ValueError):
            T.tile_records(7, 5, rows, cols)
    for overlap in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="overlap"):
            T.tile_records(96, 128, 2, 2, overlap)
    with pytest.raises(ValueError):
        T.tile_records(0, 5, 1, 1)


# ---- the reference merge on hand-worked cases ----------------------------------------------------------------------------------
def _img(entries, size=(100, 100), **kw):
    """entries: [(tile, score, label, (x0, y0, x1, y1) in image pixels)] with every tile a whole-image window of `size`, so that
    the mapping is the identity up to the scale; -> the reference's result."""
    H, W = size
    T_ = 1 + max(e[0] for e in entries)
    Q = max(sum(1 for e in entries if e[0] == t) for t in range(T_))
    scores, labels, boxes = np.zeros((T_, Q), F), np.full((T_, Q), 9), np.zeros((T_, Q, 4), F)
    at = [0] * T_
    for t, s, l, (x0, y0, x1, y1) in entries:
        q = at[t]
        at[t] += 1
        scores[t, q], labels[t, q] = s, l
        boxes[t, q] = ((x0 + x1) / 2 / W, (y0 + y1) / 2 / H, (x1 - x0) / W, (y1 - y0) / H)
    windows = np.array([(0, 0, H, W)] * T_, np.int32)
    return M.merge_image(scores, labels, boxes, windows, size, 9, **kw)


def test_ref_identical_boxes_the_lower_tile_wins():
    b, l, s, q, t, n = _img([(0, 0.5, 1, (10, 10, 50, 50)), (1, 0.5, 1, (10, 10, 50, 50)), (2, 0.5, 1, (10, 10, 50, 50))])
    assert n == 3 and t.tolist() == [0] and q.tolist() == [0] and np.allclose(b, [[10, 10, 50, 50]], rtol=1e-6)
    b, l, s, q, t, n = _img([(0, 0.5, 1, (10, 10, 50, 50)), (1, 0.75, 1, (10, 10, 50, 50))])       # unless a later one scores higher
    assert t.tolist() == [1] and s.tolist() == [0.75]


def test_ref_the_threshold_is_strict():
    pair = [(0, 0.75, 1, (0, 0, 2, 1)), (0, 0.5, 1, (0, 0, 1, 1))]                  # IoU = 1 / 2 exactly
    assert M.measure((0, 0, 2, 1), (0, 0, 1, 1), "iou") == 0.5
    assert _img(pair, size=(4, 4), nms_threshold=0.5)[3].tolist() == [0, 1]         # kept: 0.5 > 0.5 is false
    assert _img(pair, size=(4, 4), nms_threshold=0.4999)[3].tolist() == [0]


def test_ref_labels_and_class_agnostic():
    pair = [(0, 0.75, 1, (10, 10, 50, 50)), (0, 0.5, 2, (10, 10, 50, 50))]
    assert _img(pair)[1].tolist() == [1, 2]
    assert _img(pair, class_agnostic=True)[1].tolist() == [1]


def test_ref_ios_drops_a_part_box_that_iou_keeps():
    pair = [(0, 0.75, 1, (0, 0, 80, 80)), (1, 0.5, 1, (40, 40, 80, 80))]            # a quarter of the object, inside it: IoU 0.25, IoS 1
    assert M.measure((0, 0, 80, 80), (40, 40, 80, 80), "iou") == 0.25 and M.measure((0, 0, 80, 80), (40, 40, 80, 80), "ios") == 1.0
    assert _img(pair, match="iou")[4].tolist() == [0, 1]
    assert _img(pair, match="ios")[4].tolist() == [0]


def test_ref_zero_area_and_greedy_order():
    assert M.measure((5, 5, 5, 5), (5, 5, 5, 5), "iou") == 0.0 and M.measure((5, 5, 5, 9), (0, 0, 9, 9), "ios") == 0.0
    # A suppresses B, B would have suppressed C, A does not touch C: C survives
    chain = [(0, 0.9, 1, (0, 0, 40, 10)), (0, 0.8, 1, (15, 0, 55, 10)), (0, 0.7, 1, (30, 0, 70, 10))]
    assert M.measure((0, 0, 40, 10), (15, 0, 55, 10), "iou") > 0.4 > M.measure((0, 0, 40, 10), (30, 0, 70, 10), "iou")
    assert _img(chain, nms_threshold=0.4)[3].tolist() == [0, 2]
    assert _img(chain, nms_threshold=0.4, max_detections=1)[3].tolist() == [0]


def test_ref_edge_rule_drops_only_at_interior_edges():
    size = (100, 200)
    windows = np.array([(0, 0, 100, 120), (0, 80, 100, 120), (0, 0, 100, 200)], np.int32)   # left tile, right tile, the whole image
    # one box per tile, given in tile-normalised (cx, cy, w, h): it touches the tile's right edge, top edge and bottom edge
    right = np.array([[[0.9, 0.5, 0.2, 1.0]]] * 3, F)
    scores, labels = np.full((3, 1), 0.5, F), np.ones((3, 1), int)
    kw = dict(score_threshold=0.1, nms_threshold=1.0)
    assert M.merge_image(scores, labels, right, windows, size, 9, **kw)[4].tolist() == [0, 1, 2]          # no margin: nothing drops
    # margin 4: tile 0's right edge (x = 120) is interior -> dropped; tile 1's right edge is the image border, its left edge (x = 80)
    # is 96 px away, top and bottom are the image border -> kept; the whole image never drops
    assert M.merge_image(scores, labels, right, windows, size, 9, edge_margin=4.0, **kw)[4].tolist() == [1, 2]
    left = np.array([[[0.1, 0.5, 0.2, 0.5]]] * 3, F)                                # touches the tile's left edge
    assert M.merge_image(scores, labels, left, windows, size, 9, edge_margin=4.0, **kw)[4].tolist() == [0, 2]
    # a corner BEYOND an interior edge drops too; one exactly margin away drops, one a pixel further does not
    beyond = np.array([[[1.0, 0.5, 0.2, 0.5]]] * 3, F)
    assert M.merge_image(scores, labels, beyond, windows, size, 9, edge_margin=4.0, **kw)[4].tolist() == [1, 2]
    at = np.array([[[(116 - 12) / 120, 0.5, 0.2, 0.5]]], F)                          # x1 = 116 in tile 0: 120 - 116 = 4
    assert M.map_box(at[0, 0], windows[0])[1][2] == F(116)
    assert M.merge_image(scores[:1], labels[:1], at, windows[:1], size, 9, edge_margin=4.0, **kw)[5] == 0
    assert M.merge_image(scores[:1], labels[:1], at, windows[:1], size, 9, edge_margin=3.5, **kw)[5] == 1


def test_ref_mapping_threshold_background_cap_and_formats():
    size = (100, 200)
    windows = np.array([(20, 80, 50, 100)], np.int32)
    boxes = np.array([[[0.5, 0.5, 0.2, 0.4], [0.1, 0.1, 0.6, 0.6], [0.5, 0.5, 0.2, 0.4], [0.5, 0.5, 0.2, 0.4]]], F)
    scores = np.array([[0.75, 0.5, 0.25, np.nan]], F)
    labels = np.array([[1, 2, 3, 1]])
    out = {f: M.merge_image(scores, labels, boxes, windows, size, 3, score_threshold=0.3, bbox_format=f) for f in M.FORMATS}
    assert out["xyxy"][3].tolist() == [0, 1] and out["xyxy"][5] == 2                # background and NaN are no candidates
    np.testing.assert_allclose(out["xy_center"][0], [[130, 45, 20, 20], [90, 25, 60, 30]], rtol=1e-6)
    np.testing.assert_allclose(out["xyxy"][0], [[120, 35, 140, 55], [60, 10, 120, 40]], rtol=1e-6)
    np.testing.assert_allclose(out["yxyx"][0], [[35, 120, 55, 140], [10, 60, 40, 120]], rtol=1e-6)
    np.testing.assert_allclose(out["xywh"][0], [[120, 35, 20, 20], [60, 10, 60, 30]], rtol=1e-6)
    far = np.array([[[1.5, 0.5, 1.0, 0.4]]], F)                                     # x from 180 to 280: clipped to the IMAGE, not the tile
    np.testing.assert_allclose(M.merge_image(scores[:, :1], labels[:, :1], far, windows, size, 3)[0], [[180, 35, 200, 55]], rtol=1e-6)
    np.testing.assert_allclose(M.merge_image(scores[:, :1], labels[:, :1], far, windows, size, 3, clip=False)[0], [[180, 35, 280, 55]], rtol=1e-6)


# ---- the C entry point ---------------------------------------------------------------------------------------------------------
def test_tile_merge_symbol_declared_exported_appended():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    name = "detr_hip_tile_merge"
    assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9 and "#define DETR_HIP_ABI_VERSION 9" in hdr
    assert hdr.index("detr_tile_merge_desc;") > hdr.index("detr_hip_coco_match(")   # appended, behind the newest entry
    assert f"#define DETR_TILE_MAX_CAND {_hip.TILE_MAX_CAND}" in hdr and _hip.TILE_MAX_CAND >= 17 * 100
    assert sorted(_hip.TILE_BAD) == [int(re.search(rf"#define {n} (\d+)", hdr).group(1)) for n in ("DETR_TILE_OVER_CAP", "DETR_TILE_BAD_START")]


def test_tile_merge_desc_layout_matches_the_header():
    _hip, lib = _lib()
    assert abi_header.header_structs()["detr_tile_merge_desc"] == list(_hip.TileMergeDesc._fields_)   # names, order and types of the C declaration
    assert {w: S for w, S in _hip.LAYOUT_STRUCTS.items() if 200 <= w < 300} == {200: _hip.TileMergeDesc}
    _hip.check_struct_layouts(lib)                     # the load-time check covers it; library, unknown ids, drift: test_abi_layout_cpu.py


def test_tile_merge_rejects_bad_arguments_without_a_gpu():
    _hip, lib = _lib()
    fake = 4096                                   # never dereferenced: every call below fails its checks first
    ptrs = ("logits", "boxes", "tile_start", "windows", "sizes", "out_boxes", "out_labels", "out_scores", "out_query", "out_tile",
            "counts", "status")
    start = np.array([0, 1, 4], np.int32)

    def desc(**kw):
        d = _hip.TileMergeDesc()
        d.B, d.N, d.Q, d.C = 2, 4, 100, 92
        for n in ptrs:
            setattr(d, n, fake)
        d.tile_start_host = start.ctypes.data
        d.sL_b, d.sL_q, d.sB_b, d.sB_q = 9200, 92, 400, 4
        d.background_class, d.score_threshold, d.max_detections, d.bbox_format, d.clip = 91, 0.7, 100, 1, 1
        d.match, d.class_agnostic, d.edge_margin, d.nms_threshold = 0, 0, 0.0, 0.5
        for n, v in kw.items():
            setattr(d, n, v)
        return d

    def rejected(d, text):
        rc = lib.detr_hip_tile_merge(ctypes.byref(d) if d is not None else None, None)
        msg = lib.detr_hip_last_error().decode()
        assert rc < 0 and text in msg, (rc, msg, text)

    rejected(None, "null descriptor")
    for n in ptrs + ("tile_start_host",):
        rejected(desc(**{n: None}), "null operand")
    for kw in (dict(B=0), dict(B=-1), dict(N=0), dict(Q=0), dict(Q=1025), dict(C=0)):
        rejected(desc(**kw), "bad shape")
    for kw in (dict(sL_q=91), dict(sB_q=3), dict(sL_b=-1), dict(sB_b=-400)):
        rejected(desc(**kw), "strides")
    rejected(desc(N=5), "tile_start must run from 0 to N")
    for bad in ([1, 2, 4], [0, 5, 4], [0, -1, 4]):
        arr = np.array(bad, np.int32)
        rejected(desc(tile_start_host=arr.ctypes.data), "tile_start")
    for k in (0, -1, _hip.TILE_MAX_CAND + 1):
        rejected(desc(max_detections=k), "max_detections")
    for f in (-1, 4):
        rejected(desc(bbox_format=f), "bbox_format")
    for name in ("clip", "match", "class_agnostic"):
        for v in (-1, 2):
            rejected(desc(**{name: v}), name)
    for t in (float("nan"), float("inf"), float("-inf")):
        rejected(desc(score_threshold=t), "score_threshold is not finite")
        rejected(desc(nms_threshold=t), "nms_threshold is not finite")
    for m in (float("nan"), float("inf"), -1.0):
        rejected(desc(edge_margin=m), "edge_margin")
    rejected(desc(out_boxes=fake + 4), "16-byte aligned")


# ---- Detector arguments --------------------------------------------------------------------------------------------------------
class _Cfg:
    background_class = 91
    image_size = (64, 96)
    normalized_method = "torch_resnet"


def test_detector_tile_arguments():
    from detr_tf.inference import Detections, Detector, TiledDetections
    assert Detections._fields == ("boxes", "labels", "scores", "query")             # unchanged
    assert TiledDetections._fields == Detections._fields + ("tile",)
    with pytest.raises(ValueError, match="shortest_side"):
        Detector(None, _Cfg(), tiles=(2, 2), resize="fixed")
    for kw in (dict(tiles=(0, 2)), dict(tiles=(2, 2), overlap=1.0), dict(tiles=(2, 2), tile_batch=0), dict(nms_threshold=float("nan")),
               dict(nms_threshold=0.5, match="giou"), dict(tiles=(2, 2), edge_margin=-1.0)):
        with pytest.raises(ValueError):
            Detector(None, _Cfg(), **kw)
    det = Detector(None, _Cfg(), tiles=(2, 3), shortest_side=64, max_size=96)
    assert det.nms_threshold == 0.5 and det.tiles == (2, 3)                         # the tiled path defaults to NMS at 0.5
    assert Detector(None, _Cfg()).nms_threshold is None and Detector(None, _Cfg()).tiles is None
    image = np.zeros((96, 128, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="need_weights"):
        det(image, need_weights=True)
    with pytest.raises(ValueError, match="does not fit"):                           # a grid larger than the image
        Detector(None, _Cfg(), tiles=(2, 200)).tile_records([image])
    from detr_tf.data import transformation as T
    assert det.tile_records([image]) == [T.tile_records(96, 128, 2, 3, 0.2, 64, 96, T.CUBIC, True)]
