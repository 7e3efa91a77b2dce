"""Fusion of views without a GPU: transformation.view_records, the NumPy restatement of the fusion on hand-worked cases
(tests/fuse_views_ref.py is the reference the GPU tests compare detr_hip_fuse_views with, so it is pinned here first), the C entry
point's declaration / export / argument checks, and the argument validation of inference.fuse_views and the Detector."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import abi_header
import fuse_views_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

_lib = abi_header.hip_lib


# ---- view_records --------------------------------------------------------------------------------------------------------------
def test_view_records_order_scales_and_flip():
    from detr_tf.data import transformation as T
    h0, w0 = 96, 128
    plain = T.view_records(h0, w0)
    assert plain == [T.eval_record(h0, w0, 800, 1333, T.LINEAR)]
    recs = T.view_records(h0, w0, (64, 48, 80), 96, True, T.CUBIC)
    assert len(recs) == 6
    assert recs[:3] == [T.eval_record(h0, w0, s, 96, T.CUBIC) for s in (64, 48, 80)]            # the scales in the order given
    assert [r.flip for r in recs] == [False] * 3 + [True] * 3
    assert [r._replace(flip=False) for r in recs[3:]] == recs[:3]                                # the same list again, flipped
    assert [(r.hd, r.wd) for r in recs[:3]] == [T.target_size(h0, w0, s, 96) for s in (64, 48, 80)]
    for r in recs:
        T.check_padded_record(r)
    assert T.view_records(h0, w0, [64], 96, flip=False) == [T.eval_record(h0, w0, 64, 96)]
    assert T.view_records(h0, w0, (np.int64(64),), 96) == [T.eval_record(h0, w0, 64, 96)]


def test_view_records_tiles_and_flipped_windows():
    from detr_tf.data import transformation as T
    h0, w0 = 100, 200
    recs = T.view_records(h0, w0, (64, 48), 96, True, T.CUBIC, tiles=(1, 2), overlap=0.2)
    per_scale = [T.tile_records(h0, w0, 1, 2, 0.2, s, 96, T.CUBIC, True) for s in (64, 48)]
    assert recs[:6] == per_scale[0] + per_scale[1] and len(recs) == 12
    # a flipped record's window is a window of the MIRRORED image: the windows repeat unchanged, only the flag differs
    assert [(r.y0, r.x0, r.hc, r.wc, r.hd, r.wd) for r in recs[6:]] == [(r.y0, r.x0, r.hc, r.wc, r.hd, r.wd) for r in recs[:6]]
    assert all(r.flip for r in recs[6:]) and not any(r.flip for r in recs[:6])
    assert recs[1].x0 == 0 and recs[2].x0 + recs[2].wc == w0
    no_full = T.view_records(h0, w0, (64,), 96, False, T.CUBIC, tiles=(1, 2), include_full=False)
    assert no_full == T.tile_records(h0, w0, 1, 2, 0.2, 64, 96, T.CUBIC, False)


def test_view_records_rejects_bad_arguments():
    from detr_tf.data import transformation as T
    for scales in ((), [], (0,), (-8,), (64, 0), (64.5,), (True,), ("64",), 64, None):
        with pytest.raises(ValueError, match="scales"):
            T.view_records(96, 128, scales)
    for h0, w0 in ((0, 5), (5, 0), (-1, 5)):
        with pytest.raises(ValueError):
            T.view_records(h0, w0)
    for tiles in ((8, 1), (1, 6), (0, 1), (1, 0), (-1, 2)):                                     # everything tile_records rejects
        with pytest.raises(ValueError):
            T.view_records(7, 5, tiles=tiles)
    for overlap in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="overlap"):
            T.view_records(96, 128, tiles=(2, 2), overlap=overlap)
    with pytest.raises(ValueError, match="tiles"):
        T.view_records(96, 128, tiles=(2,))


# ---- the reference on hand-worked cases ------------------------------------------------------------------------------------------
def _img(entries, size=(128, 256), flips=None, **kw):
    """entries: [(view, score, label, (x0, y0, x1, y1) in pixels OF THE VIEW'S OWN FRAME)], every view a whole-image window; -> the
    reference's result.  Sizes and coordinates that are multiples of powers of two keep the mapping exact."""
    H, W = size
    V = 1 + max(e[0] for e in entries)
    Q = max(sum(1 for e in entries if e[0] == t) for t in range(V))
    scores, labels, boxes = np.zeros((V, Q), F), np.full((V, Q), 9), np.zeros((V, Q, 4), F)
    at = [0] * V
    for t, s, l, (x0, y0, x1, y1) in entries:
        q = at[t]
        at[t] += 1
        scores[t, q], labels[t, q] = s, l
        boxes[t, q] = ((x0 + x1) / 2 / W, (y0 + y1) / 2 / H, (x1 - x0) / W, (y1 - y0) / H)
    windows = np.array([(0, 0, H, W)] * V, np.int32)
    return R.fuse_image(scores, labels, boxes, windows, [0] * V if flips is None else flips, size, 9, **kw)


def test_ref_a_mirrored_view_maps_onto_the_box_itself():
    box, seen_mirrored = (32, 16, 96, 80), (160, 16, 224, 80)                                   # W = 256: 256 - 96 = 160, 256 - 32 = 224
    pair = [(0, 0.5, 1, box), (1, 0.5, 1, seen_mirrored)]
    for method in R.METHODS:
        b, l, s, q, t, m, c = _img(pair, flips=[0, 1], method=method)
        assert c["candidates"] == 2 and b[0].tolist() == list(box), method
    b, l, s, q, t, m, c = _img(pair, flips=[0, 1], method="wbf")
    assert len(b) == 1 and m.tolist() == [2] and t.tolist() == [0] and s.tolist() == [0.5]
    assert len(_img(pair, flips=[0, 1], method="nms")[0]) == 1
    assert len(_img(pair, flips=[0, 0], method="wbf")[0]) == 2                                  # unmirrored they are two objects
    # the mirror applies to the UNCLIPPED corners, the clip follows: a box leaving the mirrored image on its left leaves the image on its right
    out = _img([(0, 0.5, 1, (-32, 16, 32, 80))], flips=[1], method="nms", clip=False)[0]
    assert out.tolist() == [[224, 16, 288, 80]]
    assert _img([(0, 0.5, 1, (-32, 16, 32, 80))], flips=[1], method="nms")[0].tolist() == [[224, 16, 256, 80]]
    assert _img([(0, 0.5, 1, (-32, 16, 32, 80))], flips=[1], method="nms", bbox_format="xy_center")[0].tolist() == [[240, 48, 32, 64]]


A, B = (0, 0, 40, 10), (30, 0, 70, 10)                                                          # IoU 10 / 70: two clusters at 0.3


def test_ref_wbf_two_clusters_the_argmax_decides():
    assert R.measure(A, B, "iou") < 0.3
    for third, cluster in (((12, 0, 52, 10), 0), ((18, 0, 58, 10), 1)):
        assert R.measure(A, third, "iou") > 0.3 and R.measure(B, third, "iou") > 0.3               # over the threshold on BOTH
        assert (R.measure(A, third, "iou") > R.measure(B, third, "iou")) == (cluster == 0)
        b, l, s, q, t, m, c = _img([(0, 0.875, 1, A), (0, 0.75, 1, B), (0, 0.5, 1, third)], method="wbf", threshold=0.3)
        assert c["multi"] == 1 and c["sizes"] == {1: 1, 2: 1}
        # by the founder's query: members and score, the mean of the members' scores; the output is ordered by that score
        got = {query: (members, score) for query, members, score in zip(q.tolist(), m.tolist(), s.tolist())}
        assert got == ({0: (2, 0.6875), 1: (1, 0.75)} if cluster == 0 else {0: (1, 0.875), 1: (2, 0.625)})
        assert s.tolist() == sorted(s.tolist(), reverse=True)


def test_ref_wbf_an_exact_tie_goes_to_the_lower_cluster():
    left, right, middle = (0, 0, 40, 10), (40, 0, 80, 10), (20, 0, 60, 10)
    assert R.measure(left, middle, "iou") == R.measure(right, middle, "iou") == 20 / 60
    b, l, s, q, t, m, c = _img([(0, 0.875, 1, left), (0, 0.75, 1, right), (0, 0.5, 1, middle)], method="wbf", threshold=0.3)
    assert c["multi"] == 1 and list(zip(q.tolist(), m.tolist(), s.tolist())) == [(1, 1, 0.75), (0, 2, 0.6875)]   # `left` founded cluster 0 and takes it
    b, l, s, q, t, m, c = _img([(0, 0.75, 1, left), (0, 0.875, 1, right), (0, 0.5, 1, middle)], method="wbf", threshold=0.3)
    assert list(zip(q.tolist(), m.tolist(), s.tolist())) == [(0, 1, 0.75), (1, 2, 0.6875)]       # now `right` founded cluster 0


def test_ref_wbf_a_join_and_a_refusal_only_because_the_fused_box_moved():
    first, second = (0, 0, 40, 10), (16, 0, 56, 10)                                             # IoU 24 / 56; fused with equal scores: (8, 0, 48, 10)
    late = (28, 0, 68, 10)                                                                      # founder: 12 / 68, fused: 20 / 60
    assert R.measure(first, late, "iou") < 0.3 < R.measure((8, 0, 48, 10), late, "iou")
    b, l, s, q, t, m, c = _img([(0, 0.75, 1, first), (0, 0.75, 1, second), (0, 0.5, 1, late)], method="wbf", threshold=0.3)
    assert m.tolist() == [3] and c["moved_joins"] == 1 and c["moved_refusals"] == 0
    sw = 0.75 + 0.75 + 0.5
    assert b[0].tolist() == [F((0.75 * 16 + 0.5 * 28) / sw), 0, F((0.75 * 40 + 0.75 * 56 + 0.5 * 68) / sw), 10] and s.tolist() == [F(sw / 3)]
    near = (0, 0, 26, 10)                                                                       # founder: 26 / 40, fused: 18 / 48
    assert R.measure(first, near, "iou") > 0.4 > R.measure((8, 0, 48, 10), near, "iou")
    b, l, s, q, t, m, c = _img([(0, 0.75, 1, first), (0, 0.75, 1, second), (0, 0.5, 1, near)], method="wbf", threshold=0.4)
    assert m.tolist() == [2, 1] and c["moved_joins"] == 0 and c["moved_refusals"] == 1
    assert b.tolist() == [[8, 0, 48, 10], list(near)]                                           # a founder's box is copied, not divided back


def test_ref_wbf_min_members_expected_views_and_labels():
    box, far = (32, 16, 96, 80), (128, 16, 192, 80)
    entries = [(0, 0.75, 1, box), (1, 0.5, 1, box), (2, 0.25, 1, box), (0, 0.625, 1, far), (1, 0.5, 2, box)]
    b, l, s, q, t, m, c = _img(entries, method="wbf")
    assert m.tolist() == [1, 3, 1] and l.tolist() == [1, 1, 2] and s.tolist() == [0.625, 0.5, 0.5] and c["sizes"] == {3: 1, 1: 2}
    assert t.tolist() == [0, 0, 1] and q.tolist() == [1, 0, 1]                                  # equal scores: the lower cluster first
    b, l, s, q, t, m, c = _img(entries, method="wbf", min_members=2)
    assert m.tolist() == [3] and c["sizes"] == {3: 1, 1: 2}                                     # dropped after the walk, not before
    b, l, s, q, t, m, c = _img(entries, method="wbf", expected_views=4)
    assert sorted(zip(m.tolist(), s.tolist())) == [(1, 0.5 / 4), (1, 0.625 / 4), (3, 0.5 * 3 / 4)] and m.tolist()[0] == 3
    b, l, s, q, t, m, c = _img(entries, method="wbf", expected_views=2)                         # min(cnt, E): never more than the mean
    assert sorted(zip(m.tolist(), s.tolist())) == [(1, 0.25), (1, 0.3125), (3, 0.5)]
    assert _img(entries, method="wbf", class_agnostic=True)[5].tolist() == [1, 4]               # 0.625 alone, then (0.75 + 0.5 + 0.5 + 0.25) / 4
    assert _img(entries, method="wbf", max_detections=1)[5].tolist() == [1]


def test_ref_soft_nms_linear_decays_a_box_below_score_min():
    same, partly = (0, 0, 40, 10), (16, 0, 56, 10)
    b, l, s, q, t, m, c = _img([(0, 0.9, 1, same), (0, 0.5, 1, same), (0, 0.25, 1, partly)], method="soft_nms", threshold=0.3)
    # the copy: 0.5 * (1 - 1) = 0 < 0.001, it dies; the partial overlap: 0.25 * (1 - 24 / 56) survives with that score
    assert q.tolist() == [0, 2] and m.tolist() == [1, 1]
    assert s.tolist() == [F(0.9), F(0.25 * (1.0 - 24 / 56))]
    kept = _img([(0, 0.9, 1, same), (0, 0.5, 1, same), (0, 0.25, 1, partly)], method="soft_nms", threshold=0.3, score_min=0.0)
    assert kept[3].tolist() == [0, 2, 1] and kept[2].tolist()[2] == 0.0                         # 0 < 0 is false: it stays, with score 0
    under = _img([(0, 0.9, 1, same), (0, 0.25, 1, partly)], method="soft_nms", threshold=0.5)   # 24 / 56 is not over 0.5: untouched
    assert under[2].tolist() == [F(0.9), F(0.25)]
    other = _img([(0, 0.9, 1, same), (0, 0.5, 2, same)], method="soft_nms")                     # another label is not decayed ...
    assert other[2].tolist() == [F(0.9), F(0.5)]
    assert _img([(0, 0.9, 1, same), (0, 0.5, 2, same)], method="soft_nms", class_agnostic=True)[3].tolist() == [0]   # ... unless asked
    # the order follows the CURRENT scores: B is decayed under C
    b, l, s, q, t, m, c = _img([(0, 0.9, 1, same), (0, 0.8, 1, partly), (0, 0.6, 1, (100, 0, 140, 10))], method="soft_nms", threshold=0.3)
    assert q.tolist() == [0, 2, 1] and s.tolist() == [F(0.9), F(0.6), F(float(F(0.8)) * (1.0 - 24 / 56))]
    assert c["select_gap"] < 1 and c["min_gap"] > 1


def test_ref_soft_nms_gaussian_leaves_the_bits_alone_at_zero_overlap():
    rng = np.random.default_rng(0)
    scores = rng.uniform(0.05, 1.0, 6).astype(F)
    entries = [(0, float(s), 1, (40 * i, 0, 40 * i + 32, 16)) for i, s in enumerate(scores)]    # disjoint: m = 0 for every pair
    b, l, s, q, t, m, c = _img(entries, method="soft_nms_gaussian")
    assert sorted(s.tobytes() for s in s) == sorted(v.tobytes() for v in scores) and len(s) == 6
    assert s.tolist() == sorted(scores.tolist(), reverse=True)
    # with overlap every box is decayed, over the threshold or not: exp(-m * m / sigma)
    b, l, s, q, t, m, c = _img([(0, 0.9, 1, (0, 0, 40, 10)), (0, 0.5, 1, (30, 0, 70, 10))], method="soft_nms_gaussian", sigma=0.25)
    assert s.tolist() == [F(0.9), F(0.5 * math.exp(-((10 / 70) ** 2) / 0.25))]


def test_ref_nms_is_the_tile_merge_reference():
    import tile_merge_ref as M
    rng = np.random.default_rng(1)
    V, Q = 3, 40
    scores, labels = rng.random((V, Q)).astype(F), rng.integers(0, 4, (V, Q))
    boxes = np.concatenate([rng.random((V, Q, 2)), rng.uniform(0.05, 0.5, (V, Q, 2))], -1).astype(F)
    windows = np.array([(0, 0, 100, 200), (0, 0, 100, 111), (0, 89, 100, 111)], np.int32)
    for fmt in ("xyxy", "yxyx", "xywh"):
        kw = dict(score_threshold=0.2, bbox_format=fmt, match="ios", edge_margin=3.0, max_detections=30)
        want = M.merge_image(scores, labels, boxes, windows, (100, 200), 3, nms_threshold=0.4, **kw)
        got = R.fuse_image(scores, labels, boxes, windows, [0, 0, 0], (100, 200), 3, method="nms", threshold=0.4, **kw)
        assert 0 < len(want[3]) < want[5] and got[6]["candidates"] == want[5] and got[5].tolist() == [1] * len(want[3])
        for g, w in zip(got[:5], want[:5]):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()


# ---- the C entry point ---------------------------------------------------------------------------------------------------------
def test_fuse_views_symbol_declared_exported_appended():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    names = re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr)
    name = "detr_hip_fuse_views"
    assert name in names and name in _hip.EXPORTED_SYMBOLS and name in _hip._SIGNATURES and hasattr(lib, name)
    assert names[-1] == name and hdr.index("detr_hip_fuse_views(") > hdr.index("detr_hip_workspace_bytes_track_motion(")   # appended last
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9 and "#define DETR_HIP_ABI_VERSION 9" in hdr
    define = lambda n: int(re.search(rf"#define {n} (\d+)", hdr).group(1))                      # noqa: E731
    assert define("DETR_FUSE_PARAMS") == _hip.FUSE_PARAMS == 6
    assert define("DETR_FUSE_OVER_CLUSTERS") == _hip.FUSE_OVER_CLUSTERS == 4
    assert define("DETR_FUSE_MAX_CLUSTERS") == _hip.FUSE_MAX_CLUSTERS <= _hip.TILE_MAX_CAND
    assert sorted(_hip.FUSE_BAD) == [define("DETR_TILE_OVER_CAP"), define("DETR_TILE_BAD_START"), define("DETR_FUSE_OVER_CLUSTERS")]
    assert all(_hip.FUSE_BAD[bit] == text for bit, text in _hip.TILE_BAD.items())               # merge_tiles' wording
    assert _hip.FUSE_METHODS == {"nms": 0, "soft_nms": 1, "soft_nms_gaussian": 2, "wbf": 3}
    # no struct, no mirror, no layout id: the descriptor is detr_tile_merge_desc
    assert _hip._SIGNATURES[name][0]._type_ is _hip.TileMergeDesc
    assert len(abi_header.header_structs()) == 18 and not [n for n in vars(_hip) if n.endswith("Desc") and "Fuse" in n]


def test_fuse_views_rejects_bad_arguments_without_a_gpu():
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

    good = (3.0, 0.5, 0.001, 4.0, 1.0, 0.0)

    def rejected(d, text, fuse=good, members=fake, flip=fake):
        block = None if fuse is None else ctypes.byref((ctypes.c_double * _hip.FUSE_PARAMS)(*fuse))
        rc = lib.detr_hip_fuse_views(ctypes.byref(d) if d is not None else None, flip, block, members, None)
        msg = lib.detr_hip_last_error().decode()
        assert rc < 0 and text in msg and msg.startswith("fuse_views:"), (rc, msg, text)

    def block(**kw):
        v = list(good)
        for i, x in kw.items():
            v[int(i[1:])] = x
        return tuple(v)

    # its own arguments
    rejected(desc(), "null operand (fuse, out_members)", fuse=None)
    rejected(desc(), "null operand (fuse, out_members)", members=None)
    for i in range(6):
        for bad in (float("nan"), float("inf"), float("-inf")):
            rejected(desc(), f"fuse[{i}] is not finite", fuse=block(**{f"i{i}": bad}))
    for method in (-1.0, 4.0, 0.5, 2.5, 1e9):
        rejected(desc(), "method", fuse=block(i0=method))
    for sigma in (0.0, -0.5):
        rejected(desc(), "sigma", fuse=block(i0=2.0, i1=sigma))
    for method in (1.0, 2.0):
        rejected(desc(), "score_min", fuse=block(i0=method, i2=-0.001))
    for views in (0.5, 3.25, -1.0, 1e12):
        rejected(desc(), "expected_views", fuse=block(i3=views))
    for members in (0.0, 1.5, -2.0, 1e12):
        rejected(desc(), "min_members", fuse=block(i4=members))
    for reserved in (1.0, -1.0, 1e-300):
        rejected(desc(), "reserved", fuse=block(i5=reserved))
    # everything detr_hip_tile_merge rejects, by the same check
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
    # and detr_hip_tile_merge still speaks with its own name
    assert lib.detr_hip_tile_merge(ctypes.byref(desc(Q=0)), None) < 0 and lib.detr_hip_last_error().decode().startswith("tile_merge: bad shape")


# ---- fuse_views and Detector arguments -------------------------------------------------------------------------------------------
class _Cfg:
    background_class = 91
    image_size = (64, 96)
    normalized_method = "torch_resnet"


def test_fuse_views_argument_validation():
    import torch
    from detr_tf import inference as I
    assert I.FusedDetections._fields == I.TiledDetections._fields + ("members",)
    out = {"pred_logits": torch.zeros(2, 5, 4), "pred_boxes": torch.zeros(2, 5, 4)}
    args = (out, [0, 2], np.zeros((2, 4), np.int32), [0, 1], [[8, 8]], 3)
    for kw, text in ((dict(method="average"), "method"), (dict(threshold=float("nan")), "threshold"), (dict(match="giou"), "match"),
                     (dict(edge_margin=-1.0), "edge_margin"), (dict(max_detections=0), "max_detections"), (dict(sigma=0.0), "sigma"),
                     (dict(sigma=float("inf")), "sigma"), (dict(score_min=-0.1), "score_min"), (dict(expected_views=0), "expected_views"),
                     (dict(expected_views=2.5), "expected_views"), (dict(min_members=0), "min_members"), (dict(min_members=1.5), "min_members")):
        with pytest.raises(ValueError, match=text):
            I.fuse_views(*args, **kw)
    with pytest.raises(RuntimeError, match="bbox_format"):
        I.fuse_views(*args, bbox_format="cxcywh")
    with pytest.raises(RuntimeError, match="GPU"):                                              # valid arguments: it gets as far as the device check
        I.fuse_views(*args)
    assert [I._check_fuse_args(m, None, "iou", 0.0, 100, 0.5, 0.001, None, 1)[1] for m in R.METHODS] == [0.5, 0.5, 0.5, 0.55]
    assert I._check_fuse_args("wbf", 0.7, "iou", 0.0, 100, 0.5, 0.001, 4, 2) == ((3, 0.5, 0.001, 4, 2, 0), 0.7)
    assert I.FUSE_THRESHOLDS == R.THRESHOLDS


def test_detector_view_arguments():
    from detr_tf.inference import Detector
    for kw in (dict(merge="average"), dict(scales=()), dict(scales=(0,)), dict(scales=(64.5,)), dict(merge="wbf", min_members=0),
               dict(merge="soft_nms_gaussian", sigma=0.0), dict(merge="soft_nms", score_min=-1.0), dict(flip=True, nms_threshold=float("nan")),
               dict(flip=True, tile_batch=0), dict(flip=True, match="giou")):
        with pytest.raises(ValueError):
            Detector(None, _Cfg(), **kw)
    for kw in (dict(flip=True), dict(scales=(64,)), dict(merge="wbf")):
        with pytest.raises(ValueError, match="shortest_side"):
            Detector(None, _Cfg(), resize="fixed", **kw)
    det = Detector(None, _Cfg(), flip=True, scales=(64, 48), merge="wbf", shortest_side=64, max_size=96)
    assert det.views and det.fuse_threshold == 0.55 and det.scales == (64, 48) and det.nms_threshold is None
    assert Detector(None, _Cfg(), merge="soft_nms").fuse_threshold == 0.5 and Detector(None, _Cfg(), flip=True).fuse_threshold == 0.5
    assert Detector(None, _Cfg(), merge="wbf", nms_threshold=0.7).fuse_threshold == 0.7        # nms_threshold doubles as the fusion threshold
    assert Detector(None, _Cfg(), merge="wbf", tiles=(2, 2)).fuse_threshold == 0.55
    image = np.zeros((96, 128, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="need_weights"):
        det(image, need_weights=True)
    from detr_tf.data import transformation as T
    assert det.view_records([image]) == [T.view_records(96, 128, (64, 48), 96, True, T.CUBIC)]
    assert Detector(None, _Cfg(), flip=True, shortest_side=64, max_size=96).view_records([image]) == [T.view_records(96, 128, (64,), 96, True, T.CUBIC)]
    tiled = Detector(None, _Cfg(), flip=True, tiles=(1, 2), shortest_side=64, max_size=96)
    assert tiled.view_records([image]) == [T.view_records(96, 128, (64,), 96, True, T.CUBIC, (1, 2), 0.2, True)]


class _Stage:
    """Stands in for DeviceInputStage: CPU tensors of the right shapes, and a record of what was asked."""
    last_upload = None

    def __init__(self):
        self.calls = []

    def augmented_padded(self, srcs, records, canvas=None):
        import torch
        self.calls.append(("padded", len(records)))
        return torch.zeros(len(srcs), 64, 96, 3), torch.zeros(len(srcs), 64, 96, dtype=torch.bool)

    def augmented_tiles(self, srcs, records, canvas=None):
        import torch
        n = [len(r) for r in records]
        self.calls.append(("tiles", n))
        return torch.zeros(sum(n), 64, 96, 3), torch.zeros(sum(n), 64, 96, dtype=torch.bool), np.concatenate([[0], np.cumsum(n)]).astype(np.int32)


def _stub_detector(monkeypatch, **kw):
    """A Detector on a stub stage and a stub model, with the three post-model entry points replaced by recorders."""
    import torch
    from detr_tf import inference as I
    seen = []
    for name in ("detect_batched", "merge_tiles", "fuse_views"):
        def recorder(m_outputs, *a, _name=name, **k):
            seen.append((_name, int(m_outputs["pred_logits"].shape[0]), k))
            return [_name] * (len(a[0]) - 1 if _name != "detect_batched" else len(a[0]))
        monkeypatch.setattr(I, name, recorder)

    def model(inputs, training=False, need_weights=None):
        n = inputs[0].shape[0]
        return {"pred_logits": torch.zeros(n, 5, 92), "pred_boxes": torch.zeros(n, 5, 4)}

    det = I.Detector(model, _Cfg(), shortest_side=64, max_size=96, **kw)
    det._stage = _Stage()
    return det, seen


def test_a_detector_built_as_before_never_reaches_fuse_views(monkeypatch):
    images = [np.zeros((96, 128, 3), np.uint8), np.zeros((80, 150, 3), np.uint8)]
    det, seen = _stub_detector(monkeypatch)
    assert (det.flip, det.scales, det.merge, det.views) == (False, None, "nms", False)
    assert (det.tiles, det.nms_threshold, det.tile_batch, det.match, det.class_agnostic, det.edge_margin) == (None, None, None, "iou", False, 0.0)
    assert det(images) == ["detect_batched"] * 2 and det(images[0]) == "detect_batched"
    assert [s[0] for s in seen] == ["detect_batched"] * 2 and det._stage.calls == [("padded", 2), ("padded", 1)]
    det, seen = _stub_detector(monkeypatch, nms_threshold=0.6)
    assert not det.views and det(images) == ["merge_tiles"] * 2 and [(s[0], s[1], s[2]["nms_threshold"]) for s in seen] == [("merge_tiles", 2, 0.6)]
    det, seen = _stub_detector(monkeypatch, tiles=(1, 2), tile_batch=4)
    assert not det.views and det.nms_threshold == 0.5
    assert det(images) == ["merge_tiles"] * 2 and [(s[0], s[1]) for s in seen] == [("merge_tiles", 6)] and det._stage.calls == [("tiles", [3, 3])]
    det, seen = _stub_detector(monkeypatch, flip=False, scales=None, merge="nms", tiles=None)     # spelled out: still the plain path
    assert det(images) == ["detect_batched"] * 2 and [s[0] for s in seen] == ["detect_batched"]


def test_a_detector_with_views_calls_fuse_views_once(monkeypatch):
    images = [np.zeros((96, 128, 3), np.uint8), np.zeros((80, 150, 3), np.uint8)]
    det, seen = _stub_detector(monkeypatch, flip=True, scales=(64, 48), merge="wbf", tile_batch=3, min_members=2)
    assert det(images) == ["fuse_views"] * 2 and det._stage.calls == [("tiles", [4, 4])]
    (name, n, kw), = seen
    assert (name, n) == ("fuse_views", 8) and kw["method"] == "wbf" and kw["threshold"] == 0.55 and kw["expected_views"] == 4
    assert kw["min_members"] == 2 and kw["sigma"] == 0.5 and kw["score_min"] == 0.001
    det, seen = _stub_detector(monkeypatch, merge="soft_nms", nms_threshold=0.4)                 # one view is enough to ask for another rule
    assert det(images[0]) == "fuse_views" and seen[0][1] == 1 and seen[0][2]["expected_views"] == 1 and seen[0][2]["threshold"] == 0.4
    det, seen = _stub_detector(monkeypatch, flip=True, tiles=(1, 2))
    assert det(images) == ["fuse_views"] * 2 and seen[0][1] == 12 and seen[0][2]["expected_views"] is None and seen[0][2]["method"] == "nms"
