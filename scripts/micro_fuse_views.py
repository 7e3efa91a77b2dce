"""Time of one detr_hip_fuse_views launch per method (NOTEBOOK §28), beside detr_hip_tile_merge on the same inputs -- this tree's and,
with --parent-lib, another build's, e.g. the parent commit's libdetr_hip.so -- and the host NumPy loop on read-back rows.  Device
events around windows of back-to-back launches.  Usage: python scripts/micro_fuse_views.py [--parent-lib PATH] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cli = argparse.ArgumentParser()
cli.add_argument("--parent-lib", default=None)
cli.add_argument("--out", default=None)
cli = cli.parse_args()
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "detr-tensorflow_amd"), ROOT]
import numpy as np
import torch

import fuse_views_ref as R
import test_gpu_fuse_views as T
from detr_tf import _hip
from detr_tf.inference import DETECT_FORMATS, MATCH_MODES

DEV = "cuda"
lib = _hip.load()
parent = None
if cli.parent_lib:
    parent = ctypes.CDLL(cli.parent_lib)
    parent.detr_hip_tile_merge.argtypes = [ctypes.POINTER(_hip.TileMergeDesc), ctypes.c_void_p]
    parent.detr_hip_tile_merge.restype = ctypes.c_int32


def setup(case, K, thr):
    lg, bx = torch.from_numpy(case["logits"].copy()).to(DEV), torch.from_numpy(case["boxes"].copy()).to(DEV)
    B, (N, Q, C) = len(case["sizes"]), lg.shape
    start_h = np.ascontiguousarray(case["view_start"], np.int32)
    keep = [lg, bx, start_h] + [torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV) for a in (start_h, case["windows"], case["sizes"], case["flips"])]
    outs = [torch.zeros(B * K * 4, device=DEV), torch.zeros(B * K, dtype=torch.int64, device=DEV), torch.zeros(B * K, device=DEV)] + \
           [torch.zeros(B * K, dtype=torch.int32, device=DEV) for _ in range(3)] + [torch.zeros(B + 1, dtype=torch.int32, device=DEV)]
    d = _hip.TileMergeDesc()
    d.B, d.N, d.Q, d.C = B, N, Q, C
    d.logits, d.sL_b, d.sL_q = lg.data_ptr(), lg.stride(0), lg.stride(1)
    d.boxes, d.sB_b, d.sB_q = bx.data_ptr(), bx.stride(0), bx.stride(1)
    d.tile_start, d.tile_start_host, d.windows, d.sizes = keep[3].data_ptr(), start_h.ctypes.data, keep[4].data_ptr(), keep[5].data_ptr()
    d.background_class, d.score_threshold, d.max_detections = case["bg"], thr, K
    d.bbox_format, d.clip, d.match, d.class_agnostic, d.edge_margin = DETECT_FORMATS["xyxy"], 1, MATCH_MODES["iou"], 0, 0.0
    d.out_boxes, d.out_labels, d.out_scores, d.out_query, d.out_tile = (o.data_ptr() for o in outs[:5])
    d.counts, d.status = outs[6].data_ptr(), outs[6].data_ptr() + 4 * B
    return d, keep, outs


def timed(launch, iters):
    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    best = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            launch()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) * 1000.0 / iters)
    return dict(us_median=round(float(np.median(best)), 2), us_min=round(min(best), 2), us_max=round(max(best), 2), iters=iters)


def point(name, case, thr, K=100):
    d, keep, outs = setup(case, K, thr)
    stream = _hip._stream()
    row = dict(point=name, score_threshold=thr, max_detections=K)
    for method in R.METHODS:
        d.nms_threshold = R.THRESHOLDS[method]
        block = (ctypes.c_double * _hip.FUSE_PARAMS)(_hip.FUSE_METHODS[method], 0.5, 0.001, 0, 1, 0)
        launch = lambda: lib.detr_hip_fuse_views(ctypes.byref(d), keep[6].data_ptr(), ctypes.byref(block), outs[5].data_ptr(), stream)   # noqa: E731
        assert launch() == 0
        torch.cuda.synchronize()
        counts = outs[6].cpu().tolist()
        row[method] = dict(timed(launch, 200), kept=counts[:-1], status=counts[-1])
        outs[6].zero_()
    d.nms_threshold = 0.5
    row["merge_tiles"] = timed(lambda: lib.detr_hip_tile_merge(ctypes.byref(d), stream), 200)
    if parent is not None:
        row["merge_tiles_parent"] = timed(lambda: parent.detr_hip_tile_merge(ctypes.byref(d), stream), 200)
    # the host loop: read the rows back, score them, run the sequential reference
    for method in ("nms", "wbf"):
        t0 = time.perf_counter()
        lg, bx = keep[0].cpu().numpy(), keep[1].cpu().numpy()
        e = np.exp(lg - lg.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        want = R.fuse(p.max(-1).astype(np.float32), p.argmax(-1), bx, case["view_start"], case["windows"], case["flips"], case["sizes"], case["bg"],
                      method=method, score_threshold=thr, max_detections=K)
        row["host_numpy_" + method] = dict(ms=round((time.perf_counter() - t0) * 1000.0, 2), candidates=[w[6]["candidates"] for w in want],
                                           clusters=[sum(w[6]["sizes"].values()) for w in want])
    print(json.dumps(row), flush=True)
    return row


four = T.make_case(21, [(0, 1, 0, 1)], [(800, 1200)], 100, 92, 30, clutter=0.5)
cap = T.make_case(22, [tuple([0, 1] * 10)], [(800, 1200)], 100, 92, 70, seen=1.1, clutter=1.1)      # 20 views x 100 = 2000 candidates, 70 objects
worst = T.make_case(23, [tuple([0, 1] * 5)], [(800, 1200)], 100, 92, 0, seen=1.1, clutter=1.1)       # 1000 candidates, nearly all singletons
rows = [point("4 views, Q=100, thr 0.7", four, 0.7), point("4 views, Q=100, thr 0.05", four, 0.05),
        point("20 views, Q=100, thr 0 (2000 candidates)", cap, 0.0), point("10 views, Q=100, thr 0, clutter only (WBF walk worst case)", worst, 0.0, K=1000)]
if cli.out:
    json.dump(rows, open(cli.out, "w"), indent=1)
