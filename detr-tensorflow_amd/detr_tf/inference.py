"""Post-processing of the model outputs (reference detr_tf/inference.py:68-95).

`get_model_inference(m_outputs, background_class, bbox_format)` keeps the reference's signature and semantics (batch
element 0 only).  `get_model_inference_batched` is the same for EVERY image of the batch in one launch of the HIP kernel
`detr_hip_postprocess` (csrc/postprocess.hip): softmax score / arg-max label per query, background queries dropped with the
order preserved, boxes converted (xyxy / yxyx clipped to [0, 1] like bbox.py:171-183).  CUDA inputs only -- there is no
eager fallback; tensors on the CPU are moved to the model's device first by the caller.

`detect_batched` goes the rest of the way to what a user draws (webcam_inference.py:26-34, eval.py:41-55), in one launch of
`detr_hip_detect` (csrc/detect.hip): score threshold, detections sorted by score with a top-k cap, boxes in PIXELS of each image's
own original size.  `Detector` wraps the whole chain: raw uint8 images -> input stage -> model -> `detect_batched`.  With
`scoring="sigmoid", multilabel=True` the launch is `detr_hip_detect_multilabel` (csrc/detect_multilabel.hip): the K best (query,
class) pairs of every image, so one query may give several detections.

`merge_tiles` is the last step of SLICED inference (the model run on overlapping windows of a large image, plus the whole image):
one launch of `detr_hip_tile_merge` (csrc/tile_merge.hip) maps every window's boxes back to image pixels and removes the duplicates
the overlaps create with a class-wise greedy NMS.  `Detector(tiles=(rows, cols))` runs that chain; `Detector(nms_threshold=...)`
alone puts the same NMS behind the single-pass outputs.

`fuse_views` is the last step of TEST-TIME AUGMENTATION (the model run on the mirrored image and / or at several shortest sides):
one launch of `detr_hip_fuse_views` (csrc/fuse_views.hip) maps every view's boxes back -- a flipped view's through the mirror -- and
combines them by hard NMS, soft-NMS (linear or Gaussian) or weighted box fusion.  `Detector(flip=, scales=, merge=)` runs that chain.

`draw_detections` / `numpy_bbox_to_image` (detr_tf/overlay.py; reference inference.py:10-65) draw boxes, labels and an attention heat map
onto the frames in one call of `detr_hip_overlay` (csrc/overlay.hip); `Detector.draw` feeds it the detector's own frames and maps.

`Tracker` carries detections across the frames of a video: its tracks live on the device and one launch of `detr_hip_track`
(csrc/track.hip) per batch of frames associates, updates, spawns and emits -- `Detector.track` feeds it the detector's raw rows.
`Tracker(motion=True)` puts `detr_hip_track_motion` (csrc/track_motion.hip) in front: a global shift per frame, estimated on the
device from the frames themselves, moves the tracks with the camera before they are associated.
"""
import math
from ctypes import byref, c_double
from typing import NamedTuple

import numpy as np
import torch

from . import _hip as hip
from .overlay import class_palette, draw_detections, numpy_bbox_to_image  # noqa: F401  (the reference keeps them in inference.py)

BBOX_FORMATS = {"xy_center": 0, "xyxy": 1, "yxyx": 2}
DETECT_FORMATS = {"xy_center": 0, "xyxy": 1, "yxyx": 2, "xywh": 3}       # xywh: top-left + width / height, the COCO results form


def _check_model_outputs(who, lead, logits, boxes):
    if logits.dim() != 3 or boxes.dim() != 3 or boxes.shape[-1] != 4 or tuple(boxes.shape[:2]) != tuple(logits.shape[:2]):
        raise RuntimeError(f"{who}: expected pred_logits [{lead}, Q, C] and pred_boxes [{lead}, Q, 4], got {tuple(logits.shape)} and {tuple(boxes.shape)}")


def _model_outputs(who, step, logits, boxes):
    """pred_logits and pred_boxes as the kernels read them: on the GPU, float32, last stride 1.  `step` names the work in the message."""
    if not (logits.is_cuda and boxes.is_cuda):
        raise RuntimeError(f"{who}: the outputs must live on the GPU (the {step} is a HIP kernel; no CPU fallback)")
    logits, boxes = logits.float(), boxes.float()
    return (logits if logits.stride(-1) == 1 else logits.contiguous()), (boxes if boxes.stride(-1) == 1 else boxes.contiguous())


def _fill_model_outputs(d, logits, boxes, background_class):
    """The descriptor fields detr_hip_postprocess, detr_hip_detect and detr_hip_tile_merge share."""
    d.Q, d.C = logits.shape[1:]
    d.logits, d.sL_b, d.sL_q = logits.data_ptr(), logits.stride(0), logits.stride(1)
    d.boxes, d.sB_b, d.sB_q = boxes.data_ptr(), boxes.stride(0), boxes.stride(1)
    d.background_class = int(background_class)


def _scoring(scoring):
    """The `scoring` argument of the *_scored entry points: "softmax" (max softmax probability, background queries dropped) or
    "sigmoid" (sigmoid of the best non-background logit, every query a candidate: the class head of the focal criterion)."""
    if scoring not in hip.SCORINGS:
        raise ValueError(f"scoring must be one of {tuple(hip.SCORINGS)}, got {scoring!r}")
    return hip.SCORINGS[scoring]


MULTILABEL_DEFAULT_K = 100        # max_detections=None with multilabel: the K of the detectors that introduced the rule


def _multilabel(who, scoring, multilabel):
    """The `multilabel` keyword: whether a query may emit several classes (the K best (query, class) pairs of an image).  It
    needs scoring="sigmoid": a softmax row has one class by construction."""
    if multilabel and scoring != "sigmoid":
        raise ValueError(f"{who}: multilabel=True needs scoring='sigmoid', got {scoring!r}: a softmax row has one class by construction")
    return bool(multilabel)


def scoring_of(config):
    """The scoring that goes with a config's class criterion: "sigmoid" for class_criterion = "focal", else "softmax"."""
    return "sigmoid" if getattr(config, "class_criterion", "softmax") == "focal" else "softmax"


def _post(logits, boxes, background_class, bbox_format, scoring="softmax"):
    if bbox_format not in BBOX_FORMATS:
        raise NotImplementedError()                                     # inference.py:92-93
    mode = _scoring(scoring)
    logits, boxes = _model_outputs("get_model_inference", "post-processing", logits, boxes)
    B, Q, _ = logits.shape
    dev = logits.device
    out_b = torch.zeros(B, Q, 4, dtype=torch.float32, device=dev)
    out_l = torch.zeros(B, Q, dtype=torch.int64, device=dev)
    out_s = torch.zeros(B, Q, dtype=torch.float32, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    d = hip.PostprocessDesc()
    _fill_model_outputs(d, logits, boxes, background_class)
    d.B, d.bbox_format = B, BBOX_FORMATS[bbox_format]
    d.out_boxes, d.out_labels, d.out_scores, d.counts = out_b.data_ptr(), out_l.data_ptr(), out_s.data_ptr(), counts.data_ptr()
    if mode == 0:
        hip._check(hip.load().detr_hip_postprocess(byref(d), hip._stream()), "detr_hip_postprocess")
    else:
        hip._check(hip.load().detr_hip_postprocess_scored(byref(d), mode, hip._stream()), "detr_hip_postprocess_scored")
    return out_b, out_l, out_s, counts


def _post_multilabel(logits, boxes, background_class, bbox_format, max_detections=MULTILABEL_DEFAULT_K, score_threshold=0.0):
    """_post's rows under the multi-label rule: the max_detections best (query, class) pairs of every image, best first, as
    [B, K] rows (detr_hip_postprocess_multilabel) -- what the evaluation matchers read with K as their row capacity."""
    if bbox_format not in BBOX_FORMATS:
        raise NotImplementedError()
    K = int(max_detections)
    if not 1 <= K <= hip.MULTILABEL_MAX:
        raise ValueError(f"multilabel: max_detections={max_detections} must be in 1..{hip.MULTILABEL_MAX}")
    logits, boxes = _model_outputs("get_model_inference", "post-processing", logits, boxes)
    B, dev = logits.shape[0], logits.device
    out_b, out_l, out_s = _ranked_rows(B, K, dev, 0)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    d = hip.PostprocessDesc()
    _fill_model_outputs(d, logits, boxes, background_class)
    d.B, d.bbox_format = B, BBOX_FORMATS[bbox_format]
    d.out_boxes, d.out_labels, d.out_scores, d.counts = out_b.data_ptr(), out_l.data_ptr(), out_s.data_ptr(), counts.data_ptr()
    hip._check(hip.load().detr_hip_postprocess_multilabel(byref(d), K, float(score_threshold), hip._stream()), "detr_hip_postprocess_multilabel")
    return out_b, out_l, out_s, counts


def get_model_inference_batched(m_outputs: dict, background_class, bbox_format="xy_center", scoring="softmax"):
    """[(boxes [k_b, 4], labels [k_b] int64, scores [k_b])] for every image b of the batch: one kernel launch and ONE
    host synchronisation (the per-image detection counts).  scoring="sigmoid": all Q queries of every image, in query order,
    scored by the sigmoid of their best non-background logit."""
    out_b, out_l, out_s, counts = _post(m_outputs["pred_logits"], m_outputs["pred_boxes"], background_class, bbox_format, scoring)
    n = counts.tolist()
    return [(out_b[b, :k], out_l[b, :k], out_s[b, :k]) for b, k in enumerate(n)]


def get_model_inference(m_outputs: dict, background_class, bbox_format="xy_center", scoring="softmax"):
    """inference.py:68-95: (predicted_bbox, predicted_labels, predicted_scores) of batch element 0; scoring as
    get_model_inference_batched."""
    out_b, out_l, out_s, counts = _post(m_outputs["pred_logits"][0:1], m_outputs["pred_boxes"][0:1], background_class, bbox_format, scoring)
    k = int(counts[0])
    return out_b[0, :k], out_l[0, :k], out_s[0, :k]


def _feature_maps(model, image_shape, attn):
    """Attention maps [B, T, S] -> [B, T, Hf, Wf] over the feature map of a [B, H, W, 3] input (a decoder self-attention map, whose
    keys are the object queries, stays [B, Q, Q])."""
    from .engine import feature_size
    Hf, Wf = feature_size(int(image_shape[1]), int(image_shape[2]), model.engine.dilate)
    maps = {}
    for name, w in attn.items():
        B, T, S = w.shape
        maps[name] = w if "/decoder/" in name and name.endswith("/self_attn") else w.reshape(B, T, Hf, Wf)
    return maps


def get_attention_maps(model, images, need_weights=True):
    """(m_outputs, maps): one evaluation forward with `need_weights` (DetrModel.__call__: True = last encoder self-attention and last
    decoder cross-attention, or an iterable of site names), every map [B, T, S] reshaped to [B, T, Hf, Wf] over the Hf x Wf feature map
    (engine.feature_size of the input) -- the shape a user overlays on the image.  Encoder maps and decoder cross-attention maps have
    S = Hf * Wf keys; a decoder self-attention map (keys = object queries) is returned as [B, Q, Q].  `images` may be the
    (images, masks) pair of a padded batch: the map is then zero on the padded feature positions."""
    m_outputs = model(images, training=False, need_weights=need_weights)
    imgs = images[0] if isinstance(images, (tuple, list)) else images
    return m_outputs, _feature_maps(model, imgs.shape, m_outputs["attn"])


class Detections(NamedTuple):
    """The detections of ONE image, best first: boxes [k, 4] float32 in pixels, labels [k] int64, scores [k] float32 and
    query [k] int32, the object query each came from (the row of a decoder attention map)."""
    boxes: torch.Tensor
    labels: torch.Tensor
    scores: torch.Tensor
    query: torch.Tensor


def _check_detect_args(bbox_format, score_threshold, max_detections, Q=None, multilabel=False):
    if bbox_format not in DETECT_FORMATS:
        raise RuntimeError(f"detect: unknown bbox_format {bbox_format!r}, expected one of {tuple(DETECT_FORMATS)}")
    if not math.isfinite(float(score_threshold)):
        raise RuntimeError(f"detect: score_threshold={score_threshold} is not finite")
    if multilabel:                                   # K bounds the (query, class) pairs, not the queries
        if max_detections is not None and not 1 <= int(max_detections) <= hip.MULTILABEL_MAX:
            raise RuntimeError(f"detect: max_detections={max_detections} must be in 1..{hip.MULTILABEL_MAX} with multilabel")
        return
    if max_detections is not None and (int(max_detections) < 1 or (Q is not None and int(max_detections) > Q)):
        raise RuntimeError(f"detect: max_detections={max_detections} must be in 1..Q" + ("" if Q is None else f"={Q} (the number of queries)"))


def _ranked_rows(B, K, dev, n_index):
    """boxes, labels, scores and n_index int32 columns of K rows per image; the kernels write every row: detections, then zeros."""
    return (torch.empty(B, K, 4, dtype=torch.float32, device=dev), torch.empty(B, K, dtype=torch.int64, device=dev),
            torch.empty(B, K, dtype=torch.float32, device=dev), *(torch.empty(B, K, dtype=torch.int32, device=dev) for _ in range(n_index)))


def _detect(logits, boxes, sizes, background_class, score_threshold, max_detections, bbox_format, clip, scoring="softmax", multilabel=False):
    mode = _scoring(scoring)
    multilabel = _multilabel("detect", scoring, multilabel)
    _check_model_outputs("detect", "B", logits, boxes)
    B, Q, _ = logits.shape
    _check_detect_args(bbox_format, score_threshold, max_detections, Q, multilabel)
    logits, boxes = _model_outputs("detect_batched", "post-processing", logits, boxes)
    K = (MULTILABEL_DEFAULT_K if multilabel else Q) if max_detections is None else int(max_detections)
    dev = logits.device
    sizes = torch.as_tensor(sizes).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(sizes.shape) != (B, 2):
        raise RuntimeError(f"detect: sizes must be [B, 2] = (height, width) of every image, got {tuple(sizes.shape)} for B={B}")
    out_b, out_l, out_s, out_q = _ranked_rows(B, K, dev, 1)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    d = hip.DetectDesc()
    _fill_model_outputs(d, logits, boxes, background_class)
    d.B, d.sizes, d.score_threshold = B, sizes.data_ptr(), float(score_threshold)
    d.max_detections, d.bbox_format, d.clip = K, DETECT_FORMATS[bbox_format], int(bool(clip))
    d.out_boxes, d.out_labels, d.out_scores, d.out_query, d.counts = (out_b.data_ptr(), out_l.data_ptr(), out_s.data_ptr(), out_q.data_ptr(),
                                                                      counts.data_ptr())
    if multilabel:
        hip._check(hip.load().detr_hip_detect_multilabel(byref(d), hip._stream()), "detr_hip_detect_multilabel")
    elif mode == 0:
        hip._check(hip.load().detr_hip_detect(byref(d), hip._stream()), "detr_hip_detect")
    else:
        hip._check(hip.load().detr_hip_detect_scored(byref(d), mode, hip._stream()), "detr_hip_detect_scored")
    return out_b, out_l, out_s, out_q, counts


def detect_batched(m_outputs: dict, sizes, background_class, *, score_threshold=0.0, max_detections=None, bbox_format="xyxy", clip=True,
                   scoring="softmax", multilabel=False):
    """[Detections] for every image of the batch, in pixels.  `sizes` [B, 2] = (height, width) of every ORIGINAL image (host
    array or device tensor): the model's boxes are normalised to the image's own extent -- in a padded batch too, where the canvas
    is larger --, so that is what they are scaled by.  A query is kept when its label is not `background_class` and its score
    (max softmax probability, exactly get_model_inference's) is >= score_threshold; the kept ones are sorted by descending score
    (ties: lower query index first) and cut to max_detections (None: all Q).  bbox_format: "xy_center" (cx, cy, w, h), "xyxy",
    "yxyx" or "xywh" (top-left + width / height); clip clamps the corners of the last three to the image.  One launch of
    detr_hip_detect and ONE host synchronisation (the per-image counts).  CUDA inputs only.
    scoring="sigmoid" (a model trained with class_criterion = "focal"): the score is the sigmoid of the best non-background logit, the
    label its first arg-max, and every query is a candidate: the threshold alone decides (detr_hip_detect_scored).
    multilabel=True (scoring="sigmoid" only; "softmax" raises ValueError): a query may emit several classes.  The candidates are all
    Q x (C - 1) (query, non-background class) pairs with sigmoid(logit) >= score_threshold; the max_detections best are returned (None:
    100; 1..1024, independent of Q), descending score, ties by lower query, then lower class -- the rule Deformable DETR, DINO and
    RT-DETR are evaluated under.  `query` repeats where a query emits several classes; every row carries its query's box.  One
    launch of detr_hip_detect_multilabel."""
    out_b, out_l, out_s, out_q, counts = _detect(m_outputs["pred_logits"], m_outputs["pred_boxes"], sizes, background_class,
                                                 score_threshold, max_detections, bbox_format, clip, scoring, multilabel)
    return [Detections(out_b[b, :k], out_l[b, :k], out_s[b, :k], out_q[b, :k]) for b, k in enumerate(counts.tolist())]


MATCH_MODES = {"iou": 0, "ios": 1}                   # ios: intersection over the SMALLER area


class TiledDetections(NamedTuple):
    """The merged detections of ONE image of sliced inference, best first: Detections' four fields plus tile [k] int32, the index
    of the tile (within its image; 0 is the whole image with include_full) each came from -- (tile, query) names the model output row."""
    boxes: torch.Tensor
    labels: torch.Tensor
    scores: torch.Tensor
    query: torch.Tensor
    tile: torch.Tensor


def _check_merge_args(nms_threshold, match, edge_margin, max_detections):
    if match not in MATCH_MODES:
        raise ValueError(f"merge_tiles: match must be one of {tuple(MATCH_MODES)}, got {match!r}")
    if not math.isfinite(float(nms_threshold)):
        raise ValueError(f"merge_tiles: nms_threshold={nms_threshold} is not finite")
    if not (math.isfinite(float(edge_margin)) and float(edge_margin) >= 0.0):
        raise ValueError(f"merge_tiles: edge_margin={edge_margin} must be finite and >= 0")
    if not 1 <= int(max_detections) <= hip.TILE_MAX_CAND:
        raise ValueError(f"merge_tiles: max_detections={max_detections} must be in 1..{hip.TILE_MAX_CAND} (the candidate cap)")


def merge_tiles(m_outputs: dict, tile_start, windows, sizes, background_class, *, score_threshold=0.0, max_detections=100,
                bbox_format="xyxy", clip=True, nms_threshold=0.5, match="iou", class_agnostic=False, edge_margin=0.0, scoring="softmax"):
    """[TiledDetections] for every image of a sliced batch.  m_outputs holds pred_logits [N, Q, C] / pred_boxes [N, Q, 4] of all N
    tiles, the tiles of image b at rows [tile_start[b], tile_start[b + 1]) (tile_start: host int array [B + 1], as
    DeviceInputStage.augmented_tiles returns it); windows [N, 4] = (y0, x0, hc, wc) of every tile in pixels of its image (the fields
    of its PaddedRecord); sizes [B, 2] = (height, width) of every ORIGINAL image.  Per image: candidates as detect_batched keeps
    them (label != background_class, score >= score_threshold), boxes mapped to image pixels (x = x0 + x_tile * wc, ...), the edge
    rule (edge_margin > 0: a box of a window that is not the whole image is dropped when a corner lies within edge_margin pixels of,
    or beyond, a window edge interior to the image -- a truncated object another tile sees whole), then greedy NMS by descending
    score (ties: lower tile, then lower query): a box is dropped when an earlier kept box of its label (any label with
    class_agnostic) matches it by MORE than nms_threshold; match "iou", or "ios" = intersection over the smaller area, which also
    removes a part-box lying inside the box of the whole object.  The first max_detections survivors are returned.  One launch of
    detr_hip_tile_merge and ONE host synchronisation (counts + status).  An image with more than _hip.TILE_MAX_CAND candidates
    raises ValueError.  CUDA inputs only.
    scoring: "softmax" only; "sigmoid" raises NotImplementedError (this kernel scores from the logits itself, by softmax)."""
    if _scoring(scoring) != 0:
        raise NotImplementedError(f"merge_tiles: scoring={scoring!r}: the kernel scores from the logits itself, by softmax only")
    _check_model_outputs("merge_tiles", "N", m_outputs["pred_logits"], m_outputs["pred_boxes"])
    _check_detect_args(bbox_format, score_threshold, None)
    _check_merge_args(nms_threshold, match, edge_margin, max_detections)
    logits, boxes = _model_outputs("merge_tiles", "merge", m_outputs["pred_logits"], m_outputs["pred_boxes"])
    N, K = logits.shape[0], int(max_detections)
    dev = logits.device
    start_h = np.ascontiguousarray(np.asarray(tile_start.cpu() if isinstance(tile_start, torch.Tensor) else tile_start), np.int32)
    if start_h.ndim != 1 or start_h.shape[0] < 2:
        raise RuntimeError(f"merge_tiles: tile_start must be [B + 1] offsets, got shape {tuple(start_h.shape)}")
    B = start_h.shape[0] - 1
    sizes = torch.as_tensor(sizes).to(device=dev, dtype=torch.int32).contiguous()
    windows = torch.as_tensor(windows).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(sizes.shape) != (B, 2) or tuple(windows.shape) != (N, 4):
        raise RuntimeError(f"merge_tiles: sizes must be [B, 2] and windows [N, 4], got {tuple(sizes.shape)} and {tuple(windows.shape)} "
                           f"for B={B}, N={N}")
    start_d = torch.from_numpy(start_h).to(dev)
    out_b, out_l, out_s, out_q, out_t = _ranked_rows(B, K, dev, 2)
    tail = torch.zeros(B + 1, dtype=torch.int32, device=dev)              # counts [B], then the status word
    d = hip.TileMergeDesc()
    _fill_model_outputs(d, logits, boxes, background_class)
    d.B, d.N, d.score_threshold = B, N, float(score_threshold)
    d.tile_start, d.tile_start_host, d.windows, d.sizes = start_d.data_ptr(), start_h.ctypes.data, windows.data_ptr(), sizes.data_ptr()
    d.max_detections, d.bbox_format, d.clip = K, DETECT_FORMATS[bbox_format], int(bool(clip))
    d.match, d.class_agnostic, d.edge_margin, d.nms_threshold = MATCH_MODES[match], int(bool(class_agnostic)), float(edge_margin), float(nms_threshold)
    d.out_boxes, d.out_labels, d.out_scores, d.out_query, d.out_tile = (out_b.data_ptr(), out_l.data_ptr(), out_s.data_ptr(), out_q.data_ptr(),
                                                                        out_t.data_ptr())
    d.counts, d.status = tail.data_ptr(), tail.data_ptr() + 4 * B
    hip._check(hip.load().detr_hip_tile_merge(byref(d), hip._stream()), "detr_hip_tile_merge")
    *counts, status = tail.tolist()
    if status:
        raise ValueError("merge_tiles: " + "; ".join(text for bit, text in hip.TILE_BAD.items() if status & bit))
    return [TiledDetections(out_b[b, :k], out_l[b, :k], out_s[b, :k], out_q[b, :k], out_t[b, :k]) for b, k in enumerate(counts)]


class FusedDetections(NamedTuple):
    """The fused detections of ONE image seen through several views, best first: TiledDetections' five fields -- tile is the VIEW
    (its index within the image, in view_records' order) -- plus members [k] int32, the number of candidates the box was fused from
    (1 except with method "wbf", where (tile, query) name the cluster's first, i.e. best-scoring, member)."""
    boxes: torch.Tensor
    labels: torch.Tensor
    scores: torch.Tensor
    query: torch.Tensor
    tile: torch.Tensor
    members: torch.Tensor


FUSE_THRESHOLDS = {"nms": 0.5, "soft_nms": 0.5, "soft_nms_gaussian": 0.5, "wbf": 0.55}


def _check_fuse_args(method, threshold, match, edge_margin, max_detections, sigma, score_min, expected_views, min_members):
    """-> the fuse[] block of detr_hip_fuse_views and the threshold (the method's default for None)."""
    if method not in hip.FUSE_METHODS:
        raise ValueError(f"fuse_views: method must be one of {tuple(hip.FUSE_METHODS)}, got {method!r}")
    if threshold is None:
        threshold = FUSE_THRESHOLDS[method]
    try:
        _check_merge_args(threshold, match, edge_margin, max_detections)
    except ValueError as e:
        raise ValueError(str(e).replace("merge_tiles", "fuse_views").replace("nms_threshold", "threshold")) from None
    if not (math.isfinite(float(sigma)) and float(sigma) > 0.0):
        raise ValueError(f"fuse_views: sigma={sigma} must be finite and > 0")
    if not (math.isfinite(float(score_min)) and float(score_min) >= 0.0):
        raise ValueError(f"fuse_views: score_min={score_min} must be finite and >= 0")
    if expected_views is not None and (float(expected_views) != int(expected_views) or int(expected_views) < 1):
        raise ValueError(f"fuse_views: expected_views={expected_views} must be None or an integer >= 1")
    if float(min_members) != int(min_members) or int(min_members) < 1:
        raise ValueError(f"fuse_views: min_members={min_members} must be an integer >= 1")
    block = (hip.FUSE_METHODS[method], float(sigma), float(score_min), 0 if expected_views is None else int(expected_views), int(min_members), 0)
    return block, float(threshold)


def fuse_views(m_outputs: dict, view_start, windows, flips, sizes, background_class, *, method="wbf", threshold=None, score_threshold=0.0,
               max_detections=100, bbox_format="xyxy", clip=True, match="iou", class_agnostic=False, edge_margin=0.0, sigma=0.5,
               score_min=0.001, expected_views=None, min_members=1, scoring="softmax"):
    """[FusedDetections] for every image of a batch seen through several VIEWS (test-time augmentation: mirrored, at several shortest
    sides, whole or tiled -- transformation.view_records).  m_outputs, view_start, windows and sizes are merge_tiles' m_outputs,
    tile_start, windows and sizes with a view for a tile; flips [N] says which views saw the MIRRORED image (a flipped record's window
    is a window of the mirrored image).  Candidates, mapping to image pixels and the edge rule are merge_tiles'; a flipped view's box is
    mapped in its own frame and then mirrored back, (x0, x1) <- (W - x1, W - x0).  Then, per image, `method`:
      "nms": merge_tiles' greedy NMS (with no flipped view and a format other than "xy_center", merge_tiles' bits);
      "soft_nms" / "soft_nms_gaussian" (Bodla et al. 2017): the best remaining box is emitted with its CURRENT score, then the scores of
        the remaining boxes of its label (any label with class_agnostic) that match it are decayed -- by (1 - m) where m > threshold, or
        by exp(-m * m / sigma) for every m -- and a box whose score is below score_min is removed;
      "wbf" (weighted box fusion, Solovyev et al. 2021): the candidates are walked by descending score; each joins the cluster of its
        label whose fused box matches it best if by more than `threshold`, else founds one; a cluster's box is the score-weighted mean of
        its members' corners, its score their mean score, times min(members, expected_views) / expected_views when expected_views is
        given (a box only some views found is marked down); clusters of fewer than min_members boxes are dropped.
    `threshold` (strict; None: 0.5, or 0.55 for "wbf") is the match threshold of every method; match, class_agnostic, edge_margin,
    clip and bbox_format as in merge_tiles, except that "xy_center" is derived from the final corners.  The first max_detections
    results are returned, best first.  The defaults are the published methods' conventions (soft-NMS: sigma 0.5, minimum score 0.001;
    WBF: 0.55) carried over, UNTUNED for DETR: there are no trained weights here to tune them on.  One launch of detr_hip_fuse_views
    and ONE host synchronisation (counts + status).  An image with more than _hip.TILE_MAX_CAND candidates, or with "wbf" more than
    _hip.FUSE_MAX_CLUSTERS clusters, raises ValueError.  CUDA inputs only.
    scoring: "softmax" only; "sigmoid" raises NotImplementedError (this kernel scores from the logits itself, by softmax)."""
    if _scoring(scoring) != 0:
        raise NotImplementedError(f"fuse_views: scoring={scoring!r}: the kernel scores from the logits itself, by softmax only")
    _check_model_outputs("fuse_views", "N", m_outputs["pred_logits"], m_outputs["pred_boxes"])
    _check_detect_args(bbox_format, score_threshold, None)
    block, threshold = _check_fuse_args(method, threshold, match, edge_margin, max_detections, sigma, score_min, expected_views, min_members)
    logits, boxes = _model_outputs("fuse_views", "fusion", m_outputs["pred_logits"], m_outputs["pred_boxes"])
    N, K = logits.shape[0], int(max_detections)
    dev = logits.device
    start_h = np.ascontiguousarray(np.asarray(view_start.cpu() if isinstance(view_start, torch.Tensor) else view_start), np.int32)
    if start_h.ndim != 1 or start_h.shape[0] < 2:
        raise RuntimeError(f"fuse_views: view_start must be [B + 1] offsets, got shape {tuple(start_h.shape)}")
    B = start_h.shape[0] - 1
    sizes = torch.as_tensor(sizes).to(device=dev, dtype=torch.int32).contiguous()
    windows = torch.as_tensor(windows).to(device=dev, dtype=torch.int32).contiguous()
    flips = torch.as_tensor(np.asarray(flips.cpu() if isinstance(flips, torch.Tensor) else flips).astype(bool).astype(np.int32)).to(dev)
    if tuple(sizes.shape) != (B, 2) or tuple(windows.shape) != (N, 4) or tuple(flips.shape) != (N,):
        raise RuntimeError(f"fuse_views: sizes must be [B, 2], windows [N, 4] and flips [N], got {tuple(sizes.shape)}, {tuple(windows.shape)} "
                           f"and {tuple(flips.shape)} for B={B}, N={N}")
    start_d = torch.from_numpy(start_h).to(dev)
    out_b, out_l, out_s, out_q, out_t, out_m = _ranked_rows(B, K, dev, 3)
    tail = torch.zeros(B + 1, dtype=torch.int32, device=dev)              # counts [B], then the status word
    d = hip.TileMergeDesc()
    _fill_model_outputs(d, logits, boxes, background_class)
    d.B, d.N, d.score_threshold = B, N, float(score_threshold)
    d.tile_start, d.tile_start_host, d.windows, d.sizes = start_d.data_ptr(), start_h.ctypes.data, windows.data_ptr(), sizes.data_ptr()
    d.max_detections, d.bbox_format, d.clip = K, DETECT_FORMATS[bbox_format], int(bool(clip))
    d.match, d.class_agnostic, d.edge_margin, d.nms_threshold = MATCH_MODES[match], int(bool(class_agnostic)), float(edge_margin), threshold
    d.out_boxes, d.out_labels, d.out_scores, d.out_query, d.out_tile = (out_b.data_ptr(), out_l.data_ptr(), out_s.data_ptr(), out_q.data_ptr(),
                                                                        out_t.data_ptr())
    d.counts, d.status = tail.data_ptr(), tail.data_ptr() + 4 * B
    params = (c_double * hip.FUSE_PARAMS)(*block)
    hip._check(hip.load().detr_hip_fuse_views(byref(d), flips.data_ptr(), byref(params), out_m.data_ptr(), hip._stream()), "detr_hip_fuse_views")
    *counts, status = tail.tolist()
    if status:
        raise ValueError("fuse_views: " + "; ".join(text for bit, text in hip.FUSE_BAD.items() if status & bit))
    return [FusedDetections(out_b[b, :k], out_l[b, :k], out_s[b, :k], out_q[b, :k], out_t[b, :k], out_m[b, :k]) for b, k in enumerate(counts)]


class TrackedDetections(NamedTuple):
    """The detections of ONE frame that belong to a confirmed track, in the detector's order: Detections' four fields, copied bit for
    bit, plus ids [k] int32, the track each belongs to (>= 1, never reused within a stream), and hits [k] int32, the number of frames
    that track has been matched in."""
    boxes: torch.Tensor
    labels: torch.Tensor
    scores: torch.Tensor
    query: torch.Tensor
    ids: torch.Tensor
    hits: torch.Tensor


_T = hip.TRACK_MAX
# one stream of the device state (include/detr_hip.h: detr_track_desc); detr_hip_track_state_bytes is what sizes the buffer
TRACK_STATE = np.dtype([("x", "<f4", (_T, 4)), ("v", "<f4", (_T, 4)), ("label", "<i8", (_T,)), ("score", "<f4", (_T,)), ("id", "<i4", (_T,)),
                        ("hits", "<i4", (_T,)), ("miss", "<i4", (_T,)), ("confirmed", "<i4", (_T,)), ("frame", "<i4"), ("next_id", "<i4"),
                        ("pad", "<i4", (2,))])
TRACK_STATE_KEYS = ("x", "v", "label", "id", "hits", "miss", "confirmed", "score", "frame", "next_id")
# one stream of the motion state (include/detr_hip.h: detr_track_motion_desc); detr_hip_track_motion_state_bytes sizes the buffer
MOTION_STATE = np.dtype([("head", "<i4", (16,)), ("thumb", "u1", (2, hip.MOTION_SIDE * hip.MOTION_SIDE))])
MOTION_HEAD = ("h", "w", "f", "tw", "th", "valid", "slot", "estimated", "sx", "sy", "n", "agree")


class Tracker:
    """Multi-object tracking whose state lives on the device: `streams` independent videos, at most _hip.TRACK_MAX tracks each.

        tracker = Tracker()                                  # one stream
        for frame in video:
            tracked = detector.track(frame, tracker)         # TrackedDetections: the detector's rows plus ids and hits

    Per frame and stream (include/detr_hip.h: detr_track_desc is the normative text): every track is moved by its velocity; the
    detections with score >= track_threshold are associated with the tracks of their label (any label with class_agnostic) by greedy
    descending IoU above match_threshold (ties: lower id, then lower detection); the tracks left over that are confirmed and were
    matched in the frame before get a second chance against the low-score detections above low_match_threshold; a matched track moves
    to prediction + alpha * residual and its velocity by beta * residual; an unmatched one coasts, and is dropped when it is not yet
    confirmed or has missed more than max_age frames; an unmatched detection with score >= new_threshold (None: track_threshold)
    starts a track, confirmed after min_hits matched frames; only detections of confirmed tracks are returned.
    The defaults are ByteTrack's and SORT's conventions carried over; nobody has tuned them for DETR outputs.  The association is
    greedy, not Hungarian; there is no Kalman covariance.

    embed_dim=E turns on tracking by APPEARANCE (include/detr_hip.h: detr_track_embed_desc; one launch as before): every frame also
    hands in an embedding per detection, and every track keeps a unit embedding, an exponential average (momentum) of the detections it
    was matched to.  The first association then walks its pairs -- still only those above match_threshold in IoU -- by
    (1 - appearance_weight) * IoU + appearance_weight * cosine similarity, which keeps the ids of two objects of one class that pass
    each other; and a confirmed track that was lost is found again, wherever it reappears, by a similarity above reid_threshold to an
    unmatched detection that would otherwise start a track (None: no such stage).  Detector.track feeds the model's own descriptor
    (DetrModel return_embeddings, E = 256); update_rows takes any [S, R, E] tensor.  appearance_weight, reid_threshold and momentum are
    the conventions of BoT-SORT-like trackers carried over, UNTUNED: nobody has measured how well DETR's hidden states tell the objects
    of a real video apart.  embed_dim=None (the default) is the tracker described above in every respect.

    motion=True compensates CAMERA MOTION (include/detr_hip.h: detr_track_motion_desc; at most three launches more, no read-back and no
    further synchronisation): every call also hands in the frames (frames=; Detector.track passes the ones it has just uploaded).  Each
    frame is reduced to a luma thumbnail of at most 384 x 384 pixels, its 16 x 16 blocks are matched against the previous frame's
    thumbnail within +-motion_radius thumbnail pixels, and when the blocks' median displacement is one most of them agree on, every
    track of the stream is moved by it before the association -- so a hand-held or vehicle-mounted camera, which moves every box at
    once by more than the IoU gate forgives, no longer costs every track its id.  There is no estimate on the first frame, after a
    change of frame size, on a frame too small or too flat, or when the blocks disagree (a scene cut, a frame filled by moving
    foreground): the frame is then tracked as without motion.  last_motion holds the [S, 6] int32 device tensor (estimated, sx, sy, n,
    agree, f) of the last call, not synchronised.  Translation only: zoom and roll are not modelled.  The shift is quantised to f
    pixels, the thumbnail's reduction factor (4 for 800 x 1333, 5 for 1080p); the alpha-beta update absorbs the remainder.  The
    defaults (radius 8, at least 4 textured blocks, half of them within one pixel of the median) are reasoned, not tuned: what the
    compensation is worth on real hand-held video is UNMEASURED, there is no such video here.  motion=False (the default) launches and
    returns exactly what the tracker above does."""

    def __init__(self, streams=1, device=None, *, track_threshold=0.7, new_threshold=None, match_threshold=0.3, low_match_threshold=0.5,
                 max_age=30, min_hits=3, alpha=0.75, beta=0.25, class_agnostic=False, embed_dim=None, appearance_weight=0.5,
                 reid_threshold=0.8, momentum=0.9, motion=False, motion_radius=8):
        if new_threshold is None:
            new_threshold = track_threshold
        if not 1 <= int(streams) <= 65535:
            raise ValueError(f"Tracker: streams={streams} must be in 1..65535")
        for name, value in (("track_threshold", track_threshold), ("new_threshold", new_threshold), ("match_threshold", match_threshold),
                            ("low_match_threshold", low_match_threshold), ("alpha", alpha), ("beta", beta)):
            if not math.isfinite(float(value)):
                raise ValueError(f"Tracker: {name}={value} is not finite")
        if int(max_age) < 0 or int(min_hits) < 1:
            raise ValueError(f"Tracker: max_age={max_age} must be >= 0 and min_hits={min_hits} >= 1")
        self.embed_dim = None if embed_dim is None else int(embed_dim)
        if self.embed_dim is not None:
            E = self.embed_dim
            if E % 4 or not 4 <= E <= 512:
                raise ValueError(f"Tracker: embed_dim={embed_dim} must be a multiple of 4 in 4..512")
            if not 0.0 <= float(appearance_weight) <= 1.0 or not 0.0 <= float(momentum) <= 1.0:
                raise ValueError(f"Tracker: appearance_weight={appearance_weight} and momentum={momentum} must be in [0, 1]")
            if reid_threshold is not None and not math.isfinite(float(reid_threshold)):
                raise ValueError(f"Tracker: reid_threshold={reid_threshold} is not finite")
            self.appearance_weight, self.momentum = float(appearance_weight), float(momentum)
            self.reid_threshold = None if reid_threshold is None else float(reid_threshold)
        self.motion, self.motion_radius = bool(motion), int(motion_radius)
        if self.motion and not 1 <= self.motion_radius <= hip.MOTION_MAX_RADIUS:
            raise ValueError(f"Tracker: motion_radius={motion_radius} must be in 1..{hip.MOTION_MAX_RADIUS}")
        self.last_motion = None                      # [S, 6] int32 on the device: what the last call estimated
        self.streams = int(streams)
        self.track_threshold, self.new_threshold = float(track_threshold), float(new_threshold)
        self.match_threshold, self.low_match_threshold = float(match_threshold), float(low_match_threshold)
        self.max_age, self.min_hits, self.alpha, self.beta = int(max_age), int(min_hits), float(alpha), float(beta)
        self.class_agnostic = bool(class_agnostic)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RuntimeError(f"Tracker: the state lives on the GPU (the tracker is a HIP kernel; no CPU fallback), not on {self.device}")
        nbytes = int(hip.load().detr_hip_track_state_bytes(self.streams))
        if nbytes != self.streams * TRACK_STATE.itemsize:
            raise RuntimeError(f"Tracker: the library's state is {nbytes} bytes for {self.streams} streams, this binding lays out "
                               f"{self.streams * TRACK_STATE.itemsize}: rebuild the library")
        self._state = torch.empty(self.streams, TRACK_STATE.itemsize, dtype=torch.uint8, device=self.device)
        self._all_active = torch.ones(self.streams, dtype=torch.int32, device=self.device)
        if self.embed_dim is not None:
            E = self.embed_dim
            nbytes = int(hip.load().detr_hip_track_embed_state_bytes(self.streams, E))
            if nbytes != self.streams * _T * E * 4:
                raise RuntimeError(f"Tracker: the library's embedding bank is {nbytes} bytes, this binding lays out {self.streams * _T * E * 4}: "
                                   "rebuild the library")
            self._bank = torch.empty(self.streams, _T, E, dtype=torch.float32, device=self.device)
            self._table = None                       # the kernel's scratch, sized by the widest frame seen
        if self.motion:
            nbytes = int(hip.load().detr_hip_track_motion_state_bytes(self.streams))
            if nbytes != self.streams * MOTION_STATE.itemsize:
                raise RuntimeError(f"Tracker: the library's motion state is {nbytes} bytes, this binding lays out "
                                   f"{self.streams * MOTION_STATE.itemsize}: rebuild the library")
            self._motion = torch.empty(self.streams, MOTION_STATE.itemsize, dtype=torch.uint8, device=self.device)
            d = hip.TrackMotionDesc()
            d.S = self.streams
            self._votes = torch.empty(int(hip.load().detr_hip_workspace_bytes_track_motion(byref(d))), dtype=torch.uint8, device=self.device)
        self.reset()

    # ---- state
    def reset(self, stream=None):
        """Forget every track of `stream` (None: of all streams); its ids start at 1 again.  With motion its motion state is zeroed:
        the next frame has no predecessor."""
        fresh = np.zeros(1, TRACK_STATE)
        fresh["next_id"] = 1
        row = torch.from_numpy(fresh.view(np.uint8).reshape(1, -1)).to(self.device)
        if stream is None:
            self._state.copy_(row.expand(self.streams, -1))
        else:
            if not 0 <= int(stream) < self.streams:
                raise ValueError(f"Tracker.reset: stream={stream} outside 0..{self.streams - 1}")
            self._state[int(stream)].copy_(row[0])
        if self.embed_dim is not None:
            (self._bank if stream is None else self._bank[int(stream)]).zero_()
        if self.motion:
            (self._motion if stream is None else self._motion[int(stream)]).zero_()

    def state_dict(self):
        """The whole state as named host arrays, leading axis = stream: x, v float32 [S, T, 4]; label int64, id, hits, miss int32,
        confirmed bool, score float32 [S, T]; frame, next_id int32 [S] (T = _hip.TRACK_MAX; a free slot is all zeros).  One copy to the
        host.  With embed_dim: plus embed float32 [S, T, E], the unit embedding of every slot (a second copy).  With motion: plus
        motion_head int32 [S, 16] (MOTION_HEAD names the first twelve) and motion_thumb uint8 [S, 2, 384 * 384], the two thumbnail slots."""
        raw = self._state.cpu().numpy().reshape(-1).view(TRACK_STATE)
        out = {k: np.ascontiguousarray(raw[k]) for k in TRACK_STATE_KEYS}
        out["confirmed"] = out["confirmed"] != 0
        if self.embed_dim is not None:
            out["embed"] = self._bank.cpu().numpy()
        if self.motion:
            raw = self._motion.cpu().numpy().reshape(-1).view(MOTION_STATE)
            out["motion_head"], out["motion_thumb"] = np.ascontiguousarray(raw["head"]), np.ascontiguousarray(raw["thumb"])
        return out

    def load_state_dict(self, state):
        """Take over a state_dict(): the video goes on bit-identically."""
        missing = [k for k in TRACK_STATE_KEYS + (("embed",) if self.embed_dim is not None else ())
                   + (("motion_head", "motion_thumb") if self.motion else ()) if k not in state]
        if missing:
            raise ValueError(f"Tracker.load_state_dict: missing {missing}")
        if self.embed_dim is not None:
            bank = np.asarray(state["embed"])
            if bank.shape != tuple(self._bank.shape):
                raise ValueError(f"Tracker.load_state_dict: embed has shape {bank.shape}, expected {tuple(self._bank.shape)}")
        if self.motion:
            moved = np.zeros(self.streams, MOTION_STATE)
            for k, name in (("head", "motion_head"), ("thumb", "motion_thumb")):
                value = np.asarray(state[name])
                if value.shape != moved[k].shape:
                    raise ValueError(f"Tracker.load_state_dict: {name} has shape {value.shape}, expected {moved[k].shape}")
                moved[k] = value
        raw = np.zeros(self.streams, TRACK_STATE)
        for k in TRACK_STATE_KEYS:
            value = np.asarray(state[k])
            if value.shape != raw[k].shape:
                raise ValueError(f"Tracker.load_state_dict: {k} has shape {value.shape}, expected {raw[k].shape} ({self.streams} streams)")
            raw[k] = value
        self._state.copy_(torch.from_numpy(raw.view(np.uint8).reshape(self.streams, -1)))
        if self.embed_dim is not None:
            self._bank.copy_(torch.from_numpy(np.ascontiguousarray(bank, np.float32)))
        if self.motion:
            self._motion.copy_(torch.from_numpy(moved.view(np.uint8).reshape(self.streams, -1)))

    # ---- frames
    def _launch_motion(self, frames, active, status):
        """detr_hip_track_motion on the current stream: the tracks of every stream move with its camera.  `status` is the device
        address of the status word the tracker's launch behind it shares."""
        from .overlay import RaggedFrames, _check_frames, _upload_frames
        S = self.streams
        if isinstance(frames, RaggedFrames):
            sizes, offsets, buf = frames.sizes, frames.offsets, frames.buffer
            if not (isinstance(buf, torch.Tensor) and buf.device == self._state.device and buf.dtype == torch.uint8 and buf.is_contiguous()):
                raise ValueError(f"Tracker: frames.buffer must be a contiguous uint8 tensor on {self._state.device}")
            keep, base, nbytes = [buf], buf.data_ptr(), buf.numel()
        else:
            try:
                images, sizes, on_device = _check_frames(frames)
            except (TypeError, ValueError) as e:
                raise type(e)(str(e).replace("draw_detections", "Tracker: frames")) from None
            if on_device and any(im.device != self._state.device for im in images):
                raise ValueError(f"Tracker: frames on the device must be on {self._state.device}")
            with torch.cuda.device(self.device):
                keep, base, offsets = _upload_frames(images, on_device, self.device)
            nbytes = int((offsets + sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3).max())
        if sizes.shape[0] != S:
            raise ValueError(f"Tracker: {sizes.shape[0]} frames for {S} streams")
        # offsets (int64) | sizes (int32) in one transfer; the result behind them
        meta = torch.from_numpy(np.concatenate([np.ascontiguousarray(offsets, np.int64).view(np.uint8),
                                                np.ascontiguousarray(sizes, np.int32).reshape(-1).view(np.uint8)])).to(self.device)
        out = torch.empty(S, 6, dtype=torch.int32, device=self.device)
        d = hip.TrackMotionDesc()
        d.S, d.frames, d.frames_bytes, d.offsets, d.sizes = S, base, nbytes, meta.data_ptr(), meta.data_ptr() + 8 * S
        d.active, d.radius = active.data_ptr(), self.motion_radius
        d.motion_state, d.motion_state_bytes = self._motion.data_ptr(), self._motion.numel()
        d.state, d.state_bytes = self._state.data_ptr(), self._state.numel()
        d.workspace, d.workspace_bytes = self._votes.data_ptr(), self._votes.numel()
        d.out_motion, d.status = out.data_ptr(), status
        with torch.cuda.device(self.device):
            hip._check(hip.load().detr_hip_track_motion(byref(d), hip._stream()), "detr_hip_track_motion")
        del keep                    # (freed blocks are reused in stream order: the launches above still own them)
        self.last_motion = out

    def _launch(self, boxes, labels, scores, query, counts, active, embeddings=None, frames=None):
        S = self.streams
        if boxes.dim() != 3 or boxes.shape[0] != S or boxes.shape[2] != 4 or not 1 <= boxes.shape[1] <= 1024:
            raise ValueError(f"Tracker: boxes must be [S={S}, D, 4] with D in 1..1024, got {tuple(boxes.shape)}")
        D = int(boxes.shape[1])
        for name, t, dtype, shape in (("boxes", boxes, torch.float32, (S, D, 4)), ("labels", labels, torch.int64, (S, D)),
                                      ("scores", scores, torch.float32, (S, D)), ("query", query, torch.int32, (S, D)),
                                      ("counts", counts, torch.int32, (S,)), ("active", active, torch.int32, (S,))):
            if t is None and name == "query":
                continue
            if t.device != self._state.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"Tracker: {name} must be a contiguous {dtype} tensor {shape} on {self._state.device}, got {t.dtype} "
                                 f"{tuple(t.shape)} on {t.device}")
        if (embeddings is None) != (self.embed_dim is None):
            raise ValueError("Tracker: embeddings= is mandatory with embed_dim and refused without: this tracker was built with "
                             f"embed_dim={self.embed_dim}")
        if embeddings is not None:
            e = embeddings
            if (not torch.is_tensor(e) or e.device != self._state.device or e.dtype != torch.float32 or e.dim() != 3 or e.shape[0] != S
                    or e.shape[1] < 1 or e.shape[2] != self.embed_dim or e.stride(2) != 1 or e.stride(1) < self.embed_dim or e.stride(0) < 0
                    or e.data_ptr() % 16):
                raise ValueError(f"Tracker: embeddings must be a float32 tensor [S={S}, R, E={self.embed_dim}] on {self._state.device} with "
                                 "contiguous, 16-byte aligned rows, got "
                                 f"{(e.dtype, tuple(e.shape), e.stride(), e.device) if torch.is_tensor(e) else type(e).__name__}")
        if (frames is None) == self.motion:
            raise ValueError(f"Tracker: frames= is mandatory with motion and refused without: this tracker was built with motion={self.motion}")
        out_b, out_l, out_s, out_q, out_i, out_h = _ranked_rows(S, D, self.device, 3)
        tail = torch.zeros(S + 1, dtype=torch.int32, device=self.device)       # counts [S], then the status word
        if self.motion:
            self._launch_motion(frames, active, tail.data_ptr() + 4 * S)
        d = hip.TrackDesc() if embeddings is None else hip.TrackEmbedDesc()
        d.S, d.D, d.state, d.state_bytes = S, D, self._state.data_ptr(), self._state.numel()
        d.boxes, d.labels, d.scores, d.query = boxes.data_ptr(), labels.data_ptr(), scores.data_ptr(), hip.ptr(query)
        d.counts, d.active = counts.data_ptr(), active.data_ptr()
        d.track_threshold, d.new_threshold = self.track_threshold, self.new_threshold
        d.match_threshold, d.low_match_threshold = self.match_threshold, self.low_match_threshold
        d.max_age, d.min_hits, d.alpha, d.beta, d.class_agnostic = self.max_age, self.min_hits, self.alpha, self.beta, int(self.class_agnostic)
        d.out_boxes, d.out_labels, d.out_scores = out_b.data_ptr(), out_l.data_ptr(), out_s.data_ptr()
        d.out_query, d.out_ids, d.out_hits = out_q.data_ptr(), out_i.data_ptr(), out_h.data_ptr()
        d.out_counts, d.status = tail.data_ptr(), tail.data_ptr() + 4 * S
        with torch.cuda.device(self.device):
            if embeddings is None:
                hip._check(hip.load().detr_hip_track(byref(d), hip._stream()), "detr_hip_track")
                return (out_b, out_l, out_s, out_q, out_i, out_h), tail
            d.embed, d.sE_s, d.sE_r, d.R, d.E = embeddings.data_ptr(), embeddings.stride(0), embeddings.stride(1), embeddings.shape[1], self.embed_dim
            d.embed_state, d.embed_state_bytes = self._bank.data_ptr(), self._bank.numel() * 4
            need = hip._ws_query("detr_hip_workspace_bytes_track_embed", ("track_embed", S, D), byref(d))
            if self._table is None or self._table.numel() * 8 < need:
                self._table = torch.empty(need // 8, dtype=torch.float64, device=self.device)
            d.workspace, d.workspace_bytes = self._table.data_ptr(), self._table.numel() * 8
            d.appearance_weight, d.momentum = self.appearance_weight, self.momentum
            d.reid, d.reid_threshold = int(self.reid_threshold is not None), 0.0 if self.reid_threshold is None else self.reid_threshold
            hip._check(hip.load().detr_hip_track_embed(byref(d), hip._stream()), "detr_hip_track_embed")
        return (out_b, out_l, out_s, out_q, out_i, out_h), tail

    def _active(self, active):
        if active is None:
            return self._all_active
        flags = np.asarray(active.cpu() if isinstance(active, torch.Tensor) else active).astype(bool)
        if flags.shape != (self.streams,):
            raise ValueError(f"Tracker: active must hold one flag per stream ({self.streams}), got shape {flags.shape}")
        return torch.from_numpy(flags.astype(np.int32)).to(self.device)

    def update_rows(self, boxes, labels, scores, query, counts, active=None, embeddings=None, frames=None):
        """One frame per stream from padded DEVICE rows, as detr_hip_detect / detr_hip_tile_merge write them with bbox_format "xyxy":
        boxes [S, D, 4] float32, labels [S, D] int64, scores [S, D] float32, query [S, D] int32 or None, counts [S] int32 -- D <= 1024;
        rows behind counts[s] are not read.  active: one flag per stream (None: all); a stream whose flag is 0 keeps its state and
        returns nothing, e.g. a video that delivered no frame.  No packing and no synchronisation before the launch; ONE host
        synchronisation after it (the emitted counts and the status word).  -> [TrackedDetections], one per stream.  A stream with more
        than _hip.TRACK_MAX live tracks raises ValueError AFTER the state has been updated: the state stays valid, the detections
        that found no slot are not tracked.
        embeddings (mandatory with embed_dim, refused without): float32 [S, R, E] on the device, rows contiguous; the embedding of
        detection d of stream s is row query[s, d] (row d with query None).  A row index outside [0, R) or a non-finite row raises
        ValueError the same way: the frame has been tracked with the zero embedding for that detection.
        frames (mandatory with motion, refused without): the frame of every stream, as draw_detections takes them -- an
        overlay.RaggedFrames (DeviceInputStage.last_upload), or a list of uint8 [h, w, 3] host arrays (uploaded once) or device tensors
        (used where they are).  The tracks are moved by the estimated camera shift first (last_motion), then associated as above."""
        rows, tail = self._launch(boxes, labels, scores, query, counts, self._active(active), embeddings, frames)
        *n, status = tail.tolist()
        if status:
            raise ValueError("Tracker: " + "; ".join(text for bit, text in hip.TRACK_ALL_BAD.items() if status & bit))
        return [TrackedDetections(*(r[s, :k] for r in rows)) for s, k in enumerate(n)]

    def update(self, detections, active=None, embeddings=None, frames=None):
        """One frame per stream: `detections` holds, per stream, a Detections / TiledDetections with boxes in "xyxy" pixels, or a
        (boxes [k, 4], labels [k], scores [k]) triple (its query is 0); a single one is taken as the frame of a one-stream tracker.
        They are packed into padded rows (as draw_detections packs them) and go through update_rows.  embeddings: update_rows'; the
        rows are the detections' query, and for a triple, which has none, its k detections take the rows 0..k-1 (and are emitted with
        those as query).  frames: update_rows'."""
        if isinstance(detections, (Detections, TiledDetections, FusedDetections)) or (isinstance(detections, tuple) and len(detections) == 3
                                                                       and not isinstance(detections[0], (tuple, list))):
            detections = [detections]
        if len(detections) != self.streams:
            raise ValueError(f"Tracker.update: {len(detections)} frames for {self.streams} streams")
        from .overlay import _pack_detections
        rows = [(torch.as_tensor(d[0]).reshape(-1, 4), torch.as_tensor(d[1]).reshape(-1), torch.as_tensor(d[2]).reshape(-1)) for d in detections]
        if max(int(r[0].shape[0]) for r in rows) > 1024:
            raise ValueError("Tracker.update: more than 1024 detections in one frame")
        boxes, labels, scores, counts = _pack_detections(rows, True, self.device)
        query = torch.zeros(labels.shape, dtype=torch.int32, device=self.device)
        for s, d in enumerate(detections):
            if hasattr(d, "query") and counts[s]:
                query[s, :counts[s]] = d.query.to(self.device)
            elif embeddings is not None and counts[s]:
                query[s, :counts[s]] = torch.arange(int(counts[s]), dtype=torch.int32, device=self.device)
        return self.update_rows(boxes, labels, scores, query, torch.from_numpy(counts).to(self.device), active, embeddings, frames)


class Detector:
    """Raw images in, pixel-space detections out (what the reference's webcam_inference.py:26-34 and eval.py:41-55 assemble by hand).

        detector = Detector(model, config, score_threshold=0.7)
        detections = detector([image_a, image_b])            # uint8 [h, w, 3] arrays of any, mixed sizes
        for box, label, score in zip(detections[0].boxes.tolist(), detections[0].labels.tolist(), detections[0].scores.tolist()): ...

    resize="shortest_side" (the DETR evaluation rule): every image keeps its aspect ratio -- transformation.eval_record, the record
    the loaders' "shortest_side" mode draws: shortest side `shortest_side`, longest side <= max_size --, the batch is padded
    (DeviceInputStage.augmented_padded) and the model runs on the (images, masks) pair.  `canvas` = (H, W) fixes the padded shape,
    so that the model's captured evaluation graph keeps replaying from call to call; None sizes it per call.
    resize="fixed" (the reference's path): every image is resized to config.image_size (DeviceInputStage.images); the images of one
    call must then have one size.
    The boxes come back in pixels of each ORIGINAL image whichever way it was resized.  The remaining arguments are
    detect_batched's; background_class defaults to config.background_class.

    tiles=(rows, cols) turns on SLICED inference (resize="shortest_side" only): every image is cut into rows x cols windows that
    overlap by `overlap` (transformation.tile_records; plus the whole image with include_full), each window is resized by the same
    shortest-side rule, the model runs on all tiles of the call (in chunks of at most tile_batch; None: one batch) and ONE
    merge_tiles launch maps the boxes back and removes the duplicates (nms_threshold, default 0.5 here; match, class_agnostic,
    edge_margin: see merge_tiles).  The results are TiledDetections.  nms_threshold without tiles runs the same class-wise NMS behind
    the single pass (one whole-image window per image).  With neither, the call is the plain path above.

    flip=True, scales=(s0, s1, ...) and merge= turn on TEST-TIME AUGMENTATION (resize="shortest_side" only): every image is seen at
    every shortest side of `scales` (None: shortest_side alone) and, with flip, mirrored as well (transformation.view_records; with
    tiles, every view is the tiled one), the model runs on all views (in chunks of at most tile_batch) and ONE fuse_views launch
    maps the boxes back -- mirrored views included -- and combines them by `merge`: "nms", "soft_nms", "soft_nms_gaussian" or "wbf"
    (sigma, score_min, min_members: see fuse_views; nms_threshold, when given, is the fusion threshold; expected_views is the number of
    views without tiles, None with them).  The results are FusedDetections.  The cost is one forward pass per view.  With
    flip=False, scales=None and merge="nms" (the defaults) nothing of this runs.

    scoring: "softmax" or "sigmoid" (detect_batched's); None takes it from config.class_criterion ("focal" -> "sigmoid").  The
    plain path and track() score that way; tiles, nms_threshold, flip, scales and merge with "sigmoid" raise NotImplementedError.

    multilabel=True (sigmoid scoring only; ValueError otherwise): the plain path and track() return the max_detections best (query,
    class) pairs of every image instead of one detection per query (detect_batched's multilabel; max_detections up to 1024).  The
    rows have the same layout, so track(), draw() and to_coco_results() take them unchanged; `query` repeats where a query emits
    several classes.  What "sigmoid" rejects stays rejected."""

    RESIZE_MODES = ("shortest_side", "fixed")

    def __init__(self, model, config, *, background_class=None, score_threshold=0.7, max_detections=100, bbox_format="xyxy",
                 resize="shortest_side", shortest_side=800, max_size=1333, canvas=None, interpolation="cubic",
                 tiles=None, overlap=0.2, include_full=True, tile_batch=None, nms_threshold=None, match="iou", class_agnostic=False,
                 edge_margin=0.0, flip=False, scales=None, merge="nms", sigma=0.5, score_min=0.001, min_members=1, scoring=None,
                 multilabel=False):
        from .data import processing, transformation
        self.scoring = scoring_of(config) if scoring is None else scoring
        _scoring(self.scoring)
        if self.scoring != "softmax" and (tiles is not None or nms_threshold is not None or flip or scales is not None or merge != "nms"):
            raise NotImplementedError(f"Detector: scoring={self.scoring!r} with tiles / nms_threshold / flip / scales / merge: merge_tiles and "
                                      "fuse_views score from the logits themselves, by softmax only; use the plain path")
        self.multilabel = _multilabel("Detector", self.scoring, multilabel)
        if resize not in self.RESIZE_MODES:
            raise ValueError(f"Detector: resize must be one of {self.RESIZE_MODES}, got {resize!r}")
        names = transformation.INTERP_NAMES if resize == "shortest_side" else tuple(processing.INTERPOLATIONS)
        if interpolation not in names:
            raise ValueError(f"Detector: interpolation must be one of {names} with resize={resize!r}, got {interpolation!r}")
        _check_detect_args(bbox_format, score_threshold, max_detections, multilabel=self.multilabel)
        if background_class is None:
            background_class = getattr(config, "background_class", None)
        if background_class is None:
            raise ValueError("Detector: background_class is not given and config.background_class is not set")
        if int(shortest_side) < 1 or (max_size is not None and int(max_size) < 1):
            raise ValueError(f"Detector: bad shortest_side={shortest_side} / max_size={max_size}")
        self.model, self.config = model, config
        self.background_class, self.score_threshold, self.max_detections = int(background_class), float(score_threshold), int(max_detections)
        self.bbox_format, self.resize, self.interpolation = bbox_format, resize, interpolation
        self.shortest_side, self.max_size = int(shortest_side), None if max_size is None else int(max_size)
        self.canvas = None if canvas is None else (int(canvas[0]), int(canvas[1]))
        if merge not in hip.FUSE_METHODS:
            raise ValueError(f"Detector: merge must be one of {tuple(hip.FUSE_METHODS)}, got {merge!r}")
        self.flip, self.merge = bool(flip), merge
        self.scales = None if scales is None else tuple(scales)
        self.views = self.flip or self.scales is not None or merge != "nms"         # False: every path below is the one it was
        if self.views:
            if resize != "shortest_side":
                raise ValueError(f"Detector: flip / scales / merge need resize='shortest_side', not {resize!r} (every view is resized by the "
                                 "shortest-side rule)")
            if tile_batch is not None and int(tile_batch) < 1:
                raise ValueError(f"Detector: tile_batch={tile_batch} must be positive")
            transformation.view_records(1, 1, (self.shortest_side,) if self.scales is None else self.scales, self.max_size)    # validates scales
            _, self.fuse_threshold = _check_fuse_args(merge, nms_threshold, match, edge_margin, max_detections, sigma, score_min, None, min_members)
        self.sigma, self.score_min, self.min_members = float(sigma), float(score_min), int(min_members)
        if tiles is not None:
            if resize != "shortest_side":
                raise ValueError(f"Detector: tiles needs resize='shortest_side', not {resize!r} (every window is resized by the shortest-side rule)")
            tiles = (int(tiles[0]), int(tiles[1]))
            if tiles[0] < 1 or tiles[1] < 1 or not (0.0 <= float(overlap) < 1.0):
                raise ValueError(f"Detector: bad tiles={tiles} / overlap={overlap} (a grid of at least 1 x 1, overlap in [0, 1))")
            if tile_batch is not None and int(tile_batch) < 1:
                raise ValueError(f"Detector: tile_batch={tile_batch} must be positive")
            if nms_threshold is None:
                nms_threshold = 0.5
        if nms_threshold is not None:
            _check_merge_args(nms_threshold, match, edge_margin, max_detections)
        self.tiles, self.overlap, self.include_full = tiles, float(overlap), bool(include_full)
        self.tile_batch = None if tile_batch is None else int(tile_batch)
        self.nms_threshold = None if nms_threshold is None else float(nms_threshold)
        self.match, self.class_agnostic, self.edge_margin = match, bool(class_agnostic), float(edge_margin)
        self._stage = None
        self._last_frames = None                     # the frames of the last call: draw(images=None) draws on them

    def stage(self):
        if self._stage is None:
            from .data.processing import DeviceInputStage
            self._stage = DeviceInputStage(self.config, device=self.model.device,
                                           interpolation=self.interpolation if self.resize == "fixed" else "cubic")
        return self._stage

    def records(self, images):
        """The evaluation PaddedRecord of every image (resize="shortest_side")."""
        from .data import transformation as T
        interp = T.INTERP_NAMES.index(self.interpolation)
        return [T.eval_record(im.shape[0], im.shape[1], self.shortest_side, self.max_size, interp) for im in images]

    def tile_records(self, images):
        """Per image, the PaddedRecords of its tiles (tiles=(rows, cols)): transformation.tile_records."""
        from .data import transformation as T
        interp = T.INTERP_NAMES.index(self.interpolation)
        return [T.tile_records(im.shape[0], im.shape[1], self.tiles[0], self.tiles[1], self.overlap, self.shortest_side, self.max_size,
                               interp, self.include_full) for im in images]

    def _merge(self, m_outputs, tile_start, windows, sizes):
        return merge_tiles(m_outputs, tile_start, windows, sizes, self.background_class, score_threshold=self.score_threshold,
                           max_detections=self.max_detections, bbox_format=self.bbox_format, nms_threshold=self.nms_threshold,
                           match=self.match, class_agnostic=self.class_agnostic, edge_margin=self.edge_margin)

    def view_records(self, images):
        """Per image, the PaddedRecords of its views (flip / scales, with tiles the tiles of every view): transformation.view_records."""
        from .data import transformation as T
        interp = T.INTERP_NAMES.index(self.interpolation)
        scales = (self.shortest_side,) if self.scales is None else self.scales
        return [T.view_records(im.shape[0], im.shape[1], scales, self.max_size, self.flip, interp, self.tiles, self.overlap, self.include_full)
                for im in images]

    def _viewed(self, srcs, sizes):
        """Test-time augmentation: one upload per image, the model on chunks of views, one fusion launch."""
        recs = self.view_records(srcs)
        images, masks, view_start = self.stage().augmented_tiles(srcs, recs, canvas=self.canvas)
        windows = np.array([(t.y0, t.x0, t.hc, t.wc) for r in recs for t in r], np.int32)
        flips = np.array([t.flip for r in recs for t in r], np.int32)
        # a tile sees only part of the image: rescaling by the number of views would mark every object down
        expected = None if self.tiles is not None else len(recs[0])
        return fuse_views(self._run_chunks(images, masks), view_start, windows, flips, sizes, self.background_class, method=self.merge,
                          threshold=self.fuse_threshold, score_threshold=self.score_threshold, max_detections=self.max_detections,
                          bbox_format=self.bbox_format, match=self.match, class_agnostic=self.class_agnostic, edge_margin=self.edge_margin,
                          sigma=self.sigma, score_min=self.score_min, expected_views=expected, min_members=self.min_members)

    def _tiled(self, srcs, sizes):
        """Sliced inference: one upload per image, the model on chunks of tiles, one merge launch."""
        recs = self.tile_records(srcs)
        images, masks, tile_start = self.stage().augmented_tiles(srcs, recs, canvas=self.canvas)
        windows = np.array([(t.y0, t.x0, t.hc, t.wc) for r in recs for t in r], np.int32)
        return self._merge(self._run_chunks(images, masks), tile_start, windows, sizes)

    def _run_chunks(self, images, masks):
        """The model on the N staged tiles / views in chunks of at most tile_batch -> pred_logits and pred_boxes of all N."""
        N = images.shape[0]
        step = N if self.tile_batch is None else self.tile_batch
        logits = boxes = None
        for at in range(0, N, step):
            out = self.model((images[at:at + step], masks[at:at + step]), training=False)
            if logits is None:
                logits = torch.empty((N,) + tuple(out["pred_logits"].shape[1:]), dtype=torch.float32, device=images.device)
                boxes = torch.empty((N,) + tuple(out["pred_boxes"].shape[1:]), dtype=torch.float32, device=images.device)
            logits[at:at + step] = out["pred_logits"]                  # a replayed graph reuses its output buffers: copy out
            boxes[at:at + step] = out["pred_boxes"]
        return {"pred_logits": logits, "pred_boxes": boxes}

    def _forward(self, srcs, sizes, need_weights=None, return_embeddings=False):
        """The single pass: input stage and model on the frames `srcs` -> (m_outputs, the input's shape)."""
        extra = dict(return_embeddings=True) if return_embeddings else {}
        if self.resize == "fixed":
            if (sizes != sizes[0]).any():
                raise ValueError(f"Detector: resize='fixed' takes images of ONE size per call, got {sorted(set(map(tuple, sizes.tolist())))}; "
                                 "resize='shortest_side' batches mixed sizes")
            inputs = self.stage().images(np.stack(srcs))
            shape = inputs.shape
            self._last_frames = srcs                                    # (this path uploads one dense batch: kept on the host)
        else:
            inputs = self.stage().augmented_padded(srcs, self.records(srcs), canvas=self.canvas)
            shape = inputs[0].shape
            self._last_frames = self.stage().last_upload                # already on the device: they cross PCIe once
        return self.model(inputs, training=False, need_weights=need_weights, **extra), shape

    def __call__(self, images, need_weights=None):
        """images: one uint8 [h, w, 3] array -> Detections, or a list of them -> [Detections] (TiledDetections with tiles or
        nms_threshold).  With need_weights (DetrModel.__call__) the result is (detections, maps), maps as get_attention_maps returns
        them; not with tiles."""
        single = not isinstance(images, (list, tuple))
        srcs = [np.asarray(im) for im in ([images] if single else images)]
        if not srcs or any(s.dtype != np.uint8 or s.ndim != 3 or s.shape[-1] != 3 for s in srcs):
            raise TypeError("Detector expects a uint8 image [h, w, 3] or a non-empty list of them")
        sizes = np.array([s.shape[:2] for s in srcs], np.int32)
        if self.views:
            if need_weights:
                raise NotImplementedError("Detector: need_weights with flip / scales / merge: there is one attention map per view and no single "
                                          "image to overlay it on; call the model on DeviceInputStage.augmented_tiles yourself")
            detections = self._viewed(srcs, sizes)
            self._last_frames = self.stage().last_upload
            return detections[0] if single else detections
        if self.tiles is not None:
            if need_weights:
                raise NotImplementedError("Detector: need_weights with tiles: there is one attention map per tile and no single image to "
                                          "overlay it on; call the model on DeviceInputStage.augmented_tiles yourself")
            detections = self._tiled(srcs, sizes)
            self._last_frames = self.stage().last_upload
            return detections[0] if single else detections
        m_outputs, shape = self._forward(srcs, sizes, need_weights)
        if self.nms_threshold is not None:                              # one whole-image window per image
            windows = np.concatenate([np.zeros_like(sizes), sizes], 1)
            detections = self._merge(m_outputs, np.arange(len(srcs) + 1, dtype=np.int32), windows, sizes)
        else:
            detections = detect_batched(m_outputs, sizes, self.background_class, score_threshold=self.score_threshold,
                                        max_detections=self.max_detections, bbox_format=self.bbox_format, scoring=self.scoring,
                                        multilabel=self.multilabel)
        detections = detections[0] if single else detections
        if "attn" in m_outputs:
            return detections, _feature_maps(self.model, shape, m_outputs["attn"])
        return detections

    def track(self, images, tracker, active=None):
        """One video frame per stream of `tracker` (a Tracker with as many streams as there are images): the detections of __call__
        that belong to a confirmed track, as TrackedDetections (a list for a list of images).  The plain path hands detr_hip_detect's
        raw rows and device counts to Tracker.update_rows: one launch more than __call__ and ONE host synchronisation per frame, the
        tracker's counts.  With tiles / nms_threshold the frame goes through merge_tiles first, which synchronises once itself: two per
        frame.  Needs bbox_format="xyxy".  active: Tracker.update_rows'.
        A tracker with embed_dim (it must be 256) tracks by appearance: the model is called with return_embeddings and its out["embed"]
        goes to update_rows with detr_hip_detect's query rows -- one launch more (the copy of the embeddings), no further
        synchronisation.  Not with tiles / nms_threshold: that path keeps no per-tile embeddings.
        A tracker with motion is handed the frames this call has just uploaded (DeviceInputStage.last_upload; the host frames with
        resize="fixed", which uploads a dense batch) on every path -- with tiles they are the whole images --: at most three launches
        more, no further synchronisation."""
        if self.bbox_format != "xyxy":
            raise ValueError(f"Detector.track: boxes must be 'xyxy' pixels: build the Detector with bbox_format='xyxy', not {self.bbox_format!r}")
        if not isinstance(tracker, Tracker):
            raise TypeError(f"Detector.track: tracker must be a Tracker, got {type(tracker).__name__}")
        single = not isinstance(images, (list, tuple))
        srcs = [np.asarray(im) for im in ([images] if single else images)]
        if not srcs or any(s.dtype != np.uint8 or s.ndim != 3 or s.shape[-1] != 3 for s in srcs):
            raise TypeError("Detector expects a uint8 image [h, w, 3] or a non-empty list of them")
        if len(srcs) != tracker.streams:
            raise ValueError(f"Detector.track: {len(srcs)} images for a tracker of {tracker.streams} streams")
        appearance = tracker.embed_dim is not None
        if appearance and tracker.embed_dim != 256:
            raise ValueError(f"Detector.track: the model's embeddings have 256 elements, the tracker was built with embed_dim={tracker.embed_dim}")
        if self.tiles is not None or self.nms_threshold is not None or self.views:
            if appearance:
                raise NotImplementedError("Detector.track: tracking by appearance with tiles / nms_threshold / views: that path keeps no per-tile "
                                          "embeddings; use a Tracker without embed_dim, or a Detector without tiles, nms_threshold and views")
            detections = self(srcs)
            tracked = tracker.update(detections, active, frames=self._last_frames if tracker.motion else None)
        else:
            sizes = np.array([s.shape[:2] for s in srcs], np.int32)
            m_outputs, _ = self._forward(srcs, sizes, return_embeddings=appearance)
            rows = _detect(m_outputs["pred_logits"], m_outputs["pred_boxes"], sizes, self.background_class, self.score_threshold,
                           self.max_detections, self.bbox_format, True, self.scoring, self.multilabel)
            tracked = tracker.update_rows(*rows, active, m_outputs["embed"] if appearance else None,
                                          self._last_frames if tracker.motion else None)
        return tracked[0] if single else tracked

    def attention_site(self, site="dec"):
        """The key of `maps` a site names: "dec" = the last decoder cross-attention (one row per object query), "enc" = the last
        encoder self-attention; anything else is taken as the key itself."""
        sites = self.model.default_attn_sites()
        for name in sites:
            if (site == "dec" and "/decoder/" in name) or (site == "enc" and "/encoder/" in name):
                return name
        return site

    def heat_map(self, detections, maps, sizes, site="dec"):
        """(heat [B, Hf, Wf], heat_scale [B], heat_extent [B, 2]) for draw_detections: per image the sum of the rows
        Detections.query of maps[site] [B, Q, Hf, Wf], 1 / its maximum (0 for an all-zero map) -- both computed on the device, nothing
        is read back -- and the part of the map the image covers: its resized hd x wd inside the canvas divided by the backbone's
        total stride (engine.backbone_stride); the whole map with resize="fixed".  sizes [B, 2]: (height, width) of the frames."""
        from .engine import backbone_stride
        m = maps[self.attention_site(site)]
        if m.dim() != 4 or m.shape[0] != len(detections):
            raise ValueError(f"Detector.heat_map: maps[{site!r}] must be [B={len(detections)}, Q, Hf, Wf], got {tuple(m.shape)}")
        heat = torch.stack([m[b].index_select(0, d.query.to(torch.int64)).sum(0) for b, d in enumerate(detections)]).float().contiguous()
        peak = heat.amax(dim=(1, 2))
        scale = torch.where(peak > 0, 1.0 / peak, torch.zeros_like(peak))
        Hf, Wf = int(m.shape[2]), int(m.shape[3])
        if self.resize == "fixed":
            extent = [(Hf, Wf)] * len(detections)
        else:
            from .data import transformation as T
            stride = backbone_stride(self.model.engine.dilate)
            interp = T.INTERP_NAMES.index(self.interpolation)
            recs = [T.eval_record(int(h), int(w), self.shortest_side, self.max_size, interp) for h, w in np.asarray(sizes).tolist()]
            extent = [(r.hd / stride, r.wd / stride) for r in recs]
        return heat, scale, extent

    def draw(self, images, detections, class_names, maps=None, site="dec", **kw):
        """The frames with `detections` (this detector's own output) drawn on them: draw_detections' list of uint8 device tensors.
        images=None draws on the frames of the detector's last call, which are still on the device.  maps (the second value of a
        call with need_weights) puts the attention of the drawn detections under the boxes as a heat map: heat_map(..., site).  Tiled
        results draw like plain ones; maps with tiles stays refused.  Further keywords are draw_detections'."""
        if self.bbox_format != "xyxy":
            raise ValueError(f"Detector.draw: boxes must be 'xyxy' pixels: build the Detector with bbox_format='xyxy', not {self.bbox_format!r}")
        if maps is not None and (self.tiles is not None or self.views):
            raise NotImplementedError("Detector.draw: maps with tiles: there is one attention map per tile and no single image to overlay it on")
        if images is None:
            images = self._last_frames
            if images is None:
                raise ValueError("Detector.draw: images=None draws on the frames of the last call, and there has been none")
        elif isinstance(images, np.ndarray) and images.ndim == 3:
            images = [images]
        single = isinstance(detections, (Detections, TiledDetections, FusedDetections))
        dets = [detections] if single else list(detections)
        if maps is not None:
            sizes = images.sizes if hasattr(images, "sizes") else [im.shape[:2] for im in images]
            heat, scale, extent = self.heat_map(dets, maps, sizes, site)
            kw = dict(kw, heat=heat, heat_scale=scale, heat_extent=extent)
        out = draw_detections(images, dets, class_names, **kw)
        return out[0] if single else out

    def to_coco_results(self, detections, image_ids, category_ids=None):
        """COCO results records [{"image_id", "category_id", "bbox": [x, y, w, h], "score"}] (Python numbers) of the detections
        of the images `image_ids`; needs bbox_format="xywh".  category_ids maps a label to its COCO category id (a dict or a
        sequence indexed by label; None: the label itself).  One copy to the host for the whole list."""
        if self.bbox_format != "xywh":
            raise ValueError(f"to_coco_results: COCO boxes are [x, y, w, h]: build the Detector with bbox_format='xywh', not {self.bbox_format!r}")
        if isinstance(detections, (Detections, TiledDetections, FusedDetections)):
            detections, image_ids = [detections], [image_ids]
        if len(detections) != len(image_ids):
            raise ValueError(f"to_coco_results: {len(detections)} images of detections, {len(image_ids)} image ids")
        if not detections:
            return []
        boxes = torch.cat([d.boxes.reshape(-1, 4) for d in detections]).cpu().tolist()
        labels = torch.cat([d.labels for d in detections]).cpu().tolist()
        scores = torch.cat([d.scores for d in detections]).cpu().tolist()
        owner = [image_id for image_id, d in zip(image_ids, detections) for _ in range(int(d.scores.shape[0]))]
        return [{"image_id": image_id, "category_id": label if category_ids is None else category_ids[label],
                 "bbox": [float(v) for v in box], "score": float(score)}
                for image_id, box, label, score in zip(owner, boxes, labels, scores)]
