"""mAP evaluation loop -- what the reference's eval.py:30-61 `eval_model` does, for any batch size: forward (eval mode),
batched device post-processing (one launch per batch instead of one get_model_inference per image), header-stripped
targets converted to [y1, x1, y2, x2] (bbox.py:186-196), the vectorised COCO-style accumulator, the reference's table.

accumulate="device" keeps the per-image matching on the device as well (loss/compute_map.py: DeviceAPAccumulator, one more
launch per batch): nothing is read back per batch, so the loop enqueues batch i+1 while batch i still runs; the result is the
same to the last bit.

protocol="coco" evaluates by the COCO protocol instead (loss/coco_eval.py: crowd regions, area ranges, maxDets, AP and AR): the
loader must yield 4-tuples (images, t_bbox, t_class, meta), as DetectionDataset(with_meta=True) does; accumulate keeps its meaning."""
import numpy as np
import torch

from . import bbox
from .inference import _multilabel, _post_multilabel, _scoring, get_model_inference_batched, scoring_of
from .loss.coco_eval import COCOAccumulator, DeviceCOCOAccumulator, check_meta
from .loss.compute_map import APAccumulator, DeviceAPAccumulator


def _detections_host(m_outputs, background_class, scoring, multilabel):
    """[(boxes, labels, scores)] per image in "yxyx": get_model_inference_batched's, or with multilabel = K the K best (query, class)
    pairs of every image (detr_hip_postprocess_multilabel), best first."""
    if not multilabel:
        return get_model_inference_batched(m_outputs, background_class, bbox_format="yxyx", scoring=scoring)
    out_b, out_l, out_s, counts = _post_multilabel(m_outputs["pred_logits"], m_outputs["pred_boxes"], background_class, "yxyx", multilabel)
    return [(out_b[b, :k], out_l[b, :k], out_s[b, :k]) for b, k in enumerate(counts.tolist())]


def _add_batch_host(acc, model, m_outputs, target_bbox, target_class, background_class, scoring="softmax", multilabel=None):
    dets = _detections_host(m_outputs, background_class, scoring, multilabel)
    if getattr(model, "engine", None) is not None:
        model.engine.check_mask_status()      # (padded batches with a device mask; the detections are read on the host anyway)
    tb = torch.as_tensor(np.asarray(target_bbox) if not torch.is_tensor(target_bbox) else target_bbox).float().cpu()
    tc = torch.as_tensor(np.asarray(target_class) if not torch.is_tensor(target_class) else target_class).cpu()
    for b, (p_bbox, p_labels, p_scores) in enumerate(dets):
        n = int(tb[b, 0, 0])                                          # header row (data/processing.py:35-55)
        t_bbox = bbox.xcycwh_to_yx_min_yx_max(tb[b, 1:1 + n])
        t_class = tc[b, 1:1 + n].reshape(-1)
        acc.add_image(p_bbox.cpu().numpy(), p_labels.cpu().numpy(), p_scores.cpu().numpy(), t_bbox.numpy(), t_class.numpy())


def _host(x):
    return (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).cpu()


def _add_batch_host_coco(acc, model, m_outputs, target_bbox, target_class, meta, background_class, scoring="softmax", multilabel=None):
    dets = _detections_host(m_outputs, background_class, scoring, multilabel)
    if getattr(model, "engine", None) is not None:
        model.engine.check_mask_status()
    tb, tc = _host(target_bbox).float(), _host(target_class)
    crowd, area, size = _host(meta["crowd"]).numpy(), _host(meta["area"]).numpy(), _host(meta["size"]).numpy()
    for b, (p_bbox, p_labels, p_scores) in enumerate(dets):
        n = int(tb[b, 0, 0])
        t_bbox = bbox.xcycwh_to_yx_min_yx_max(tb[b, 1:1 + n])
        acc.add_image(p_bbox.cpu().numpy(), p_labels.cpu().numpy(), p_scores.cpu().numpy(), t_bbox.numpy(), tc[b, 1:1 + n].reshape(-1).numpy(),
                      crowd[b, 1:1 + n], area[b, 1:1 + n], size[b])


def _eval_model_coco(model, config, class_names, valid_dt, max_batches, print_result, accumulate, scoring="softmax", multilabel=None):
    acc = COCOAccumulator(len(class_names))
    for it, batch in enumerate(valid_dt):
        if not isinstance(batch, (tuple, list)) or len(batch) != 4:
            raise TypeError('eval_model: protocol="coco" takes (images, t_bbox, t_class, meta) batches -- build the loader with '
                            f"with_meta=True (and keep_crowd=True); got a batch of {len(batch) if isinstance(batch, (tuple, list)) else type(batch).__name__}")
        images, target_bbox, target_class, meta = batch
        check_meta(meta, "eval_model")
        m_outputs = model(images, training=False)
        if accumulate == "device":
            if it == 0:
                acc = DeviceCOCOAccumulator(len(class_names), device=m_outputs["pred_logits"].device)
            acc.add_batch(m_outputs, target_bbox, target_class, meta, config.background_class, scoring, multilabel)
            if getattr(model, "engine", None) is not None:
                model.engine.check_mask_status()
        else:
            _add_batch_host_coco(acc, model, m_outputs, target_bbox, target_class, meta, config.background_class, scoring, multilabel)
        if max_batches is not None and it + 1 >= max_batches:
            break
    return acc.result(class_names, print_result=print_result)


def eval_model(model, config, class_names, valid_dt, max_batches=None, print_result=True, accumulate="host", *, protocol="reference",
               **options):
    """options: weights="model" (default) | "ema", keyword-only.  "ema" evaluates the averaged weights kept by config.ema_decay:
    the whole evaluation runs inside optimizers.ema_weights(model), and the trained weights are back, bit for bit, when it
    returns.  scoring="softmax" | "sigmoid" (get_model_inference_batched's), keyword-only; None (default) takes it from
    config.class_criterion: "focal" -> "sigmoid".  multilabel=True (keyword-only, sigmoid scoring only; ValueError otherwise):
    every image is evaluated on the max_detections (default 100, 1..1024) best (query, class) pairs instead of one detection per
    query -- the rule the detectors trained with a sigmoid focal loss are evaluated under; both protocols, both accumulate modes."""
    weights = options.pop("weights", "model")
    scoring = options.pop("scoring", None)
    scoring = scoring_of(config) if scoring is None else scoring
    _scoring(scoring)
    max_detections = options.pop("max_detections", 100)
    # the row capacity K of the multi-label rows, None without them: the defaults launch what they always did
    multilabel = int(max_detections) if _multilabel("eval_model", scoring, options.pop("multilabel", False)) else None
    if options:
        raise TypeError(f"eval_model() got an unexpected keyword argument {sorted(options)[0]!r}")
    if accumulate not in ("host", "device"):
        raise ValueError(f"eval_model: accumulate must be 'host' or 'device', got {accumulate!r}")
    if protocol not in ("reference", "coco"):
        raise ValueError(f"eval_model: protocol must be 'reference' or 'coco', got {protocol!r}")
    if weights not in ("model", "ema"):
        raise ValueError(f"eval_model: weights must be 'model' or 'ema', got {weights!r}")
    if weights == "ema":
        from .optimizers import ema_weights
        with ema_weights(model):
            return eval_model(model, config, class_names, valid_dt, max_batches, print_result, accumulate, protocol=protocol, scoring=scoring,
                              multilabel=multilabel is not None, max_detections=max_detections)
    if protocol == "coco":
        return _eval_model_coco(model, config, class_names, valid_dt, max_batches, print_result, accumulate, scoring, multilabel)
    acc = APAccumulator(len(class_names))
    for it, (images, target_bbox, target_class) in enumerate(valid_dt):
        m_outputs = model(images, training=False)
        if accumulate == "device":
            if it == 0:
                acc = DeviceAPAccumulator(len(class_names), device=m_outputs["pred_logits"].device)
            acc.add_batch(m_outputs, target_bbox, target_class, config.background_class, scoring, multilabel)
            if getattr(model, "engine", None) is not None:
                model.engine.check_mask_status()  # (reads the mask status words of a padded batch; a no-op for an unpadded one)
        else:
            _add_batch_host(acc, model, m_outputs, target_bbox, target_class, config.background_class, scoring, multilabel)
        if max_batches is not None and it + 1 >= max_batches:
            break
    return acc.result(class_names, print_result=print_result)
