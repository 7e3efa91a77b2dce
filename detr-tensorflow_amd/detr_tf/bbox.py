"""Box helpers of the hot path (torch tensors on any device) -- the TF half of the reference's
detr_tf/bbox.py (:171-196); the pairwise IoU/GIoU arithmetic itself runs inside the HIP set-loss
kernels (csrc/setloss.hip).  The np_* helpers are the host-side numpy half (bbox.py:230-294) for callers that rescale boxes
themselves; the Detector (detr_tf/inference.py) does the same on the device in csrc/detect.hip."""
import numpy as np
import torch


def xcycwh_to_xy_min_xy_max(bbox):
    """bbox.py:171-183 -- including the clip to [0, 1]."""
    xyxy = torch.cat([bbox[:, :2] - (bbox[:, 2:] / 2), bbox[:, :2] + (bbox[:, 2:] / 2)], dim=-1)
    return torch.clamp(xyxy, 0.0, 1.0)


def xy_min_xy_max_to_yx_min_yx_max(bbox):
    """bbox.py:126-139."""
    return torch.cat([bbox[:, 1:2], bbox[:, 0:1], bbox[:, 3:4], bbox[:, 2:3]], dim=-1)


def xcycwh_to_yx_min_yx_max(bbox):
    """bbox.py:186-196."""
    return xy_min_xy_max_to_yx_min_yx_max(xcycwh_to_xy_min_xy_max(bbox))


def np_xcycwh_to_xy_min_xy_max(bbox):
    """bbox.py:230-240 -- [xc, yc, w, h] -> [xmin, ymin, xmax, ymax] on [n, 4] arrays, NOT clipped."""
    bbox = np.asarray(bbox)
    half = bbox[:, 2:] / 2
    return np.concatenate([bbox[:, :2] - half, bbox[:, :2] + half], axis=-1)


def _np_rescale(bbox, factors):
    return np.array(bbox) * np.array(factors)


def np_rescale_bbox_xcycwh(bbox_xcycwh, img_size):
    """bbox.py:261-270 -- normalised [xc, yc, w, h] rows to pixels of an image of img_size = (height, width)."""
    return _np_rescale(bbox_xcycwh, [img_size[1], img_size[0], img_size[1], img_size[0]])


def np_rescale_bbox_yx_min_yx_max(bbox_yxyx, img_size):
    """bbox.py:273-282 -- normalised [ymin, xmin, ymax, xmax] rows to pixels; img_size = (height, width)."""
    return _np_rescale(bbox_yxyx, [img_size[0], img_size[1], img_size[0], img_size[1]])


def np_rescale_bbox_xy_min_xy_max(bbox, img_size):
    """bbox.py:285-294 -- normalised [xmin, ymin, xmax, ymax] rows to pixels; img_size = (height, width)."""
    return _np_rescale(bbox, [img_size[1], img_size[0], img_size[1], img_size[0]])
