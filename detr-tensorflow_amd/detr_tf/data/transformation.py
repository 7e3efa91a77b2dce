"""Training augmentation of the drop-in API (reference detr_tf/data/transformation.py:54-94,163-196).

The reference runs imgaug on the host for every image: `Fliplr(0.5)`, then `Sometimes(0.5, OneOf([Resize, CropToFixedSize,
Affine(scale)]))`, then a final `Resize` with a random interpolation, and moves the boxes with the image.  Here the host
only draws one transform record per image (`draw_transform`) and moves the boxes in NumPy (`transform_boxes`); the pixels
are produced on the device by csrc/augment.hip (`DeviceInputStage.augmented`), together with the resize to
`config.image_size` and the normalisation.

Record semantics (one per image, applied in this order):
  flip    horizontal mirror (p = 0.5)
  kind    stage B: "none" (p = 0.5) or, with p = 1/6 each, "resize" to the target size with interpolation `ia`,
          "crop" to min(Hd, h0) x min(Wd, w0) at (y0, x0), "affine" zoom by (sx, sy) in [0.5, 1.5] about the image centre
  iff     interpolation of the final resize to (Hd, Wd) (identity when the sizes already agree)
Interpolations are imgaug's `ia.ALL`: nearest, linear, area, cubic.  imgaug's random stream and OpenCV's fixed-point
rounding cannot be reproduced: the distributions are the reference's, the individual draws are not.
"""
from typing import NamedTuple

import numpy as np

INTERP_NAMES = ("nearest", "linear", "cubic", "area")        # index = the kernel's interpolation code
INTERP_ALL = (0, 1, 3, 2)                                    # imgaug ia.ALL: nearest, linear, area, cubic
CUBIC = 2
KINDS = {"none": 0, "resize": 1, "crop": 2, "affine": 3}
IREC, FREC = 10, 2                                           # include/detr_hip.h: DETR_AUG_IREC / DETR_AUG_FREC


class Transform(NamedTuple):
    """One image's augmentation record (see the module docstring)."""
    h0: int
    w0: int
    flip: bool = False
    kind: int = 0                # KINDS
    ia: int = CUBIC              # stage-B resize interpolation (kind == resize)
    iff: int = CUBIC             # final resize interpolation
    y0: int = 0                  # crop offset (kind == crop)
    x0: int = 0
    sx: float = 1.0              # affine zoom (kind == affine)
    sy: float = 1.0


def crop_size(h0, w0, image_size):
    """CropToFixedSize never pads: the window is min(Hd, h0) x min(Wd, w0)."""
    return min(int(image_size[0]), int(h0)), min(int(image_size[1]), int(w0))


def draw_transform(rng, h0, w0, image_size, augmentation):
    """One record for an h0 x w0 image, drawn with the numpy Generator `rng` (detr_aug_seq, transformation.py:54-94).
    augmentation=False: no flip, no stage B, final cubic resize (imgaug Resize's default)."""
    h0, w0 = int(h0), int(w0)
    if not augmentation:
        return Transform(h0, w0)
    flip = bool(rng.random() < 0.5)
    kind = 0
    if rng.random() < 0.5:                                    # Sometimes(0.5, OneOf([...]))
        kind = 1 + int(rng.integers(0, 3))
    ia = INTERP_ALL[int(rng.integers(0, 4))]
    iff = INTERP_ALL[int(rng.integers(0, 4))]
    hc, wc = crop_size(h0, w0, image_size)
    y0, x0 = int(rng.integers(0, h0 - hc + 1)), int(rng.integers(0, w0 - wc + 1))
    sx, sy = float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.5, 1.5))
    if kind != KINDS["resize"]:
        ia = CUBIC
    if kind != KINDS["crop"]:
        y0 = x0 = 0
    if kind != KINDS["affine"]:
        sx = sy = 1.0
    return Transform(h0, w0, flip, kind, ia, iff, y0, x0, sx, sy)


def stage_b_size(t, image_size):
    """(height, width) of stage B's output."""
    if t.kind == KINDS["resize"]:
        return int(image_size[0]), int(image_size[1])
    if t.kind == KINDS["crop"]:
        return crop_size(t.h0, t.w0, image_size)
    return t.h0, t.w0


def check_record(t, image_size):
    """Host validation of one record (the kernel also clamps, but a wrong record is a caller's bug)."""
    if t.h0 < 1 or t.w0 < 1:
        raise ValueError(f"transform record: bad source size {t.h0} x {t.w0}")
    if t.kind not in KINDS.values() or t.ia not in range(4) or t.iff not in range(4):
        raise ValueError(f"transform record: bad kind / interpolation {t}")
    hc, wc = crop_size(t.h0, t.w0, image_size)
    if t.kind == KINDS["crop"] and not (0 <= t.y0 <= t.h0 - hc and 0 <= t.x0 <= t.w0 - wc):
        raise ValueError(f"transform record: crop window at ({t.y0}, {t.x0}) leaves the {t.h0} x {t.w0} image")
    if not (np.isfinite(t.sx) and np.isfinite(t.sy) and t.sx > 0 and t.sy > 0):
        raise ValueError(f"transform record: bad scale ({t.sx}, {t.sy})")


def pack_records(records, offsets):
    """records + byte offsets of the images in the packed source -> (irec int32 [B, IREC], frec float32 [B, FREC]) in the
    layout of detr_hip_augment.  1/sx and 1/sy are computed once here, in float64, and rounded to float32."""
    B = len(records)
    irec = np.zeros((B, IREC), np.int32)
    frec = np.zeros((B, FREC), np.float32)
    for b, (t, off) in enumerate(zip(records, offsets)):
        irec[b, 0:2] = np.array([int(off)], "<i8").view("<i4")
        irec[b, 2:] = [t.h0, t.w0, int(bool(t.flip)), t.kind, t.ia, t.iff, t.y0, t.x0]
        frec[b] = [np.float32(1.0 / t.sx), np.float32(1.0 / t.sy)]
    return irec, frec


def transform_boxes(bbox_xcycwh, t_class, h0, w0, record, image_size):
    """Move normalised (cx, cy, w, h) boxes with the image (NumPy, float64), then imgaug's
    remove_out_of_image_fraction(0.7) + clip_out_of_image in the (Hd, Wd) frame.  Returns (boxes float32 [n, 4] normalised
    to (Wd, Hd), classes of the kept boxes)."""
    t = record
    Hd, Wd = int(image_size[0]), int(image_size[1])
    b = np.asarray(bbox_xcycwh, np.float64).reshape(-1, 4)
    cls = np.asarray(t_class)
    x1, x2 = (b[:, 0] - b[:, 2] / 2) * w0, (b[:, 0] + b[:, 2] / 2) * w0
    y1, y2 = (b[:, 1] - b[:, 3] / 2) * h0, (b[:, 1] + b[:, 3] / 2) * h0
    if t.flip:
        x1, x2 = w0 - x2, w0 - x1
    if t.kind == KINDS["resize"]:
        x1, x2, y1, y2 = x1 * (Wd / w0), x2 * (Wd / w0), y1 * (Hd / h0), y2 * (Hd / h0)
    elif t.kind == KINDS["crop"]:
        x1, x2, y1, y2 = x1 - t.x0, x2 - t.x0, y1 - t.y0, y2 - t.y0
    elif t.kind == KINDS["affine"]:
        x1, x2 = (x1 - w0 / 2) * t.sx + w0 / 2, (x2 - w0 / 2) * t.sx + w0 / 2
        y1, y2 = (y1 - h0 / 2) * t.sy + h0 / 2, (y2 - h0 / 2) * t.sy + h0 / 2
    hb, wb = stage_b_size(t, image_size)
    x1, x2, y1, y2 = x1 * (Wd / wb), x2 * (Wd / wb), y1 * (Hd / hb), y2 * (Hd / hb)
    area = (x2 - x1) * (y2 - y1)
    inside = np.clip(np.minimum(x2, Wd) - np.maximum(x1, 0), 0, None) * np.clip(np.minimum(y2, Hd) - np.maximum(y1, 0), 0, None)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac_out = np.where(area > 0, 1.0 - inside / np.where(area > 0, area, 1.0), 1.0)
    fully_out = (x2 <= 0) | (x1 >= Wd) | (y2 <= 0) | (y1 >= Hd)
    keep = (frac_out < 0.7) & ~fully_out
    x1, x2 = np.clip(x1[keep], 0, Wd), np.clip(x2[keep], 0, Wd)
    y1, y2 = np.clip(y1[keep], 0, Hd), np.clip(y2[keep], 0, Hd)
    out = np.stack([(x1 + x2) / 2 / Wd, (y1 + y2) / 2 / Hd, (x2 - x1) / Wd, (y2 - y1) / Hd], 1).astype(np.float32)
    return out.reshape(-1, 4), cls[keep]


_rng = np.random.default_rng()
_stages = {}


def detr_transform(image, bbox, t_class, config, augmentation):
    """transformation.py:163-196: (image uint8 [h0, w0, 3], normalised boxes, classes) -> (image float32 [Hd, Wd, 3] with
    values 0..255, not normalised; boxes; classes), through the device kernel with an identity table."""
    import torch
    from .processing import DeviceInputStage
    image = np.ascontiguousarray(np.asarray(image).astype(np.uint8, copy=False))
    h0, w0 = image.shape[:2]
    image_size = tuple(int(v) for v in config.image_size)
    record = draw_transform(_rng, h0, w0, image_size, augmentation)
    key = (torch.cuda.current_device(), image_size)
    if key not in _stages:
        stage = DeviceInputStage(config)
        stage.lut = torch.arange(256, dtype=torch.float32).repeat(3).to(stage.device)
        stage.perm = (0, 1, 2)
        _stages[key] = stage
    out = _stages[key].augmented([image], [record])[0].cpu().numpy()
    boxes, classes = transform_boxes(bbox, t_class, h0, w0, record, image_size)
    return out, boxes, np.asarray(classes)
