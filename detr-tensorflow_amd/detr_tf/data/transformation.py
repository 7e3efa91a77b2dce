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

Aspect-preserving multi-scale input (padded batches).  The reference names the constants of the recipe DETR is trained with
(transformation.py:59-64) and keeps the evaluation rule as commented-out code (:96-112) but resizes every image to one fixed
size.  `draw_multiscale` / `eval_record` draw a `PaddedRecord` per image: flip, a source window, and the image's own
destination size from `target_size` (shortest side S, longest side <= max_size, aspect ratio kept); csrc/augment_padded.hip
(`DeviceInputStage.augmented_padded`) writes every image at the top-left of a zero-padded canvas with its padding mask, and
`transform_boxes_padded` moves the boxes, normalised to the image's own (wd, hd), not to the canvas.
One deviation from resize -> crop -> resize: the intermediate resize of the crop branch is not materialised.  The crop window
drawn in the intermediate image is mapped back to the source and its edges are rounded to WHOLE source pixels (at least one
pixel, inside the image); the destination size is `target_size` of that window.
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


# ------------------------------------------------------------------------------------------------------------------------------
# aspect-preserving multi-scale records (padded batches, csrc/augment_padded.hip)
# ------------------------------------------------------------------------------------------------------------------------------
LINEAR = 1
PADDED_IREC = 12                                             # include/detr_hip.h: DETR_AUGP_IREC
MULTISCALE_SCALES = tuple(range(480, 801, 32))
MULTISCALE_MAX_SIZE = 1333
CROP_SCALES = (400, 500, 600)                                # the crop branch: intermediate shortest side, no maximum
CROP_MIN, CROP_MAX = 384, 600                                # side range of the window drawn in the intermediate image


class PaddedRecord(NamedTuple):
    """One image's record of the padded path: the window (y0, x0, hc, wc) of the flipped h0 x w0 source, in whole source
    pixels, is resized to hd x wd with interpolation `interp`."""
    h0: int
    w0: int
    flip: bool
    y0: int
    x0: int
    hc: int
    wc: int
    hd: int
    wd: int
    interp: int = LINEAR


def target_size(h, w, short, max_size=None):
    """(height, width) of an h x w image resized so that its shortest side is `short` unless its longest side would then
    exceed `max_size` (None: no limit), which then binds instead.  Integer arithmetic only: the reference's commented rule
    takes int() of a float scale, which can land one pixel off."""
    h, w, short = int(h), int(w), int(short)
    mn, mx = min(h, w), max(h, w)
    if max_size is not None and short * mx > int(max_size) * mn:
        lng = int(max_size)
        sht = max(1, lng * mn // mx)
    else:
        sht = short
        lng = short * mx // mn
    return (sht, lng) if h <= w else (lng, sht)


def _to_source(v, n0, n1):
    """Coordinate v of the n1-pixel intermediate axis on the n0-pixel source axis, rounded half up to a whole pixel."""
    return (2 * v * n0 + n1) // (2 * n1)


def draw_multiscale(rng, h0, w0, scales=MULTISCALE_SCALES, max_size=MULTISCALE_MAX_SIZE, interp=LINEAR):
    """One training record for an h0 x w0 image, drawn with the numpy Generator `rng`: flip (p = 0.5), then with p = 0.5 the
    full image at a random shortest side S of `scales`, otherwise a random crop (resize to 400 / 500 / 600, window sides uniform
    in [384, min(side, 600)] at a uniform origin) resized to a random S; longest side <= max_size both times."""
    h0, w0 = int(h0), int(w0)
    scales = tuple(int(v) for v in scales)
    flip = bool(rng.random() < 0.5)
    if rng.random() < 0.5:
        y0, x0, hc, wc = 0, 0, h0, w0
    else:
        h1, w1 = target_size(h0, w0, CROP_SCALES[int(rng.integers(0, len(CROP_SCALES)))])
        wn = int(rng.integers(min(CROP_MIN, w1), min(w1, CROP_MAX) + 1))
        hn = int(rng.integers(min(CROP_MIN, h1), min(h1, CROP_MAX) + 1))
        yn, xn = int(rng.integers(0, h1 - hn + 1)), int(rng.integers(0, w1 - wn + 1))
        y0, x0 = min(_to_source(yn, h0, h1), h0 - 1), min(_to_source(xn, w0, w1), w0 - 1)
        hc = min(max(_to_source(yn + hn, h0, h1) - y0, 1), h0 - y0)
        wc = min(max(_to_source(xn + wn, w0, w1) - x0, 1), w0 - x0)
    hd, wd = target_size(hc, wc, scales[int(rng.integers(0, len(scales)))], max_size)
    return PaddedRecord(h0, w0, flip, y0, x0, hc, wc, hd, wd, int(interp))


def eval_record(h0, w0, short=800, max_size=MULTISCALE_MAX_SIZE, interp=LINEAR):
    """The evaluation record: no flip, the full image, shortest side `short`, longest side <= max_size."""
    h0, w0 = int(h0), int(w0)
    hd, wd = target_size(h0, w0, short, max_size)
    return PaddedRecord(h0, w0, False, 0, 0, h0, w0, hd, wd, int(interp))


def _tile_axis(length, n, num, den):
    """(window size, origins) of n equal windows over `length` pixels: the first starts at 0, the last ends at `length`, the origins
    are i * (length - size) // (n - 1), and `size` is the smallest one at which two neighbours share at least num * size // den
    pixels (their largest distance is ceil((length - size) / (n - 1)))."""
    if n == 1:
        return length, [0]
    size = -(-length // n)
    while size - -(-(length - size) // (n - 1)) < num * size // den:        # size = length always passes: the distance is 0
        size += 1
    return size, [i * (length - size) // (n - 1) for i in range(n)]


def tile_records(h0, w0, rows, cols, overlap=0.2, short=800, max_size=MULTISCALE_MAX_SIZE, interp=LINEAR, include_full=True):
    """The records of sliced inference on an h0 x w0 image: rows x cols overlapping windows in row-major order, behind the whole
    image (eval_record) when `include_full`.  All windows have ONE size (hc, wc) -- so one destination size,
    target_size(hc, wc, short, max_size), and a uniform batch --, the first starts at 0, the last ends exactly at h0 / w0, the
    origins are evenly spaced up to integer rounding and neighbours share at least floor(overlap * hc) rows and
    floor(overlap * wc) columns.  Integer arithmetic only: `overlap` is read as the exact decimal fraction it prints as."""
    from fractions import Fraction
    h0, w0, rows, cols = int(h0), int(w0), int(rows), int(cols)
    if h0 < 1 or w0 < 1:
        raise ValueError(f"tile_records: bad image size {h0} x {w0}")
    if not (1 <= rows <= h0 and 1 <= cols <= w0):
        raise ValueError(f"tile_records: a {rows} x {cols} grid does not fit a {h0} x {w0} image (1 <= rows <= height, 1 <= cols <= width)")
    if not (0.0 <= float(overlap) < 1.0):
        raise ValueError(f"tile_records: overlap={overlap} must be in [0, 1)")
    frac = Fraction(repr(float(overlap)))
    hc, ys = _tile_axis(h0, rows, frac.numerator, frac.denominator)
    wc, xs = _tile_axis(w0, cols, frac.numerator, frac.denominator)
    hd, wd = target_size(hc, wc, short, max_size)
    records = [eval_record(h0, w0, short, max_size, interp)] if include_full else []
    records += [PaddedRecord(h0, w0, False, y, x, hc, wc, hd, wd, int(interp)) for y in ys for x in xs]
    return records


def view_records(h0, w0, scales=(800,), max_size=MULTISCALE_MAX_SIZE, flip=False, interp=LINEAR, tiles=None, overlap=0.2, include_full=True):
    """The records of test-time augmentation on an h0 x w0 image: for every shortest side s of `scales`, in order, the records of
    that scale -- eval_record(h0, w0, s, ...), or with tiles=(rows, cols) tile_records(h0, w0, rows, cols, overlap, s, ...) --, and
    with `flip` the same list once more with flip=True.  A flipped record's window is a window of the MIRRORED image (the kernel's
    rule: flip, then window), so the windows of the second half equal those of the first.  Integer arithmetic only."""
    h0, w0 = int(h0), int(w0)
    if h0 < 1 or w0 < 1:
        raise ValueError(f"view_records: bad image size {h0} x {w0}")
    try:
        scales = tuple(scales)
    except TypeError:
        raise ValueError(f"view_records: scales={scales!r} must be a non-empty sequence of positive integers") from None
    if not scales or any(isinstance(s, bool) or not isinstance(s, (int, np.integer)) or int(s) < 1 for s in scales):
        raise ValueError(f"view_records: scales={scales!r} must be a non-empty sequence of positive integers")
    if max_size is not None and int(max_size) < 1:
        raise ValueError(f"view_records: max_size={max_size} must be positive or None")
    if tiles is not None and len(tuple(tiles)) != 2:
        raise ValueError(f"view_records: tiles={tiles!r} must be (rows, cols) or None")
    records = []
    for s in scales:
        if tiles is None:
            records.append(eval_record(h0, w0, int(s), max_size, interp))
        else:
            records += tile_records(h0, w0, tiles[0], tiles[1], overlap, int(s), max_size, interp, include_full)
    if flip:
        records += [r._replace(flip=True) for r in records]
    return records


def check_padded_record(t, canvas=None):
    """Host validation of one padded record (the kernel also clamps, but a wrong record is a caller's bug)."""
    if t.h0 < 1 or t.w0 < 1:
        raise ValueError(f"padded record: bad source size {t.h0} x {t.w0}")
    if t.interp not in range(4):
        raise ValueError(f"padded record: bad interpolation {t}")
    if t.hc < 1 or t.wc < 1 or not (0 <= t.y0 <= t.h0 - t.hc and 0 <= t.x0 <= t.w0 - t.wc):
        raise ValueError(f"padded record: window {t.hc} x {t.wc} at ({t.y0}, {t.x0}) leaves the {t.h0} x {t.w0} image")
    if t.hd < 1 or t.wd < 1:
        raise ValueError(f"padded record: bad destination size {t.hd} x {t.wd}")
    if canvas is not None and (t.hd > int(canvas[0]) or t.wd > int(canvas[1])):
        raise ValueError(f"padded record: destination {t.hd} x {t.wd} does not fit the {int(canvas[0])} x {int(canvas[1])} canvas")


def pack_padded_records(records, offsets):
    """records + byte offsets of the images in the packed source -> irec int32 [B, PADDED_IREC] in the layout of
    detr_hip_augment_padded."""
    irec = np.zeros((len(records), PADDED_IREC), np.int32)
    for b, (t, off) in enumerate(zip(records, offsets)):
        irec[b, 0:2] = np.array([int(off)], "<i8").view("<i4")
        irec[b, 2:] = [t.h0, t.w0, int(bool(t.flip)), t.y0, t.x0, t.hc, t.wc, t.hd, t.wd, t.interp]
    return irec


def transform_boxes_padded(bbox_xcycwh, t_class, h0, w0, record):
    """Move normalised (cx, cy, w, h) boxes with the image (NumPy, float64): flip, shift by the window and clip to it, drop
    the boxes whose clipped width or height is not positive.  Returns (boxes float32 [n, 4] normalised to the image's own
    (wd, hd) -- what the per-image sine encoding and the set loss assume, not the canvas -- and the classes of the kept boxes)."""
    t = record
    b = np.asarray(bbox_xcycwh, np.float64).reshape(-1, 4)
    cls = np.asarray(t_class)
    x1, x2 = (b[:, 0] - b[:, 2] / 2) * w0, (b[:, 0] + b[:, 2] / 2) * w0
    y1, y2 = (b[:, 1] - b[:, 3] / 2) * h0, (b[:, 1] + b[:, 3] / 2) * h0
    if t.flip:
        x1, x2 = w0 - x2, w0 - x1
    x1, x2 = np.clip(x1 - t.x0, 0, t.wc), np.clip(x2 - t.x0, 0, t.wc)
    y1, y2 = np.clip(y1 - t.y0, 0, t.hc), np.clip(y2 - t.y0, 0, t.hc)
    keep = (x2 - x1 > 0) & (y2 - y1 > 0)
    # window pixels -> destination pixels -> normalised by the destination size: the two factors of wd (hd) cancel
    x1, x2, y1, y2 = x1[keep] / t.wc, x2[keep] / t.wc, y1[keep] / t.hc, y2[keep] / t.hc
    out = np.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], 1).astype(np.float32)
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
