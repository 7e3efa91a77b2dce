"""The batch pipeline shared by the COCO, VOC and CSV loaders (the reference's tf.data pipelines, data/coco.py:95-126,
voc.py:79-127, tfcsv.py:51-77).

The host decodes JPEG / PNG (PIL, a small thread pool with one batch of lookahead), draws the transform records and moves
the boxes (transformation.py); the uint8 images go to the device, where csrc/augment.hip applies flip / stage B / final resize
and the normalisation (csrc/augment_padded.hip for the aspect-preserving modes, which yield a padded (images, masks) pair),
and DeviceInputStage.targets builds the padded target layout.  Each iteration is a new shuffled epoch;
`len()` is the number of whole batches (drop remainder).

Evaluation by the COCO protocol (loss/coco_eval.py) needs more: `with_meta=True` adds a fourth element to every batch, the
per-target crowd flags and annotation areas, the original image sizes and the image ids; `shuffle=False` with
`drop_remainder=False` gives the whole set once, in file order, with a last short batch.
"""
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import transformation as T


class Sample(NamedTuple):
    path: str
    boxes: np.ndarray            # float32 [n, 4] normalised (cx, cy, w, h)
    classes: np.ndarray          # int64 [n, 1]
    crowd: Optional[np.ndarray] = None           # uint8 [n] iscrowd
    area: Optional[np.ndarray] = None            # float32 [n] annotation area, pixels^2 of the original image
    image_id: Optional[int] = None
    size: Optional[Tuple[int, int]] = None       # (h, w) of the original image, from the annotation file


def resolve(data_dir, path):
    """A dataset path as the reference joins it (config.data joins data_dir in already; an explicit argument is relative)."""
    if path is None or data_dir is None or os.path.isabs(path) or os.path.exists(path):
        return path
    return os.path.join(data_dir, path)


def decode_image(path):
    """JPEG / PNG -> uint8 [h, w, 3] RGB (grey and RGBA converted)."""
    try:
        from PIL import Image
    except ImportError as e:                     # pragma: no cover - PIL is a declared requirement of the loaders
        raise ImportError("the dataset loaders decode images with Pillow (PIL): install it to use detr_tf.data") from e
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


class DetectionDataset:
    """Re-iterable dataset of (images, t_bbox, t_class) batches on the device, in the layout fit / eval take.

    augmentation: True = the reference's training augmentation, False = resize to config.image_size (cubic), None = no
    transform at all: batch size 1 gives the image at its native size, a larger batch a padded (images, masks) pair.
    "multiscale" (training) and "shortest_side" (evaluation) keep the aspect ratio (transformation.draw_multiscale /
    eval_record: shortest side from `scales` -- "shortest_side" takes the largest --, longest side <= max_size) and yield
    ((images, masks), t_bbox, t_class) with the boxes normalised per image; `canvas` = (H, W) fixes the padded shape, so that a
    captured training or evaluation graph keeps replaying (and every rank of a data-parallel run sees one shape); None sizes
    each batch's canvas to its largest image, rounded up to 32.
    An image that loses all its boxes to augmentation is skipped (the next one takes its place), so an epoch can yield fewer
    than len() batches; with_meta keeps such an image, with no targets (an evaluation counts its detections as false positives).
    with_meta=True (augmentation False, None or "shortest_side" only; the samples must carry crowd / area / image_id / size) yields
    (images, t_bbox, t_class, meta) with meta = {"crowd": uint8 [B, R], "area": float32 [B, R], "size": int32 [B, 2] the ORIGINAL
    (h, w), "image_id": int64 [B]} on the device; the rows of crowd / area line up with the rows of t_bbox (row 0, the header, is
    unused).  shuffle=False walks the samples in their order; drop_remainder=False also yields the last, shorter batch."""

    PADDED_MODES = ("multiscale", "shortest_side")

    @staticmethod
    def is_training_mode(augmentation):
        """True and "multiscale" draw random transforms; False, None and "shortest_side" are the evaluation modes."""
        return augmentation == "multiscale" if isinstance(augmentation, str) else bool(augmentation)

    def __init__(self, samples, config, batch_size, augmentation=False, seed=None, num_workers=4, device=None, scales=None,
                 max_size=None, canvas=None, with_meta=False, shuffle=True, drop_remainder=True):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if isinstance(augmentation, str) and augmentation not in self.PADDED_MODES:
            raise ValueError(f"augmentation must be True, False, None or one of {self.PADDED_MODES}, got {augmentation!r}")
        samples = list(samples)
        training = self.is_training_mode(augmentation)
        if with_meta and training:
            raise ValueError(f"with_meta=True is for evaluation: augmentation must be False, None or 'shortest_side', got {augmentation!r}")
        if with_meta and any(s.crowd is None or s.area is None or s.image_id is None or s.size is None for s in samples):
            raise ValueError("with_meta=True needs samples that carry crowd, area, image_id and size (coco_samples fills them)")
        if training and any(s.crowd is not None and np.any(s.crowd) for s in samples):
            raise ValueError(f"augmentation={augmentation!r} is a training mode and a crowd box would be a wrong target: "
                             "load the samples without keep_crowd")
        self.with_meta, self.shuffle, self.drop_remainder = bool(with_meta), bool(shuffle), bool(drop_remainder)
        self.padded = isinstance(augmentation, str)
        self.scales = T.MULTISCALE_SCALES if scales is None else tuple(int(v) for v in scales)
        self.max_size = T.MULTISCALE_MAX_SIZE if max_size is None else int(max_size)
        self.canvas = None if canvas is None else (int(canvas[0]), int(canvas[1]))
        self.samples = samples
        self.config = config
        self.batch_size = int(batch_size)
        self.augmentation = augmentation
        self.image_size = tuple(int(v) for v in config.image_size)
        self.num_workers = max(1, int(num_workers))
        self.device = device
        self.rng = np.random.default_rng(seed)
        self._stage = None

    def __len__(self):
        return len(self.samples) // self.batch_size if self.drop_remainder else -(-len(self.samples) // self.batch_size)

    def stage(self):
        if self._stage is None:
            from .processing import DeviceInputStage
            self._stage = DeviceInputStage(self.config, device=self.device)
        return self._stage

    def host_batches(self):
        """One epoch on the host: lists of (image uint8 [h, w, 3], record or None, boxes, classes), batch_size each; with_meta
        appends (crowd, area, image_id, size) of the kept boxes to every entry."""
        order = self.rng.permutation(len(self.samples)) if self.shuffle else np.arange(len(self.samples))
        lookahead = 2 * self.batch_size                       # the batch being assembled + one batch ahead
        with ThreadPoolExecutor(max_workers=self.num_workers) as pool:
            pending = deque()
            nxt = 0

            def fill():
                nonlocal nxt
                while len(pending) < lookahead and nxt < len(order):
                    s = self.samples[int(order[nxt])]
                    pending.append((s, pool.submit(decode_image, s.path)))
                    nxt += 1

            batch = []
            fill()
            while pending:
                s, fut = pending.popleft()
                fill()
                image = fut.result()
                h0, w0 = image.shape[:2]
                # the box transforms return the classes of the boxes they keep: handed the box INDICES instead, they tell which
                # boxes were kept, in which order -- classes and metadata are gathered by those
                index = np.arange(len(s.boxes))
                if self.augmentation is None:
                    rec, boxes, kept = None, s.boxes, None
                elif self.padded:
                    if self.augmentation == "multiscale":
                        rec = T.draw_multiscale(self.rng, h0, w0, self.scales, self.max_size)
                    else:
                        rec = T.eval_record(h0, w0, max(self.scales), self.max_size)
                    boxes, kept = T.transform_boxes_padded(s.boxes, index, h0, w0, rec)
                else:
                    rec = T.draw_transform(self.rng, h0, w0, self.image_size, self.augmentation)
                    boxes, kept = T.transform_boxes(s.boxes, index, h0, w0, rec, self.image_size)
                if len(boxes) == 0 and not self.with_meta:
                    continue                                   # (an evaluation keeps the image: its detections are false positives)
                kept = index if kept is None else np.asarray(kept, np.int64).reshape(-1)
                entry = (image, rec, boxes, s.classes if rec is None else np.asarray(s.classes)[kept])
                if self.with_meta:
                    entry += (np.asarray(s.crowd, np.uint8).reshape(-1)[kept], np.asarray(s.area, np.float32).reshape(-1)[kept],
                              int(s.image_id), (int(s.size[0]), int(s.size[1])))
                batch.append(entry)
                if len(batch) == self.batch_size:
                    yield batch
                    batch = []
            if batch and not self.drop_remainder:
                yield batch

    def __iter__(self):
        st = self.stage()
        for batch in self.host_batches():
            images = [b[0] for b in batch]
            if self.augmentation is None:
                if len(images) == 1:                     # the native size: images() copies without resizing
                    st.image_size = images[0].shape[:2]
                    try:
                        dev = st.images(images[0][None])
                    finally:
                        st.image_size = self.image_size
                else:
                    dev = st.images_padded(images)
            elif self.padded:
                dev = st.augmented_padded(images, [b[1] for b in batch], canvas=self.canvas)
            else:
                dev = st.augmented(images, [b[1] for b in batch])
            t_bbox, t_class = st.targets([b[2] for b in batch], [b[3] for b in batch])
            if self.with_meta:
                yield dev, t_bbox, t_class, self._meta(batch, t_bbox)
            else:
                yield dev, t_bbox, t_class

    @staticmethod
    def _meta(batch, t_bbox):
        import torch
        B, R = len(batch), int(t_bbox.shape[1])
        crowd, area = np.zeros((B, R), np.uint8), np.zeros((B, R), np.float32)
        for b, entry in enumerate(batch):
            n = len(entry[4])
            crowd[b, 1:1 + n], area[b, 1:1 + n] = entry[4], entry[5]
        size = np.array([entry[7] for entry in batch], np.int32).reshape(B, 2)
        image_id = np.array([entry[6] for entry in batch], np.int64)
        return {k: torch.from_numpy(v).to(t_bbox.device) for k, v in (("crowd", crowd), ("area", area), ("size", size), ("image_id", image_id))}
