"""COCO loader (reference detr_tf/data/coco.py:30-126): the annotation JSON is read with `json` (no pycocotools)."""
import json
import os
from collections import defaultdict

import numpy as np

from .loader import DetectionDataset, Sample, resolve

COCO_CLASS_NAME = [
    'N/A', 'person', 'bicycle', 'car', 'motorcycle', 'airplane', 'bus',
    'train', 'truck', 'boat', 'traffic light', 'fire hydrant', 'N/A',
    'stop sign', 'parking meter', 'bench', 'bird', 'cat', 'dog', 'horse',
    'sheep', 'cow', 'elephant', 'bear', 'zebra', 'giraffe', 'N/A', 'backpack',
    'umbrella', 'N/A', 'N/A', 'handbag', 'tie', 'suitcase', 'frisbee', 'skis',
    'snowboard', 'sports ball', 'kite', 'baseball bat', 'baseball glove',
    'skateboard', 'surfboard', 'tennis racket', 'bottle', 'N/A', 'wine glass',
    'cup', 'fork', 'knife', 'spoon', 'bowl', 'banana', 'apple', 'sandwich',
    'orange', 'broccoli', 'carrot', 'hot dog', 'pizza', 'donut', 'cake',
    'chair', 'couch', 'potted plant', 'bed', 'N/A', 'dining table', 'N/A',
    'N/A', 'toilet', 'N/A', 'tv', 'laptop', 'mouse', 'remote', 'keyboard',
    'cell phone', 'microwave', 'oven', 'toaster', 'sink', 'refrigerator', 'N/A',
    'book', 'clock', 'vase', 'scissors', 'teddy bear', 'hair drier',
    'toothbrush', "back"
]


def coco_samples(ann_file, img_dir, keep_crowd=False):
    """(samples, class_names, background_class) of a COCO annotation file.  Images without a box or with any crowd
    annotation are left out (the reference filters them after loading, coco.py:119); keep_crowd=True keeps the images with
    crowd annotations (the COCO evaluation protocol needs them: loss/coco_eval.py).  Every sample carries its per-box crowd flags
    and areas (the annotation's own `area`, or w * h of the box where the file has none), the image id and the (h, w) of the file."""
    with open(ann_file) as f:
        ann = json.load(f)
    cats = ann["categories"]
    max_id = int(max(c["id"] for c in cats))
    class_names = ["N/A"] * (max_id + 2)             # + 2 for the background class, last
    class_names[-1] = "back"
    for c in cats:
        class_names[c["id"]] = c["name"]
    per_image = defaultdict(list)
    for a in ann.get("annotations", []):
        per_image[a["image_id"]].append(a)
    samples = []
    for img in ann["images"]:
        anns = per_image.get(img["id"], [])
        if not anns or (not keep_crowd and any(a.get("iscrowd", 0) for a in anns)):
            continue
        W, H = float(img["width"]), float(img["height"])
        boxes = np.array([[(x + w / 2) / W, (y + h / 2) / H, w / W, h / H] for x, y, w, h in (a["bbox"] for a in anns)], np.float32)
        classes = np.array([[a["category_id"]] for a in anns], np.int64)
        crowd = np.array([1 if a.get("iscrowd", 0) else 0 for a in anns], np.uint8)
        area = np.array([a["area"] if a.get("area") is not None else a["bbox"][2] * a["bbox"][3] for a in anns], np.float32)
        samples.append(Sample(os.path.join(img_dir, img["file_name"]), boxes, classes, crowd, area, int(img["id"]),
                              (int(img["height"]), int(img["width"]))))
    return samples, class_names, max_id + 1


def load_coco_dataset(config, batch_size, augmentation=False, ann_dir=None, ann_file=None, img_dir=None, ann_fil=None, seed=None,
                      num_workers=4, device=None, scales=None, max_size=None, canvas=None, keep_crowd=False, with_meta=False, shuffle=True,
                      drop_remainder=True):
    """coco.py:95-126.  Returns (dataset, class_names) and sets config.background_class = max category id + 1.
    `ann_fil` is accepted as an alias of `ann_file` (train_coco.py:51 passes that spelling); `seed` makes the order, the
    augmentation records and therefore the batches reproducible.  For an evaluation by the COCO protocol over the whole file:
    keep_crowd=True, with_meta=True, shuffle=False, drop_remainder=False (DetectionDataset); keep_crowd with a training
    augmentation is a ValueError, a crowd box would be a wrong target."""
    if keep_crowd and DetectionDataset.is_training_mode(augmentation):
        raise ValueError(f"keep_crowd=True is for evaluation: augmentation must be False, None or 'shortest_side', got {augmentation!r}")
    ann_file = ann_fil if ann_file is None else ann_file
    ann_file = config.data.ann_file if ann_file is None else resolve(config.data.data_dir, ann_file)
    img_dir = config.data.img_dir if img_dir is None else resolve(config.data.data_dir, img_dir)
    samples, class_names, background = coco_samples(ann_file, img_dir, keep_crowd=keep_crowd)
    config.background_class = background
    return DetectionDataset(samples, config, batch_size, augmentation, seed=seed, num_workers=num_workers, device=device, scales=scales,
                            max_size=max_size, canvas=canvas, with_meta=with_meta, shuffle=shuffle, drop_remainder=drop_remainder), class_names
