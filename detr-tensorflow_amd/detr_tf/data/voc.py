"""Pascal VOC loader (reference detr_tf/data/voc.py:22-55,79-127)."""
import os
import xml.etree.ElementTree as ET

import numpy as np

from .loader import DetectionDataset, Sample, resolve

VOC_CLASS_NAME = [
    "back", 'aeroplane', 'bicycle', 'bird', 'boat',
    'bottle', 'bus', 'car', 'cat', 'chair',
    'cow', 'diningtable', 'dog', 'horse',
    'motorbike', 'person', 'pottedplant',
    'sheep', 'sofa', 'train', 'tvmonitor'
]


def _objects(anno_path):
    root = ET.parse(anno_path)
    size = root.find("size")
    width, height = float(size.find("width").text), float(size.find("height").text)
    out = []
    for obj in root.findall("object"):
        name = obj.find("name").text.lower().strip()
        bb = obj.find("bndbox")
        xmin, ymin, xmax, ymax = ((float(bb.find(k).text) - 1) for k in ("xmin", "ymin", "xmax", "ymax"))
        xmin, xmax, ymin, ymax = xmin / width, xmax / width, ymin / height, ymax / height
        out.append((name, [xmin + (xmax - xmin) / 2, ymin + (ymax - ymin) / 2, xmax - xmin, ymax - ymin]))
    return out


def voc_samples(image_dir, anno_dir):
    """(samples, class_names): ids from the image directory (sorted), class names in order of first appearance after
    "back".  Images without an object are left out (the reference filters them after loading, voc.py:119)."""
    files = sorted(os.listdir(image_dir))
    class_names = ["back"]
    parsed = []
    for fn in files:
        objs = _objects(os.path.join(anno_dir, fn[:-4] + ".xml"))
        for name, _ in objs:
            if name not in class_names:
                class_names.append(name)
        parsed.append((fn, objs))
    samples = []
    for fn, objs in parsed:
        if not objs:
            continue
        boxes = np.array([b for _, b in objs], np.float32)
        classes = np.array([[class_names.index(n)] for n, _ in objs], np.int64)
        samples.append(Sample(os.path.join(image_dir, fn), boxes, classes))
    return samples, class_names


def load_voc_dataset(config, batch_size, augmentation=False, ann_dir=None, ann_file=None, img_dir=None, seed=None, num_workers=4,
                     device=None, scales=None, max_size=None, canvas=None):
    """voc.py:79-127.  Returns (dataset, class_names) and sets config.background_class = 0."""
    config.background_class = 0
    image_dir = config.data.img_dir if img_dir is None else resolve(config.data.data_dir, img_dir)
    anno_dir = config.data.ann_dir if ann_dir is None else resolve(config.data.data_dir, ann_dir)
    samples, class_names = voc_samples(image_dir, anno_dir)
    return DetectionDataset(samples, config, batch_size, augmentation, seed=seed, num_workers=num_workers, device=device, scales=scales,
                            max_size=max_size, canvas=canvas), class_names
