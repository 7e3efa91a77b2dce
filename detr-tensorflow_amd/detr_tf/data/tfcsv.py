"""CSV loader for TensorFlow-object-detection style annotation files (reference detr_tf/data/tfcsv.py:12-77): one row per
box with filename, width, height, class, xmin, ymin, xmax, ymax."""
import os

import numpy as np

from .loader import DetectionDataset, Sample, resolve


def tfcsv_samples(csv_path, img_dir, exclude=()):
    """(samples, class_names): ["background"] + the sorted class names left after `exclude`."""
    import pandas as pd
    anns = pd.read_csv(csv_path)
    for name in exclude:
        anns = anns[anns["class"] != name]
    unique_class = anns["class"].unique()
    unique_class.sort()
    class_names = ["background"] + unique_class.tolist()
    samples = []
    for fn in anns["filename"].unique().tolist():
        rows = anns[anns["filename"] == fn]
        width, height = float(rows["width"].to_numpy()[0]), float(rows["height"].to_numpy()[0])
        xy = rows[["xmin", "ymin", "xmax", "ymax"]].to_numpy().astype(np.float64) / [width, height, width, height]
        boxes = np.stack([(xy[:, 0] + xy[:, 2]) / 2, (xy[:, 1] + xy[:, 3]) / 2, xy[:, 2] - xy[:, 0], xy[:, 3] - xy[:, 1]], 1)
        classes = np.array([[class_names.index(c)] for c in rows["class"]], np.int64)
        samples.append(Sample(os.path.join(img_dir, fn), boxes.astype(np.float32), classes))
    return samples, class_names


def load_tfcsv_dataset(config, batch_size, augmentation=False, exclude=[], ann_dir=None, ann_file=None, img_dir=None, seed=None,
                       num_workers=4, device=None, scales=None, max_size=None, canvas=None):
    """tfcsv.py:51-77.  Returns (dataset, class_names) and sets config.background_class = 0."""
    config.background_class = 0
    csv_path = config.data.ann_file if ann_file is None else resolve(config.data.data_dir, ann_file)
    img_dir = config.data.img_dir if img_dir is None else resolve(config.data.data_dir, img_dir)
    samples, class_names = tfcsv_samples(csv_path, img_dir, exclude)
    return DetectionDataset(samples, config, batch_size, augmentation, seed=seed, num_workers=num_workers, device=device, scales=scales,
                            max_size=max_size, canvas=canvas), class_names
