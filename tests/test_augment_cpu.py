"""Dataset loaders and training augmentation, host side: the C entry point's argument checks, the transform records and their
distributions, the box transform, the area model of tests/augment_ref.py, and the COCO / VOC / CSV loaders on tiny datasets."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (96, 128)


class _Cfg:
    def __init__(self, data_dir=None, img_dir=None, ann_file=None, ann_dir=None, size=SIZE):
        from detr_tf.training_config import DataConfig
        self.normalized_method, self.image_size, self.background_class = "torch_resnet", size, -1
        self.data = DataConfig(data_dir, img_dir, ann_file, ann_dir)


def _lib():
    from detr_tf import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip, _hip.load()


def test_augment_symbol_declared_exported_mirrored():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    assert "detr_hip_augment" in declared and "detr_hip_augment" in _hip.EXPORTED_SYMBOLS and hasattr(lib, "detr_hip_augment")
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9
    from detr_tf.data import transformation as T
    assert f"#define DETR_AUG_IREC {T.IREC}" in hdr and f"#define DETR_AUG_FREC {T.FREC}" in hdr


def test_augment_rejects_bad_arguments_without_a_gpu():
    _, lib = _lib()
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every call below fails its checks first
    good = (ctypes.c_int32 * 3)(0, 1, 2)
    bad = (ctypes.c_int32 * 3)(0, 3, 2)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert lib.detr_hip_augment(fake, 1000, fake, fake, 1, 8, 8, fake, p(bad), fake, None) < 0
    assert "permutation" in lib.detr_hip_last_error().decode()
    for B, Hd, Wd in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -4), (70000, 8, 8)):
        assert lib.detr_hip_augment(fake, 1000, fake, fake, B, Hd, Wd, fake, p(good), fake, None) < 0
        assert "bad shape" in lib.detr_hip_last_error().decode()
    assert lib.detr_hip_augment(None, 1000, fake, fake, 1, 8, 8, fake, p(good), fake, None) < 0
    assert lib.detr_hip_augment(fake, 2, fake, fake, 1, 8, 8, fake, p(good), fake, None) < 0


def test_draw_transform_is_reproducible_and_in_range():
    from detr_tf.data import transformation as T
    a = [T.draw_transform(np.random.default_rng(7), 300 + i, 500 - i, SIZE, True) for i in range(50)]
    b = [T.draw_transform(np.random.default_rng(7), 300 + i, 500 - i, SIZE, True) for i in range(50)]
    assert a == b
    rng = np.random.default_rng(3)
    for i in range(2000):
        h0, w0 = int(rng.integers(20, 400)), int(rng.integers(20, 400))
        t = T.draw_transform(rng, h0, w0, SIZE, True)
        T.check_record(t, SIZE)
        hc, wc = T.crop_size(h0, w0, SIZE)
        assert 0 <= t.y0 <= h0 - hc and 0 <= t.x0 <= w0 - wc
        assert 0.5 <= t.sx <= 1.5 and 0.5 <= t.sy <= 1.5
    assert T.draw_transform(rng, 50, 60, SIZE, False) == T.Transform(50, 60, False, 0, T.CUBIC, T.CUBIC, 0, 0, 1.0, 1.0)


def test_draw_transform_frequencies():
    from detr_tf.data import transformation as T
    rng = np.random.default_rng(0)
    N = 20000
    ts = [T.draw_transform(rng, 480, 640, (200, 300), True) for _ in range(N)]

    def within(count, p):
        return abs(count / N - p) <= 3 * np.sqrt(p * (1 - p) / N)

    assert within(sum(t.flip for t in ts), 0.5)
    assert within(sum(t.kind == 0 for t in ts), 0.5)
    for k in (1, 2, 3):
        assert within(sum(t.kind == k for t in ts), 1 / 6), k
    for m in range(4):
        assert within(sum(t.iff == m for t in ts), 0.25), m
    resized = [t for t in ts if t.kind == 1]
    for m in range(4):
        c = sum(t.ia == m for t in resized)
        assert abs(c / len(resized) - 0.25) <= 3 * np.sqrt(0.25 * 0.75 / len(resized)), m
    crops = [t for t in ts if t.kind == 2]
    assert len({(t.y0, t.x0) for t in crops}) > 100


def _xyxy_norm(x1, y1, x2, y2, W, H):
    return [(x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H]


def test_transform_boxes_flip_and_resize():
    from detr_tf.data import transformation as T
    h0, w0 = 200, 100
    box = np.array([_xyxy_norm(10, 20, 30, 60, w0, h0)], np.float32)
    cls = np.array([[5]])
    # flip only, final resize 200 x 100 -> 96 x 128
    t = T.Transform(h0, w0, flip=True)
    got, c = T.transform_boxes(box, cls, h0, w0, t, SIZE)
    np.testing.assert_allclose(got[0], _xyxy_norm(70, 20, 90, 60, w0, h0), atol=1e-6)
    assert c.tolist() == [[5]]
    # stage-B resize then the identity final resize: normalised coordinates do not move
    t = T.Transform(h0, w0, kind=T.KINDS["resize"], ia=3)
    got, _ = T.transform_boxes(box, cls, h0, w0, t, SIZE)
    np.testing.assert_allclose(got, box, atol=1e-6)


def test_transform_boxes_crop_drops_and_clips():
    from detr_tf.data import transformation as T
    h0, w0 = 200, 300                                     # crop window 96 x 128 at (50, 100)
    t = T.Transform(h0, w0, kind=T.KINDS["crop"], y0=50, x0=100)
    boxes = np.array([
        _xyxy_norm(70, 60, 110, 80, w0, h0),              # 30 of 40 px outside to the left: 75 % out -> dropped
        _xyxy_norm(76, 60, 116, 80, w0, h0),              # 24 of 40 px outside: 60 % out -> kept, clipped
        _xyxy_norm(120, 70, 140, 90, w0, h0),             # inside
        _xyxy_norm(0, 0, 20, 20, w0, h0),                 # wholly outside
    ], np.float32)
    cls = np.array([[1], [2], [3], [4]])
    got, c = T.transform_boxes(boxes, cls, h0, w0, t, SIZE)
    assert c.ravel().tolist() == [2, 3]
    Hd, Wd = SIZE
    np.testing.assert_allclose(got[0], _xyxy_norm(0, 10, 16, 30, Wd, Hd), atol=1e-6)
    np.testing.assert_allclose(got[1], _xyxy_norm(20, 20, 40, 40, Wd, Hd), atol=1e-6)


def test_transform_boxes_affine():
    from detr_tf.data import transformation as T
    h0, w0 = 96, 128                                      # = target size: the final resize is the identity
    boxes = np.array([_xyxy_norm(0, 0, 32, 24, w0, h0), _xyxy_norm(96, 72, 128, 96, w0, h0)], np.float32)
    cls = np.array([[1], [2]])
    t = T.Transform(h0, w0, kind=T.KINDS["affine"], sx=0.5, sy=0.5)
    got, c = T.transform_boxes(boxes, cls, h0, w0, t, SIZE)
    assert c.ravel().tolist() == [1, 2]
    np.testing.assert_allclose(got[0], _xyxy_norm(32, 24, 48, 36, w0, h0), atol=1e-6)     # pulled toward the centre
    np.testing.assert_allclose(got[1], _xyxy_norm(80, 60, 96, 72, w0, h0), atol=1e-6)
    # 1.5: a corner box is pushed out (x1 -> -32, x2 -> 16: 2/3 of its width out, 0.89 of its area) and dropped,
    # a central one grows
    boxes = np.array([_xyxy_norm(0, 0, 32, 24, w0, h0), _xyxy_norm(56, 40, 72, 56, w0, h0)], np.float32)
    t = T.Transform(h0, w0, kind=T.KINDS["affine"], sx=1.5, sy=1.5)
    got, c = T.transform_boxes(boxes, cls, h0, w0, t, SIZE)
    assert c.ravel().tolist() == [2]
    np.testing.assert_allclose(got[0], _xyxy_norm(52, 36, 76, 60, w0, h0), atol=1e-6)


def test_no_augmentation_leaves_boxes_unchanged():
    from detr_tf.data import transformation as T
    rng = np.random.default_rng(1)
    c = rng.uniform(0.2, 0.8, (20, 2))
    wh = rng.uniform(0.01, 0.3, (20, 2))
    boxes = np.concatenate([c, wh], 1).astype(np.float32)
    t = T.draw_transform(rng, 333, 517, SIZE, False)
    got, cls = T.transform_boxes(boxes, np.arange(20)[:, None], 333, 517, t, SIZE)
    assert len(cls) == 20
    np.testing.assert_allclose(got, boxes, atol=1e-6)


def test_area_model_constant_and_block_means():
    import augment_ref as A
    img = np.full((37, 53, 3), 77, np.uint8)
    for hd, wd in ((10, 20), (5, 7), (60, 80), (37, 20)):
        assert (A.area_resize_uint8(img, hd, wd) == 77).all(), (hd, wd)
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (48, 60, 3)).astype(np.uint8)
    got = A.area_resize_uint8(img, 12, 20)                # 4 x 3 blocks
    ref = np.rint(img.astype(np.float64).reshape(12, 4, 20, 3, 3).mean(axis=(1, 3)))
    assert np.abs(got.astype(np.int64) - ref).max() == 0


def _png(path, h, w, mode="RGB", seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    if mode == "L":
        Image.fromarray(rng.integers(0, 256, (h, w)).astype(np.uint8), "L").save(path)
    elif mode == "RGBA":
        Image.fromarray(rng.integers(0, 256, (h, w, 4)).astype(np.uint8), "RGBA").save(path)
    else:
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8), "RGB").save(path)


def make_coco(tmp_path, n=7):
    """n images with boxes (sizes vary, one grey, one RGBA), one crowd image, one image without annotations."""
    img_dir = tmp_path / "images"
    img_dir.mkdir()
    images, anns = [], []
    aid = 1
    for i in range(n + 2):
        h, w = 40 + 7 * i, 60 + 5 * i
        mode = "L" if i == 1 else "RGBA" if i == 2 else "RGB"
        _png(img_dir / f"{i:03d}.png", h, w, mode, seed=i)
        images.append({"id": 100 + i, "file_name": f"{i:03d}.png", "height": h, "width": w})
        if i == n + 1:
            continue                                       # no annotation
        for k in range(2):
            anns.append({"id": aid, "image_id": 100 + i, "category_id": [1, 3, 7][(i + k) % 3], "iscrowd": int(i == n and k == 1),
                         "bbox": [5.0 + k * 10, 6.0, w / 3, h / 3]})
            aid += 1
    cats = [{"id": 1, "name": "person"}, {"id": 3, "name": "car"}, {"id": 7, "name": "train"}]
    ann_file = tmp_path / "ann.json"
    ann_file.write_text(json.dumps({"images": images, "annotations": anns, "categories": cats}))
    return str(ann_file), str(img_dir)


def test_coco_loader_host_side(tmp_path):
    from detr_tf.data import COCO_CLASS_NAME, load_coco_dataset
    from detr_tf.data.loader import decode_image
    assert len(COCO_CLASS_NAME) == 92 and COCO_CLASS_NAME[-1] == "back"
    ann_file, img_dir = make_coco(tmp_path)
    cfg = _Cfg()
    ds, names = load_coco_dataset(cfg, 3, augmentation=True, ann_fil=ann_file, img_dir=img_dir, seed=0)
    assert names == ["N/A", "person", "N/A", "car", "N/A", "N/A", "N/A", "train", "back"]
    assert cfg.background_class == 8
    assert len(ds.samples) == 7                           # the crowd image and the empty one are skipped
    assert sorted(os.path.basename(s.path) for s in ds.samples) == [f"{i:03d}.png" for i in range(7)]
    assert len(ds) == 2                                   # drop remainder
    s = [s for s in ds.samples if s.path.endswith("003.png")][0]
    np.testing.assert_allclose(s.boxes[0], [(5 + 75 / 6) / 75, (6 + 61 / 6) / 61, 1 / 3, 1 / 3], rtol=1e-6)
    assert s.classes.tolist() == [[1], [3]]
    for i in range(3):
        im = decode_image(os.path.join(img_dir, f"{i:03d}.png"))
        assert im.dtype == np.uint8 and im.shape == (40 + 7 * i, 60 + 5 * i, 3)
    b1 = list(ds.host_batches())
    ds2, _ = load_coco_dataset(_Cfg(), 3, augmentation=True, ann_file=ann_file, img_dir=img_dir, seed=0)
    b2 = list(ds2.host_batches())
    assert len(b1) == len(b2) >= 1 and all(len(b) == 3 for b in b1)
    for x, y in zip(b1, b2):
        for (ia, ra, ba, ca), (ib, rb, bb, cb) in zip(x, y):
            assert np.array_equal(ia, ib) and ra == rb and np.array_equal(ba, bb) and np.array_equal(ca, cb)


def test_voc_loader_host_side(tmp_path):
    from detr_tf.data import load_voc_dataset
    (tmp_path / "JPEGImages").mkdir()
    (tmp_path / "Annotations").mkdir()
    objs = {"a1": [("Dog ", (11, 21, 51, 41))], "a2": [("cat", (1, 1, 10, 10)), ("dog", (5, 5, 20, 30))], "a3": [],
            "a4": [("Person", (2, 3, 4, 5))], "a5": [("cat", (3, 3, 9, 9))]}
    for name, ob in objs.items():
        _png(tmp_path / "JPEGImages" / f"{name}.png", 50, 80)
        xml = "".join(f"<object><name>{n}</name><bndbox><xmin>{b[0]}</xmin><ymin>{b[1]}</ymin><xmax>{b[2]}</xmax><ymax>{b[3]}</ymax>"
                      "</bndbox></object>" for n, b in ob)
        (tmp_path / "Annotations" / f"{name}.xml").write_text(
            f"<annotation><size><width>80</width><height>50</height><depth>3</depth></size>{xml}</annotation>")
    cfg = _Cfg(str(tmp_path), "JPEGImages", None, "Annotations")
    ds, names = load_voc_dataset(cfg, 2, augmentation=False, seed=1)
    assert names == ["back", "dog", "cat", "person"] and cfg.background_class == 0
    assert len(ds.samples) == 4 and len(ds) == 2           # a3 has no object
    s = [s for s in ds.samples if s.path.endswith("a1.png")][0]
    np.testing.assert_allclose(s.boxes[0], [(10 + 50) / 2 / 80, (20 + 40) / 2 / 50, 40 / 80, 20 / 50], rtol=1e-6)
    assert s.classes.tolist() == [[1]]


def test_tfcsv_loader_host_side(tmp_path):
    from detr_tf.data import load_tfcsv_dataset
    (tmp_path / "img").mkdir()
    rows = ["filename,width,height,class,xmin,ymin,xmax,ymax"]
    for i in range(5):
        _png(tmp_path / "img" / f"f{i}.png", 60, 90, seed=i)
        rows.append(f"f{i}.png,90,60,{['helmet', 'head', 'person'][i % 3]},10,12,40,42")
        rows.append(f"f{i}.png,90,60,head,0,0,9,6")
    (tmp_path / "ann.csv").write_text("\n".join(rows) + "\n")
    cfg = _Cfg(str(tmp_path), "img", "ann.csv")
    ds, names = load_tfcsv_dataset(cfg, 2, augmentation=True, seed=0)
    assert names == ["background", "head", "helmet", "person"] and cfg.background_class == 0
    assert len(ds.samples) == 5 and len(ds) == 2
    s = ds.samples[0]
    np.testing.assert_allclose(s.boxes[0], [25 / 90, 27 / 60, 30 / 90, 30 / 60], rtol=1e-6)
    assert s.classes.ravel().tolist() == [2, 1]
    ds, names = load_tfcsv_dataset(_Cfg(str(tmp_path), "img", "ann.csv"), 2, exclude=["person", "helmet"])
    assert names == ["background", "head"] and len(ds.samples) == 5
