"""Aspect-preserving multi-scale input, host side: target_size, the multi-scale / evaluation records and their distributions,
the box transform of the padded path, the C entry point's declaration and argument checks, the NumPy model of
csrc/augment_padded.hip (tests/augment_padded_ref.py) and the loaders' new modes on a tiny COCO dataset."""
import ctypes
import os
import re

import numpy as np
import pytest

import augment_padded_ref as P
import augment_ref as A
from test_augment_cpu import _Cfg, _lib, make_coco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_target_size_hand_worked():
    from detr_tf.data.transformation import target_size
    table = [
        # h, w, short, max -> (hd, wd)
        ((480, 640, 800, 1333), (800, 1066)),      # 800 * 640 // 480 = 1066 <= 1333
        ((640, 480, 800, 1333), (1066, 800)),      # portrait: the same, transposed
        ((500, 500, 800, 1333), (800, 800)),       # square
        ((300, 1200, 800, 1333), (333, 1333)),     # panorama: 800 * 1200 > 1333 * 300, short = 1333 * 300 // 1200 = 333
        ((1200, 300, 800, 1333), (1333, 333)),
        ((427, 640, 800, 1333), (800, 1199)),      # 800 * 640 // 427 = 1199 (1199.06)
        ((426, 640, 800, 1333), (800, 1201)),      # 800 * 640 // 426 = 1201 (1201.9)
        ((375, 640, 800, 1333), (781, 1333)),      # 800 * 640 = 512000 > 1333 * 375 = 499875: 1333 * 375 // 640 = 781
        ((480, 640, 480, 1333), (480, 640)),       # already there
        ((480, 640, 600, None), (600, 800)),       # no maximum
        ((1, 5000, 800, 1333), (1, 1333)),         # never below one pixel
    ]
    for args, want in table:
        assert target_size(*args) == want, (args, target_size(*args), want)


def test_target_size_sweep():
    from detr_tf.data.transformation import target_size
    rng = np.random.default_rng(0)
    sizes = [(int(h), int(w)) for h, w in rng.integers(16, 2400, (1500, 2))]
    sizes += [(h, w) for h in (100, 333, 480, 799, 800, 801) for w in (100, 480, 1332, 1333, 1334, 2000)]
    for h, w in sizes:
        for short, max_size in ((800, 1333), (480, 1333), (608, 1000), (96, 160)):
            hd, wd = target_size(h, w, short, max_size)
            s, l = min(hd, wd), max(hd, wd)
            assert (hd <= wd) == (h <= w) or hd == wd, (h, w, hd, wd)
            assert 1 <= s <= short and l <= max_size, (h, w, short, max_size, hd, wd)
            assert s == short or l == max_size, (h, w, short, max_size, hd, wd)
            # the side that was not pinned is the exact aspect-preserving length, less than one pixel off
            mn, mx = min(h, w), max(h, w)
            if s == short and short * mx <= max_size * mn:
                assert 0 <= short * mx / mn - l < 1, (h, w, short, max_size, hd, wd)
            else:
                assert l == max_size and 0 <= max_size * mn / mx - s < 1, (h, w, short, max_size, hd, wd)


def _within(count, n, p, sigmas=4):
    return abs(count / n - p) <= sigmas * np.sqrt(p * (1 - p) / n)


def test_draw_multiscale_distribution_and_validity():
    from detr_tf.data import transformation as T
    assert T.MULTISCALE_SCALES == tuple(range(480, 801, 32)) and T.MULTISCALE_MAX_SIZE == 1333
    a = [T.draw_multiscale(np.random.default_rng(7), 300 + i, 500 - i) for i in range(50)]
    assert a == [T.draw_multiscale(np.random.default_rng(7), 300 + i, 500 - i) for i in range(50)]
    rng = np.random.default_rng(1)
    N = 20000
    h0, w0 = 800, 1200                                # the crop branch can never take the whole image: 600 < the intermediate width
    recs = [T.draw_multiscale(rng, h0, w0) for _ in range(N)]
    full = [r for r in recs if (r.y0, r.x0, r.hc, r.wc) == (0, 0, h0, w0)]
    crops = [r for r in recs if (r.y0, r.x0, r.hc, r.wc) != (0, 0, h0, w0)]
    assert _within(sum(r.flip for r in recs), N, 0.5)
    assert _within(len(full), N, 0.5)
    for s in T.MULTISCALE_SCALES:                     # branch A: min side = S unless the maximum binds (1200 / 800 * S <= 1333 always here)
        assert _within(sum(min(r.hd, r.wd) == s for r in full), len(full), 1 / len(T.MULTISCALE_SCALES)), s
    assert len({(r.y0, r.x0, r.hc, r.wc) for r in crops}) > 1000
    # the window mapped to the intermediate image (shortest side 400 / 500 / 600) has sides in [384, 600], to whole-pixel rounding
    for r in crops[:2000]:
        ok = False
        for s1 in T.CROP_SCALES:
            f = s1 / h0
            ok |= (T.CROP_MIN - 2 * f <= r.hc * f <= T.CROP_MAX + 2 * f) and (T.CROP_MIN - 2 * f <= r.wc * f <= T.CROP_MAX + 2 * f)
        assert ok, r
    # every size: valid records, windows inside the image, long side <= 1333
    rng = np.random.default_rng(2)
    for _ in range(5000):
        h0, w0 = int(rng.integers(1, 2500)), int(rng.integers(1, 2500))
        r = T.draw_multiscale(rng, h0, w0)
        T.check_padded_record(r, (1333, 1333))
        assert 0 <= r.y0 and r.y0 + r.hc <= h0 and 0 <= r.x0 and r.x0 + r.wc <= w0 and r.hc >= 1 and r.wc >= 1
        assert max(r.hd, r.wd) <= 1333 and min(r.hd, r.wd) >= 1
        assert (r.hd, r.wd) == T.target_size(r.hc, r.wc, min(r.hd, r.wd), 1333) or max(r.hd, r.wd) == 1333
    r = T.draw_multiscale(rng, 480, 640, scales=(96, 128), max_size=160, interp=2)
    assert max(r.hd, r.wd) <= 160 and r.interp == 2


def test_eval_record_and_validation():
    from detr_tf.data import transformation as T
    assert T.eval_record(480, 640) == T.PaddedRecord(480, 640, False, 0, 0, 480, 640, 800, 1066, T.LINEAR)
    assert T.eval_record(300, 1200, 800, 1333)[-3:-1] == (333, 1333)
    good = T.PaddedRecord(50, 70, True, 5, 6, 40, 60, 80, 120, 3)
    T.check_padded_record(good)
    T.check_padded_record(good, (80, 120))
    for bad in (good._replace(h0=0), good._replace(interp=4), good._replace(y0=11), good._replace(x0=-1), good._replace(wc=65),
                good._replace(hc=0), good._replace(hd=0), good._replace(wd=-3)):
        with pytest.raises(ValueError):
            T.check_padded_record(bad)
    with pytest.raises(ValueError, match="canvas"):
        T.check_padded_record(good, (79, 120))
    irec = T.pack_padded_records([good, T.eval_record(480, 640)], [0, (1 << 33) + 12])
    assert irec.dtype == np.int32 and irec.shape == (2, T.PADDED_IREC)
    assert irec[0].tolist() == [0, 0, 50, 70, 1, 5, 6, 40, 60, 80, 120, 3]
    assert irec[1].tolist() == [12, 2, 480, 640, 0, 0, 0, 480, 640, 800, 1066, 1]


def _norm(x1, y1, x2, y2, W, H):
    return [(x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H]


def _boxes_brute(boxes, classes, h0, w0, r):
    """Per box, per corner, in pixels of each frame in turn."""
    out, cls = [], []
    for (cx, cy, w, h), c in zip(np.asarray(boxes, np.float64), classes):
        x1, x2, y1, y2 = (cx - w / 2) * w0, (cx + w / 2) * w0, (cy - h / 2) * h0, (cy + h / 2) * h0
        if r.flip:
            x1, x2 = w0 - x2, w0 - x1
        x1, x2, y1, y2 = x1 - r.x0, x2 - r.x0, y1 - r.y0, y2 - r.y0                      # window frame
        x1, x2, y1, y2 = max(x1, 0.0), min(x2, float(r.wc)), max(y1, 0.0), min(y2, float(r.hc))
        if x2 - x1 <= 0 or y2 - y1 <= 0:
            continue
        sx, sy = r.wd / r.wc, r.hd / r.hc                                                # destination pixels
        out.append(_norm(x1 * sx, y1 * sy, x2 * sx, y2 * sy, r.wd, r.hd))
        cls.append(c)
    return np.array(out, np.float64).reshape(-1, 4), cls


def test_transform_boxes_padded_against_brute_force():
    from detr_tf.data import transformation as T
    h0, w0 = 200, 300
    boxes = np.array([
        _norm(10, 20, 60, 90, w0, h0),               # 0: outside the inner window without flip, inside part of it with flip
        _norm(90, 40, 150, 100, w0, h0),             # 1: straddles the window's left and top edges
        _norm(120, 70, 160, 110, w0, h0),            # 2: inside
        _norm(0, 0, 300, 200, w0, h0),               # 3: covers the window (and the image)
        _norm(250, 150, 290, 190, w0, h0),           # 4: fully outside the inner window either way
        _norm(100, 10, 200, 48, w0, h0),             # 5: above the window, overlapping it in x only: no height after clipping
    ], np.float32)
    cls = np.arange(6)[:, None] + 10
    inner = dict(y0=50, x0=100, hc=100, wc=120)
    for flip in (False, True):
        for r in (T.PaddedRecord(h0, w0, flip, 0, 0, h0, w0, 400, 600), T.PaddedRecord(h0, w0, flip, hd=333, wd=401, **inner)):
            got, c = T.transform_boxes_padded(boxes, cls, h0, w0, r)
            want, wc = _boxes_brute(boxes, cls.ravel().tolist(), h0, w0, r)
            assert got.dtype == np.float32 and c.ravel().tolist() == wc, (r, c.ravel().tolist(), wc)
            np.testing.assert_allclose(got, want, atol=1e-6)
            assert (got[:, 2:] > 0).all() and (got[:, :2] - got[:, 2:] / 2 >= -1e-6).all() and (got[:, :2] + got[:, 2:] / 2 <= 1 + 1e-6).all()
    # spelled out: inner window, no flip
    got, c = T.transform_boxes_padded(boxes, cls, h0, w0, T.PaddedRecord(h0, w0, False, hd=50, wd=60, **inner))
    assert c.ravel().tolist() == [11, 12, 13]
    np.testing.assert_allclose(got[0], _norm(0, 0, 50, 50, 120, 100), atol=1e-6)         # clipped to the window's corner
    np.testing.assert_allclose(got[1], _norm(20, 20, 60, 60, 120, 100), atol=1e-6)
    np.testing.assert_allclose(got[2], [0.5, 0.5, 1.0, 1.0], atol=1e-6)                  # the covering box becomes the whole image
    # flip: box 0 (x 10..60) lands at x 240..290, outside the window 100..220; box 4 (x 250..290) lands at 10..50: outside too
    got, c = T.transform_boxes_padded(boxes, cls, h0, w0, T.PaddedRecord(h0, w0, True, hd=50, wd=60, **inner))
    assert 10 not in c.ravel().tolist() and 14 not in c.ravel().tolist() and 13 in c.ravel().tolist()
    empty, c = T.transform_boxes_padded(np.zeros((0, 4), np.float32), np.zeros((0, 1), np.int64), h0, w0, T.eval_record(h0, w0))
    assert empty.shape == (0, 4) and len(c) == 0


def test_augment_padded_symbol_declared_exported_mirrored():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    name = "detr_hip_augment_padded"
    assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9
    from detr_tf.data import transformation as T
    assert f"#define DETR_AUGP_IREC {T.PADDED_IREC}" in hdr and P.IREC == T.PADDED_IREC == len(T.PaddedRecord._fields) + 2


def test_augment_padded_rejects_bad_arguments_without_a_gpu():
    _, lib = _lib()
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every call below fails its checks first
    good = (ctypes.c_int32 * 3)(0, 1, 2)
    bad = (ctypes.c_int32 * 3)(0, 3, 2)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    f = lib.detr_hip_augment_padded
    assert f(fake, 1000, fake, 1, 8, 8, fake, p(bad), fake, fake, None) < 0
    assert "permutation" in lib.detr_hip_last_error().decode()
    for B, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -4), (70000, 8, 8), (1, 40000, 40000)):
        assert f(fake, 1000, fake, B, H, W, fake, p(good), fake, fake, None) < 0
        assert "bad shape" in lib.detr_hip_last_error().decode()
    assert f(None, 1000, fake, 1, 8, 8, fake, p(good), fake, fake, None) < 0
    assert f(fake, 1000, fake, 1, 8, 8, fake, p(good), fake, None, None) < 0          # no mask
    assert f(fake, 2, fake, 1, 8, 8, fake, p(good), fake, fake, None) < 0


def test_padded_model_placement_and_identity():
    from detr_tf.data import transformation as T
    from detr_tf.data.processing import normalization_table
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((20, 30), (33, 17))]
    lut, perm = normalization_table("tf_resnet")
    recs = [T.PaddedRecord(20, 30, True, 0, 0, 20, 30, 20, 30), T.PaddedRecord(33, 17, False, 3, 2, 10, 12, 10, 12)]
    out, mask = P.augment_padded(imgs, recs, 40, 32, lut, perm)
    assert out.shape == (2, 40, 32, 3) and mask.dtype == bool
    assert np.array_equal(out[0, :20, :30], A.normalise(imgs[0][:, ::-1], lut, perm))               # identity resize: the flipped image
    assert np.array_equal(out[1, :10, :12], A.normalise(imgs[1][3:13, 2:14], lut, perm))            # the window itself
    for b, r in enumerate(recs):
        assert not mask[b, :r.hd, :r.wd].any() and mask[b, r.hd:].all() and mask[b, :, r.wd:].all()
        assert (out[b, r.hd:] == 0).all() and (out[b, :, r.wd:] == 0).all()
    # constant images stay constant through every interpolation, enlarging and reducing
    img = np.full((37, 53, 3), 77, np.uint8)
    for interp in range(4):
        for hd, wd in ((10, 20), (60, 80), (37, 20)):
            for f in (P.padded_uint8, P.padded_uint8_f64):
                assert (f(img, T.PaddedRecord(37, 53, False, 4, 5, 30, 40, hd, wd, interp)) == 77).all(), (interp, hd, wd)


def test_padded_model_meets_the_acceptance_rule_alone():
    """The fp32 model against the float64 restatement on the kernel test's own inputs, under the kernel test's rule (share of
    elements off by more than 1e-6 below 1e-3, maximum below 1.6 quantisation levels): the rule leaves room for fp32 rounding
    of the coefficients (a pixel that lands within ~1e-4 of a .5 boundary may round the other way: one level) and for nothing
    else, so a kernel that passes it computes these formulas."""
    from detr_tf.data import transformation as T
    from detr_tf.data.processing import normalization_table
    cases = list(P.kernel_cases(T))
    assert len(cases) == 2 * 4 * 2 * 2
    assert {(r.interp, r.flip, (r.hc, r.wc) == (r.h0, r.w0)) for _, _, recs, _ in cases for r in recs} == \
        {(i, f, w) for i in range(4) for f in (False, True) for w in (False, True)}
    worst = {}
    for method in ("torch_resnet", "tf_resnet"):
        lut, perm = normalization_table(method)
        lvl = 1.0 / (255.0 * 0.224) if method == "torch_resnet" else 1.0
        for tag, images, recs, (H, W) in cases:
            for r in recs:
                T.check_padded_record(r, (H, W))
            ref, m32 = P.augment_padded(images, recs, H, W, lut, perm)
            f64, m64 = P.augment_padded(images, recs, H, W, lut, perm, resize=P.padded_uint8_f64)
            assert np.array_equal(m32, m64)
            diff = np.abs(ref - f64)
            share, mx = float((diff > 1e-6).mean()), float(diff.max())
            worst[method] = max(worst.get(method, (0, 0)), (share, mx / lvl))
            assert share < 1e-3 and mx < 1.6 * lvl, (method, tag, share, mx)
    print("fp32 model vs float64 restatement, worst (share, levels):", worst)


def test_loader_padded_modes_host_side(tmp_path):
    from detr_tf.data import load_coco_dataset
    from detr_tf.data import transformation as T
    from detr_tf.data.loader import DetectionDataset
    ann_file, img_dir = make_coco(tmp_path)
    kw = dict(ann_file=ann_file, img_dir=img_dir, seed=0, scales=(64, 80, 96), max_size=128, canvas=(128, 128))
    ds, _ = load_coco_dataset(_Cfg(), 3, augmentation="multiscale", **kw)
    ds2, _ = load_coco_dataset(_Cfg(), 3, augmentation="multiscale", **kw)
    b1, b2 = list(ds.host_batches()), list(ds2.host_batches())
    assert len(b1) == len(b2) >= 1 and all(len(b) == 3 for b in b1)
    for x, y in zip(b1, b2):
        for (ia, ra, ba, ca), (ib, rb, bb, cb) in zip(x, y):
            assert np.array_equal(ia, ib) and ra == rb and np.array_equal(ba, bb) and np.array_equal(ca, cb)
            assert isinstance(ra, T.PaddedRecord) and (ra.h0, ra.w0) == ia.shape[:2]
            T.check_padded_record(ra, (128, 128))
            assert len(ba) >= 1 and len(ba) == len(ca) and max(ra.hd, ra.wd) <= 128
    ev, _ = load_coco_dataset(_Cfg(), 2, augmentation="shortest_side", **kw)
    for batch in ev.host_batches():
        for im, r, boxes, classes in batch:
            h0, w0 = im.shape[:2]
            assert r == T.eval_record(h0, w0, 96, 128)
            # full window, no flip: normalised boxes do not move
            assert any(len(s.boxes) == len(boxes) and np.allclose(boxes, s.boxes, atol=1e-6) for s in ev.samples)
    with pytest.raises(ValueError, match="augmentation"):
        DetectionDataset([], _Cfg(), 1, augmentation="multi_scale")
    # the existing modes are untouched by the new arguments
    old, _ = load_coco_dataset(_Cfg(), 3, augmentation=True, ann_file=ann_file, img_dir=img_dir, seed=0)
    assert not old.padded and all(isinstance(b[1], T.Transform) for batch in old.host_batches() for b in batch)
