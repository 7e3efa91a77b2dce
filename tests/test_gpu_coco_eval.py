"""GPU tests of the COCO-protocol evaluation: the kernel csrc/coco_match.hip (detr_hip_coco_match) against the loop oracle
tests/coco_eval_ref.py -- score bits, class, rank, every flag word, npig and the status word compared with ==, with guard rows
around every output -- repeatability, and evaluation.eval_model(protocol="coco") on the device against the host path."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coco_eval_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64                                        # sentinel words on each side of every output
SENTINEL = 0x5A5A5A5A


def _launch(hip, bt, C, thresholds=None, area_ranges=None, npig_dev=None):
    """One detr_hip_coco_match launch with every output inside a sentinel-filled buffer.  Returns (rec_score, rec_class, rec_rank,
    rec_flags, npig, status) as the oracle returns them; asserts that no guard word changed."""
    thresholds = CR.THRESHOLDS if thresholds is None else thresholds
    area_ranges = CR.AREA_RANGES if area_ranges is None else area_ranges
    B, Q = bt["labels"].shape
    R, na = bt["t_bbox"].shape[1], len(area_ranges)
    ins = {k: torch.from_numpy(np.ascontiguousarray(bt[k])).to(DEV) for k in CR.KEYS}
    sizes = [B * Q, B * Q, B * Q, na * B * Q, 1]                       # score, class, rank, flags, status (int32 words)
    offs = np.cumsum([GUARD] + [n + GUARD for n in sizes])[:-1]
    buf = torch.full((int(offs[-1]) + sizes[-1] + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    buf[int(offs[4])] = 0                                              # the status word starts at zero
    if npig_dev is None:
        npig_dev = torch.full((C * na + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
        npig_dev[GUARD:GUARD + C * na] = 0
    d = hip.CocoMatchDesc()
    d.B, d.Q, d.R, d.nb_class, d.n_thr, d.n_area = B, Q, R, C, len(thresholds), na
    d.boxes, d.labels, d.scores, d.counts, d.sD_b = ins["boxes"].data_ptr(), ins["labels"].data_ptr(), ins["scores"].data_ptr(), ins["counts"].data_ptr(), Q
    d.t_bbox, d.sT_b, d.t_class, d.sC_b = ins["t_bbox"].data_ptr(), R * 4, ins["t_class"].data_ptr(), R
    d.t_crowd, d.t_area, d.sM_b, d.sizes = ins["t_crowd"].data_ptr(), ins["t_area"].data_ptr(), R, ins["sizes"].data_ptr()
    for t, th in enumerate(thresholds):
        d.thresholds[t] = th
    for a, (lo, hi) in enumerate(area_ranges):
        d.area_ranges[2 * a], d.area_ranges[2 * a + 1] = lo, hi
    base = buf.data_ptr()
    d.rec_score, d.rec_class, d.rec_rank, d.rec_flags, d.status = [base + 4 * int(o) for o in offs]
    d.npig = npig_dev.data_ptr() + 8 * GUARD
    assert d.boxes % 16 == 0
    hip._check(hip.load().detr_hip_coco_match(ctypes.byref(d), hip._stream()), "detr_hip_coco_match")
    torch.cuda.synchronize()
    host, npig_h = buf.cpu().numpy(), npig_dev.cpu().numpy()
    inside = np.zeros(len(host), bool)
    for o, n in zip(offs, sizes):
        inside[int(o):int(o) + n] = True
    assert (host[~inside] == SENTINEL).all(), "a guard word around the records was written"
    assert (npig_h[:GUARD] == SENTINEL).all() and (npig_h[GUARD + C * na:] == SENTINEL).all(), "a guard word around npig was written"
    parts = [host[int(o):int(o) + n] for o, n in zip(offs, sizes)]
    return (parts[0].view(np.float32).reshape(B, Q), parts[1].reshape(B, Q), parts[2].reshape(B, Q), parts[3].view(np.uint32).reshape(na, B, Q),
            npig_h[GUARD:GUARD + C * na].reshape(C, na), int(parts[4][0])), npig_dev


def _assert_equal(got, want):
    for name, g, w in zip(("score", "class", "rank", "flags", "npig"), got, want):
        g, w = [x.view(np.uint32) if x.dtype == np.float32 else x for x in (g, w)]
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:5])
    assert got[5] == want[5], "status"


def _special_batch(kind):
    rng = np.random.default_rng(17)
    if kind == "ranks_past_100":                   # Q = 130, 120 detections of one class in image 0: ranks 100 .. 119 appear
        bt = CR.random_batches(2, 130, 20, 4, seed=5)[1]
        t = np.concatenate([rng.uniform(0.2, 0.8, (6, 2)), rng.uniform(0.05, 0.4, (6, 2))], 1).astype(np.float32)
        y = CR._yxyx(t)
        dets = [(y[i % 6] if i % 3 else np.sort(rng.uniform(0, 1, (2, 2)), 0).reshape(4).astype(np.float32), 2,
                 np.float32(round(float(rng.uniform(0.05, 0.99)), 2))) for i in range(120)]
        dets += [(y[0], 1, np.float32(0.5))] * 5
        CR.fill_image(bt, 0, dets, t, np.array([2, 2, 2, 2, 1, 2]), np.array([0, 0, 1, 0, 0, 0], np.uint8),
                      np.array([500, 5000, 9000, 20000, 800, 100], np.float32), (300, 400), rng.permutation(125))
        return bt, 4
    if kind == "q1_r1":                            # one query slot, a header row and nothing else
        bt = CR.empty_batch(3, 1, 1)
        bt["sizes"][:] = (64, 96)
        bt["boxes"][:, 0] = (0.1, 0.1, 0.5, 0.5)
        bt["scores"][:, 0], bt["labels"][:, 0], bt["counts"][:] = 0.5, (0, 1, 0), (1, 1, 0)
        return bt, 2
    raise KeyError(kind)


def test_records_equal_the_oracle_with_255_matched_ground_truths(hip):
    """R = 256 with 255 ground truths in every image AND detections on them: exact and shrunk copies drawn from every quarter of the
    index range, crowds, score ties and a ground truth duplicated at the last index (tests/coco_eval_ref.py: dense_batch).  The
    oracle reports which ground truths were matched: every 64-wide chunk of the kernel's candidate ballot is exercised."""
    bt, want, taken = CR.dense_case()
    assert int(bt["t_bbox"][:, 0, 0].min()) == 255 and bt["t_bbox"].shape[1] == 256 and want[5] == 0
    CR.assert_every_chunk_matched(taken)
    got, _ = _launch(hip, bt, 3)
    _assert_equal(got, want)
    flags = want[3].reshape(4, -1)
    assert (flags & 0x3FF).any(1).all() and (flags >> 16).any(1).all()


@pytest.mark.parametrize("case", ["4x100x100", "r256", "small", "ranks_past_100", "q1_r1"])
def test_records_equal_the_oracle(hip, case):
    """(The r256 case has its 255 ground truths in an image WITHOUT detections: the header and staging path; the matching on
    ground truths past index 63 is test_records_equal_the_oracle_with_255_matched_ground_truths.)
    Seeded batches with every rule planted (tests/coco_eval_ref.py: random_batches -- the later index on ties, crowds that absorb,
    regular before crowd, ignored unmatched detections, score ties, a NaN score, a zero-area pair, an image without detections, an
    all-crowd image, an image without targets), 255 ground truths in 256 rows, ranks past 100, and Q = R = 1."""
    if case in ("ranks_past_100", "q1_r1"):
        bt, C = _special_batch(case)
        batches = [bt]
    else:
        B, Q, R, C = {"4x100x100": (4, 100, 100, 92), "r256": (2, 50, 256, 5), "small": (3, 12, 9, 3)}[case]
        batches = CR.random_batches(B, Q, R, C, seed=7)
    seen_flags = []
    for bt in batches:
        want = CR.coco_match_ref(*CR.as_args(bt), C)
        got, _ = _launch(hip, bt, C)
        _assert_equal(got, want)
        assert want[5] == 0
        seen_flags.append(want)
    if case == "ranks_past_100":
        assert seen_flags[0][2].max() == 119
    if case == "r256":
        assert max(int(bt["t_bbox"][:, 0, 0].max()) for bt in batches) == 255
    if case == "4x100x100":
        flags = np.concatenate([w[3].reshape(4, -1) for w in seen_flags], 1)
        assert (flags & 0x3FF).any() and (flags >> 16).any() and any(np.isnan(w[0]).any() for w in seen_flags)
        assert any((bt["counts"] == 0).any() for bt in batches) and any((bt["t_bbox"][:, 0, 0] == 0).any() for bt in batches)


def test_one_threshold_one_range_and_odd_counts(hip):
    bt = CR.random_batches(4, 40, 30, 6, seed=21)[0]
    for thr, rng_a in (([0.5], [[0.0, 1e10]]), ([0.9, 0.3, 0.6], [[100.0, 5000.0], [0.0, 1e10], [0.0, 0.0]]), (CR.THRESHOLDS[:7], CR.AREA_RANGES[:3])):
        want = CR.coco_match_ref(*CR.as_args(bt), 6, thr, rng_a)
        got, _ = _launch(hip, bt, 6, thr, rng_a)
        _assert_equal(got, want)


def test_status_bits_and_nothing_out_of_bounds(hip):
    """A bad label, target class, header, count or size sets its status bit, the item is skipped / clamped as the oracle does, and the
    guard rows around every output stay untouched (_launch asserts it)."""
    C = 6
    clean = CR.random_batches(4, 40, 30, C, seed=33)[1]
    for what, bit in (("label", CR.BAD_LABEL), ("label_neg", CR.BAD_LABEL), ("tclass", CR.BAD_TARGET_CLASS), ("header", CR.BAD_HEADER),
                      ("header_neg", CR.BAD_HEADER), ("header_nan", CR.BAD_HEADER), ("count", CR.BAD_COUNT), ("count_neg", CR.BAD_COUNT),
                      ("size", CR.BAD_SIZE), ("size_neg", CR.BAD_SIZE)):
        bt = {k: v.copy() for k, v in clean.items()}
        img = 1
        assert bt["counts"][img] > 0 and bt["t_bbox"][img, 0, 0] > 0
        if what == "label":
            bt["labels"][img, 0] = C
        elif what == "label_neg":
            bt["labels"][img, 0] = -7
        elif what == "tclass":
            bt["t_class"][img, 1, 0] = 1 << 40
        elif what == "header":
            bt["t_bbox"][img, 0, 0] = 30.0
        elif what == "header_neg":
            bt["t_bbox"][img, 0, 0] = -3.0
        elif what == "header_nan":
            bt["t_bbox"][img, 0, 0] = np.nan
        elif what == "count":
            bt["counts"][img] = 1 << 20
        elif what == "count_neg":
            bt["counts"][img] = -5
        elif what == "size":
            bt["sizes"][img] = (0, 50)
        else:
            bt["sizes"][img] = (40, -50)
        want = CR.coco_match_ref(*CR.as_args(bt), C)
        assert want[5] == bit, what
        got, _ = _launch(hip, bt, C)
        _assert_equal(got, want)


def test_two_launches_are_bit_identical_and_npig_accumulates(hip):
    C = 92
    batches = CR.random_batches(4, 100, 100, C, seed=7)
    a, npig_dev = _launch(hip, batches[0], C)
    b, _ = _launch(hip, batches[0], C)
    _assert_equal(a, b)
    c, _ = _launch(hip, batches[1], C, npig_dev=npig_dev)                # the same counters: the second batch adds to them
    want = CR.coco_match_ref(*CR.as_args(batches[0]), C)[4] + CR.coco_match_ref(*CR.as_args(batches[1]), C)[4]
    assert np.array_equal(c[4], want) and want.sum() > a[4].sum() > 0


def test_device_accumulator_equals_the_host_accumulator(hip):
    from detr_tf.loss.coco_eval import COCOAccumulator, DeviceCOCOAccumulator
    from map_match_ref import targets_to_yxyx
    C = 92
    batches = CR.random_batches(4, 100, 100, C, seed=7)
    host, dev = COCOAccumulator(C), DeviceCOCOAccumulator(C)
    for bt in batches:
        dev.add_detections(*[torch.from_numpy(np.ascontiguousarray(bt[k])).to(DEV) for k in CR.KEYS])
        for i in range(4):
            k, n = int(bt["counts"][i]), int(bt["t_bbox"][i, 0, 0])
            host.add_image(bt["boxes"][i, :k], bt["labels"][i, :k], bt["scores"][i, :k], targets_to_yxyx(bt["t_bbox"][i, 1:1 + n]),
                           bt["t_class"][i, 1:1 + n, 0], bt["t_crowd"][i, 1:1 + n], bt["t_area"][i, 1:1 + n], bt["sizes"][i])
    got = dev.to_host()
    for g, w in zip(got.records(), host.records()):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
    assert np.array_equal(got.npig, host.npig)
    assert got.result() == host.result() and 0 < host.result()["AP"] < 1
    bad = {k: v.copy() for k, v in batches[0].items()}
    bad["sizes"][0] = (0, 0)
    flagged = DeviceCOCOAccumulator(C)
    flagged.add_detections(*[torch.from_numpy(np.ascontiguousarray(bad[k])).to(DEV) for k in CR.KEYS])
    with pytest.raises(ValueError, match="image size"):
        flagged.to_host()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _cfg():
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.image_size = (64, 96)
    return cfg


def _dataset(tmp_path, model):
    """Five 64 x 96 images whose annotations are the model's own detections (so that the matching finds something), one of them a
    crowd; batch 2 -> a short last batch."""
    from PIL import Image
    from detr_tf.data import load_coco_dataset
    img_dir = tmp_path / "images"
    img_dir.mkdir()
    rng = np.random.default_rng(4)
    images = [{"id": 10 + i, "file_name": f"{i}.png", "height": 64, "width": 96} for i in range(5)]
    for im in images:
        Image.fromarray(rng.integers(0, 256, (64, 96, 3)).astype(np.uint8), "RGB").save(img_dir / im["file_name"])
    cats = [{"id": i, "name": f"c{i}"} for i in range(1, 91)]
    ann_file = tmp_path / "ann.json"
    kw = dict(augmentation=False, ann_file=str(ann_file), img_dir=str(img_dir), keep_crowd=True, with_meta=True, shuffle=False, drop_remainder=False)
    placeholder = [{"id": i, "image_id": 10 + i, "category_id": 1, "iscrowd": 0, "bbox": [1.0, 1.0, 10.0, 10.0], "area": 100.0} for i in range(5)]
    ann_file.write_text(json.dumps({"images": images, "annotations": placeholder, "categories": cats}))
    anns = []
    for (imgs, _tb, _tc, meta) in load_coco_dataset(_cfg(), 2, **kw)[0]:
        out = model(imgs, training=False)
        lab = out["pred_logits"].softmax(-1).argmax(-1).cpu()
        boxes = out["pred_boxes"].cpu().numpy()
        for b, image_id in enumerate(meta["image_id"].tolist()):
            keep = [q for q in torch.nonzero((lab[b] != 91) & (lab[b] != 0)).flatten().tolist()][:5]
            for n, q in enumerate(keep):
                cx, cy, w, h = [float(v) for v in boxes[b, q]]
                shrink = 1.0 if n % 2 == 0 else 0.8                    # half the targets are looser than the prediction
                anns.append({"id": len(anns), "image_id": image_id, "category_id": int(lab[b, q]), "iscrowd": int(image_id == 11 and n == 1),
                             "bbox": [(cx - w * shrink / 2) * 96, (cy - h * shrink / 2) * 64, w * shrink * 96, h * shrink * 64],
                             "area": w * shrink * 96 * h * shrink * 64 * 0.7})
    assert len({a["image_id"] for a in anns}) == 5 and any(a["iscrowd"] for a in anns), "the model must detect something in every image"
    ann_file.write_text(json.dumps({"images": images, "annotations": anns, "categories": cats}))
    cfg = _cfg()
    ds, names = load_coco_dataset(cfg, 2, **kw)
    assert cfg.background_class == 91 and len(names) == 92
    return ds, names, cfg


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_eval_model_coco_device_equals_host(hip, tmp_path, graph):
    from detr_tf.evaluation import eval_model
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref as R
    model = get_detr_model(_cfg(), include_top=True, num_encoder_layers=1, num_decoder_layers=2, device="cuda:0", dropout=0.0)
    assert not model.load_weights(R.make_params(7, num_enc=1, num_dec=2))
    model.eval_graph = False
    ds, names, cfg = _dataset(tmp_path, model)
    batches = list(ds)
    assert [len(b) for b in batches] == [4, 4, 4] and [int(b[1].shape[0]) for b in batches] == [2, 2, 1]       # the short last batch
    assert sum(int(b[3]["crowd"].sum()) for b in batches) == 1
    model.eval_graph = graph
    host = eval_model(model, cfg, names, iter(batches), print_result=False, protocol="coco")
    device = eval_model(model, cfg, names, iter(batches), print_result=False, protocol="coco", accumulate="device")
    assert device == host
    assert list(host)[:12] == list(CR.STAT_NAMES) and host["AP50"] > 0 and host["AR100"] > 0
    if graph:
        assert model._eval_graph is not None
    with pytest.raises(TypeError, match="with_meta"):
        eval_model(model, cfg, names, iter([b[:3] for b in batches]), print_result=False, protocol="coco")
    # the reference protocol is untouched: the same batches as 3-tuples, on both paths
    ref_host = eval_model(model, cfg, names, iter([b[:3] for b in batches]), print_result=False)
    ref_dev = eval_model(model, cfg, names, iter([b[:3] for b in batches]), print_result=False, accumulate="device", protocol="reference")
    assert ref_host == ref_dev and set(ref_host) == {"box", "mask"} and list(ref_host["box"])[0] == "all"
