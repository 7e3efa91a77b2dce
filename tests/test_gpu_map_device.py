"""GPU tests of the device mAP accumulation: the kernel csrc/map_match.hip (detr_hip_map_match) behind
compute_map.DeviceAPAccumulator against the host accumulator APAccumulator -- flags, scores and ground-truth counts compared
with ==, never with a tolerance -- and evaluation.eval_model(accumulate="device") against accumulate="host"."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import map_match_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(batch):
    boxes, labels, scores, counts, t_bbox, t_class = batch
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (boxes, labels, scores, counts, t_bbox, t_class)]


def _records(acc):
    """(score, class, flags) of every batch as the kernel wrote them."""
    return [(r[0].view(torch.float32).cpu().numpy(), r[1].cpu().numpy(), r[2].cpu().numpy().view(np.uint32)) for r in acc._records]


def test_golden_fixture_through_add_detections(hip):
    """refpy_map.npz (the outputs of the reference's own cal_map / calc_map) through the kernel: the bounds of
    test_vectorised_map_equals_reference_code_outputs -- per-class AP within 1e-12, the result values equal, the printed table
    character for character."""
    from detr_tf.loss.compute_map import DeviceAPAccumulator, average_precision
    for ci in range(3):
        nb, boxes, labels, scores, counts, t_bbox, t_class, images, fx = MR.golden_case(ci)
        dacc = DeviceAPAccumulator(nb)
        dacc.add_detections(*_dev((boxes, labels, scores, counts, t_bbox, t_class)))
        acc = dacc.to_host()
        ref_pc = fx[f"m{ci}_per_class_ap"]
        for c in range(nb):
            empty = len(acc.scores[c]) == 0 and acc.num_gt[c] == 0
            assert empty == bool(ref_pc[0, c] < 0)
            if empty:
                continue
            flags = np.concatenate(acc.flags[c], 0) if acc.flags[c] else np.zeros((0, 10), bool)
            for t in range(10):
                ap = average_precision(acc.scores[c], flags[:, t], int(acc.num_gt[c]))
                assert abs(ap - ref_pc[t, c]) < 1e-12, (ci, c, t, ap, ref_pc[t, c])
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            maps = dacc.result([f"class_{i}" for i in range(nb)], print_result=True)
        assert [str(k) for k in maps["box"].keys()] == [str(k) for k in fx[f"m{ci}_box_keys"]]
        assert list(maps["box"].values()) == list(fx[f"m{ci}_box_vals"])
        assert list(maps["mask"].values()) == list(fx[f"m{ci}_mask_vals"])
        assert buf.getvalue() == str(fx[f"m{ci}_table"])


@pytest.mark.parametrize("B,Q,C", MR.RANDOM_SHAPES)
def test_random_batches_equal_the_host_accumulator(hip, B, Q, C):
    """Seeded random batches (tests/map_match_ref.py: random_batches) with every corner case of the matching rules planted and
    asserted on the host result; scores lists, concatenated flags and num_gt equal APAccumulator's on the same post-processed
    detections, and the raw records equal the NumPy restatement."""
    from detr_tf.loss.compute_map import DeviceAPAccumulator
    batches = MR.random_batches(B, Q, C, seed=1000 * B + Q + C)
    assert len(batches) >= 3
    want = MR.assert_planted_cases_occur(batches, C)
    dacc = DeviceAPAccumulator(C)
    for bt in batches:
        dacc.add_detections(*_dev(bt))
    got = dacc.to_host()
    MR.assert_same_accumulator(got, want)
    assert got.result() == want.result()
    for bt, (rs, rc, rf) in zip(batches, _records(dacc)):
        ws, wc, wf, _, status = MR.map_match_ref(*bt, C)
        assert status == 0
        assert np.array_equal(rs.view(np.uint32), ws.view(np.uint32)) and np.array_equal(rc, wc) and np.array_equal(rf, wf)


def test_other_thresholds_and_full_width(hip):
    """Sixteen unsorted thresholds; Q = 1024 detections in every image, four classes (then one), against 99 targets -- the
    largest shapes -- and the same targets in R = 256 padded rows."""
    from detr_tf.loss.compute_map import APAccumulator, DeviceAPAccumulator
    rng = np.random.default_rng(5)
    thr = [float(x) for x in rng.permutation(np.linspace(0.2, 0.95, 16))]
    batches = [MR.dense_batch(2, 1024, 4, seed=9), MR.dense_batch(2, 1024, 1, seed=10)]
    wide = []
    for boxes, labels, scores, counts, t_bbox, t_class in batches:      # the same targets in 256 padded rows
        tb, tc = np.zeros((2, 256, 4), np.float32), np.zeros((2, 256, 1), np.int64)
        tb[:, :MR.R_PAD], tc[:, :MR.R_PAD] = t_bbox, t_class
        wide.append((boxes, labels, scores, counts, tb, tc))
    for bs in (batches, wide):
        want, dacc = APAccumulator(4, thr), DeviceAPAccumulator(4, thr)
        for bt in bs:
            MR.host_accumulate(want, *bt)
            dacc.add_detections(*_dev(bt))
        MR.assert_same_accumulator(dacc.to_host(), want)
        flags = np.concatenate([np.concatenate(f, 0) for f in want.flags if f], 0)
        assert flags.shape == (4 * 1024, 16) and flags.any(0).all() and (~flags).any(0).all()


class _Echo:
    """A 'model' that predicts the targets of the current batch, shrunk by a per-box factor (IoU 0.5 .. 1), plus a few confident
    false positives: a non-trivial mAP at every threshold."""

    def __init__(self, seed):
        self.rng, self.cur = np.random.default_rng(seed), None

    def __call__(self, images, training=False):
        assert training is False
        tb, tc = self.cur
        B = tb.shape[0]
        logits = torch.full((B, 100, 92), -10.0)
        logits[:, :, 91] = 10.0
        boxes = torch.full((B, 100, 4), 0.5)
        for b in range(B):
            n = int(tb[b, 0, 0])
            jit = tb[b, 1:1 + n].copy()
            shrink = self.rng.uniform(0.5, 1.0, (n, 1))
            jit[:, 2:] *= np.where(self.rng.random((n, 1)) < 0.3, 1.0, shrink).astype(np.float32)      # 30 % exact copies
            boxes[b, :n] = torch.from_numpy(jit)
            logits[b, torch.arange(n), torch.from_numpy(tc[b, 1:1 + n, 0])] = torch.from_numpy(self.rng.uniform(12, 20, n).astype(np.float32))
            logits[b, 90:95, 3] = 15.0                                  # five false positives of class 3 at the default box
        return {"pred_logits": logits.to(DEV), "pred_boxes": boxes.to(DEV)}


def _cfg():
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    return cfg


def test_eval_model_device_equals_host_on_an_echo_model(hip, capsys):
    from detr_tf.evaluation import eval_model
    from oracle import set_loss_ref as L
    batches = []
    for i in range(3):
        tb, tc = L.make_targets(4, seed=60 + i, force_full=False)
        batches.append((np.zeros((4, 32, 32, 3), np.float32), tb, tc))
    names = [f"c{i}" for i in range(92)]
    res, tables = {}, {}
    for how, on_device in (("host", False), ("device", False), ("device", True)):
        echo = _Echo(7)

        def stream():
            for im, tb, tc in batches:
                echo.cur = (tb, tc)
                yield (im, torch.from_numpy(tb).to(DEV), torch.from_numpy(tc).to(DEV)) if on_device else (im, tb, tc)

        res[how, on_device] = eval_model(echo, _cfg(), names, stream(), accumulate=how)
        tables[how, on_device] = capsys.readouterr().out
    assert res["device", False] == res["host", False] == res["device", True]
    assert tables["device", False] == tables["host", False] == tables["device", True] and "  box |" in tables["host", False]
    box = res["host", False]["box"]
    assert 0 < box[95] < box[50] < 100.0                                # neither trivial end
    assert eval_model(_Echo(7), _cfg(), names, iter(()), accumulate="device", print_result=False) == \
        eval_model(_Echo(7), _cfg(), names, iter(()), print_result=False)
    with pytest.raises(ValueError):
        eval_model(_Echo(7), _cfg(), names, iter(()), accumulate="both")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_eval_model_device_equals_host_on_a_real_model(hip, graph):
    """A small DetrModel with seeded weights: two unpadded batches of one shape (with eval_graph the second and third call are
    the capture and a replay) and one padded (images, masks) batch.  The targets are taken from the model's own predictions so
    that detections match."""
    from detr_tf.evaluation import eval_model
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref as R
    cfg = _cfg()
    model = get_detr_model(cfg, include_top=True, num_encoder_layers=1, num_decoder_layers=2, device="cuda:0", dropout=0.0)
    assert not model.load_weights(R.make_params(7, num_enc=1, num_dec=2))
    model.eval_graph = False
    rng = np.random.default_rng(2)
    inputs = [rng.normal(size=(2, 96, 128, 3)).astype(np.float32) for _ in range(3)]
    masks = np.zeros((2, 96, 128), bool)
    masks[1, 64:, :] = True
    masks[1, :, 96:] = True
    padded = rng.normal(size=(2, 96, 128, 3)).astype(np.float32)
    padded[1][masks[1]] = 0.0
    inputs.append((padded, masks))
    batches = []
    for im in inputs:
        out = model(im)
        prob = out["pred_logits"].softmax(-1).cpu()
        tb, tc = np.zeros((2, 100, 4), np.float32), np.zeros((2, 100, 1), np.int64)
        for b in range(2):
            lab = prob[b].argmax(-1)
            keep = torch.nonzero(lab != 91).flatten()[:6]
            tb[b, 0, 0] = len(keep)
            tb[b, 1:1 + len(keep)] = out["pred_boxes"][b, keep].cpu().numpy()
            tc[b, 1:1 + len(keep), 0] = lab[keep].numpy()
        batches.append((im, tb, tc))
    assert sum(int(tb[:, 0, 0].sum()) for _, tb, _ in batches) > 0
    model.eval_graph = graph
    names = [f"c{i}" for i in range(92)]
    host = eval_model(model, cfg, names, iter(batches), print_result=False)
    device = eval_model(model, cfg, names, iter(batches), print_result=False, accumulate="device")
    assert device == host
    assert host["box"][50] > 0
    if graph:
        assert model._eval_graph is not None


def _logit_batch(seed=4, B=8, Q=300, C=92):
    rng = np.random.default_rng(seed)
    logits = torch.from_numpy(rng.normal(size=(B, Q, C)).astype(np.float32) * 2).to(DEV)
    boxes = torch.from_numpy(np.concatenate([rng.uniform(0.1, 0.9, (B, Q, 2)), rng.uniform(0.05, 0.6, (B, Q, 2))], -1).astype(np.float32)).to(DEV)
    bt = MR.random_batches(B, Q, C, seed=12)[1]
    return {"pred_logits": logits, "pred_boxes": boxes}, bt[4], bt[5]


def test_add_batch_does_not_synchronise(hip):
    """add_batch under torch.cuda.set_sync_debug_mode("error"), with device targets and with host (NumPy) targets."""
    from detr_tf.loss.compute_map import DeviceAPAccumulator
    out, tb, tc = _logit_batch()
    tb_d, tc_d = torch.from_numpy(tb).to(DEV), torch.from_numpy(tc).to(DEV)
    warm = DeviceAPAccumulator(92)                     # the first launch (code object load, pinned pool) outside the checked region
    warm.add_batch(out, tb, tc, 91)
    torch.cuda.synchronize()
    acc = DeviceAPAccumulator(92)
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            live = False
        except RuntimeError:
            live = True
        if live:
            acc.add_batch(out, tb_d, tc_d, 91)
            acc.add_batch(out, tb, tc, 91)             # NumPy targets: uploaded without blocking
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a .item() read-back in this torch build: the mode is not live")
    a, b = _records(acc)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    host = acc.to_host()
    assert sum(len(s) for s in host.scores) > 0 and int(host.num_gt.sum()) > 0


def test_two_runs_give_bit_identical_records(hip):
    from detr_tf.loss.compute_map import DeviceAPAccumulator
    out, tb, tc = _logit_batch()
    runs = [DeviceAPAccumulator(92) for _ in range(2)]
    for r in runs:
        for _ in range(2):
            r.add_batch(out, tb, tc, 91)
    for x, y in zip(_records(runs[0]), _records(runs[1])):
        assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(x, y))
    MR.assert_same_accumulator(runs[1].to_host(), runs[0].to_host())
    assert np.array_equal(runs[0]._num_gt.cpu().numpy(), runs[1]._num_gt.cpu().numpy())


def test_status_word(hip):
    """An out-of-range label, target class or header count sets the status word: to_host() raises, the offending item is
    skipped and every other image's records are what they were."""
    from detr_tf.loss.compute_map import DeviceAPAccumulator
    C = 92
    clean = MR.random_batches(5, 100, C, seed=31)[2]
    base = DeviceAPAccumulator(C)
    base.add_detections(*_dev(clean))
    base.to_host()
    ref = _records(base)[0]
    for what, bit in (("label", MR.BAD_LABEL), ("label_neg", MR.BAD_LABEL), ("tclass", MR.BAD_TARGET_CLASS), ("header", MR.BAD_HEADER),
                      ("header_neg", MR.BAD_HEADER), ("count", MR.BAD_COUNT)):
        boxes, labels, scores, counts, t_bbox, t_class = [x.copy() for x in clean]
        img = 1
        assert counts[img] > 0 and t_bbox[img, 0, 0] > 0
        if what == "label":
            labels[img, 0] = C
        elif what == "label_neg":
            labels[img, 0] = -7
        elif what == "tclass":
            t_class[img, 1, 0] = 1 << 40
        elif what == "header":
            t_bbox[img, 0, 0] = 100.0
        elif what == "header_neg":
            t_bbox[img, 0, 0] = -3.0
        else:
            counts[img] = 101
        bt = (boxes, labels, scores, counts, t_bbox, t_class)
        dacc = DeviceAPAccumulator(C)
        dacc.add_detections(*_dev(bt))
        with pytest.raises(ValueError):
            dacc.to_host()
        assert int(dacc._status.item()) == bit
        got = _records(dacc)[0]
        want = MR.map_match_ref(*bt, C)
        assert want[4] == bit
        for g, w, r in zip(got, want[:3], ref):
            g, w, r = [x.view(np.uint32) if x.dtype == np.float32 else x for x in (g, w, r)]
            assert np.array_equal(g, w), what
            others = np.arange(5) != img
            assert np.array_equal(g[others], r[others]), what
        assert np.array_equal(dacc._num_gt.cpu().numpy(), want[3])
