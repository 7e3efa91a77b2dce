"""GPU tests of the sigmoid focal class criterion (the _focal_ entry points of csrc/setloss.hip, the _scored entry points of
csrc/postprocess.hip and csrc/detect.hip, and the host path above them) against tests/focal_ref.py: every (parameter set, case) of that
module -- cost against the float32 reference, the assignment against SciPy on the device's own cost, values and gradients against the
float64 reference on that matching --, determinism, empty batches, the additivity of the sums, NaN and invalid labels, get_losses and
the graphed training step across a softmax -> focal switch, and sigmoid scoring.  The bounds are those of
tests/test_gpu_setloss_edges.py and tests/test_gpu_criterion.py; tests/test_focal_cpu.py measures the float32 reference against them
without a GPU."""
import ctypes
import gc
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criterion_ref as CR                 # noqa: E402
import focal_ref as FR                     # noqa: E402
import setloss_cases as SC                 # noqa: E402
from test_gpu_setloss_edges import SENTINEL, _check_values, _device_view, close, g       # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOSS_SCALE = 0.5
GUARD = 64                                  # sentinel floats in front of and behind the gradient tensors


class Rig:
    """The device tensors of one problem set and the launches of the _focal_ entry points on them."""

    def __init__(self, hip, w, f, logits, boxes, t_bbox, t_class, bg, layout="contiguous"):
        from detr_tf.loss.hungarian_matching import make_desc
        self.hip, self.w, self.f = hip, w, f
        self.Lv, self.B, self.Q, self.C = logits.shape
        self.R = t_bbox.shape[1]
        self.P = self.Lv * self.B
        self.lgd = _device_view(logits, layout, SC.C_SLACK)
        self.bxd = _device_view(boxes, layout, SC.BOX_SLACK)
        self.tbd, self.tcd = g(torch.from_numpy(t_bbox)), g(torch.from_numpy(t_class).reshape(self.B, self.R))
        self.d = make_desc(self.lgd, self.bxd, self.tbd, self.tcd, bg)
        self.block, self.fblock = CR.host_block(w), FR.focal_block(f)

    def cost(self):
        cost = torch.full((self.P, self.Q, self.R - 1), float(SENTINEL), device=DEV)
        self.hip.call("detr_hip_match_cost_focal_f32", ctypes.byref(self.d), self.block, self.fblock, cost.data_ptr())
        return cost

    def assign(self, cost):
        tfp = torch.full((self.P, self.Q), SENTINEL, device=DEV, dtype=torch.int32)
        pft = torch.full((self.P, self.R - 1), SENTINEL, device=DEV, dtype=torch.int32)
        st = torch.full((self.P,), SENTINEL, device=DEV, dtype=torch.int32)
        self.hip.call("detr_hip_assign_f32", cost.data_ptr(), self.P, self.Q, self.R - 1, self.tbd.data_ptr(), self.B, self.R,
                      tfp.data_ptr(), pft.data_ptr(), st.data_ptr())
        return tfp, pft, st

    def sums(self, tfp):
        sums = torch.zeros(self.Lv * 10, device=DEV)
        self.hip.call("detr_hip_set_loss_sums_focal_f32", ctypes.byref(self.d), self.block, self.fblock, tfp.data_ptr(), sums.data_ptr())
        return sums

    def finalize(self, sums):
        out = torch.zeros(self.Lv, 6, device=DEV)
        tot = torch.zeros(1, device=DEV)
        self.hip.call("detr_hip_set_loss_finalize_focal_f32", sums.data_ptr(), self.Lv, self.block, self.fblock, out.data_ptr(), tot.data_ptr())
        return out, tot

    def grad(self, tfp, sums):
        """Contiguous gradient tensors inside guard bands of sentinels (the kernel addresses them with the strides of the inputs)."""
        assert self.lgd.is_contiguous() and self.bxd.is_contiguous()
        bufs = []
        for ref in (self.lgd, self.bxd):
            buf = torch.full((ref.numel() + 2 * GUARD,), float(SENTINEL), device=DEV)
            bufs.append((buf, buf[GUARD:GUARD + ref.numel()].view(ref.shape)))
        (bl, dl), (bb, dbx) = bufs
        self.hip.call("detr_hip_set_loss_grad_focal_f32", ctypes.byref(self.d), self.block, self.fblock, tfp.data_ptr(), sums.data_ptr(),
                      ctypes.c_float(LOSS_SCALE), dl.data_ptr(), dbx.data_ptr())
        for buf in (bl, bb):
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), "a gradient kernel wrote outside its tensor"
        return dl, dbx

    def run(self, grad=True):
        cost = self.cost()
        tfp, pft, st = self.assign(cost)
        sums = self.sums(tfp)
        out, tot = self.finalize(sums)
        r = SimpleNamespace(tfp_dev=tfp, sums_dev=sums)
        if grad:
            dl, dbx = self.grad(tfp, sums)
            r.d_logits, r.d_boxes = dl.cpu(), dbx.cpu()
        torch.cuda.synchronize()
        r.cost, r.tfp, r.pft, r.status, r.sums, r.out, r.total = (cost.cpu(), tfp.cpu().numpy(), pft.cpu().numpy(), st.cpu().numpy(),
                                                                  sums.cpu(), out.cpu(), float(tot))
        return r


def _reference64(logits, boxes, t_bbox, t_class, bg, w, f, match=None, nan_invalid=True):
    lg = torch.from_numpy(logits).double().requires_grad_(True)
    bx = torch.from_numpy(boxes).double().requires_grad_(True)
    total, losses, match = FR.focal_losses(lg, bx, torch.from_numpy(t_bbox).double(), torch.from_numpy(t_class), bg, w, f, match=match,
                                           nan_invalid=nan_invalid)
    return lg, bx, total, losses, match


def _device_match(r, t_bbox, t_class, Lv, B, Q, n_list):
    """SciPy on the DEVICE's cost matrix, problem by problem: the assignment must equal it index for index; returned in the form
    the reference takes."""
    def cost_fn(lv, b, tb, tc):
        p, n = lv * B + b, n_list[b]
        c = r.cost[p, :, :n].numpy()
        status, pft = SC.scipy_solve(c)
        assert status == 0 and r.status[p] == 0
        assert np.array_equal(r.pft[p, :n], pft), f"problem {p}: the device assignment differs from SciPy on the device's own cost"
        assert (r.pft[p, n:] == -1).all()
        inv = np.full(Q, -1)
        inv[pft] = np.arange(n)
        assert np.array_equal(r.tfp[p], inv)
        return c
    return CR.match_from_cost(cost_fn, torch.from_numpy(t_bbox).double(), torch.from_numpy(t_class), Lv, B, Q)


def _check_cost(r, logits, boxes, t_bbox, t_class, n_list, w, f, key):
    """Against the float32 reference: 2e-6 absolute at weights up to 1, scaled by the largest cost weight above that (4x the float32
    reference's own error where focal_ref records one); columns >= n untouched."""
    from oracle import set_loss_ref as L
    Lv, B = logits.shape[:2]
    bound = FR.cost_atol(key) or 2e-6 * max(1.0, w.cost_class, w.cost_bbox, w.cost_giou)
    worst = 0.0
    for lv in range(Lv):
        for b in range(B):
            n = n_list[b]
            tbs, tcs = L.strip_header(torch.from_numpy(t_bbox[b]), torch.from_numpy(t_class[b]))
            ref = FR.cost_matrix(tbs, tcs, torch.from_numpy(boxes[lv, b]), torch.from_numpy(logits[lv, b]), w, f)
            got = r.cost[lv * B + b]
            assert bool((got[:, n:] == SENTINEL).all()), f"cost lv{lv} b{b}: written past n = {n}"
            err = float((got[:, :n] - ref).abs().max()) if n else 0.0
            worst = max(worst, err)
            assert err <= bound, f"cost lv{lv} b{b}: max abs err {err:.3e} > {bound:.1e}"
    print(f"cost: max abs err {worst:.3e}, bound {bound:.1e}")


def _check_grads(r, lg64, bx64, key, what=""):
    close(r.d_logits, LOSS_SCALE * lg64.grad, rtol=2e-5, what=what + "d_logits", atol=FR.d_logits_atol(key))
    close(r.d_boxes, LOSS_SCALE * bx64.grad, rtol=5e-5, what=what + "d_boxes", atol=FR.d_boxes_atol(key))


def _check_counts(r, match, Lv, B, Q):
    for lv in range(Lv):
        npos = match[lv][2].numel()
        s = r.sums[lv * 8:lv * 8 + 8]
        assert float(s[1]) == 0.0 and float(s[7]) == 0.0                                   # slot 1 stays 0 under focal
        assert float(s[4]) == npos and float(s[3]) == B * Q - npos
        for k in (2, 5, 6):
            assert float(s[k]) == int(s[k]) and 0 <= float(s[k]) <= (B * Q - npos if k == 2 else npos)


# ------------------------------------------------------------------------------------------
# 1 + 2. every (parameter set, case): cost, assignment, values, gradients
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,case", FR.PAIRS, ids=FR.PAIR_IDS)
def test_focal_case_vs_reference(hip, ps, case):
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    w, f = FR.param_set(ps)
    key = (ps, name.rsplit("-", 1)[0])
    logits, boxes, t_bbox, t_class, _ = FR.inputs(case)
    contiguous = layout == "contiguous"
    r = Rig(hip, w, f, logits, boxes, t_bbox, t_class, bg, layout).run(grad=contiguous)     # the gradient tensors follow contiguous heads
    _check_cost(r, logits, boxes, t_bbox, t_class, n_list, w, f, key)
    match = _device_match(r, t_bbox, t_class, Lv, B, Q, n_list)
    lg64, bx64, total, losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w, f, match=match)
    _check_values(r, losses, total, Lv, what=f"{ps} ")
    _check_counts(r, match, Lv, B, Q)
    for lv in range(Lv):                                              # the metric counts, exactly: numerators of the reference's means
        tb, tc, ti, pi, sel = match[lv]
        pred = FR.predicted_class(torch.from_numpy(logits[lv]).double().reshape(-1, C), bg)
        s = r.sums[lv * 8:lv * 8 + 8]
        assert float(s[2]) == int((pred[~sel] == bg).sum()) and float(s[5]) == int((pred[pi] != bg).sum())
        assert float(s[6]) == int((pred[pi] == tc[ti].long()).sum())
    if contiguous:
        total.backward()
        _check_grads(r, lg64, bx64, key)
        for b, n in enumerate(n_list):
            if n == 0:
                assert all(bool((r.d_boxes[lv, b] == 0).all()) for lv in range(Lv))


# ------------------------------------------------------------------------------------------
# 3. determinism, empty batches, additivity, NaN, invalid labels
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CR.CONTIGUOUS if c[3] in (17, 100)], ids=lambda c: c[0])
def test_two_runs_give_the_same_gradients(hip, case):
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    w, f = FR.param_set("F0")
    logits, boxes, t_bbox, t_class, _ = FR.inputs(case)
    rig = Rig(hip, w, f, logits, boxes, t_bbox, t_class, bg)
    a, b = rig.run(), rig.run()
    assert torch.equal(a.cost, b.cost) and np.array_equal(a.tfp, b.tfp)
    assert torch.equal(a.d_logits, b.d_logits) and torch.equal(a.d_boxes, b.d_boxes)
    sa, sb = a.sums[:Lv * 8].view(Lv, 8), b.sums[:Lv * 8].view(Lv, 8)
    assert torch.equal(sa[:, 1:7], sb[:, 1:7])


@pytest.mark.parametrize("ps", ["F0", "F2"])
def test_all_images_empty(hip, ps):
    Lv, B, Q, C, bg, R = 2, 2, 9, 5, 4, 6
    rng = np.random.default_rng(11)
    logits = (rng.normal(size=(Lv, B, Q, C)) * 2).astype(np.float32)
    boxes = rng.uniform(0.1, 0.6, (Lv, B, Q, 4)).astype(np.float32)
    t_bbox, t_class = SC.make_targets([0, 0], R, C, bg, rng)
    w, f = FR.param_set(ps)
    lg64, bx64, total, losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w, f)
    r = Rig(hip, w, f, logits, boxes, t_bbox, t_class, bg).run()
    assert (r.status == 0).all() and (r.tfp == -1).all() and bool((r.cost == SENTINEL).all())
    _check_values(r, losses, total, Lv)
    label_sum = sum(losses["label_cost" + ("" if lv == Lv - 1 else f"_{lv}")] for lv in range(Lv))
    for lv in range(Lv):                                              # the class term always clamps: the sum over max(0, 1)
        assert math.isfinite(float(r.out[lv, 0])) and float(r.out[lv, 0]) > 0
        assert math.isnan(float(r.out[lv, 2])) and math.isnan(float(r.out[lv, 3]))          # true_pos, pos_accuracy: 0 / 0
    if w.min_one:
        assert math.isfinite(r.total) and float(r.out[0, 4]) == 0.0 and float(r.out[0, 5]) == 0.0
        total.backward()
    else:
        assert math.isnan(r.total) and math.isnan(float(total))      # the box terms follow num_boxes_min_one
        (w.class_coef * label_sum).backward()
    assert bool((r.d_boxes == 0).all()) and bool(torch.isfinite(r.d_logits).all())
    close(r.d_logits, LOSS_SCALE * lg64.grad, rtol=2e-5, what="d_logits")


def test_sums_of_half_batches_add_up(hip):
    case = next(c for c in CR.CONTIGUOUS if c[3] == 17)
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    assert B == 2
    w, f = FR.param_set("F2")
    logits, boxes, t_bbox, t_class, _ = FR.inputs(case)
    rig = Rig(hip, w, f, logits, boxes, t_bbox, t_class, bg)
    whole = rig.run()
    added = torch.zeros(Lv * 10, device=DEV)
    for b in range(B):
        half = Rig(hip, w, f, np.ascontiguousarray(logits[:, b:b + 1]), np.ascontiguousarray(boxes[:, b:b + 1]), t_bbox[b:b + 1],
                   t_class[b:b + 1], bg).run(grad=False)
        assert np.array_equal(half.tfp, whole.tfp[b::B])               # a problem is matched alone as it is inside the batch
        added += half.sums_dev
    sw, sa = whole.sums[:Lv * 8].view(Lv, 8), added.cpu()[:Lv * 8].view(Lv, 8)
    assert torch.equal(sw[:, 1:7], sa[:, 1:7])                         # the counts, exactly
    out, tot = rig.finalize(added)
    dl, dbx = rig.grad(whole.tfp_dev, added)
    torch.cuda.synchronize()
    r = SimpleNamespace(out=out.cpu(), total=float(tot), d_logits=dl.cpu(), d_boxes=dbx.cpu())
    match = _device_match(whole, t_bbox, t_class, Lv, B, Q, n_list)
    lg64, bx64, total, losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w, f, match=match)
    total.backward()
    _check_values(r, losses, total, Lv, what="added ")
    _check_grads(r, lg64, bx64, ("F2", name.rsplit("-", 1)[0]), what="added ")
    assert torch.equal(r.d_logits, whole.d_logits) and torch.equal(r.d_boxes, whole.d_boxes)     # the gradients read slot 4 only


def test_a_nan_logit_stays_in_its_level(hip):
    case = next(c for c in CR.CONTIGUOUS if c[3] == 17)               # Lv 3, B 2, Q 17, C 65, bg 0
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    w, f = FR.param_set("F0")
    logits, boxes, t_bbox, t_class, _ = FR.inputs(case)
    clean = Rig(hip, w, f, logits, boxes, t_bbox, t_class, bg).run()
    lv, b, q = 1, 0, Q - 1
    used = set(t_class[b, 1:1 + n_list[b], 0].tolist()) | {bg, int(np.argmax(logits[lv, b, q]))}
    c = next(c for c in range(C) if c not in used)                    # a column the matcher's cost never reads, not the row's arg-max
    bad = logits.copy()
    bad[lv, b, q, c] = np.nan
    r = Rig(hip, w, f, bad, boxes, t_bbox, t_class, bg).run()
    assert (r.status == 0).all() and torch.equal(r.cost, clean.cost) and np.array_equal(r.tfp, clean.tfp)
    assert math.isnan(float(r.out[lv, 0])) and math.isnan(r.total)
    for k in range(Lv):
        for j in range(6):
            if (k, j) != (lv, 0):
                got, want = float(r.out[k, j]), float(clean.out[k, j])
                assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (k, j, got, want)
    assert torch.equal(r.sums[:Lv * 8].view(Lv, 8)[:, 1:7], clean.sums[:Lv * 8].view(Lv, 8)[:, 1:7])
    nan = torch.isnan(r.d_logits)
    assert int(nan.sum()) == 1 and bool(nan[lv, b, q, c])
    assert torch.equal(r.d_logits[~nan], clean.d_logits[~nan]) and torch.equal(r.d_boxes, clean.d_boxes)


@pytest.mark.parametrize("label", [-1, 65, 2 ** 31 + 7])
def test_an_invalid_matched_label(hip, label):
    """The level's label_cost and the total are NaN, the row's gradient is that of a row without a positive class, the class cost of
    that target is 0, and nothing is read out of bounds (the logits sit in a buffer filled with 1e30 outside the view)."""
    case = next(c for c in SC.LOSS_CASES if c[-1] == "strided" and c[4] == 65)
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    w, f = FR.param_set("F0")
    logits, boxes, t_bbox, t_class, _ = FR.inputs(case)
    t_class = t_class.copy()
    t_class[1, 2, 0] = label                                          # target 1 of image 1
    r = Rig(hip, w, f, logits, boxes, t_bbox, t_class, bg, layout).run(grad=False)
    _check_cost(r, logits, boxes, t_bbox, t_class, n_list, w, f, None)
    match = _device_match(r, t_bbox, t_class, Lv, B, Q, n_list)
    _, _, total, losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w, f, match=match)
    assert math.isnan(float(total)) and all(math.isnan(float(losses["label_cost" + ("" if lv == Lv - 1 else f"_{lv}")])) for lv in range(Lv))
    _check_values(r, losses, total, Lv)
    _check_counts(r, match, Lv, B, Q)
    # the gradients, on contiguous heads
    rc = Rig(hip, w, f, logits, boxes, t_bbox, t_class, bg).run()
    assert np.array_equal(rc.tfp, r.tfp)
    lg64, bx64, total, _, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w, f, match=match, nan_invalid=False)
    total.backward()
    assert bool(torch.isfinite(rc.d_logits).all())
    _check_grads(rc, lg64, bx64, None)


# ------------------------------------------------------------------------------------------
# 4. get_losses and the graphed training step across a switch of the class criterion
# ------------------------------------------------------------------------------------------
API_CASE = CR.API_CASE
ONE_WG_CASE = ("api-one-workgroup", 2, 1, 7, 5, 0, 6, [4], "contiguous")     # B = 1, Q <= SL_QCHUNK: one workgroup adds into a level's sums


def _get_losses(config, case):
    from detr_tf.loss.loss import SetLoss, get_losses
    logits, boxes, t_bbox, t_class, _ = SC.loss_inputs(case)
    Lv, B, Q, C, bg, R = case[1:7]
    lgd, bxd = g(torch.from_numpy(logits)), g(torch.from_numpy(boxes))
    m_out = {"pred_logits": lgd[Lv - 1], "pred_boxes": bxd[Lv - 1],
             "aux": [{"pred_logits": lgd[i], "pred_boxes": bxd[i]} for i in range(Lv - 1)]}
    total, log = get_losses(m_out, t_bbox, t_class, config)
    sl = SetLoss.get(Lv, B, Q, C, R, torch.device(DEV, torch.cuda.current_device()))
    dl, dbx = sl.grad(LOSS_SCALE)
    res = SimpleNamespace(total=float(total), log={k: float(v) for k, v in log.items()}, d_logits=dl.cpu().clone(), d_boxes=dbx.cpu().clone(),
                          tfp=sl.matcher.tgt_for_pred.cpu().clone(), criterion=sl.criterion,
                          bits=(total.cpu().numpy().tobytes(), tuple(v.cpu().numpy().tobytes() for v in log.values())))
    return res, (logits, boxes, t_bbox, t_class)


def _check_api(res, ref_total, ref_losses):
    assert list(res.log) == list(ref_losses) and len(res.log) == 6 * API_CASE[1]
    for nm, ref in ref_losses.items():
        got, ref = res.log[nm], float(ref)
        print(f"{nm}: got {got!r}, reference {ref!r}")
        assert (math.isnan(got) and math.isnan(ref)) or abs(got - ref) <= 2e-5 * max(1.0, abs(ref)), (nm, got, ref)
    print(f"total: got {res.total!r}, reference {float(ref_total)!r}")
    assert abs(res.total - float(ref_total)) <= 1e-5 * abs(float(ref_total))


@pytest.mark.parametrize("case", [API_CASE, ONE_WG_CASE], ids=lambda c: c[0])
def test_get_losses_follows_a_switch_of_the_class_criterion(hip, case):
    """One config object: softmax (the defaults), focal, softmax again.  Each step equals its reference; the focal step runs the focal
    entry points (its total is far from the softmax one); the softmax steps before and after give the same matching and bit-identical
    gradients, and -- where one workgroup adds into a level's sums, so that no order of float atomics is left open -- bit-identical
    totals and logged values."""
    Lv, B, Q, C, bg, R = case[1:7]
    w, f = FR.param_set("F2")
    cfg = SimpleNamespace(background_class=bg)
    steps = []
    for kind in ("softmax", "focal", "softmax"):
        asked = FR.config_of(w, f) if kind == "focal" else CR.config_of(CR.DEFAULTS, class_criterion="softmax")
        for k, v in vars(asked).items():
            setattr(cfg, k, v)
        res, (logits, boxes, t_bbox, t_class) = _get_losses(cfg, case)
        assert res.criterion.is_focal == (kind == "focal") and res.criterion.is_default == (kind == "softmax")
        if case is API_CASE:
            if kind == "focal":
                _, _, ref_total, ref_losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w, f)
            else:
                lg, bx = torch.from_numpy(logits).double(), torch.from_numpy(boxes).double()
                ref_total, ref_losses, _ = SC.oracle_losses(lg, bx, torch.from_numpy(t_bbox).double(), torch.from_numpy(t_class), bg)
            _check_api(res, ref_total, ref_losses)
        steps.append(res)
    before, focal, after = steps
    assert abs(focal.total - before.total) > 1e-2 * abs(before.total)
    assert torch.equal(before.tfp, after.tfp) and torch.equal(before.d_logits, after.d_logits) and torch.equal(before.d_boxes, after.d_boxes)
    assert not torch.equal(before.d_logits, focal.d_logits)
    if case is ONE_WG_CASE:
        assert before.bits == after.bits


def test_graphed_step_follows_a_switch_of_the_class_criterion(hip):
    """training.train_step against GraphedTrainStep(launch="graph") on the model, data and bounds of
    test_gpu_criterion.py::test_graphed_step_follows_a_criterion_change (96 x 128 images, B = 2, one encoder and two decoder layers;
    logits 1e-5 of their scale, loss 1e-5, update 2e-2 in relative L2).  At step 3 class_criterion becomes "focal" on both configs:
    the recorded step is dropped (one eager step, a new recording) and every later graphed step equals the eager one."""
    from detr_tf import training
    from oracle import detr_ref as R
    from test_gpu_adamw import _build, _cfg
    from test_gpu_training import _batches
    weights = R.make_params(5, num_enc=1, num_dec=2)
    data = _batches(6, seed=3)
    cfg_e, cfg_g = _cfg(), _cfg()
    (m_e, o_e), (m_g, o_g) = _build(weights, cfg_e), _build(weights, cfg_g)
    stepper = training.GraphedTrainStep(m_g, o_g, cfg_g, eager_steps=1, launch="graph")
    recorded, totals = [], []
    for i, (im, tb, tc) in enumerate(data):
        if i == 3:
            recorded.append(stepper.step_graph)
            assert recorded[0] is not None
            for c in (cfg_e, cfg_g):
                c.class_criterion, c.set_cost_class = "focal", 2.0
        for src, dst in ((m_e.engine.P.flat, m_g.engine.P.flat), (m_e.engine.P.adam_m, m_g.engine.P.adam_m),
                         (m_e.engine.P.adam_v, m_g.engine.P.adam_v)):
            dst.copy_(src)
        m_g.engine.bump_weights_version()
        before = m_e.engine.P.flat.clone()
        out_e, tot_e, log_e = training.train_step(m_e, im, tb, tc, o_e, cfg_e, i)
        lg_e = out_e["pred_logits"].clone()
        out_g, tot_g, log_g = stepper(im, tb, tc, i)
        lg_g = out_g["pred_logits"].clone()
        assert float((lg_e - lg_g).abs().max()) <= 1e-5 * float(lg_e.abs().max()), (i, float((lg_e - lg_g).abs().max()))
        print(f"step {i}: total eager {float(tot_e)!r} graph {float(tot_g)!r}")
        assert abs(float(tot_e) - float(tot_g)) <= 1e-5 * abs(float(tot_e)), (i, float(tot_e), float(tot_g))
        de, dg = m_e.engine.P.flat - before, m_g.engine.P.flat - before
        rel = float((de - dg).norm()) / float(de.norm())
        assert rel <= 2e-2, (i, rel)
        totals.append(float(tot_g))
    # a replay that kept the softmax launches would report a softmax total: the two differ by far more than the bound
    assert abs(totals[3] - totals[2]) > 1e-2 * abs(totals[2])
    assert stepper.step_graph is not None and stepper.step_graph is not recorded[0] and stepper.calls == 3
    del stepper, m_e, m_g, o_e, o_g
    gc.collect()


# ------------------------------------------------------------------------------------------
# 5. sigmoid scoring
# ------------------------------------------------------------------------------------------
SCORE_GRID = np.arange(0.04, 0.96, 0.002)            # target scores 2e-3 apart: the float32 order is the float64 order
SCORE_BOUND = 1e-6                                   # tests/test_gpu_detect.py's bound on its softmax score
THRESHOLD = 0.3011                                   # between two grid values


def scoring_case(Q, C, bg):
    """logits [3, Q, C] float32 whose best non-background logit is logit(a distinct grid score) per query of an image; image 1 has a
    row with tied best logits (and, from Q = 5 on, two identical rows: an exact score tie), image 2 a row with a NaN; the background
    logit is anything, the largest of its row included.  boxes [3, Q, 4], sizes [3, 2]."""
    rng = np.random.default_rng(1000 * Q + 10 * C + bg)
    B = 3
    fg = [c for c in range(C) if c != bg]
    logits = np.empty((B, Q, C), np.float32)
    for b in range(B):
        target = rng.choice(SCORE_GRID, Q, replace=False)
        best = np.log(target / (1 - target))
        for q in range(Q):
            row = best[q] - rng.uniform(0.5, 6.0, C)
            row[fg[int(rng.integers(len(fg)))]] = best[q]
            row[bg] = rng.normal() * 6
            logits[b, q] = row
    if len(fg) >= 3:                                  # tied best logits inside a row: the first wins
        q = Q // 2
        logits[1, q, fg[-1]] = logits[1, q, fg[1]] = logits[1, q].astype(np.float32)[fg].max()
    if Q >= 5:
        logits[1, 3] = logits[1, 1]                   # two identical rows: equal scores, the lower query first
    logits[2, Q - 1, fg[0]] = np.nan
    boxes = np.empty((B, Q, 4), np.float32)
    boxes[..., :2] = rng.uniform(0.2, 0.8, (B, Q, 2))
    boxes[..., 2:] = rng.uniform(0.05, 0.3, (B, Q, 2))
    sizes = np.array([(96, 128), (120, 80), (64, 64)], np.int32)
    return logits, boxes, sizes


def _scored(hip, logits, boxes, sizes, bg, scoring, thr=THRESHOLD, old=False):
    """(postprocess rows, detect rows) through the _scored entry points (old: through detr_hip_postprocess / detr_hip_detect)."""
    from detr_tf.inference import _detect, _post
    lg, bx = g(torch.from_numpy(logits)), g(torch.from_numpy(boxes))
    if old:
        assert scoring == "softmax"
        B, Q, _ = logits.shape
        d = hip.PostprocessDesc()
        from detr_tf.inference import _fill_model_outputs
        outs = (torch.zeros(B, Q, 4, device=DEV), torch.zeros(B, Q, dtype=torch.int64, device=DEV), torch.zeros(B, Q, device=DEV),
                torch.zeros(B, dtype=torch.int32, device=DEV))
        _fill_model_outputs(d, lg, bx, bg)
        d.B, d.bbox_format = B, 0
        d.out_boxes, d.out_labels, d.out_scores, d.counts = (t.data_ptr() for t in outs)
        hip.call("detr_hip_postprocess_scored", ctypes.byref(d), 0)
        post = outs
        det = _detect(lg, bx, sizes, bg, thr, None, "xyxy", True)
        dd = hip.DetectDesc()
        _fill_model_outputs(dd, lg, bx, bg)
        sz = g(torch.from_numpy(sizes))
        douts = (torch.zeros(B, Q, 4, device=DEV), torch.zeros(B, Q, dtype=torch.int64, device=DEV), torch.zeros(B, Q, device=DEV),
                 torch.zeros(B, Q, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV))
        dd.B, dd.sizes, dd.score_threshold, dd.max_detections, dd.bbox_format, dd.clip = B, sz.data_ptr(), thr, Q, 1, 1
        dd.out_boxes, dd.out_labels, dd.out_scores, dd.out_query, dd.counts = (t.data_ptr() for t in douts)
        hip.call("detr_hip_detect_scored", ctypes.byref(dd), 0)
        torch.cuda.synchronize()
        return [t.cpu() for t in post], [t.cpu() for t in douts], [t.cpu() for t in _post(lg, bx, bg, "xy_center")], [t.cpu() for t in det]
    post = _post(lg, bx, bg, "xy_center", scoring)
    det = _detect(lg, bx, sizes, bg, thr, None, "xyxy", True, scoring)
    torch.cuda.synchronize()
    return [t.cpu() for t in post], [t.cpu() for t in det]


@pytest.mark.parametrize("Q", [1, 5, 100])
@pytest.mark.parametrize("C,bg", [(2, 0), (2, 1), (65, 0), (65, 64), (130, 0), (130, 129)])
def test_sigmoid_scoring(hip, Q, C, bg):
    logits, boxes, sizes = scoring_case(Q, C, bg)
    score, label = FR.scores_labels(logits, bg)
    assert math.isnan(score[2, Q - 1]) and int(np.isnan(score).sum()) == 1
    (p_boxes, p_labels, p_scores, p_counts), (d_boxes, d_labels, d_scores, d_query, d_counts) = _scored(hip, logits, boxes, sizes, bg, "sigmoid")
    # postprocess: every query, in order
    assert p_counts.tolist() == [Q] * 3
    assert np.array_equal(p_labels.numpy(), label) and bool((p_labels != bg).all())
    ps = p_scores.numpy()
    assert np.array_equal(np.isnan(ps), np.isnan(score))
    err = np.nanmax(np.abs(ps - score))
    print(f"Q{Q} C{C} bg{bg}: max score err {err:.3e}, bound {SCORE_BOUND:.0e}")
    assert err < SCORE_BOUND
    assert torch.equal(p_boxes, torch.from_numpy(boxes))                     # xy_center: the boxes as they are
    # detect: threshold, then a stable descending order; scores are the bits of postprocess
    for b in range(3):
        keep = np.nonzero(score[b] >= THRESHOLD)[0]                          # NaN fails the comparison
        assert (np.abs(score[b][~np.isnan(score[b])] - THRESHOLD) > 1e-4).all()
        order = keep[np.argsort(-score[b, keep], kind="stable")]
        k = int(d_counts[b])
        assert k == len(order) and d_query[b, :k].tolist() == order.tolist(), (b, d_query[b, :k].tolist(), order.tolist())
        assert d_labels[b, :k].tolist() == label[b, order].tolist()
        assert d_scores[b, :k].numpy().tobytes() == p_scores[b, order].numpy().tobytes()
        assert bool((d_scores[b, k:] == 0).all()) and bool((d_boxes[b, k:] == 0).all())
    if Q >= 5:                                                               # the exact tie of image 1: lower query first
        assert score[1, 1] == score[1, 3]
        if score[1, 1] >= THRESHOLD:
            qs = d_query[1, :int(d_counts[1])].tolist()
            assert qs.index(1) + 1 == qs.index(3)


@pytest.mark.parametrize("Q,C,bg", [(5, 65, 0), (100, 130, 129)])
def test_scoring_zero_is_the_old_entry_points(hip, Q, C, bg):
    logits, boxes, sizes = scoring_case(Q, C, bg)
    logits = np.nan_to_num(logits, nan=0.25)
    new_post, new_det, old_post, old_det = _scored(hip, logits, boxes, sizes, bg, "softmax", thr=0.05, old=True)
    for a, b in zip(new_post + new_det, old_post + old_det):
        assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()
    assert 0 < int(old_post[3].sum()) < 3 * Q and int(old_det[4].sum()) > 0


def test_scoring_refuses_a_single_class(hip):
    from detr_tf.inference import detect_batched, get_model_inference_batched
    out = {"pred_logits": torch.zeros(1, 4, 1, device=DEV), "pred_boxes": torch.full((1, 4, 4), 0.5, device=DEV)}
    with pytest.raises(RuntimeError, match="C=1"):
        get_model_inference_batched(out, 0, scoring="sigmoid")
    with pytest.raises(RuntimeError, match="C=1"):
        detect_batched(out, [(8, 8)], 0, scoring="sigmoid")
    assert len(get_model_inference_batched(out, 0)) == 1                      # softmax scoring takes it as before
    with pytest.raises(ValueError, match="scoring"):
        get_model_inference_batched(out, 0, scoring="logistic")


def _config():
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.image_size = (64, 96)
    return cfg


@pytest.fixture(scope="module")
def model(hip):
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref as R
    m = get_detr_model(_config(), include_top=True, num_encoder_layers=1, num_decoder_layers=1, dropout=0.0)
    assert not m.load_weights(R.make_params(2, num_enc=1, num_dec=1))
    return m


def test_detector_with_sigmoid_scoring(hip, model):
    from detr_tf.data import transformation as T
    from detr_tf.data.processing import DeviceInputStage
    from detr_tf.inference import Detector, detect_batched, fuse_views, merge_tiles
    cfg = _config()
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((96, 128), (120, 80))]
    canvas = (96, 96)
    assert Detector(model, cfg).scoring == "softmax"
    cfg.class_criterion = "focal"
    det = Detector(model, cfg, score_threshold=0.0, max_detections=20, shortest_side=64, max_size=96, canvas=canvas)
    assert det.scoring == "sigmoid"                                           # scoring=None: from config.class_criterion
    assert Detector(model, cfg, scoring="softmax").scoring == "softmax"
    got = det(imgs)
    recs = [T.eval_record(96, 128, 64, 96, T.CUBIC), T.eval_record(120, 80, 64, 96, T.CUBIC)]
    x, m = DeviceInputStage(cfg).augmented_padded(imgs, recs, canvas=canvas)
    out = model((x, m), training=False)
    hand = detect_batched(out, [(96, 128), (120, 80)], 91, score_threshold=0.0, max_detections=20, scoring="sigmoid")
    score, label = FR.scores_labels(out["pred_logits"].cpu().numpy(), 91)
    for d, h, b in zip(got, hand, range(2)):
        assert d.scores.shape[0] == 20                                        # every query is a candidate: the cut decides
        for s, t in zip(d, h):
            assert s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()
        q = d.query.cpu().numpy()
        assert d.labels.tolist() == label[b, q].tolist() and np.abs(d.scores.cpu().numpy() - score[b, q]).max() < SCORE_BOUND
        assert (np.diff(d.scores.cpu().numpy()) <= 0).all() and bool((d.labels != 91).all())
    softmax = Detector(model, cfg, scoring="softmax", score_threshold=0.0, max_detections=20, shortest_side=64, max_size=96, canvas=canvas)(imgs)
    assert any(a.scores.shape != b.scores.shape or not torch.equal(a.scores, b.scores) for a, b in zip(got, softmax))
    # the tiled / fused paths score from the logits themselves
    for extra in (dict(tiles=(1, 2)), dict(nms_threshold=0.5), dict(flip=True), dict(scales=(64, 80)), dict(merge="wbf")):
        with pytest.raises(NotImplementedError, match="scoring"):
            Detector(model, cfg, **extra)
        Detector(model, cfg, scoring="softmax", **extra)
    with pytest.raises(NotImplementedError, match="scoring"):
        merge_tiles(out, np.arange(3, dtype=np.int32), np.zeros((2, 4), np.int32), [(96, 128), (120, 80)], 91, scoring="sigmoid")
    with pytest.raises(NotImplementedError, match="scoring"):
        fuse_views(out, np.arange(3, dtype=np.int32), np.zeros((2, 4), np.int32), np.zeros(2, np.int32), [(96, 128), (120, 80)], 91, scoring="sigmoid")


def test_set_class_prior(hip, model):
    from detr_tf.inference import get_model_inference_batched
    eng = model.engine
    name = eng._head_layers()[0][0]
    saved = eng.P.views[f"{name}/bias"].clone()
    version = eng._weights_version
    try:
        value = model.set_class_prior(0.01)
        assert abs(value + math.log(99.0)) < 1e-12 and eng._weights_version > version     # derived copies and recorded graphs follow
        bias = eng.P.views[f"{name}/bias"]
        assert bool((bias == np.float32(value)).all())
        # a zero input to the head gives the bias as logits: every sigmoid score is the prior
        C = bias.numel()
        logits = (torch.zeros(2, 7, 256, device=DEV) @ torch.zeros(256, C, device=DEV) + bias).contiguous()
        out = {"pred_logits": logits, "pred_boxes": torch.full((2, 7, 4), 0.5, device=DEV)}
        for boxes, labels, scores in get_model_inference_batched(out, 91, scoring="sigmoid"):
            assert scores.shape == (7,) and float((scores - 0.01).abs().max()) < SCORE_BOUND and bool((labels == 0).all())
        with pytest.raises(ValueError, match="prior"):
            model.set_class_prior(1.0)
    finally:
        eng.load_params({f"{name}/bias": saved.cpu().numpy()})
