"""GPU tests of the configurable set criterion (the _crit_ entry points of csrc/setloss.hip and the host path above them) against
tests/criterion_ref.py: every (weight set, case) of that module, the defaults through both sets of entry points, run-to-run
determinism and the exact class-weight normaliser, the data-parallel additivity of the sums, empty batches, get_losses, and the
re-recording of the graphed training step.  The bounds are those of tests/test_gpu_setloss_edges.py;
tests/test_criterion_cpu.py proves the inputs admissible without a GPU."""
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
import setloss_cases as SC                 # noqa: E402
from test_gpu_setloss_edges import SENTINEL, _check_values, _device_view, close, g       # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOSS_SCALE = 0.5


class Rig:
    """The device tensors of one problem set and the launches on them, one method per entry point.  w = None: the entry points
    with the reference's criterion compiled in; else the _crit_ ones with the weights of `w`."""

    def __init__(self, hip, w, logits, boxes, t_bbox, t_class, bg, layout="contiguous"):
        from detr_tf.loss.hungarian_matching import make_desc
        self.hip, self.w = hip, w
        self.Lv, self.B, self.Q, self.C = logits.shape
        self.R = t_bbox.shape[1]
        self.P = self.Lv * self.B
        self.lgd = _device_view(logits, layout, SC.C_SLACK)
        self.bxd = _device_view(boxes, layout, SC.BOX_SLACK)
        self.tbd, self.tcd = g(torch.from_numpy(t_bbox)), g(torch.from_numpy(t_class).reshape(self.B, self.R))
        self.d = make_desc(self.lgd, self.bxd, self.tbd, self.tcd, bg)
        self.block = None if w is None else CR.host_block(w)
        self.cw = None
        if w is not None and w.class_weights is not None:
            assert len(w.class_weights) == self.C
            self.cw = torch.tensor(w.class_weights, dtype=torch.float32, device=DEV)
        self.cwp = None if self.cw is None else self.cw.data_ptr()

    def cost(self):
        cost = torch.full((self.P, self.Q, self.R - 1), float(SENTINEL), device=DEV)
        if self.w is None:
            self.hip.call("detr_hip_match_cost_f32", ctypes.byref(self.d), cost.data_ptr())
        else:
            self.hip.call("detr_hip_match_cost_crit_f32", ctypes.byref(self.d), self.block, cost.data_ptr())
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
        if self.w is None:
            self.hip.call("detr_hip_set_loss_sums_f32", ctypes.byref(self.d), tfp.data_ptr(), sums.data_ptr())
        else:
            self.hip.call("detr_hip_set_loss_sums_crit_f32", ctypes.byref(self.d), self.block, self.cwp, tfp.data_ptr(), sums.data_ptr())
        return sums

    def finalize(self, sums):
        out = torch.zeros(self.Lv, 6, device=DEV)
        tot = torch.zeros(1, device=DEV)
        if self.w is None:
            self.hip.call("detr_hip_set_loss_finalize_f32", sums.data_ptr(), self.Lv, out.data_ptr(), tot.data_ptr())
        else:
            self.hip.call("detr_hip_set_loss_finalize_crit_f32", sums.data_ptr(), self.Lv, self.block, out.data_ptr(), tot.data_ptr())
        return out, tot

    def grad(self, tfp, sums):
        dl = torch.full_like(self.lgd, float(SENTINEL))
        dbx = torch.full_like(self.bxd, float(SENTINEL))
        if self.w is None:
            self.hip.call("detr_hip_set_loss_grad_f32", ctypes.byref(self.d), tfp.data_ptr(), sums.data_ptr(), ctypes.c_float(LOSS_SCALE),
                          dl.data_ptr(), dbx.data_ptr())
        else:
            self.hip.call("detr_hip_set_loss_grad_crit_f32", ctypes.byref(self.d), self.block, self.cwp, tfp.data_ptr(), sums.data_ptr(),
                          ctypes.c_float(LOSS_SCALE), dl.data_ptr(), dbx.data_ptr())
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


def _reference64(logits, boxes, t_bbox, t_class, bg, w, match=None):
    lg = torch.from_numpy(logits).double().requires_grad_(True)
    bx = torch.from_numpy(boxes).double().requires_grad_(True)
    total, losses, match = CR.criterion_losses(lg, bx, torch.from_numpy(t_bbox).double(), torch.from_numpy(t_class), bg, w, match=match)
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


def _check_cost(r, logits, boxes, t_bbox, t_class, n_list, w):
    """Against the float32 reference (the same arithmetic): 2e-6 absolute at weights up to 1, scaled by the largest cost weight above
    that (the error is linear in the weights); columns >= n untouched."""
    from oracle import set_loss_ref as L
    Lv, B = logits.shape[:2]
    bound = 2e-6 * max(1.0, w.cost_class, w.cost_bbox, w.cost_giou)
    worst = 0.0
    for lv in range(Lv):
        for b in range(B):
            n = n_list[b]
            tbs, tcs = L.strip_header(torch.from_numpy(t_bbox[b]), torch.from_numpy(t_class[b]))
            ref = CR.cost_matrix(tbs, tcs, torch.from_numpy(boxes[lv, b]), torch.from_numpy(logits[lv, b]), w)
            got = r.cost[lv * B + b]
            assert bool((got[:, n:] == SENTINEL).all()), f"cost lv{lv} b{b}: written past n = {n}"
            err = float((got[:, :n] - ref).abs().max()) if n else 0.0
            worst = max(worst, err)
            assert err <= bound, f"cost lv{lv} b{b}: max abs err {err:.3e} > {bound:.1e}"
    print(f"cost: max abs err {worst:.3e}, bound {bound:.1e}")


def _check_grads(r, lg64, bx64, key, what=""):
    close(r.d_logits, LOSS_SCALE * lg64.grad, rtol=2e-5, what=what + "d_logits", atol=CR.D_LOGITS_ATOL.get(key))
    close(r.d_boxes, LOSS_SCALE * bx64.grad, rtol=5e-5, what=what + "d_boxes")


# ------------------------------------------------------------------------------------------
# 1. every (weight set, case) against the reference
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws,case", CR.PAIRS, ids=CR.PAIR_IDS)
def test_criterion_case_vs_reference(hip, ws, case):
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    w = CR.weight_set(ws, C)
    logits, boxes, t_bbox, t_class, _ = CR.inputs(ws, case)
    contiguous = layout == "contiguous"
    r = Rig(hip, w, logits, boxes, t_bbox, t_class, bg, layout).run(grad=contiguous)        # the gradient tensors follow contiguous heads
    _check_cost(r, logits, boxes, t_bbox, t_class, n_list, w)
    match = _device_match(r, t_bbox, t_class, Lv, B, Q, n_list)
    lg64, bx64, total, losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w, match=match)
    _check_values(r, losses, total, Lv, what=f"{ws} ")
    for lv in range(Lv):                                            # the normaliser's slots: counts, and the class weights of the matched
        tc_m = match[lv][1][match[lv][2]]
        want = sum(round(w.class_weights[int(c)] * 64) for c in tc_m) if w.class_weights is not None else tc_m.numel()
        assert float(r.sums[lv * 8 + 1]) * (64 if w.class_weights is not None else 1) == want
        assert float(r.sums[lv * 8 + 4]) == tc_m.numel() and float(r.sums[lv * 8 + 3]) == B * Q - tc_m.numel()
    if contiguous:
        total.backward()
        _check_grads(r, lg64, bx64, (ws, name.rsplit("-", 1)[0]))
        for b, n in enumerate(n_list):
            if n == 0:
                assert all(bool((r.d_boxes[lv, b] == 0).all()) for lv in range(Lv))


# ------------------------------------------------------------------------------------------
# 2. the defaults through the run-time entry points against the compiled-in ones
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CR.CONTIGUOUS, ids=[c[0] for c in CR.CONTIGUOUS])
def test_defaults_through_both_sets_of_entry_points(hip, case):
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    logits, boxes, t_bbox, t_class, _ = CR.inputs("A", case)
    fixed = Rig(hip, None, logits, boxes, t_bbox, t_class, bg).run()
    crit = Rig(hip, CR.DEFAULTS, logits, boxes, t_bbox, t_class, bg).run()
    assert torch.equal(fixed.cost, crit.cost) and np.array_equal(fixed.tfp, crit.tfp) and np.array_equal(fixed.pft, crit.pft)
    assert torch.equal(fixed.d_logits, crit.d_logits) and torch.equal(fixed.d_boxes, crit.d_boxes)
    assert bool((fixed.sums.view(-1)[:Lv * 8].view(Lv, 8)[:, 1] == 0).all())                # slot 1 stays unused there
    assert torch.equal(crit.sums.view(-1)[:Lv * 8].view(Lv, 8)[:, 1], crit.sums.view(-1)[:Lv * 8].view(Lv, 8)[:, 4])
    # the reported values carry the atomics' last-bit noise: each within the bounds against the same reference
    match = _device_match(crit, t_bbox, t_class, Lv, B, Q, n_list)
    _, _, total, losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, CR.DEFAULTS, match=match)
    _check_values(fixed, losses, total, Lv, what="fixed ")
    _check_values(crit, losses, total, Lv, what="crit ")


# ------------------------------------------------------------------------------------------
# 3. run-to-run determinism and the exact normaliser under class weights
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CR.CONTIGUOUS if c[3] in (17, 100)], ids=lambda c: c[0])
def test_class_weighted_run_is_deterministic(hip, case):
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    w = CR.weight_set("C", C)
    logits, boxes, t_bbox, t_class, _ = CR.inputs("C", case)
    rig = Rig(hip, w, logits, boxes, t_bbox, t_class, bg)
    a, b = rig.run(), rig.run()
    assert torch.equal(a.d_logits, b.d_logits) and torch.equal(a.d_boxes, b.d_boxes)
    sa, sb = a.sums[:Lv * 8].view(Lv, 8), b.sums[:Lv * 8].view(Lv, 8)
    assert torch.equal(sa[:, [1, 3, 4]], sb[:, [1, 3, 4]])
    for lv in range(Lv):
        quanta = 0
        for bi in range(B):
            for q in range(Q):
                t = int(a.tfp[lv * B + bi, q])
                if t >= 0:
                    quanta += round(w.class_weights[int(t_class[bi, 1 + t, 0])] * 64)
        assert float(sa[lv, 1]) * 64 == quanta and quanta > 0, (lv, float(sa[lv, 1]), quanta)


# ------------------------------------------------------------------------------------------
# 4. no class term in the cost, no GIoU term in the loss
# ------------------------------------------------------------------------------------------
def test_zero_weights_switch_their_terms_off(hip):
    case = next(c for c in CR.CONTIGUOUS if c[3] == 17)
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    w = CR.weight_set("Z", C)
    logits, boxes, t_bbox, t_class, _ = CR.inputs("Z", case)
    r = Rig(hip, w, logits, boxes, t_bbox, t_class, bg).run()
    other = (logits + np.random.default_rng(4).normal(size=logits.shape)).astype(np.float32)
    r2 = Rig(hip, w, other, boxes, t_bbox, t_class, bg).run(grad=False)
    assert torch.equal(r.cost, r2.cost) and np.array_equal(r.tfp, r2.tfp)          # the cost does not see the logits
    # d_boxes is the L1 part alone: bbox_loss_coef * loss_scale / npos * sign(p - t) on the matched queries, 0 elsewhere
    want = torch.zeros(Lv, B, Q, 4, dtype=torch.float64)
    for lv in range(Lv):
        npos = float((r.tfp[lv * B:(lv + 1) * B] >= 0).sum())
        for b in range(B):
            for q in range(Q):
                t = int(r.tfp[lv * B + b, q])
                if t >= 0:
                    want[lv, b, q] = torch.from_numpy(np.sign(boxes[lv, b, q].astype(np.float64) - t_bbox[b, 1 + t])) * (w.bbox_coef * LOSS_SCALE / npos)
    close(r.d_boxes, want, rtol=5e-5, what="d_boxes (L1 part)")
    assert float((r.d_boxes.double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())      # one rounding of the factor


# ------------------------------------------------------------------------------------------
# 5. a batch without any target
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_one", [False, True])
def test_all_images_empty(hip, min_one):
    Lv, B, Q, C, bg, R = 2, 2, 9, 5, 4, 6
    rng = np.random.default_rng(11)
    logits = (rng.normal(size=(Lv, B, Q, C)) * 2).astype(np.float32)
    boxes = rng.uniform(0.1, 0.6, (Lv, B, Q, 4)).astype(np.float32)
    t_bbox, t_class = SC.make_targets([0, 0], R, C, bg, rng)
    w = CR.weight_set("B", C)._replace(min_one=min_one)
    lg64, bx64, total, losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w)
    r = Rig(hip, w, logits, boxes, t_bbox, t_class, bg).run()
    assert (r.status == 0).all() and (r.tfp == -1).all() and bool((r.cost == SENTINEL).all())
    _check_values(r, losses, total, Lv)
    label_sum = sum(losses["label_cost" + ("" if lv == Lv - 1 else f"_{lv}")] for lv in range(Lv))
    for nm in ("true_pos", "pos_accuracy"):                          # 0 / 0 either way
        assert math.isnan(float(r.out[Lv - 1, SC.LOSS_NAMES.index(nm)]))
    if min_one:
        assert math.isfinite(r.total) and abs(r.total - w.class_coef * float(label_sum)) <= 1e-5 * abs(w.class_coef * float(label_sum))
        assert float(r.out[0, 4]) == 0.0 and float(r.out[0, 5]) == 0.0
        total.backward()
    else:
        assert math.isnan(r.total) and math.isnan(float(total))
        (w.class_coef * label_sum).backward()
    assert bool((r.d_boxes == 0).all()) and bool(torch.isfinite(r.d_logits).all())
    close(r.d_logits, LOSS_SCALE * lg64.grad, rtol=2e-5, what="d_logits")


# ------------------------------------------------------------------------------------------
# 6. the sums of two half batches add up to the whole batch's (the data-parallel normaliser)
# ------------------------------------------------------------------------------------------
def test_sums_of_half_batches_add_up(hip):
    case = next(c for c in CR.CONTIGUOUS if c[3] == 17)
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    assert B == 2
    w = CR.weight_set("C", C)
    logits, boxes, t_bbox, t_class, _ = CR.inputs("C", case)
    rig = Rig(hip, w, logits, boxes, t_bbox, t_class, bg)
    whole = rig.run()
    added = torch.zeros(Lv * 10, device=DEV)
    for b in range(B):
        half = Rig(hip, w, np.ascontiguousarray(logits[:, b:b + 1]), np.ascontiguousarray(boxes[:, b:b + 1]), t_bbox[b:b + 1],
                   t_class[b:b + 1], bg).run(grad=False)
        assert np.array_equal(half.tfp, whole.tfp[b::B])               # a problem is matched alone as it is inside the batch
        added += half.sums_dev
    sw, sa = whole.sums[:Lv * 8].view(Lv, 8), added.cpu()[:Lv * 8].view(Lv, 8)
    assert torch.equal(sw[:, [1, 3, 4]], sa[:, [1, 3, 4]])
    out, tot = rig.finalize(added)
    dl, dbx = rig.grad(whole.tfp_dev, added)
    torch.cuda.synchronize()
    r = SimpleNamespace(out=out.cpu(), total=float(tot), d_logits=dl.cpu(), d_boxes=dbx.cpu())
    match = _device_match(whole, t_bbox, t_class, Lv, B, Q, n_list)
    lg64, bx64, total, losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w, match=match)
    total.backward()
    _check_values(r, losses, total, Lv, what="added ")
    _check_grads(r, lg64, bx64, ("C", name.rsplit("-", 1)[0]), what="added ")
    assert torch.equal(r.d_logits, whole.d_logits) and torch.equal(r.d_boxes, whole.d_boxes)     # the gradients read slots 1, 3, 4 only


# ------------------------------------------------------------------------------------------
# 7. through get_losses
# ------------------------------------------------------------------------------------------
API_CASE = CR.API_CASE


def _get_losses(config):
    from detr_tf.loss.loss import get_losses
    logits, boxes, t_bbox, t_class, _ = SC.loss_inputs(API_CASE)
    Lv = API_CASE[1]
    lgd, bxd = g(torch.from_numpy(logits)), g(torch.from_numpy(boxes))
    m_out = {"pred_logits": lgd[Lv - 1], "pred_boxes": bxd[Lv - 1],
             "aux": [{"pred_logits": lgd[i], "pred_boxes": bxd[i]} for i in range(Lv - 1)]}
    total, log = get_losses(m_out, t_bbox, t_class, config)
    return float(total), {k: float(v) for k, v in log.items()}, (logits, boxes, t_bbox, t_class)


def _check_api(total, log, ref_total, ref_losses):
    assert list(log) == list(ref_losses)
    for nm, ref in ref_losses.items():
        got, ref = log[nm], float(ref)
        print(f"{nm}: got {got!r}, reference {ref!r}")
        assert abs(got - ref) <= 2e-5 * max(1.0, abs(ref)), (nm, got, ref)
    print(f"total: got {total!r}, reference {float(ref_total)!r}")
    assert abs(total - float(ref_total)) <= 1e-5 * abs(float(ref_total))


def test_get_losses_reads_eos_coef_from_the_config(hip):
    bg = API_CASE[5]
    total, log, (logits, boxes, t_bbox, t_class) = _get_losses(SimpleNamespace(background_class=bg, eos_coef=0.25))
    w = CR.api_weights()[1]
    assert w == CR.DEFAULTS._replace(eos=0.25)
    _, _, ref_total, ref_losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w)
    _, _, default_total, _, _ = _reference64(logits, boxes, t_bbox, t_class, bg, CR.DEFAULTS)
    assert abs(float(ref_total) - float(default_total)) > 1e-3 * abs(float(ref_total))       # the value is visible in the total
    _check_api(total, log, ref_total, ref_losses)


def test_get_losses_follows_a_changing_config_and_rebuilds_the_class_weights(hip):
    """One config object, changed between calls: defaults (today's entry points and numbers), class weights, other class weights,
    defaults again.  The SetLoss of the shape is one cached object: its class-weight tensor follows the vector."""
    from detr_tf.loss.loss import SetLoss
    Lv, B, Q, C, bg, R = API_CASE[1:7]
    cfg = SimpleNamespace(background_class=bg)
    steps = [CR.api_weights()[k] for k in (0, 2, 3, 0)]
    assert steps[1].class_weights != steps[2].class_weights
    totals = []
    for w in steps:
        for k, v in zip(CR.CONFIG_NAMES, w):
            setattr(cfg, k, v)
        total, log, (logits, boxes, t_bbox, t_class) = _get_losses(cfg)
        _, _, ref_total, ref_losses, _ = _reference64(logits, boxes, t_bbox, t_class, bg, w)
        _check_api(total, log, ref_total, ref_losses)
        sl = SetLoss.get(Lv, B, Q, C, R, torch.device(DEV, torch.cuda.current_device()))
        assert sl.criterion.is_default == (w == CR.DEFAULTS) and sl.criterion.class_weights == w.class_weights
        if w.class_weights is not None:
            assert sl._weights[0] == w.class_weights and sl._weights[1].cpu().tolist() == list(w.class_weights)
        totals.append(total)
    # the default config gives what the oracle of the compiled-in criterion gives
    lg, bx = torch.from_numpy(logits).double(), torch.from_numpy(boxes).double()
    oracle_total, _, _ = SC.oracle_losses(lg, bx, torch.from_numpy(t_bbox).double(), torch.from_numpy(t_class), bg)
    assert abs(totals[0] - float(oracle_total)) <= 1e-5 * abs(float(oracle_total)) and len({round(t, 4) for t in totals[:3]}) == 3
    assert abs(totals[3] - totals[0]) <= 1e-5 * abs(totals[0])


def _tiny_problem():
    """Lv = 1, B = 1, Q = 4, C = 3, R = 3 with one target: the smallest shape with a matched and an unmatched query."""
    rng = np.random.default_rng(11)
    logits = rng.normal(size=(1, 1, 4, 3)).astype(np.float32)
    boxes = np.concatenate([rng.uniform(0.3, 0.7, (1, 1, 4, 2)), rng.uniform(0.1, 0.3, (1, 1, 4, 2))], -1).astype(np.float32)
    t_bbox = np.zeros((1, 3, 4), np.float32)
    t_bbox[0, 0, 0] = 1.0                                       # the header row: one target
    t_bbox[0, 1] = (0.5, 0.5, 0.2, 0.2)
    t_class = np.array([[0, 1, 0]], np.int64)
    return g(torch.from_numpy(logits)), g(torch.from_numpy(boxes)), g(torch.from_numpy(t_bbox)), g(torch.from_numpy(t_class))


def test_get_losses_calls_before_assign_once_between_cost_and_assignment(hip):
    from detr_tf.loss.loss import SetLoss, get_losses
    lg, bx, tb, tc = _tiny_problem()
    m_out = {"pred_logits": lg[0], "pred_boxes": bx[0]}
    cfg = SimpleNamespace(background_class=2)
    sl = SetLoss.get(1, 1, 4, 3, 3, lg.device)
    seen = []

    def hook():
        torch.cuda.synchronize()
        seen.append((bool(torch.isfinite(sl.matcher.cost[0, :, 0]).all()), sl.matcher.tgt_for_pred.cpu().tolist()))

    totals = []
    for k in range(2):
        sl.matcher.cost.fill_(float("nan"))
        sl.matcher.tgt_for_pred.fill_(SENTINEL)
        totals.append(float(get_losses(m_out, tb, tc, cfg, before_assign=hook)[0]))
        assert len(seen) == k + 1                               # exactly once per call
        assert seen[k] == (True, [[SENTINEL] * 4])              # the cost matrix is there, the assignment has not run
        assert sorted(sl.matcher.tgt_for_pred.cpu().tolist()[0]) == [-1, -1, -1, 0]
    assert float(get_losses(m_out, tb, tc, cfg)[0]) == totals[0] == totals[1] and len(seen) == 2      # omitted: not called


def test_two_set_losses_do_not_see_each_others_hook(hip):
    """A second SetLoss runs a whole forward without a hook INSIDE the hook of the first: a hook kept anywhere but in the call's own
    arguments would fire for it too."""
    from detr_tf.loss.loss import SetLoss
    lg, bx, tb, tc = _tiny_problem()
    a, b = SetLoss(1, 1, 4, 3, 3, lg.device), SetLoss(1, 1, 4, 3, 3, lg.device)
    calls, inner = [], []

    def hook():
        calls.append("a")
        inner.append(float(b.forward(lg, bx, tb, tc, 2)[0]))

    total_a = float(a.forward(lg, bx, tb, tc, 2, before_assign=hook)[0])
    assert calls == ["a"] and inner == [total_a]
    assert float(b.forward(lg, bx, tb, tc, 2)[0]) == total_a and calls == ["a"]


def test_hungarian_matching_with_other_cost_weights(hip):
    from scipy.optimize import linear_sum_assignment
    from detr_tf.loss.hungarian_matching import hungarian_matching
    from oracle import set_loss_ref as L
    case = next(c for c in CR.CONTIGUOUS if c[3] == 17)
    logits, boxes, t_bbox, t_class, _ = CR.inputs("B", case)
    n = case[7][0]
    got = hungarian_matching(g(torch.from_numpy(t_bbox[0])), g(torch.from_numpy(t_class[0])), g(torch.from_numpy(boxes[0, 0])),
                             g(torch.from_numpy(logits[0, 0])), 2, 3, 1.5)
    cost = L.cost_matrix(torch.from_numpy(t_bbox[0, 1:1 + n]), torch.from_numpy(t_class[0, 1:1 + n, 0]), torch.from_numpy(boxes[0, 0]),
                         torch.from_numpy(logits[0, 0]), 2, 3, 1.5).numpy()
    rows, cols = linear_sum_assignment(cost)
    assert np.array_equal(got[1].cpu().numpy(), rows) and np.array_equal(got[0].cpu().numpy(), cols)


# ------------------------------------------------------------------------------------------
# 8. the graphed training step re-records when the criterion changes
# ------------------------------------------------------------------------------------------
def test_graphed_step_follows_a_criterion_change(hip):
    """training.train_step against GraphedTrainStep(launch="graph") under weight set B on 96 x 128 images, B = 2, one encoder and
    two decoder layers, with the set-up and bounds of test_gpu_adamw.py::test_graph_replay_of_the_joint_step_equals_eager (logits 1e-5
    of their scale, loss 1e-5, update 2e-2 in relative L2).  At step 3 giou_loss_coef changes on both configs: the recorded step is
    dropped (one eager step, a new recording), and every later graphed step equals the eager one -- a replay that kept the old
    coefficient misses the loss bound."""
    from detr_tf import training
    from oracle import detr_ref as R
    from test_gpu_adamw import _build, _cfg
    from test_gpu_training import _batches
    weights = R.make_params(5, num_enc=1, num_dec=2)
    data = _batches(6, seed=3)
    cfg_e, cfg_g = _cfg(), _cfg()
    for c in (cfg_e, cfg_g):
        for k, v in zip(CR.CONFIG_NAMES, CR.weight_set("B", 92)):
            setattr(c, k, v)
    (m_e, o_e), (m_g, o_g) = _build(weights, cfg_e), _build(weights, cfg_g)
    stepper = training.GraphedTrainStep(m_g, o_g, cfg_g, eager_steps=1, launch="graph")
    recorded, totals = [], []
    for i, (im, tb, tc) in enumerate(data):
        if i == 3:
            recorded.append(stepper.step_graph)
            assert recorded[0] is not None
            cfg_e.giou_loss_coef = cfg_g.giou_loss_coef = 3.0
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
        # the total is the configured combination of the logged (unweighted) values
        coef = {"label_cost": cfg_g.class_loss_coef, "giou_loss": cfg_g.giou_loss_coef, "l1_loss": cfg_g.bbox_loss_coef}
        want = sum(float(v) * coef[k.rstrip("_0123456789")] for k, v in log_g.items() if k.rstrip("_0123456789") in coef)
        assert abs(float(tot_g) - want) <= 1e-5 * abs(want), (i, float(tot_g), want)
        if i >= 3:                                                      # the total at the old giou_loss_coef: far outside the loss bound
            old = want - (3.0 - 0.75) * sum(float(v) for k, v in log_g.items() if k.startswith("giou_loss"))
            assert abs(old - want) > 1e-3 * abs(want)
        totals.append(float(tot_g))
    assert stepper.step_graph is not None and stepper.step_graph is not recorded[0] and stepper.calls == 3
    del stepper, m_e, m_g, o_e, o_g
    gc.collect()
