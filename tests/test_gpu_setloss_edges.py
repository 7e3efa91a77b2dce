"""GPU tests of csrc/setloss.hip away from the benchmark's shape: every instantiation and column-slot edge of the one-wave
assignment solver against SciPy (exactly: the costs of tests/setloss_cases.py make every correct solver exactly optimal), and the
cost / sums / gradient kernels against the float64 oracle with autograd at small and large class counts, ragged query chunks,
strided head outputs, empty images, labels outside [0, C) and an unsolvable problem inside a batch.
tests/test_setloss_cases_cpu.py proves the inputs admissible without a GPU."""
import ctypes
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import setloss_cases as SC                 # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -7


def g(t):
    return t.to(DEV).contiguous()


def close(a, b, rtol, what="", atol=None):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    scale = float(b.abs().max()) + 1e-30
    atol = rtol * scale if atol is None else atol
    err = float((a - b).abs().max())
    print(f"{what}: max abs err {err:.3e}, bound {atol:.3e} (scale {scale:.3e})")
    assert err <= atol, f"{what}: max abs err {err:.3e} > {atol:.3e} (scale {scale:.3e})"


# ------------------------------------------------------------------------------------------
# assignment
# ------------------------------------------------------------------------------------------
def _assign(hip, cost, t_bbox, Q, R, ldc):
    """One launch over all problems of cost [P, Q, ldc] (numpy); outputs prefilled with a sentinel."""
    P, B = cost.shape[0], t_bbox.shape[0]
    cd, tbd = g(torch.from_numpy(cost)), g(torch.from_numpy(t_bbox))
    tfp = torch.full((P, Q), SENTINEL, device=DEV, dtype=torch.int32)
    pft = torch.full((P, ldc), SENTINEL, device=DEV, dtype=torch.int32)
    st = torch.full((P,), SENTINEL, device=DEV, dtype=torch.int32)
    hip.call("detr_hip_assign_f32", cd.data_ptr(), P, Q, ldc, tbd.data_ptr(), B, R, tfp.data_ptr(), pft.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    return tfp.cpu().numpy(), pft.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("case", SC.ASSIGN_CASES, ids=[c[0] for c in SC.ASSIGN_CASES])
def test_assign_case(hip, case):
    name, Q, R, ldc, n_list, levels, kind = case
    cost, t_bbox, want_status = SC.assign_problem(case)
    B = len(n_list)
    P = levels * B
    tfp, pft, st = _assign(hip, cost, t_bbox, Q, R, ldc)
    assert np.array_equal(st, want_status), (st, want_status)
    for p in range(P):
        n = n_list[p % B]
        c = cost[p, :, :n]
        ref_status, ref_pft = SC.scipy_solve(c)
        assert ref_status == want_status[p]
        if st[p] != 0:
            assert (tfp[p] == -1).all() and (pft[p] == -1).all(), f"problem {p}: status {st[p]} with indices left behind"
            continue
        got = pft[p, :n]
        assert ((got >= 0) & (got < Q)).all() and len(set(got.tolist())) == n, f"problem {p}: not an injective map into [0, Q)"
        assert (pft[p, n:] == -1).all()                             # up to ldc, beyond R - 1 where ldc > R - 1
        inv = np.full(Q, -1)
        inv[got] = np.arange(n)
        assert np.array_equal(tfp[p], inv), f"problem {p}: tgt_for_pred is not the inverse of pred_for_tgt"
        got_opt, ref_opt = SC.chosen_cost(c, got), SC.chosen_cost(c, ref_pft)
        assert got_opt == ref_opt, f"problem {p} (Q={Q}, n={n}): cost {got_opt!r}, SciPy's optimum {ref_opt!r}"
        if kind == "grid":
            assert np.array_equal(got, ref_pft), f"problem {p} (Q={Q}, n={n}) differs from SciPy"
    # every problem solved alone gives what it gave inside the launch
    for p in range(P):
        b = p % B
        tfp1, pft1, st1 = _assign(hip, cost[p:p + 1], t_bbox[b:b + 1], Q, R, ldc)
        assert st1[0] == st[p] and np.array_equal(tfp1[0], tfp[p]) and np.array_equal(pft1[0], pft[p]), f"problem {p} alone differs"


def test_assign_refuses_a_tile_beyond_the_lds(hip):
    """Q = 512 with R = 128 passes the shape check and needs 262 140 bytes of LDS: refused on the host with the numbers in the
    message, before anything is launched; the outputs are untouched and the next valid call works."""
    Q, R = 512, 128
    assert SC.assign_dispatch(Q, R) == ("<8,false>", 262140)
    cost = np.zeros((1, Q, R - 1), np.float32)
    t_bbox = np.zeros((1, R, 4), np.float32)
    t_bbox[0, 0, 0] = 3
    cd, tbd = g(torch.from_numpy(cost)), g(torch.from_numpy(t_bbox))
    tfp = torch.full((1, Q), SENTINEL, device=DEV, dtype=torch.int32)
    pft = torch.full((1, R - 1), SENTINEL, device=DEV, dtype=torch.int32)
    st = torch.full((1,), SENTINEL, device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError) as e:
        hip.call("detr_hip_assign_f32", cd.data_ptr(), 1, Q, R - 1, tbd.data_ptr(), 1, R, tfp.data_ptr(), pft.data_ptr(), st.data_ptr())
    msg = str(e.value)
    assert "Q=512" in msg and "R=128" in msg and "262140 bytes of LDS" in msg, msg
    torch.cuda.synchronize()
    assert bool((tfp == SENTINEL).all()) and bool((pft == SENTINEL).all()) and bool((st == SENTINEL).all())
    case = next(c for c in SC.ASSIGN_CASES if c[1] == 512 and c[6] == "grid")
    cost, t_bbox, want = SC.assign_problem(case)
    _, pft2, st2 = _assign(hip, cost, t_bbox, case[1], case[2], case[3])
    assert np.array_equal(st2, want)
    assert np.array_equal(pft2[0, :64], SC.scipy_solve(cost[0, :, :64])[1])


# ------------------------------------------------------------------------------------------
# cost, sums, gradients
# ------------------------------------------------------------------------------------------
SLACK_FILL = 1e30          # "strided": what the buffers hold outside the views; a stray read shows up in the values


def _device_view(x, layout, slack):
    """x [Lv, B, Q, last] numpy -> device tensor with these values: contiguous, or the [:, :, :Q, :last] view of a larger buffer."""
    t = torch.from_numpy(x)
    if layout == "contiguous":
        return g(t)
    Lv, B, Q, last = x.shape
    buf = torch.full((Lv, B, Q + SC.Q_SLACK, last + slack), SLACK_FILL, device=DEV, dtype=torch.float32)
    view = buf[:, :, :Q, :last]
    view.copy_(t)
    assert view.stride() == buf.stride() and view.stride(2) == last + slack and view.stride(3) == 1
    return view


def _pipeline(hip, logits, boxes, t_bbox, t_class, bg, layout="contiguous", grad=False):
    """cost -> assign -> sums -> finalize (-> gradients with loss_scale 0.5) on numpy inputs, through make_desc."""
    from detr_tf.loss.hungarian_matching import make_desc
    Lv, B, Q, C = logits.shape
    R = t_bbox.shape[1]
    P = Lv * B
    lgd = _device_view(logits, layout, SC.C_SLACK)
    bxd = _device_view(boxes, layout, SC.BOX_SLACK)
    tbd, tcd = g(torch.from_numpy(t_bbox)), g(torch.from_numpy(t_class).reshape(B, R))
    d = make_desc(lgd, bxd, tbd, tcd, bg)
    cost = torch.full((P, Q, R - 1), float(SENTINEL), device=DEV)
    hip.call("detr_hip_match_cost_f32", ctypes.byref(d), cost.data_ptr())
    tfp = torch.full((P, Q), SENTINEL, device=DEV, dtype=torch.int32)
    pft = torch.full((P, R - 1), SENTINEL, device=DEV, dtype=torch.int32)
    st = torch.full((P,), SENTINEL, device=DEV, dtype=torch.int32)
    hip.call("detr_hip_assign_f32", cost.data_ptr(), P, Q, R - 1, tbd.data_ptr(), B, R, tfp.data_ptr(), pft.data_ptr(), st.data_ptr())
    sums = torch.zeros(Lv * 10, device=DEV)
    hip.call("detr_hip_set_loss_sums_f32", ctypes.byref(d), tfp.data_ptr(), sums.data_ptr())
    out = torch.zeros(Lv, 6, device=DEV)
    tot = torch.zeros(1, device=DEV)
    hip.call("detr_hip_set_loss_finalize_f32", sums.data_ptr(), Lv, out.data_ptr(), tot.data_ptr())
    r = SimpleNamespace(cost=cost.cpu(), tfp=tfp.cpu().numpy(), pft=pft.cpu().numpy(), status=st.cpu().numpy(), sums=sums.cpu(),
                        out=out.cpu(), total=float(tot))
    if grad:
        dl = torch.full_like(lgd, float(SENTINEL))
        dbx = torch.full_like(bxd, float(SENTINEL))
        hip.call("detr_hip_set_loss_grad_f32", ctypes.byref(d), tfp.data_ptr(), sums.data_ptr(), ctypes.c_float(0.5), dl.data_ptr(),
                 dbx.data_ptr())
        r.d_logits, r.d_boxes = dl.cpu(), dbx.cpu()
    torch.cuda.synchronize()
    return r


def _oracle64(logits, boxes, t_bbox, t_class, bg, empty=()):
    lg = torch.from_numpy(logits).double().requires_grad_(True)
    bx = torch.from_numpy(boxes).double().requires_grad_(True)
    total, losses, match = SC.oracle_losses(lg, bx, torch.from_numpy(t_bbox).double(), torch.from_numpy(t_class), bg, empty=empty)
    return lg, bx, total, losses, match


def _check_cost(r, logits, boxes, t_bbox, t_class, n_list):
    """Against the float32 oracle (the same arithmetic: 2e-6 absolute, as tests/test_gpu_kernels.py); columns >= n untouched."""
    from oracle import set_loss_ref as L
    Lv, B = logits.shape[:2]
    worst = 0.0
    for lv in range(Lv):
        for b in range(B):
            n = n_list[b]
            tbs, tcs = L.strip_header(torch.from_numpy(t_bbox[b]), torch.from_numpy(t_class[b]))
            ref = SC.cost_matrix_ref(tbs, tcs, torch.from_numpy(boxes[lv, b]), torch.from_numpy(logits[lv, b]))
            got = r.cost[lv * B + b]
            assert bool((got[:, n:] == SENTINEL).all()), f"cost lv{lv} b{b}: written past n = {n}"
            both_nan = torch.isnan(got[:, :n]) & torch.isnan(ref)
            err = float(torch.where(both_nan, torch.zeros_like(ref), (got[:, :n] - ref).abs()).max()) if n else 0.0
            worst = max(worst, err)
            assert err <= 2e-6, f"cost lv{lv} b{b}: max abs err {err:.3e} > 2e-6"
    print(f"cost: max abs err {worst:.3e}, bound 2e-6")


def _check_values(r, losses, total, Lv, names=SC.LOSS_NAMES, what=""):
    """The six values per level within 2e-5 * max(1, |ref|), NaN exactly where the oracle's is; the total within 1e-5 relative."""
    for lv in range(Lv):
        suf = "" if lv == Lv - 1 else f"_{lv}"
        for k, nm in enumerate(SC.LOSS_NAMES):
            if nm not in names:
                continue
            got, ref = float(r.out[lv, k]), float(losses[nm + suf])
            print(f"{what}{nm}{suf}: got {got!r}, oracle {ref!r}, err {abs(got - ref):.3e}")
            if math.isnan(ref):
                assert math.isnan(got), (lv, nm, got, ref)
            else:
                assert abs(got - ref) <= 2e-5 * max(1.0, abs(ref)), (lv, nm, got, ref)
    if total is not None:
        ref = float(total)
        print(f"{what}total: got {r.total!r}, oracle {ref!r}")
        if math.isnan(ref):
            assert math.isnan(r.total)
        else:
            assert abs(r.total - ref) <= 1e-5 * abs(ref), (r.total, ref)


CONTIGUOUS = [c for c in SC.LOSS_CASES if c[-1] == "contiguous"]
STRIDED = [c for c in SC.LOSS_CASES if c[-1] == "strided"]


@pytest.mark.parametrize("case", CONTIGUOUS, ids=[c[0] for c in CONTIGUOUS])
def test_set_loss_case_vs_oracle(hip, case):
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    logits, boxes, t_bbox, t_class, _ = SC.loss_inputs(case)
    lg64, bx64, total, losses, _ = _oracle64(logits, boxes, t_bbox, t_class, bg)
    total.backward()
    r = _pipeline(hip, logits, boxes, t_bbox, t_class, bg, grad=True)
    _check_cost(r, logits, boxes, t_bbox, t_class, n_list)
    assert (r.status == 0).all()
    _check_values(r, losses, total, Lv)
    close(r.d_logits, 0.5 * lg64.grad, rtol=2e-5, what="d_logits", atol=SC.D_LOGITS_ATOL.get(name.rsplit("-", 1)[0]))
    close(r.d_boxes, 0.5 * bx64.grad, rtol=5e-5, what="d_boxes")
    for b, n in enumerate(n_list):
        if n == 0:                                                   # an image without targets: every query a negative, no box gradient
            for lv in range(Lv):
                assert (r.tfp[lv * B + b] == -1).all() and (r.pft[lv * B + b] == -1).all()
                assert bool((r.d_boxes[lv, b] == 0).all())
                assert bool((r.cost[lv * B + b] == SENTINEL).all())


@pytest.mark.parametrize("case", STRIDED, ids=[c[0] for c in STRIDED])
def test_set_loss_case_strided_heads(hip, case):
    """The cost and sums kernels on views into larger buffers (non-trivial level, image and query strides, unit last stride);
    the slack holds 1e30."""
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    logits, boxes, t_bbox, t_class, _ = SC.loss_inputs(case)
    _, _, total, losses, _ = _oracle64(logits, boxes, t_bbox, t_class, bg)
    r = _pipeline(hip, logits, boxes, t_bbox, t_class, bg, layout="strided")
    _check_cost(r, logits, boxes, t_bbox, t_class, n_list)
    assert (r.status == 0).all()
    _check_values(r, losses, total, Lv)


def test_set_loss_all_images_empty(hip):
    Lv, B, Q, C, bg, R = 2, 2, 9, 5, 4, 6
    case = ("all-empty", Lv, B, Q, C, bg, R, [0, 0], "contiguous")
    rng = np.random.default_rng(11)
    logits = (rng.normal(size=(Lv, B, Q, C)) * 2).astype(np.float32)
    boxes = rng.uniform(0.1, 0.6, (Lv, B, Q, 4)).astype(np.float32)
    t_bbox, t_class = SC.make_targets(case[7], R, C, bg, rng)
    lg64, bx64, total, losses, _ = _oracle64(logits, boxes, t_bbox, t_class, bg)
    for nm in SC.LOSS_NAMES:
        assert math.isnan(float(losses[nm])) == (nm in ("giou_loss", "l1_loss", "true_pos", "pos_accuracy")), nm
    assert math.isnan(float(total))
    sum(losses["label_cost" + ("" if lv == Lv - 1 else f"_{lv}")] for lv in range(Lv)).backward()
    r = _pipeline(hip, logits, boxes, t_bbox, t_class, bg, grad=True)
    assert (r.status == 0).all() and (r.tfp == -1).all() and bool((r.cost == SENTINEL).all())
    _check_values(r, losses, total, Lv)
    assert bool((r.d_boxes == 0).all())
    assert bool(torch.isfinite(r.d_logits).all())
    close(r.d_logits, 0.5 * lg64.grad, rtol=2e-5, what="d_logits")


@pytest.mark.parametrize("layout", SC.LAYOUTS)
def test_set_loss_label_outside_the_classes(hip, layout):
    """One target of class C and one of class -1: the cost's class term is 0 for them, the matching succeeds, the cross-entropy
    (and the total) turn NaN as csrc/setloss.hip states while the counts, L1 and GIoU stay the oracle's, nothing outside the
    views is read, and the gradients stay finite."""
    from oracle import set_loss_ref as L
    case = next(c for c in CONTIGUOUS if c[3] == 17)
    name, Lv, B, Q, C, bg, R, n_list, _ = case
    logits, boxes, t_bbox, t_class, _ = SC.loss_inputs(case)
    t_class = t_class.copy()
    t_class[0, 1 + 2, 0] = C
    t_class[1, 1 + 1, 0] = -1
    lg = torch.from_numpy(logits).double()
    bx = torch.from_numpy(boxes).double().requires_grad_(True)
    tc = torch.from_numpy(t_class)
    match = SC.oracle_match(lg, bx, torch.from_numpy(t_bbox).double(), tc)
    r = _pipeline(hip, logits, boxes, t_bbox, t_class, bg, layout=layout, grad=(layout == "contiguous"))
    _check_cost(r, logits, boxes, t_bbox, t_class, n_list)
    assert (r.status == 0).all()
    want = {}
    box_total = 0
    for lv in range(Lv):
        suf = "" if lv == Lv - 1 else f"_{lv}"
        tb, tcs, ti, pi, sel = match[lv]
        valid = torch.where((tcs >= 0) & (tcs < C), tcs, torch.zeros_like(tcs))
        _, true_neg, true_pos, _ = L.loss_labels(lg[lv].reshape(-1, C), valid, ti, pi, sel, bg)
        pos_acc = (lg[lv].reshape(-1, C)[pi].argmax(-1) == tcs[ti]).double().mean()
        giou, l1 = L.loss_boxes(bx[lv].reshape(-1, 4), tb, ti, pi)
        box_total = box_total + 2 * giou + 5 * l1
        want.update({"label_cost" + suf: float("nan"), "true_neg" + suf: true_neg, "true_pos" + suf: true_pos,
                     "pos_accuracy" + suf: pos_acc, "giou_loss" + suf: giou.detach(), "l1_loss" + suf: l1.detach()})
    _check_values(r, want, float("nan"), Lv)
    if layout == "contiguous":
        box_total.backward()
        assert bool(torch.isfinite(r.d_logits).all())
        close(r.d_boxes, 0.5 * bx.grad, rtol=5e-5, what="d_boxes")


def test_set_loss_unsolvable_problem_in_the_batch(hip):
    """A zero-area target under a coincident zero-area prediction: that one cost entry is 0 / 0, its problem reports status 1,
    its queries count as negatives, and everything else equals the oracle with that problem's image treated as empty."""
    Lv, B, Q, C, bg, R = 2, 2, 9, 5, 4, 6
    n_list = [3, 2]
    rng = np.random.default_rng(23)
    logits = (rng.normal(size=(Lv, B, Q, C)) * 2).astype(np.float32)
    boxes = np.concatenate([rng.uniform(0.2, 0.8, (Lv, B, Q, 2)), rng.uniform(0.05, 0.4, (Lv, B, Q, 2))], -1).astype(np.float32)
    t_bbox, t_class = SC.make_targets(n_list, R, C, bg, rng)
    t_bbox[1, 1] = (0.3, 0.4, 0.0, 0.0)
    boxes[1, 1, 5] = (0.3, 0.4, 0.0, 0.0)
    _, _, total, losses, _ = _oracle64(logits, boxes, t_bbox, t_class, bg, empty={(1, 1)})
    r = _pipeline(hip, logits, boxes, t_bbox, t_class, bg, grad=True)
    assert math.isnan(float(r.cost[1 * B + 1, 5, 0])) and int(torch.isnan(r.cost).sum()) == 1
    assert r.status.tolist() == [0, 0, 0, 1]
    assert (r.tfp[3] == -1).all() and (r.pft[3] == -1).all()
    assert float(r.sums[1 * 8 + 3]) == Q - n_list[0] + Q and float(r.sums[1 * 8 + 4]) == n_list[0]      # negatives / positives of level 1
    assert float(r.sums[0 * 8 + 3]) == 2 * Q - sum(n_list) and float(r.sums[0 * 8 + 4]) == sum(n_list)
    _check_values(r, losses, total, Lv)
    assert bool((r.d_boxes[1, 1] == 0).all()) and bool(torch.isfinite(r.d_logits).all()) and bool(torch.isfinite(r.d_boxes).all())


# ------------------------------------------------------------------------------------------
# through the Python entry points
# ------------------------------------------------------------------------------------------
def test_get_losses_with_background_class_zero(hip):
    from detr_tf.loss.loss import get_losses
    case = ("api", 2, 2, 9, 5, 0, 6, [5, 2], "contiguous")
    logits, boxes, t_bbox, t_class, _ = SC.loss_inputs(case)
    Lv, bg = case[1], case[5]
    _, _, total, losses, _ = _oracle64(logits, boxes, t_bbox, t_class, bg)
    lgd, bxd = g(torch.from_numpy(logits)), g(torch.from_numpy(boxes))
    m_out = {"pred_logits": lgd[Lv - 1], "pred_boxes": bxd[Lv - 1],
             "aux": [{"pred_logits": lgd[i], "pred_boxes": bxd[i]} for i in range(Lv - 1)]}
    got_total, log = get_losses(m_out, t_bbox, t_class, SimpleNamespace(background_class=bg))
    assert list(log) == list(losses)
    for nm, ref in losses.items():
        got, ref = float(log[nm]), float(ref)
        print(f"{nm}: got {got!r}, oracle {ref!r}")
        if nm.startswith(("true_neg", "true_pos")):
            assert abs(got - ref) <= 2.0 ** -23, (nm, got, ref)       # a ratio of two counts: one float32 rounding
        else:
            assert abs(got - ref) <= 2e-5 * max(1.0, abs(ref)), (nm, got, ref)
    assert abs(float(got_total) - float(total)) <= 1e-5 * abs(float(total))


def test_hungarian_matching_six_tuple_on_the_float_tile(hip):
    """The single-image wrapper (tests/test_gpu_kernels.py stops at Q = 100) at Q = 129, n = 100, R = 101: the float-tile solver
    with one column in its third slot and an odd R."""
    from scipy.optimize import linear_sum_assignment
    from detr_tf.loss.hungarian_matching import hungarian_matching
    from oracle import set_loss_ref as L
    rng = np.random.default_rng(129)
    Q, n, R, C = 129, 100, 101, 92
    t_bbox = np.zeros((R, 4), np.float32)
    t_class = np.zeros((R, 1), np.int64)
    t_bbox[0, 0] = n
    t_bbox[1:1 + n, :2] = rng.uniform(0.2, 0.8, (n, 2))
    t_bbox[1:1 + n, 2:] = rng.uniform(0.05, 0.4, (n, 2))
    t_class[1:1 + n, 0] = rng.integers(1, 91, n)
    p_bbox = np.concatenate([rng.uniform(0.1, 0.9, (Q, 2)), rng.uniform(0.05, 0.5, (Q, 2))], 1).astype(np.float32)
    p_class = rng.normal(size=(Q, C)).astype(np.float32)
    got = hungarian_matching(g(torch.from_numpy(t_bbox)), g(torch.from_numpy(t_class)), g(torch.from_numpy(p_bbox)),
                             g(torch.from_numpy(p_class)), slice_preds=True)
    assert len(got) == 6
    t_idx, p_idx, t_sel, p_sel, tb, tc = got
    cost = L.cost_matrix(torch.from_numpy(t_bbox[1:1 + n]), torch.from_numpy(t_class[1:1 + n, 0]), torch.from_numpy(p_bbox),
                         torch.from_numpy(p_class)).numpy()
    rows, cols = linear_sum_assignment(cost)                       # rows = predictions (ascending), cols = targets
    assert t_idx.dtype == torch.int64 and p_idx.dtype == torch.int64
    assert np.array_equal(p_idx.cpu().numpy(), rows) and np.array_equal(t_idx.cpu().numpy(), cols)
    assert t_sel.dtype == torch.bool and tuple(t_sel.shape) == (n,) and bool(t_sel.all())
    want_psel = np.zeros(Q, bool)
    want_psel[rows] = True
    assert p_sel.dtype == torch.bool and np.array_equal(p_sel.cpu().numpy(), want_psel)
    assert np.array_equal(tb.cpu().numpy(), t_bbox[1:1 + n]) and np.array_equal(tc.cpu().numpy(), t_class[1:1 + n, 0])
