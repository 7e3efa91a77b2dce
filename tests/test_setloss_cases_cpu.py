"""CPU proof (no GPU) that the inputs of tests/test_gpu_setloss_edges.py are admissible: SciPy and the project's own C solver
agree on every assignment case, the exact-comparison conditions hold, the float32 and float64 oracles pick the same matching on
every loss case, the forced box geometries are matched and off every gradient tie, and the case list reaches every solver
instantiation that an admitted shape can reach."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import setloss_cases as SC                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lsap_lib():
    so = os.path.join(ROOT, "oracle", "_build", "liblsap_oracle.so")
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "oracle", "lsap.c"), "-o", so, "-lm"])
    return ctypes.CDLL(so)


def _c_solve(lib, cost_qn):
    """oracle/lsap.c on one [Q, n] problem -> (status in the device's convention, pred_for_tgt)."""
    Q, n = cost_qn.shape
    if n > Q:
        return 2, None
    if n == 0:
        return 0, np.zeros(0, np.int64)
    C = np.ascontiguousarray(cost_qn, np.float64)
    a = np.zeros(n, np.int64)
    b = np.zeros(n, np.int64)
    rc = lib.lsap_oracle_solve(Q, n, C.ctypes.data_as(ctypes.c_void_p), a.ctypes.data_as(ctypes.c_void_p),
                               b.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        return 1, None
    pft = np.full(n, -1, np.int64)
    pft[b] = a
    return 0, pft


@pytest.mark.parametrize("case", SC.ASSIGN_CASES, ids=[c[0] for c in SC.ASSIGN_CASES])
def test_assign_case_references_agree(lsap_lib, case):
    name, Q, R, ldc, n_list, levels, kind = case
    cost, t_bbox, status = SC.assign_problem(case)
    B = len(n_list)
    assert cost.shape == (levels * B, Q, ldc) and cost.dtype == np.float32 and ldc >= R - 1 and max(n_list) <= R - 1
    assert Q <= SC.SL_MAXQ and R <= SC.SL_MAXR and SC.assign_dispatch(Q, R)[1] <= SC.LDS_PER_WORKGROUP
    quantum = SC.TIES_QUANTUM if kind == "ties" else SC.GRID_QUANTUM
    bound = 4 if kind == "ties" else 2 ** 20
    for p in range(levels * B):
        n = n_list[p % B]
        c = cost[p, :, :n]
        assert np.isnan(cost[p, :, n:]).all()                      # columns the solver must not read
        s_status, s_pft = SC.scipy_solve(c)
        c_status, c_pft = _c_solve(lsap_lib, c)
        assert s_status == c_status == status[p], (p, s_status, c_status, status[p])
        fin = c[np.isfinite(c)].astype(np.float64)
        if kind in ("grid", "ties") or status[p] != 1:
            k = fin / quantum                                       # the condition that justifies exact comparison on the device
            assert (k == np.round(k)).all() and (np.abs(k) <= bound).all()
        if kind in ("grid", "ties"):
            assert fin.size == c.size
        if s_status == 0:
            s_opt, c_opt = SC.chosen_cost(c, s_pft), SC.chosen_cost(c, c_pft)
            assert s_opt == c_opt and math.isfinite(s_opt)
            assert len(set(s_pft.tolist())) == n
    if kind in SC.BAD_KINDS:
        assert status[SC.bad_problem(case)] == 1 and (status == 1).sum() == 1
    if kind == "inf_feasible":
        assert np.isinf(cost).any()


def test_assign_cases_cover_the_issue_list():
    by_kind = {}
    for name, Q, R, ldc, n_list, levels, kind in SC.ASSIGN_CASES:
        by_kind.setdefault(kind, set()).add(Q)
    assert by_kind["grid"] == {1, 5, 63, 64, 65, 128, 129, 320, 321, 512, 100}
    assert {64, 100, 129, 321} <= by_kind["ties"] and {64, 100, 129, 321} <= by_kind["inf_feasible"]
    assert all(by_kind[k] for k in SC.BAD_KINDS)
    assert any(kind == "ties" and Q == 100 and n_list[:2] == [99, 99] for _, Q, _, _, n_list, _, kind in SC.ASSIGN_CASES)
    assert any(ldc > R - 1 for _, _, R, ldc, _, _, _ in SC.ASSIGN_CASES)
    assert any(n > Q for _, Q, _, _, n_list, _, _ in SC.ASSIGN_CASES for n in n_list)
    assert any(n == Q and Q > 64 for _, Q, _, _, n_list, _, _ in SC.ASSIGN_CASES for n in n_list)


def test_dispatch_arithmetic_and_instantiation_coverage():
    """Every admitted (Q, R): the launcher's LDS bytes and the instantiation it picks.  assign_kernel<2,false> needs Q <= 128 with
    more than 150 KiB for the double tile, and R <= 128 caps that tile at 132 600 bytes: no shape reaches it, so the launcher
    carries no branch for it.  Every instantiation that a shape can reach has an assignment case."""
    reach = {}
    most = {}
    for Q in range(1, SC.SL_MAXQ + 1):
        for R in range(2, SC.SL_MAXR + 1):
            inst, smem = SC.assign_dispatch(Q, R)
            assert smem == ((R + 1) & ~1) * 12 + (R - 1) * (129 * 8 if inst == "<2,true>" else ((Q + 63) // 64 * 64 + 1) * 4)
            most[inst] = max(most.get(inst, 0), smem)
            if smem <= SC.LDS_PER_WORKGROUP:
                reach.setdefault(inst, (Q, R))
    assert most["<2,true>"] == 132600 == SC.assign_dispatch(128, 128)[1]
    assert most["<8,false>"] == 127 * 513 * 4 + 1536 == 262140 > SC.LDS_PER_WORKGROUP      # admitted by the shape check alone
    assert set(reach) == {"<2,true>", "<5,false>", "<8,false>"}
    covered = {SC.assign_dispatch(Q, R)[0] for _, Q, R, _, _, _, _ in SC.ASSIGN_CASES}
    assert covered == set(reach)
    # the dispatch boundaries sit where the cases put them
    assert [SC.assign_dispatch(Q, 64)[0] for Q in (128, 129, 320, 321)] == ["<2,true>", "<5,false>", "<5,false>", "<8,false>"]


def _torch_inputs(case, dtype):
    logits, boxes, t_bbox, t_class, forced = SC.loss_inputs(case)
    return (torch.from_numpy(logits).to(dtype), torch.from_numpy(boxes).to(dtype), torch.from_numpy(t_bbox).to(dtype),
            torch.from_numpy(t_class), forced)


CONTIGUOUS = [c for c in SC.LOSS_CASES if c[-1] == "contiguous"]


def test_loss_cases_cover_the_issue_list():
    assert [c[1:8] for c in CONTIGUOUS] == [(1, 1, 1, 2, 1, 2, [1]), (2, 3, 7, 2, 0, 9, [3, 0, 7]), (1, 2, 9, 64, 63, 12, [9, 1]),
                                            (3, 2, 17, 65, 0, 20, [17, 4]), (2, 2, 100, 130, 129, 100, [99, 0]),
                                            (1, 2, 129, 92, 91, 33, [32, 5]), (6, 1, 100, 92, 91, 100, [7])]
    assert [c[1:8] for c in SC.LOSS_CASES if c[-1] == "strided"] == [c[1:8] for c in CONTIGUOUS]
    a, b = SC.LOSS_CASES[2], SC.LOSS_CASES[3]
    assert a[-1] == "contiguous" and b[-1] == "strided" and a[1:8] == b[1:8]
    for x, y in zip(SC.loss_inputs(a)[:4], SC.loss_inputs(b)[:4]):
        assert np.array_equal(x, y)                               # a layout moves the values in memory, never changes them


@pytest.mark.parametrize("case", CONTIGUOUS, ids=[c[0] for c in CONTIGUOUS])
def test_loss_case_matching_is_precision_independent_and_off_ties(case):
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    lg32, bx32, tb32, tc, forced = _torch_inputs(case, torch.float32)
    lg64, bx64, tb64, _, _ = _torch_inputs(case, torch.float64)
    assert int(tc.min()) >= 0 and int(tc.max()) < C and 0 <= bg < C
    m32 = SC.oracle_match(lg32, bx32, tb32, tc)
    m64 = SC.oracle_match(lg64, bx64, tb64, tc)
    for lv in range(Lv):
        for x, y in zip(m32[lv][2:], m64[lv][2:]):
            assert torch.equal(x, y), f"{name}: float32 and float64 oracles match differently at level {lv}: change the seed"
        tb, _, ti, pi, sel = m64[lv]
        assert ti.numel() == sum(min(n, Q) for n in n_list) and int(sel.sum()) == ti.numel()
        for t, p in zip(ti.tolist(), pi.tolist()):
            shows, off_tie = SC.pair_geometry(bx32[lv].reshape(-1, 4)[p].numpy(), tb32.new_tensor(tb[t].numpy()).numpy())
            assert off_tie, f"{name}: level {lv} prediction {p} / target {t} sits on a gradient tie"
    # every forced pair is matched, and shows the geometry it was built for
    t_off = np.concatenate([[0], np.cumsum(n_list)])
    for lv, b, k, kind in forced:
        tb, _, ti, pi, _ = m64[lv]
        pairs = dict(zip(ti.tolist(), pi.tolist()))
        assert pairs[int(t_off[b]) + k] == b * Q + k, f"{name}: forced pair {(lv, b, k, kind)} is not matched"
        shows, _ = SC.pair_geometry(bx32[lv, b, k].numpy(), tb32[b, 1 + k].numpy())
        assert kind in shows, (name, lv, b, k, kind, shows)


def test_forced_geometries_cover_every_kind():
    seen = set()
    for case in CONTIGUOUS:
        seen |= {kind for _, _, _, kind in SC.loss_inputs(case)[4]}
    assert seen == set(SC.GEOMETRIES)
    # ... and four cases carry all six at once, on every level
    full = [c for c in CONTIGUOUS if {k for _, _, _, k in SC.loss_inputs(c)[4]} == set(SC.GEOMETRIES)]
    assert len(full) >= 4


def test_oracle_driver_equals_get_losses():
    """setloss_cases.oracle_losses is oracle get_losses rebuilt from its own pieces: same numbers where both apply (an image
    without targets included), so the freedoms it adds (empty problems, labels outside [0, C)) rest on the same code."""
    from oracle import set_loss_ref as L
    for case in (CONTIGUOUS[1], CONTIGUOUS[3]):
        name, Lv, B, Q, C, bg, R, n_list, layout = case
        lg, bx, tb, tc, _ = _torch_inputs(case, torch.float64)
        total, losses, _ = SC.oracle_losses(lg, bx, tb, tc, bg)
        m_out = {"pred_logits": lg[Lv - 1], "pred_boxes": bx[Lv - 1],
                 "aux": [{"pred_logits": lg[i], "pred_boxes": bx[i]} for i in range(Lv - 1)]}
        ref_total, ref = L.get_losses(m_out, tb, tc, bg)
        assert list(losses) == list(ref) and float(total) == float(ref_total)
        assert all(float(losses[k]) == float(ref[k]) for k in ref)


def test_out_of_range_label_cost_column():
    """cost_matrix_ref: a label outside [0, C) costs what a class probability of 0 costs; every other column is the oracle's."""
    from oracle import set_loss_ref as L
    case = CONTIGUOUS[3]
    C = case[4]
    lg, bx, tb, tc, _ = _torch_inputs(case, torch.float32)
    tbs, tcs = L.strip_header(tb[0], tc[0])
    ref = L.cost_matrix(tbs, tcs, bx[0, 0], lg[0, 0])
    bad = tcs.clone()
    bad[2], bad[5] = C, -1
    got = SC.cost_matrix_ref(tbs, bad, bx[0, 0], lg[0, 0])
    keep = torch.ones(tcs.numel(), dtype=torch.bool)
    keep[[2, 5]] = False
    assert torch.equal(got[:, keep], ref[:, keep])
    prob = torch.softmax(lg[0, 0], -1)[:, tcs[[2, 5]]]
    assert torch.allclose(got[:, ~keep], ref[:, ~keep] + prob, atol=1e-6, rtol=0)


def test_recorded_float32_oracle_errors_are_what_the_oracle_gives():
    """setloss_cases.D_LOGITS_ATOL is 4x the float32 oracle's own d_logits error on the cases listed there: measured here again,
    and no other case needs it (the float32 oracle meets the relative bound of the GPU test with a factor 4 to spare)."""
    for case in CONTIGUOUS:
        name, Lv, B, Q, C, bg, R, n_list, layout = case
        grads = {}
        for dtype in (torch.float32, torch.float64):
            lg, bx, tb, tc, _ = _torch_inputs(case, dtype)
            lg.requires_grad_(True)
            total, _, _ = SC.oracle_losses(lg, bx, tb, tc, bg)
            total.backward()
            grads[dtype] = 0.5 * lg.grad.double()              # loss_scale of the GPU test
        err = float((grads[torch.float32] - grads[torch.float64]).abs().max())
        rel_bound = 2e-5 * float(grads[torch.float64].abs().max())
        key = name.rsplit("-", 1)[0]
        if key in SC.D_LOGITS_F32_ORACLE_ERR:
            assert 4 * err > rel_bound and 0.5 * SC.D_LOGITS_F32_ORACLE_ERR[key] <= err <= SC.D_LOGITS_F32_ORACLE_ERR[key] * 1.001, (name, err)
        else:
            assert 4 * err <= rel_bound, (name, err, rel_bound)
