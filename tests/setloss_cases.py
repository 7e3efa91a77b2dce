"""Shared cases of the set-loss tests (tests/test_setloss_cases_cpu.py proves them admissible, tests/test_gpu_setloss_edges.py runs
them on csrc/setloss.hip): cost matrices for every path of the one-wave assignment solver, and logits / boxes / targets for the
cost, sums and gradient kernels at the class counts, query counts, layouts and box geometries the benchmark's shape never reaches.

The inputs are plain numpy (no GPU, no torch).  The last section restates oracle/set_loss_ref.get_losses from the oracle's own
pieces with two extra freedoms the edge tests need (a per-problem "treat as empty" set and class labels outside [0, C)); it runs on
the CPU in the dtype of the tensors it is given."""
import math
import zlib

import numpy as np

# ------------------------------------------------------------------------------------------
# host-side dispatch arithmetic of detr_hip_assign_f32 (csrc/setloss.hip)
# ------------------------------------------------------------------------------------------
SL_MAXQ, SL_MAXR, SL_QCHUNK = 512, 128, 8
LDS_PER_WORKGROUP = 160 * 1024


def assign_dispatch(Q, R):
    """(instantiation, dynamic LDS bytes) by the rule the launcher was written with: the double tile for Q <= 128 while the tile and
    the row state stay below 150 KiB, otherwise the float tile with 2, 5 or 8 column slots."""
    nmax = (R + 1) & ~1
    cpl = (Q + 63) // 64
    cd = Q <= 128 and nmax * 12 + (R - 1) * 129 * 8 <= 150 * 1024
    tile = (R - 1) * (129 if cd else cpl * 64 + 1)
    smem = nmax * 8 + nmax * 4 + tile * (8 if cd else 4)
    if cpl <= 2 and cd:
        inst = "<2,true>"
    elif cpl <= 2:
        inst = "<2,false>"
    elif cpl <= 5:
        inst = "<5,false>"
    else:
        inst = "<8,false>"
    return inst, smem


# ------------------------------------------------------------------------------------------
# assignment cases: (name, Q, R, ldc, n_list, levels, kind)
# ------------------------------------------------------------------------------------------
GRID_QUANTUM = 2.0 ** -18          # "grid": integers of [-2^20, 2^20] times this: exact in float32, every dual update exact in double
TIES_QUANTUM = 0.5                 # "ties": integers of [-4, 4] times this
BAD_KINDS = ("inf_infeasible", "nan", "neg_inf")

#                  Q    R   ldc  n_list           path or edge
ASSIGN_SHAPES = [(1, 2, 1, [1, 0]),             # smallest problem
                 (5, 9, 8, [5, 3, 8]),          # n = 8 > Q: status 2
                 (63, 66, 65, [63, 1, 17]),     # slot 1 absent
                 (64, 66, 65, [64, 1, 17]),     # slot 0 full, slot 1 absent, n == Q
                 (65, 66, 65, [65, 1, 17]),     # one column in slot 1, n == Q above 64
                 (128, 128, 127, [127, 64]),    # <2,true> at its LDS maximum (132 600 bytes)
                 (129, 101, 100, [100, 2]),     # first shape of <5,false>; odd R; one column in slot 2
                 (320, 64, 63, [63, 9]),        # last shape of <5,false>
                 (321, 64, 63, [63, 9]),        # first shape of <8,false>
                 (512, 65, 64, [64, 1]),        # <8,false> at SL_MAXQ
                 (100, 100, 99, [99, 99, 50]),  # the benchmark's shape at n = Q - 1: long augmenting paths
                 (100, 40, 64, [39, 7])]        # ldc > R - 1
TIE_QS = (64, 100, 129, 321)       # "ties" and "inf_feasible" run on these
BAD_QS = (64, 100, 129, 512)       # one problem of the launch made unsolvable, on each solver instantiation


def _assign_cases():
    cases = []
    for Q, R, ldc, n_list in ASSIGN_SHAPES:
        levels = 1 if Q >= 320 else 2
        kinds = ["grid"]
        if Q in TIE_QS:
            kinds += ["ties", "inf_feasible"]
        if Q in BAD_QS:
            kinds += list(BAD_KINDS)
        for kind in kinds:
            if (Q, R) == (100, 40) and kind != "grid":
                continue
            cases.append((f"{kind}-Q{Q}-R{R}", Q, R, ldc, n_list, levels, kind))
    return cases


ASSIGN_CASES = _assign_cases()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def bad_problem(case):
    """Index of the problem a BAD_KINDS case spoils: the first solvable image of the last level."""
    name, Q, R, ldc, n_list, levels, kind = case
    B = len(n_list)
    b = next(b for b, n in enumerate(n_list) if 0 < n <= Q)
    return (levels - 1) * B + b


def assign_problem(case):
    """cost [P, Q, ldc] float32 (problem p = level * B + image; columns >= n are NaN: the solver must not read them), the header-only
    targets t_bbox [B, R, 4] and the expected status [P]."""
    name, Q, R, ldc, n_list, levels, kind = case
    rng = _rng(name)
    B = len(n_list)
    P = levels * B
    if kind == "ties":
        cost = (rng.integers(-4, 5, size=(P, Q, ldc)) * TIES_QUANTUM).astype(np.float32)
    else:
        cost = (rng.integers(-2 ** 20, 2 ** 20 + 1, size=(P, Q, ldc)) * GRID_QUANTUM).astype(np.float32)
    status = np.zeros(P, np.int32)
    for p in range(P):
        n = n_list[p % B]
        if n > Q:
            status[p] = 2
        if kind == "inf_feasible" and 0 < n <= Q:
            hole = rng.random((Q, n)) < 0.3
            hole[np.arange(n), np.arange(n)] = False          # the diagonal stays finite: a perfect matching exists
            cost[p, :, :n][hole] = np.inf
        cost[p, :, n:] = np.nan
    if kind in BAD_KINDS:
        p = bad_problem(case)
        n = n_list[p % B]
        j = int(rng.integers(0, n))
        q = int(rng.integers(0, Q))
        if kind == "inf_infeasible":
            cost[p, :, j] = np.inf
        else:
            cost[p, q, j] = np.nan if kind == "nan" else -np.inf
        status[p] = 1
    t_bbox = np.zeros((B, R, 4), np.float32)
    t_bbox[:, 0, 0] = n_list
    return cost, t_bbox, status


def scipy_solve(cost_qn):
    """(status, pred_for_tgt [n]) of one problem the way the device reports it: 0 solved, 1 where SciPy raises, 2 for n > Q."""
    from scipy.optimize import linear_sum_assignment
    Q, n = cost_qn.shape
    if n > Q:
        return 2, None
    if n == 0:
        return 0, np.zeros(0, np.int64)
    try:
        rows, cols = linear_sum_assignment(cost_qn)
    except ValueError:
        return 1, None
    pft = np.full(n, -1, np.int64)
    pft[cols] = rows
    return 0, pft


def chosen_cost(cost_qn, pred_for_tgt):
    """Exactly rounded sum of the chosen float32 entries."""
    return math.fsum(float(cost_qn[int(q), j]) for j, q in enumerate(pred_for_tgt))


# ------------------------------------------------------------------------------------------
# loss cases: (name, Lv, B, Q, C, bg, R, n_list, layout)
# ------------------------------------------------------------------------------------------
#               Lv B  Q    C    bg   R    n_list
LOSS_SHAPES = [(1, 1, 1, 2, 1, 2, [1]),               # smallest; npos = 1
               (2, 3, 7, 2, 0, 9, [3, 0, 7]),         # bg = 0, an empty image between two others, n == Q, Q < SL_QCHUNK
               (1, 2, 9, 64, 63, 12, [9, 1]),         # C fits one lane stride exactly; Q = SL_QCHUNK + 1
               (3, 2, 17, 65, 0, 20, [17, 4]),        # one class in the second lane stride; bg = 0
               (2, 2, 100, 130, 129, 100, [99, 0]),   # C above 128 (three lane strides); an empty image last
               (1, 2, 129, 92, 91, 33, [32, 5]),      # float-tile solver; Q = 16 chunks + 1
               (6, 1, 100, 92, 91, 100, [7])]         # the benchmark's levels with B = 1
LAYOUTS = ("contiguous", "strided")
Q_SLACK, C_SLACK, BOX_SLACK = 3, 5, 2                   # "strided": views [:, :, :Q, :C] of [Lv, B, Q+3, C+5] and [..., :4] of [..., 6]
LOSS_CASES = [(f"Lv{s[0]}-B{s[1]}-Q{s[2]}-C{s[3]}-bg{s[4]}-R{s[5]}-{lay}",) + s + (lay,) for s in LOSS_SHAPES for lay in LAYOUTS]

# Gradient bounds: 2e-5 (d_logits) and 5e-5 (d_boxes) of the largest reference entry, as tests/test_gpu_kernels.py, except where the
# float32 oracle itself misses that against the float64 oracle; there 4x its measured error is allowed (another, equally valid
# float32 order of operations).  Q = 1 with the one query matched to a +8 logit: d_logits = (softmax - 1) / 1 with softmax within
# 2e-4 of 1, so with loss_scale 0.5 the largest entry is 7.7e-5 and float32 cancellation leaves 3.237e-8 of absolute error (measured, float32 torch
# oracle against the float64 one; tests/test_setloss_cases_cpu.py repeats the measurement): 20x the 1.5e-9 the relative bound gives.
D_LOGITS_F32_ORACLE_ERR = {"Lv1-B1-Q1-C2-bg1-R2": 3.237e-8}
D_LOGITS_ATOL = {k: 4 * v for k, v in D_LOGITS_F32_ORACLE_ERR.items()}

GEOMETRIES = ("clip_one", "clip_both", "disjoint", "contains", "contained", "outside")


def _forced_pair(kind, yk, jit):
    """(target, prediction) as (cx, cy, w, h) of one forced match in the left strip of the image, at height yk."""
    jx, jy, jw, jh = jit
    if kind == "clip_one":        # prediction clipped at x = 0 only
        t, p = (0.06, yk, 0.08, 0.06), (0.04 + jx, yk + 0.01 + jy, 0.10 + jw, 0.07 + jh)
    elif kind == "clip_both":     # prediction clipped at x = 0 and at x = 1
        t, p = (0.503, yk + 0.005, 0.96, 0.04), (0.5 + jx, yk + jy, 1.06 + jw, 0.05 + jh)
    elif kind == "disjoint":
        t, p = (0.05, yk, 0.06, 0.06), (0.14 + jx, yk + 0.004 + jy, 0.07 + jw, 0.05 + jh)
    elif kind == "contains":      # prediction contains its target
        t, p = (0.10, yk, 0.06, 0.05), (0.102 + jx, yk + 0.003 + jy, 0.10 + jw, 0.09 + jh)
    elif kind == "contained":     # prediction contained in its target
        t, p = (0.10, yk, 0.12, 0.10), (0.103 + jx, yk - 0.004 + jy, 0.06 + jw, 0.05 + jh)
    else:                         # "outside": wholly left of the image, clipped area 0
        t, p = (0.04, yk, 0.05, 0.05), (-0.08 + jx, yk + 0.003 + jy, 0.10 + jw, 0.06 + jh)
    return t, p


def make_targets(n_list, R, C, bg, rng):
    """oracle/set_loss_ref.make_targets with explicit n per image (0 allowed): ordinary targets in the right part of the image,
    classes drawn from [0, C) without the background class (C = 1: class 0)."""
    B = len(n_list)
    t_bbox = np.zeros((B, R, 4), np.float32)
    t_class = np.zeros((B, R, 1), np.int64)
    classes = np.array([c for c in range(C) if c != bg] or [0])
    for b, n in enumerate(n_list):
        t_bbox[b, 0, 0] = n
        t_bbox[b, 1:1 + n, 0] = rng.uniform(0.5, 0.85, n)
        t_bbox[b, 1:1 + n, 1] = rng.uniform(0.15, 0.85, n)
        t_bbox[b, 1:1 + n, 2:4] = rng.uniform(0.05, 0.25, (n, 2))
        t_class[b, 1:1 + n, 0] = rng.choice(classes, n)
    return t_bbox, t_class


def loss_inputs(case, seed=0):
    """logits [Lv, B, Q, C], boxes [Lv, B, Q, 4] float32, t_bbox [B, R, 4] float32, t_class [B, R, 1] int64 and the forced matches
    [(level, image, k, geometry)]: query k and target k of that image are made to coincide closely in class and box (so the
    matcher pairs them) in one of GEOMETRIES."""
    name, Lv, B, Q, C, bg, R, n_list, layout = case
    rng = np.random.default_rng(zlib.crc32(name.rsplit("-", 1)[0].encode()) + seed)     # both layouts share their values
    t_bbox, t_class = make_targets(n_list, R, C, bg, rng)
    logits = (rng.normal(size=(Lv, B, Q, C)) * 2).astype(np.float32)
    boxes = np.empty((Lv, B, Q, 4), np.float32)
    boxes[..., 0] = rng.uniform(0.45, 0.9, (Lv, B, Q))
    boxes[..., 1] = rng.uniform(0.1, 0.9, (Lv, B, Q))
    boxes[..., 2:] = rng.uniform(0.03, 0.4, (Lv, B, Q, 2))
    forced = []
    rot = LOSS_SHAPES.index(case[1:8]) if case[1:8] in LOSS_SHAPES else 0
    for b, n in enumerate(n_list):
        m = min(n, Q, len(GEOMETRIES))
        for k in range(m):
            kind = GEOMETRIES[(k + b + rot) % len(GEOMETRIES)]
            yk = 0.08 + 0.15 * k
            t, _ = _forced_pair(kind, yk, (0, 0, 0, 0))
            t_bbox[b, 1 + k] = t
            for lv in range(Lv):
                _, p = _forced_pair(kind, yk, rng.uniform(-0.002, 0.002, 4))
                boxes[lv, b, k] = p
                logits[lv, b, k, int(t_class[b, 1 + k, 0])] += 8.0
                forced.append((lv, b, k, kind))
    return logits, boxes, t_bbox, t_class, forced


def pair_geometry(pb, tb):
    """Facts about one matched (prediction, target) pair in the kernel's float32 corner arithmetic: the GEOMETRIES it shows and
    whether it sits off every tie of the min / max / clip / abs gradients."""
    pb, tb = np.asarray(pb, np.float32), np.asarray(tb, np.float32)
    two = np.float32(2)

    def corners(b):
        raw = np.array([b[0] - b[2] / two, b[1] - b[3] / two, b[0] + b[2] / two, b[1] + b[3] / two], np.float32)
        return raw, np.clip(raw, np.float32(0), np.float32(1))
    pr, pc = corners(pb)
    tr, tc = corners(tb)
    p_clipped = (pr < 0) | (pr > 1)
    t_clipped = (tr < 0) | (tr > 1)
    iw = min(pc[2], tc[2]) - max(pc[0], tc[0])
    ih = min(pc[3], tc[3]) - max(pc[1], tc[1])
    p_area = (pc[2] - pc[0]) * (pc[3] - pc[1])
    t_area = (tc[2] - tc[0]) * (tc[3] - tc[1])
    shows = set()
    for lo, hi in ((0, 2), (1, 3)):
        if p_clipped[lo] != p_clipped[hi]:
            shows.add("clip_one")
        if pr[lo] < 0 and pr[hi] > 1:
            shows.add("clip_both")
    if p_area > 0 and t_area > 0 and (iw <= 0 or ih <= 0):
        shows.add("disjoint")
    if pc[0] < tc[0] and pc[1] < tc[1] and pc[2] > tc[2] and pc[3] > tc[3]:
        shows.add("contains")
    if pc[0] > tc[0] and pc[1] > tc[1] and pc[2] < tc[2] and pc[3] < tc[3]:
        shows.add("contained")
    if pb[2] > 0 and pb[3] > 0 and p_area == 0 and ((pr[2] < 0) or (pr[0] > 1) or (pr[3] < 0) or (pr[1] > 1)):
        shows.add("outside")
    off_tie = bool((pb != tb).all())                                          # |p - t|
    off_tie &= bool(((pr != 0) & (pr != 1) & (tr != 0) & (tr != 1)).all())    # clip
    off_tie &= bool(((pc != tc) | (p_clipped & t_clipped)).all())             # min / max of the corners
    off_tie &= bool(iw != 0 and ih != 0)                                      # relu of the intersection
    return shows, off_tie


# ------------------------------------------------------------------------------------------
# the oracle with per-problem freedoms (torch on the CPU, float32 or float64 by the dtype of its inputs)
# ------------------------------------------------------------------------------------------
LOSS_NAMES = ("label_cost", "true_neg", "true_pos", "pos_accuracy", "giou_loss", "l1_loss")


def cost_matrix_ref(tb, tc, p_bbox, p_class):
    """oracle cost_matrix with the class probability of a target whose label lies outside [0, C) set to 0."""
    import torch
    from oracle import set_loss_ref as L
    C = p_class.shape[-1]
    valid = (tc >= 0) & (tc < C)
    if bool(valid.all()):
        return L.cost_matrix(tb, tc, p_bbox, p_class)
    p_xy = L.xcycwh_to_xy_min_xy_max(p_bbox)
    t_xy = L.xcycwh_to_xy_min_xy_max(tb)
    softmax = torch.softmax(p_class, dim=-1)
    cost_class = -softmax[:, torch.where(valid, tc, torch.zeros_like(tc)).long()] * valid.to(softmax.dtype)[None, :]
    cost_bbox = (p_bbox[:, None, :] - tb[None, :, :]).abs().sum(-1)
    cost_giou = -L.giou_matrix(p_xy, t_xy)
    return 5 * cost_bbox + 1 * cost_class + 2 * cost_giou


def oracle_match(logits, boxes, t_bbox, t_class, empty=()):
    """Per level, what get_detr_losses hands to the loss functions: (tb, tc, ti, pi, sel) over the flattened batch.  A problem
    (level, image) in `empty` is treated as if its image had no target."""
    import torch
    from oracle import set_loss_ref as L
    Lv, B, Q, _ = logits.shape
    out = []
    for lv in range(Lv):
        tbs, tcs, tis, pis, sels = [], [], [], [], []
        t_off = 0
        for b in range(B):
            tb, tc = L.strip_header(t_bbox[b], t_class[b])
            if (lv, b) in empty:
                tb, tc = tb[:0], tc[:0]
            cost = cost_matrix_ref(tb, tc, boxes[lv, b], logits[lv, b])
            rows, cols, sel = L.lsap(cost.detach().numpy())
            tis.append(torch.from_numpy(cols) + t_off)
            pis.append(torch.from_numpy(rows) + b * Q)
            sels.append(torch.from_numpy(sel))
            tbs.append(tb)
            tcs.append(tc)
            t_off += tb.shape[0]
        out.append((torch.cat(tbs), torch.cat(tcs), torch.cat(tis), torch.cat(pis), torch.cat(sels)))
    return out


def oracle_losses(logits, boxes, t_bbox, t_class, bg, empty=(), match=None):
    """oracle get_losses (levels [aux 0 .. aux Lv-2, main]) -> (total, {name + suffix: value}, match)."""
    from oracle import set_loss_ref as L
    Lv, B, Q, C = logits.shape
    match = oracle_match(logits, boxes, t_bbox, t_class, empty) if match is None else match
    losses = {}
    for lv in [Lv - 1] + list(range(Lv - 1)):
        suffix = "" if lv == Lv - 1 else f"_{lv}"
        tb, tc, ti, pi, sel = match[lv]
        vals = L.loss_labels(logits[lv].reshape(-1, C), tc, ti, pi, sel, bg) + L.loss_boxes(boxes[lv].reshape(-1, 4), tb, ti, pi)
        for name, v in zip(LOSS_NAMES, vals):
            losses[name + suffix] = v
    return L.get_total_losss(losses), losses, match
