"""The multi-label detection rule (include/detr_hip.h: detr_hip_detect_multilabel) in float64 NumPy, and the synthetic logits
the tests feed it.

topk_pairs is only valid on inputs whose order cannot depend on a last bit, and asserts that itself: distinct scores are at least
MARGIN apart and no score lies within MARGIN of the threshold.  So the logits come from GRID, the multiples of 1/16 in [-6, 6]:
adjacent grid scores differ by at least 1.59e-4 (the minimum is at the ends of the grid), plus the special values ONES (all three
give exactly 1.0f in float32 and values within 1e-8 of one another in float64: one tie class), -inf (0.0f) and NaN."""
import numpy as np

MARGIN = 1e-5
SAME = 1e-7                                          # float64 scores closer than this are one value (the ONES; exact copies)
GRID = np.arange(-96, 97) / 16.0                     # 193 logits, every one exact in float32
ONES = (20.0, 40.0, np.inf)                          # 1 / (1 + expf(-x)) == 1.0f for each
SCORE_BOUND = 1e-6                                   # the project's bound on a post-model score (tests/test_gpu_detect.py)
THRESHOLDS = (0.0, 0.5 * (1 / (1 + np.exp(1.0)) + 1 / (1 + np.exp(15 / 16))), 1.5)   # all; between two grid scores; nothing
MID = THRESHOLDS[1]


def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def topk_pairs(logits, background, threshold, K):
    """(query [n], label [n], score [n] float64) of the first K candidates of one image, logits [Q, C]: the pairs (q, c),
    c != background, with sigmoid(logits[q, c]) >= threshold (a NaN never passes), by descending score, exact ties by ascending
    flat index q * C + c; n = min(K, candidates)."""
    logits = np.asarray(logits)
    Q, C = logits.shape
    s = sigmoid64(logits)
    ok = ~np.isnan(s)
    ok[:, background] = False
    flat = np.nonzero(ok.reshape(-1))[0]
    sv = s.reshape(-1)[flat]
    # (the 0.0 of a -inf logit is exact in both precisions: it may sit ON a threshold of 0, and passes it)
    assert (np.abs(sv[sv != 0.0] - threshold) > MARGIN).all(), "a score within MARGIN of the threshold"
    flat, sv = flat[sv >= threshold], sv[sv >= threshold]
    levels = np.unique(sv)
    gaps = np.diff(levels)
    assert ((gaps < SAME) | (gaps > MARGIN)).all(), "two distinct scores closer than MARGIN"
    # scores closer than SAME are the same float32 value: tie them exactly, so that the flat index decides
    level = np.concatenate([[0], np.cumsum(gaps > MARGIN)]) if len(levels) else np.zeros(0, np.int64)
    rank = level[np.searchsorted(levels, sv)]
    order = np.argsort(-rank, kind="stable")[:K]
    return (flat[order] // C).astype(np.int32), (flat[order] % C).astype(np.int64), sv[order]


def grid_image(rng, Q, C, background):
    """Regime 0: random grid logits -- far more pairs than grid values from a few queries on, so many exact ties, also across
    the cut -- with the three-way tie at 1.0f, one NaN and one -inf placed on non-background pairs where there is room."""
    lg = rng.choice(GRID, (Q, C)).astype(np.float32)
    free = [(q, c) for q in range(Q) for c in range(C) if c != background][:: max(1, (Q * (C - 1)) // 7)]
    for (q, c), v in zip(free[::-1], ONES + (np.nan, -np.inf)):          # (with one or two pairs only the first specials fit)
        lg[q, c] = v
    return lg


def equal_image(Q, C, value=-0.5):
    """Regime 1: every logit equal -- all pairs tie and the first K flat indexes win, stepping over the background column."""
    return np.full((Q, C), value, np.float32)


def counted_image(rng, Q, C, background, j):
    """Regime 2: exactly j pairs pass MID (distinct-or-tied grid logits above -15/16), the rest are at -6."""
    lg = np.full((Q, C), -6.0, np.float32)
    pairs = [(q, c) for q in range(Q) for c in range(C) if c != background]
    assert 0 <= j <= len(pairs)
    for i in rng.choice(len(pairs), j, replace=False):
        lg[pairs[i]] = rng.choice(GRID[GRID >= -15 / 16])
    return lg
