"""Shared operands of the bf16 attention tests (tests/test_gpu_attention_dma.py, test_gpu_masked_bounds.py and the CPU self-test of
oracle/attn_bounds.py): score constructions that drive the forward's lazy reference, its recompute and the run merge, key padding
masks of every kind the masked kernels treat specially, and the device operands / launches of the all-bf16 attention core
(csrc/attention_dma.hip) with sentinels past every output."""
import math

import numpy as np
import torch

from oracle import attn_bounds as AB

DEV = "cuda"
H, HD = 8, 32
D = H * HD
SITE, STEP = 77, 0xBEEF1234
A2_SUM_LIMIT = AB.A2_SUM_LIMIT           # attention_dma.hip: a lane's 16-key sum above this moves the reference

CASES = ["uniform", "ascending", "near_limit", "descending", "distant_runs", "second_chain", "ragged_max", "dropped_dominant"]


_KEEP = {}


def keep_mask(B, T, S, p):
    """The keep bits [B*H, T, S] of (SITE, STEP) (the last few shapes cached: they are read, never written)."""
    from oracle import dropout_ref as DR
    if p == 0.0:
        return None
    key = (B, T, S, p)
    if key not in _KEEP:
        if len(_KEEP) >= 4:
            _KEEP.pop(next(iter(_KEEP)))
        _KEEP[key] = torch.from_numpy(DR.keep_mask(DR.drop_key(SITE, STEP), DR.attn_index(B * H, T, S), p))
    return _KEEP[key]


def lane_groups(S):
    """key -> lane-pair half of the forward kernel: register r of lane half hi holds key 32 t + 4 hi + (r & 3) + 8 (r >> 2)."""
    j = torch.arange(S)
    return j // 32, (j % 32 // 4) % 2


def scores_case(case, B, T, S, p, parts, keep, g, key_valid=None):
    """Head-major operands [B*H, rows, 32] whose log2-unit scores s = q . k follow the case; q is the STORED query (scale * log2 e
    already applied).  Every value is a bf16 of moderate size; every score is finite.  key_valid (bool [B, S], masked cases only)
    leaves the constructions of the valid keys as they are; masked K / V rows keep non-zero content, and "masked_dominant" gives
    the masked keys scores about 30 log2 units above every valid key."""
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    BH = B * H
    q = 0.3 * rn(BH, T, HD)
    k = rn(BH, S, HD)
    v = rn(BH, S, HD)
    tile = torch.arange(S, dtype=torch.float64) // 32
    if case == "uniform":                          # O = mean of the kept V, lse = log S
        q.zero_()
    elif case == "ascending":                      # +13 log2 units per key tile: the reference moves (tile recomputed) on every tile
        k[:, :, :8] = (tile / 4).view(1, S, 1)
        q[:, :, :8] = 6.5
        q[:, :, 8:] *= 1.0 / 6
    elif case == "near_limit":                     # one key per 16-key lane group 11.5 above the first tile: lane sums near 4096
        j = torch.arange(S)
        high = ((j % 32 == 0) | (j % 32 == 4)) & (j >= 32)
        k[:, :, 0] = 1.0
        k[:, :, 1] = high.double().view(1, S)
        q[:, :, 0] = 3.0 * torch.rand(BH, T, dtype=torch.float64, generator=g) - 1.5
        q[:, :, 1] = 11.5
        q[:, :, 2:] *= 1.0 / 30
    elif case == "descending":                     # 60 .. -60 log2 units: early tiles dominate, late ones vanish
        r = 1.0 - 2.0 * torch.arange(S, dtype=torch.float64) / max(S - 1, 1)
        k[:, :, :8] = (4.0 * r).view(1, S, 1)
        q[:, :, :8] = 60.0 / 32.0
        q[:, :, 8:] *= 1.0 / 30
    elif case == "distant_runs":                   # each row's maximum in its own run, the next run 20 lower, the rest 40 lower
        rr = AB.runs(S, parts)
        k[:, :, :8] = 0.0
        for r, (j0, j1) in enumerate(rr):
            k[:, j0:j1, r] = 1.0
        n = len(rr)
        i = torch.arange(T)
        q[:, :, :8] = 0.0
        q[:, i, i % n] = 40.0
        if n > 1:
            q[:, i, (i + 1) % n] = 20.0
    elif case == "second_chain":                   # peaked rows only in the second 32 queries of each 64
        q = rn(BH, T, HD)
        q[:, torch.arange(T) % 64 < 32] = 0.0
    elif case == "ragged_max":                     # every row's maximum is the last key (the ragged last tile), 20 above the rest
        k[:, :, 0] = 0.0
        k[:, S - 1, 0] = 1.0
        q[:, :, 0] = 20.0
    elif case == "dropped_dominant":               # the dominant key of a row (15 above the rest) is one the row drops
        cand = torch.tensor([m * S // 16 for m in range(16)])
        k[:, :, :16] = 0.0
        k[:, cand, torch.arange(16)] = 1.0
        q[:, :, :16] = 0.0
        kc = keep[:, :, cand]                                                     # [BH, T, 16]
        dropped = ~kc
        m = torch.where(dropped.any(dim=2), dropped.double().argmax(dim=2), torch.zeros(BH, T, dtype=torch.long))
        q.scatter_(2, m.unsqueeze(2), 15.0)
        assert float(dropped.any(dim=2).double().mean()) > 0.5
    elif case == "masked_dominant":                # every masked key ~30 log2 units above every valid key (finite bf16 scores)
        inv = ~torch.as_tensor(key_valid).bool().repeat_interleave(H, dim=0)                      # [BH, S]
        k[:, :, 0] = inv.double()
        q[:, :, 0] = 44.0                          # valid scores: 31 terms of 0.3 N(0,1) N(0,1) (|.| < 12); masked: 44 + that
    else:
        raise ValueError(case)
    unh = lambda x: AB.bf16(AB.unheads(x, B, H))
    return unh(q), unh(k), unh(v), AB.bf16(rn(B, T, D))


def assert_below_sum_limit(qs, k, B, T, S, p, parts, key_valid=None):
    """The near-limit inputs keep every lane's 16-key sum of exp2(score - reference) (reference = the maximum of the run's first tile
    with a valid key, shifted by log2 of the dropout scale as in the kernel) below A2_SUM_LIMIT in every tile, and some come within a
    factor 2 of it.  key_valid: only valid keys count."""
    lg2scale = -np.log2(1.0 - p) if p > 0.0 else 0.0
    tile, half = lane_groups(S)
    qh, kh = AB.heads(qs, H), AB.heads(k, H)
    worst = 0.0
    for bh in range(B * H):
        s = qh[bh] @ kh[bh].T
        if key_valid is not None:
            s = s.masked_fill(~torch.as_tensor(key_valid)[bh // H].bool().unsqueeze(0), -math.inf)
        for j0, j1 in AB.runs(S, parts):
            first = next((t for t in range(j0, j1, 32) if bool(torch.isfinite(s[0, t:min(j1, t + 32)]).any())), None)
            if first is None:
                continue                                   # a run without a valid key computes nothing
            m0 = s[:, first:min(j1, first + 32)].max(dim=1, keepdim=True).values
            e = torch.exp2(s[:, first:j1] - m0 + lg2scale)
            grp = (tile[first:j1] - tile[first]) * 2 + half[first:j1]
            sums = torch.zeros(T, int(grp.max()) + 1, dtype=torch.float64).index_add_(1, grp, e)
            worst = max(worst, float(sums.max()))
    assert worst < A2_SUM_LIMIT, f"near-limit inputs cross the sum limit ({worst:.1f})"
    assert worst > A2_SUM_LIMIT / 2, f"near-limit inputs stay far from the sum limit ({worst:.1f})"
    return worst


# ------------------------------------------------------------------------------------------------------------------------------
# key padding masks: bool [B, S], True = valid key, different for every batch element, every image with a valid key
# ------------------------------------------------------------------------------------------------------------------------------
GRIDS = {333: (9, 37), 700: (20, 35), 1050: (25, 42), 1344: (32, 42), 2100: (50, 42), 8192: (64, 128)}
MASKS = ["rect", "random", "tiles", "first_half", "run_heads", "empty_runs_last", "empty_runs_first", "single_valid", "far_tiles"]


def far_tile_word(b, t):
    """A distinct word per (b, t): all valid when t % 5 == 0, all masked when t % 5 == 1, a mixed hash of (b, t) otherwise -- so
    tiles t, t +- 1 and t +- 64 (64 % 5 = 4) always differ."""
    if t % 5 == 0:
        return 0xFFFFFFFF
    if t % 5 == 1:
        return 0
    x = (t * 0x9E3779B1 + (b + 1) * 0x85EBCA77) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x ^= x >> 12
    return x if x not in (0, 0xFFFFFFFF) else 0x0F0F0F0F ^ t


def key_valid(kind, B, S, parts=1, seed=0, grid=None):
    """The mask kinds of the masked bf16 / fp32 tests.  parts: runs per workgroup of the split under test (run_heads, empty_runs_*).
        rect              a rectangle on the feature grid (GRIDS[S] or `grid`), as padding_mask_prepare produces
        random            60 % valid
        tiles             alternate whole 32-key tiles masked (tile 0 among them for element 0)
        first_half        the first half of the keys (+ 7 + 5 b) masked
        run_heads         every run: two fully masked tiles, then a partial one (sets `fresh`), then 60 % valid
        empty_runs_last   only the last run holds valid keys (empty runs merged before a real one)
        empty_runs_first  only run 0 holds valid keys (empty runs merged after it)
        single_valid      one valid key per image, in the (ragged) last tile
        far_tiles         far_tile_word(b, t) for every tile (all-valid, all-masked and mixed words, far past tile 64)"""
    rng = np.random.default_rng(seed + 7919 * S)
    v = np.zeros((B, S), bool)
    ntiles = -(-S // 32)
    rr = AB.runs(S, parts)
    for b in range(B):
        if kind == "rect":
            Hf, Wf = grid or GRIDS[S]
            assert Hf * Wf == S
            fr = [(0.72, 0.7), (1.0, 0.48), (0.5, 1.0)][b % 3]
            g = np.zeros((Hf, Wf), bool)
            g[:max(1, math.ceil(fr[0] * Hf) - b // 3), :max(1, math.ceil(fr[1] * Wf))] = True
            v[b] = g.reshape(-1)
        elif kind == "random":
            v[b] = rng.random(S) < 0.6
        elif kind == "tiles":
            v[b] = True
            for t in range(b % 2, ntiles, 2):
                v[b, 32 * t:32 * t + 32] = False
        elif kind == "first_half":
            v[b] = True
            v[b, :min(S - 1, S // 2 + 7 + 5 * b)] = False
        elif kind == "run_heads":
            v[b] = rng.random(S) < 0.6
            for j0, j1 in rr:
                v[b, j0:min(j1, j0 + 64)] = False
                if j0 + 64 < j1:
                    part = np.zeros(min(j1, j0 + 96) - (j0 + 64), bool)
                    part[rng.choice(part.size, max(1, part.size // 3), replace=False)] = True
                    if part.all() and part.size > 1:
                        part[0] = False
                    v[b, j0 + 64:j0 + 64 + part.size] = part
        elif kind in ("empty_runs_last", "empty_runs_first"):
            j0, j1 = rr[-1] if kind == "empty_runs_last" else rr[0]
            v[b, j0:j1] = rng.random(j1 - j0) < 0.6
        elif kind == "single_valid":
            last0 = 32 * (ntiles - 1)
            v[b, last0 + (5 * b + 3) % (S - last0)] = True
        elif kind == "far_tiles":
            assert S > 2048
            bits = np.array([[(far_tile_word(b, t) >> i) & 1 for i in range(32)] for t in range(ntiles)], bool)
            v[b] = bits.reshape(-1)[:S]
        else:
            raise ValueError(kind)
        if not v[b].any():
            v[b, S - 1] = True
    return v


# ------------------------------------------------------------------------------------------------------------------------------
# device operands and launches
# ------------------------------------------------------------------------------------------------------------------------------
def device_operands(hip, qs, k, v, do, B, T, S, p, extra=0, key_valid=None):
    """bf16 device copies; outputs (and the lse / delta scratch) with `extra` trailing sentinel rows / entries.  key_valid (bool
    [B, S]): the masked kernels, with the validity words followed by `extra` all-ones sentinel words that must never be read."""
    d = lambda t: t.to(torch.bfloat16).reshape(-1, D).to(DEV)
    dev = dict(q=d(qs), k=d(k), v=d(v), do=d(do))
    sent = lambda rows: torch.full((rows + extra, D), -1234.0, dtype=torch.bfloat16, device=DEV)
    dev["o"], dev["dq"], dev["dk"], dev["dv"] = sent(B * T), sent(B * T), sent(B * S), sent(B * S)
    dev["lse"] = torch.full((B * H * T + extra,), -4321.0, device=DEV)
    dev["delta"] = torch.full((2 * B * H * T + extra,), -4321.0, device=DEV)
    stepd = torch.tensor([STEP - (1 << 32)] + [0] * 7, dtype=torch.int32, device=DEV)
    dev["kw"] = dict(scale=HD ** -0.5, dropout_p=p, dropout_site=SITE, dropout_step=stepd, dropmask=None)
    if p > 0.0:
        mask = torch.zeros(hip.attention_dropmask_words(B, H, T, S), dtype=torch.int32, device=DEV)
        hip.attention_dropmask(mask, B, H, T, S, dropout_p=p, dropout_site=SITE, dropout_step=stepd)
        dev["kw"]["dropmask"] = mask
    if key_valid is not None:
        words = torch.from_numpy(hip.keymask_words_from_valid(np.asarray(key_valid))).reshape(-1)
        dev["kw"]["key_valid"] = torch.cat([words, torch.full((extra,), -1, dtype=torch.int32)]).to(DEV)
    return dev


def fwd(hip, dev, B, T, S, split, o=None, lse=None):
    o = dev["o"] if o is None else o
    lse = dev["lse"] if lse is None else lse
    hip.set_tuning("DETR_HIP_ATTN_SPLIT", split if split else None)
    try:
        hip.attention(dev["q"], dev["k"], dev["v"], o[:B * T], lse, B, H, T, S, **dev["kw"])
        torch.cuda.synchronize()
    finally:
        hip.set_tuning("DETR_HIP_ATTN_SPLIT", None)


def bwd(hip, dev, B, T, S, split, o, lse):
    hip.set_tuning("DETR_HIP_ATTN_SPLIT", split if split else None)
    try:
        hip.attention(dev["q"], dev["k"], dev["v"], o[:B * T], lse, B, H, T, S, d_o=dev["do"], dq=dev["dq"][:B * T],
                      dk=dev["dk"][:B * S], dv=dev["dv"][:B * S], delta=dev["delta"], **dev["kw"])
        torch.cuda.synchronize()
    finally:
        hip.set_tuning("DETR_HIP_ATTN_SPLIT", None)


def check(what, got, ref, bound):
    r = AB.ratio(got, ref, bound)
    assert r <= 1.0, f"{what}: max |err| / bound = {r:.3f} > 1"
    return r


def all_outputs(hip, dev, B, T, S, split):
    fwd(hip, dev, B, T, S, split)
    bwd(hip, dev, B, T, S, split, dev["o"], dev["lse"])
    return {n: dev[n].clone() for n in ("o", "lse", "dq", "dk", "dv", "delta")}


def sentinels_intact(dev, B, T, S, extra):
    for n, rows in (("o", B * T), ("dq", B * T), ("dk", B * S), ("dv", B * S)):
        assert bool((dev[n][rows:] == -1234.0).all()), f"{n}: sentinel rows overwritten"
        assert bool(torch.isfinite(dev[n][:rows].float()).all()), f"{n}: not finite"
    assert bool((dev["lse"][B * H * T:] == -4321.0).all()), "lse: sentinel entries overwritten"
    assert bool((dev["delta"][2 * B * H * T:] == -4321.0).all()), "delta: sentinel entries overwritten"
