"""ORACLE (test infrastructure only) -- fp64 reference of the all-bf16 attention core (csrc/attention_dma.hip, io_dtype = 1) with a
PER-ELEMENT error bound for every output, built by carrying absolute values through the computation (running-error analysis).

Operands are the ones the kernels read: bf16 values held in float64, q already carrying scale * log2(e) (the stored query, so a score
s = q . k is in log2 units), k, v, dO as [B, rows, H * 32].  A kernel result X passes when max |X - X_ref| / B_X <= 1 (ratio()).

Units.  u = 2^-8 is the unit roundoff of bf16 (8 significand bits, round to nearest even: |bf16(x) - x| <= 2^-8 |x|).  f = 2^-23 is
charged for every fp32 operation: twice the fp32 unit roundoff 2^-24, so that it also covers round-toward-zero accumulation inside an
MFMA and the <= 1 ulp error of v_exp_f32 / v_log_f32 / logf.  A sum of n terms formed in fp32 (any order) is charged n f times the sum
of the absolute values of its terms.  All bounds are first order in u and f; the factor (1 + 2u) on each bound covers the second-order
products (u^2, u f, ...), each at most 2u of its first-order term.

Where the kernels round (attention_dma.hip), and what each rounding costs:

* Score (all three kernels): s' = fp32(sum_32 q_d k_d + C), C = -M (forward, M the lazy reference) or -Lq (backward).  The 32 bf16
  products are exact in fp32, so |s' - (s + C)| <= 34 f (sum_d |q_d k_d| + |C|) =: E_s, with |C| <= R_i = max_j |s_ij| +
  log2(e) |lse_i| + 2 (a reference is a tile maximum or the row's log-sum-exp, shifted by log2 of the dropout scale < 1).
  An exponential of it then has relative error  e_j = ln2 E_s + f  (v_exp_f32).
* Forward.  o = sum_j keep_j bf16(p_j) v_j accumulated in fp32 (at most S adds into one register, ceil(S/32) rescalings by
  exp2(-d), 2 per merged run), l = sum_j p_j in fp32 from the UNROUNDED p (16-key tree: 4, lane pair: 1, per tile: 1, rescale: 1,
  merge: 2 per run), O = bf16(o * (dsc / l)).  The rescale factors multiply o and l alike and cancel in o / l; only their roundings
  count.  With W = keep * P / (1 - p) (the exact weights), Pv = W |V|:
      |o/l - O| <= u Pv + (1+u) (W e) |V| + (S + ntiles + 2 NP + 2) f Pv + (sum_j P_j e_j + (5 + 2 ntiles + 2 NP) f + 3 f) |O|
  (the u term: bf16(p); 3 f: 1 / (1 - p), the division, the product), and the store adds u |O|:
      B_O = (1 + 2u) (u |O| + |o/l - O|-bound)                                           c_o = 1 (u |O|) + 1 (u Pv) + fp32 terms
* LSE (fp32, natural log): lse' = fp32(M ln2 + logf(l / dsc)).  The relative error of l (above) enters as an absolute one; M ln2, the
  logf and the final add each cost f times a magnitude <= R_i + |lse| + 1; log2f(dsc) then exp2 of it inside every p and the
  division by dsc cost 8 f:
      B_lse = (1 + 2u) (sum_j P_j e_j + (5 + 2 ntiles + 2 NP) f + f (3 R_i + |lse_i|) + 8 f)
* Backward.  delta_i = sum_c dO_ic O'_ic with O' the forward's STORED bf16 output (what the kernels read; pass it as o_kernel), so
  delta carries no bf16 error: 32 products, 33 f G_i with G_i = sum_c |dO_ic O'_ic|, and / dsc costs f |delta|.  dP = dO V^T in fp32:
  32 f Hd with Hd = |dO| |V|^T.  P' = exp2(s' - Lq) with Lq = fp32(lse' log2 e) - log2 dsc: relative error
      e_P = B_lse + ln2 (E_s + 2 f log2(e) |lse| + f) + f.
  dS = P (keep dsc dP - delta) = P D, formed in fp32 (subtraction, product / fma: 2 f |dS|) and stored bf16 before both products:
      B_dS = u |dS| + (1+u) ((e_P + 2 f) |dS| + P (keep dsc 32 f Hd + 33 f G + f |delta| + f |D|))     c_S = 1
  dQ = scale dS K (gradient of the UNSCALED q; sum of S bf16 products plus NP merged partial sums in fp32, times qscale: 2 f),
  dK = ln2 dS^T Q' (T products + NP, times ln2: 2 f), dV = bf16(W')^T dO with W' the kernel's keep-masked p (B_W = u W + (1+u) e_P W):
      B_dQ = (1 + 2u) (u |dQ| + scale B_dS |K| + (S + NP + 2) f scale |dS| |K| + 2 f |dQ|)        c_Q = 1 (own store) + 1 (B_dS)
      B_dK = (1 + 2u) (u |dK| + ln2 B_dS^T |Q'| + (T + NP + 2) f ln2 |dS|^T |Q'| + 2 f |dK|)
      B_dV = (1 + 2u) (u |dV| + B_W^T |dO| + (T + NP) f W^T |dO|)                                   c_V = 1 + 1
NP = 8 is the largest number of runs per workgroup (the bounds hold for every DETR_HIP_ATTN_SPLIT).  Nothing here is fitted to a
measurement: every constant is a count of roundings.

Key padding mask (key_valid: bool [B, S], True = valid key; the MASK instantiations of the three kernels).  A masked key is exactly
absent: its score is set to -inf before anything is formed from it, so P = 0 there and m, l and lse run over the valid keys only.
The reference therefore zeroes the K and V rows of masked keys before it forms anything: every magnitude a bound is built from
(R, sum_d |q_d k_d|, |V|, Hd = |dO| |V|^T) then runs over valid keys alone, garbage in a masked row cannot loosen a bound, and the
bounds are bit-identical for any content of the masked rows.  The derivation is unchanged: a masked key adds no term to any sum
above (its P, W and dS are exact zeros, and a tile without a valid key is skipped whole), so each rounding count is at most the
unmasked one, and S, ntiles and NP stay valid upper bounds -- they are kept, not refitted.  The kernels store exact zeros in dK and
dV at masked keys, so their bound there is 0: ratio() accepts only an exact 0.  Every image needs at least one valid key (the
product rejects such masks; asserted here).

simulate() is one admissible execution of the documented roundings (bf16 P before PV, l from the unrounded p, runs merged with their
own maxima, bf16 dS / outputs, delta from the bf16 O) with optional injected faults; tests/test_attn_bounds_cpu.py uses it to show
that the bounds accept a correct kernel and reject subtly wrong ones."""
import math

import torch

U = 2.0 ** -8            # bf16 unit roundoff
F = 2.0 ** -23           # charge per fp32 operation (see above)
NP = 8                   # runs per workgroup, at most
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
TINY = 2.0 ** -120       # fp32 underflow of an exponential / a denormal store
HD = 32


def heads(x, H):
    """[B, N, H*32] -> [B*H, N, 32]"""
    B, N, D = x.shape
    return x.reshape(B, N, H, D // H).permute(0, 2, 1, 3).reshape(B * H, N, D // H)


def unheads(x, B, H):
    """[B*H, N, 32] -> [B, N, H*32]"""
    BH, N, hd = x.shape
    return x.reshape(B, H, N, hd).permute(0, 2, 1, 3).reshape(B, N, H * hd)


def bf16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def parts_for(tiles, split=0):
    """Runs per workgroup the host picks (attention_dma.hip a2_parts): 4, or the forced DETR_HIP_ATTN_SPLIT, capped at tiles // 4."""
    p = split if 1 <= split <= 8 else 4
    return max(1, min(p, tiles // 4 if tiles >= 4 else 1))


def runs(n, parts):
    """Key ranges [j0, j1) of the runs of one workgroup over a stream of n rows (32-row tiles split evenly; trailing runs may be empty)."""
    ntiles = -(-n // 32)
    nth = -(-ntiles // parts)
    out = []
    for kp in range(parts):
        t0, t1 = kp * nth, min(ntiles, kp * nth + nth)
        if t1 > t0:
            out.append((32 * t0, min(n, 32 * t1)))
    return out


def _dsc(p):
    return 1.0 / (1.0 - p) if p > 0.0 else 1.0


def _valid(key_valid, B, S):
    """bool [B, S] (every image with a valid key) or None."""
    if key_valid is None:
        return None
    kv = torch.as_tensor(key_valid).bool()
    assert tuple(kv.shape) == (B, S), f"key_valid must be [B, S] = [{B}, {S}], got {tuple(kv.shape)}"
    assert bool(kv.any(dim=1).all()), "every image needs at least one valid key"
    return kv


def _absent(x, kv):
    """x [B, S, D] with the rows of masked keys zeroed: nothing of their content reaches a value or a bound."""
    return x if kv is None else x * kv.unsqueeze(2).to(x.dtype)


def _problem_fwd(q, k, v, keep, dsc, valid=None):
    s = q @ k.T
    if valid is not None:
        s = s.masked_fill(~valid.unsqueeze(0), -math.inf)
    m = s.max(dim=1, keepdim=True).values
    e = torch.exp2(s - m)
    l = e.sum(dim=1, keepdim=True)
    P = e / l
    lse = (m + torch.log2(l)).squeeze(1) * LN2
    W = P * (keep * dsc) if keep is not None else P
    return s, P, W, lse


def _exp_err(q, k, s, lse):
    """(k: masked rows already zero; s: -inf at masked keys, which are left out of R)"""
    R = torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s)).max(dim=1, keepdim=True).values + LOG2E * lse.abs().unsqueeze(1) + 2.0
    Es = 34.0 * F * (q.abs() @ k.abs().T + R)
    return R, LN2 * Es + F


def forward(qs, k, v, H, keep=None, p=0.0, key_valid=None):
    """Exact O [B, T, D], lse [B*H, T] and their bounds.  keep: bool [B*H, T, S] or None; key_valid: bool [B, S] or None."""
    B, T, _ = qs.shape
    S = k.shape[1]
    dsc = _dsc(p)
    kv = _valid(key_valid, B, S)
    k, v = _absent(k, kv), _absent(v, kv)
    ntiles = -(-S // 32)
    qh, kh, vh = heads(qs, H), heads(k, H), heads(v, H)
    O, BO, L, BL = (torch.empty(B * H, T, HD, dtype=torch.float64), torch.empty(B * H, T, HD, dtype=torch.float64),
                    torch.empty(B * H, T, dtype=torch.float64), torch.empty(B * H, T, dtype=torch.float64))
    for bh in range(B * H):
        kp = keep[bh].double() if keep is not None else None
        s, P, W, lse = _problem_fwd(qh[bh], kh[bh], vh[bh], kp, dsc, None if kv is None else kv[bh // H])
        R, e = _exp_err(qh[bh], kh[bh], s, lse)
        o = W @ vh[bh]
        Pv = W @ vh[bh].abs()
        den = (P * e).sum(dim=1, keepdim=True) + (5 + 2 * ntiles + 2 * NP) * F
        pre = U * Pv + (1 + U) * ((W * e) @ vh[bh].abs()) + (S + ntiles + 2 * NP + 2) * F * Pv + (den + 3 * F) * o.abs()
        O[bh], L[bh] = o, lse
        BO[bh] = (1 + 2 * U) * (U * o.abs() + pre) + TINY
        BL[bh] = (1 + 2 * U) * (den.squeeze(1) + F * (3 * R.squeeze(1) + lse.abs()) + 8 * F)
    return dict(o=unheads(O, B, H), lse=L, bound_o=unheads(BO, B, H), bound_lse=BL)


def backward(qs, k, v, do, o_kernel, H, keep=None, p=0.0, scale=HD ** -0.5, key_valid=None):
    """Exact dQ (w.r.t. the unscaled q = qs / (scale log2 e)) [B, T, D], dK, dV [B, S, D] and their bounds.  delta is formed from
    o_kernel, the bf16 O the forward stored.  key_valid: bool [B, S] or None (masked keys: dK = dV = 0 with bound 0)."""
    B, T, _ = qs.shape
    S = k.shape[1]
    dsc = _dsc(p)
    kv = _valid(key_valid, B, S)
    k, v = _absent(k, kv), _absent(v, kv)
    ntiles = -(-S // 32)
    qh, kh, vh, dh, oh = heads(qs, H), heads(k, H), heads(v, H), heads(do, H), heads(o_kernel, H)
    z = lambda n: torch.empty(B * H, n, HD, dtype=torch.float64)
    dQ, BdQ, dK, BdK, dV, BdV = z(T), z(T), z(S), z(S), z(S), z(S)
    for bh in range(B * H):
        kp = keep[bh].double() if keep is not None else None
        q, kk, vv, dO = qh[bh], kh[bh], vh[bh], dh[bh]
        s, P, W, lse = _problem_fwd(q, kk, vv, kp, dsc, None if kv is None else kv[bh // H])
        R, e = _exp_err(q, kk, s, lse)
        den = (P * e).sum(dim=1, keepdim=True) + (5 + 2 * ntiles + 2 * NP) * F
        blse = (1 + 2 * U) * (den + F * (3 * R + lse.abs().unsqueeze(1)) + 8 * F)
        eP = blse + (e - F) + LN2 * (2 * F * LOG2E * lse.abs().unsqueeze(1) + F) + F        # e - F = ln2 E_s
        kd = kp * dsc if kp is not None else torch.ones_like(s)
        delta = (dO * oh[bh]).sum(dim=1, keepdim=True)
        G = (dO * oh[bh]).abs().sum(dim=1, keepdim=True)
        dP = dO @ vv.T
        Hd = dO.abs() @ vv.abs().T
        D = kd * dP - delta
        dS = P * D
        errD = kd * 32 * F * Hd + 33 * F * G + F * delta.abs() + F * D.abs()
        BdS = U * dS.abs() + (1 + U) * ((eP + 2 * F) * dS.abs() + P * errD)
        dq = scale * (dS @ kk)
        dQ[bh] = dq
        BdQ[bh] = (1 + 2 * U) * (U * dq.abs() + scale * (BdS @ kk.abs()) + (S + NP + 2) * F * scale * (dS.abs() @ kk.abs())
                                 + 2 * F * dq.abs()) + TINY
        dk = LN2 * (dS.T @ q)
        dK[bh] = dk
        BdK[bh] = (1 + 2 * U) * (U * dk.abs() + LN2 * (BdS.T @ q.abs()) + (T + NP + 2) * F * LN2 * (dS.abs().T @ q.abs())
                                 + 2 * F * dk.abs()) + TINY
        dv = W.T @ dO
        BW = U * W + (1 + U) * eP * W
        dV[bh] = dv
        BdV[bh] = (1 + 2 * U) * (U * dv.abs() + BW.T @ dO.abs() + (T + NP) * F * (W.T @ dO.abs())) + TINY
        if kv is not None:                   # masked keys: exact zeros (dS and W vanish there), nothing else is accepted
            BdK[bh][~kv[bh // H]] = 0.0
            BdV[bh][~kv[bh // H]] = 0.0
    return dict(dq=unheads(dQ, B, H), dk=unheads(dK, B, H), dv=unheads(dV, B, H),
                bound_dq=unheads(BdQ, B, H), bound_dk=unheads(BdK, B, H), bound_dv=unheads(BdV, B, H))


def ratio(got, ref, bound):
    """max |got - ref| / bound (a NaN anywhere counts as infinitely wrong; where the bound is 0 -- dK / dV of a masked key -- only an
    exact match passes: 0 / 0 counts as 0, anything else as infinitely wrong)."""
    d = (got.detach().cpu().double() - ref).abs()
    if bool(torch.isnan(d).any()):
        return math.inf
    zero = bound == 0
    if bool((d[zero] != 0).any()):
        return math.inf
    err = d / torch.where(zero, torch.ones_like(bound), bound)
    return float(err.max())


A2_SUM_LIMIT = 4096.0     # attention_dma.hip: a 16-key lane sum above this moves the forward's lazy reference
M_EMPTY = -1.0e30         # attention_dma.hip A2_M_EMPTY: the reference a run without a valid key merges with


def _lane_half(j):
    """Lane half of the bf16 forward that holds key j of its tile: register r of half hi holds key 4 hi + (r & 3) + 8 (r >> 2)."""
    return (j % 32 // 4) % 2


def _faulty_valid(val, kind, fault, S):
    """The validity a faulty masked kernel would apply in the forward and the dQ kernel (see simulate())."""
    val = val.clone()
    ntiles = -(-S // 32)
    bits = torch.zeros(ntiles * 32, dtype=torch.bool)
    bits[:S] = val
    words = bits.view(ntiles, 32)
    if kind == "leak_key":
        j = fault[2]
        assert not bool(val[j]) and bool(words[j // 32].any()), "leak_key: key j must be a masked key in a partial word"
        val[j] = True
    elif kind in ("mask_shift", "mask_half", "word_from"):
        t = fault[2]
        w = words[t].clone()
        if kind == "mask_shift":                 # key i of the tile takes the bit of key i - 1 (key 0: key 31's)
            nw = torch.roll(w, 1)
        elif kind == "mask_half":                # the lane half 1 keys (4-7, 12-15, ...) take the bits of the keys 4 lower
            i = torch.arange(32)
            nw = torch.where(_lane_half(i) == 1, w[(i - 4) % 32], w)
        else:
            nw = words[fault[3]].clone()
        assert not torch.equal(nw, w), f"{kind}: the fault leaves tile {t} unchanged"
        words[t] = nw
        val = words.reshape(-1)[:S].clone()
    return val


def _sim_fwd_masked(q, kk, vv, val, kdx, parts, T, S):
    """The masked forward of one problem: fully masked tiles skipped, each run's reference the maximum of its first tile with a valid
    key (moved up when a 32-key sum leaves the safe range, as the kernel does), runs without one merged as (M_EMPTY, 0, 0)."""
    s = (q @ kk.T).float().double()
    o = torch.zeros(T, HD, dtype=torch.float64)
    l = torch.zeros(T, 1, dtype=torch.float64)
    mn = torch.full((T, 1), -math.inf, dtype=torch.float64)
    for r, (j0, j1) in enumerate(runs(S, parts)):
        orun, lrun, m = torch.zeros(T, HD, dtype=torch.float64), torch.zeros(T, 1, dtype=torch.float64), None
        for lo in range(j0, j1, 32):
            hi_ = min(j1, lo + 32)
            vt = val[lo:hi_]
            if not bool(vt.any()):
                continue                                                  # no valid key: skipped
            st = s[:, lo:hi_].masked_fill(~vt.unsqueeze(0), -math.inf)
            if m is None:
                m = st.max(dim=1, keepdim=True).values                    # `fresh`: the first tile with a valid key
            e = torch.exp2(st - m).float().double()
            big = e.sum(dim=1, keepdim=True) > A2_SUM_LIMIT
            if bool(big.any()):
                d = torch.where(big, (st.max(dim=1, keepdim=True).values - m).clamp(min=0.0), torch.zeros_like(m))
                c = torch.exp2(-d)
                orun, lrun, m = orun * c, lrun * c, m + d
                e = torch.exp2(st - m).float().double()
            pb = bf16(e) * kdx[:, lo:hi_]
            orun = orun + pb @ vv[lo:hi_]
            lrun = lrun + e.sum(dim=1, keepdim=True)
        if m is None:
            m = torch.full((T, 1), M_EMPTY, dtype=torch.float64)
        new = torch.maximum(mn, m)
        ca, cb = torch.exp2(mn - new), torch.exp2(m - new)
        o = o * ca + orun * cb
        l = l * ca + lrun * cb
        mn = new
    return o, l, mn


def simulate(qs, k, v, do, H, keep=None, p=0.0, parts=4, scale=HD ** -0.5, fault=None, key_valid=None):
    """One execution of the documented roundings (see the module docstring), optionally with a fault:
        ("drop_tile", bh, t)        key tile t of problem bh left out of the softmax
        ("pad_from_next", bh)       the padding keys of the ragged last tile of problem bh taken from the next batch element
        ("chain_scale", bh, x0)     the P of queries x0 .. x0 + 31 of problem bh scaled by 1 + 2^-6 before the PV product
        ("delta", bh)               delta of problem bh off by 1 %
        ("merge", bh, r, w)         run r of problem bh weighted by w in the merge
    With key_valid (bool [B, S]) it follows the masked kernels instead (_sim_fwd_masked; the dQ kernel selects dS = 0 at masked keys,
    the dK / dV kernel stores exact zeros there), and these faults apply to the validity the forward and the dQ kernel see:
        ("leak_key", bh, j)         masked key j (in a partial word) treated as valid
        ("mask_shift", bh, t)       tile t's word applied one key off (key i takes the bit of key i - 1)
        ("mask_half", bh, t)        tile t's lane half 1 keys take the bits of lane half 0 (the `>> (4 * hi)` dropped)
        ("word_from", bh, t, u)     tile t uses the validity word of tile u
        ("masked_dkv", bh)          masked keys get the dK / dV a valid key would (no zeroing at the store)
    Returns o, lse (forward) and dq, dk, dv (backward, delta from the simulated bf16 O)."""
    B, T, _ = qs.shape
    S = k.shape[1]
    dsc = _dsc(p)
    kind = fault[0] if fault else None
    kvm = _valid(key_valid, B, S)
    qh, kh, vh, dh = heads(qs, H), heads(k, H), heads(v, H), heads(do, H)
    O, L = torch.empty(B * H, T, HD, dtype=torch.float64), torch.empty(B * H, T, dtype=torch.float64)
    dQ, dK, dV = torch.empty(B * H, T, HD, dtype=torch.float64), torch.empty(B * H, S, HD, dtype=torch.float64), \
        torch.empty(B * H, S, HD, dtype=torch.float64)
    for bh in range(B * H):
        hit = fault is not None and fault[1] == bh
        q, kk, vv = qh[bh], kh[bh], vh[bh]
        kd = keep[bh].double() * dsc if keep is not None else torch.ones(T, S, dtype=torch.float64)
        if kvm is not None:
            val = kvm[bh // H]
            vf = _faulty_valid(val, kind, fault, S) if hit else val
            o, l, mn = _sim_fwd_masked(q, kk, vv, vf, kd, parts, T, S)
            O[bh] = bf16(o / l)
            L[bh] = (mn.squeeze(1) * LN2 + torch.log(l.squeeze(1))).float().double()
            s = (q @ kk.T).float().double()
            P = torch.exp2(s - LOG2E * L[bh].unsqueeze(1)).float().double()      # (the dK / dV kernel: every key)
            delta = (dh[bh] * O[bh]).sum(dim=1, keepdim=True).float().double()
            dS = bf16(P * (kd * (dh[bh] @ vv.T) - delta))
            dQ[bh] = bf16(scale * (dS.masked_fill(~vf.unsqueeze(0), 0.0) @ kk))
            dK[bh] = bf16(LN2 * (dS.T @ q))
            dV[bh] = bf16(bf16(P * kd).T @ dh[bh])
            if not (hit and kind == "masked_dkv"):
                dK[bh][~val] = 0.0
                dV[bh][~val] = 0.0
            continue
        kx, vx, kdx = kk, vv, kd
        if hit and kind == "pad_from_next":
            npad = -S % 32
            assert npad > 0 and bh + H < B * H
            kx = torch.cat([kk, kh[bh + H][:npad]])
            vx = torch.cat([vv, vh[bh + H][:npad]])
            kdx = torch.cat([kd, torch.full((T, npad), dsc, dtype=torch.float64)], dim=1)
        s = (q @ kx.T).float().double()
        o = torch.zeros(T, HD, dtype=torch.float64)
        l = torch.zeros(T, 1, dtype=torch.float64)
        mn = torch.full((T, 1), -math.inf, dtype=torch.float64)
        for r, (j0, j1) in enumerate(runs(kx.shape[0], parts)):
            sr = s[:, j0:j1]
            m = sr.max(dim=1, keepdim=True).values
            e = torch.exp2(sr - m).float().double()
            if hit and kind == "drop_tile":
                t = fault[2]
                lo, hi_ = max(j0, 32 * t), min(j1, 32 * t + 32)
                if hi_ > lo:
                    e[:, lo - j0:hi_ - j0] = 0.0
            pb = bf16(e) * kdx[:, j0:j1]
            if hit and kind == "chain_scale":
                pb[fault[2]:fault[2] + 32] *= 1.0 + 2.0 ** -6
            orun, lrun = pb @ vx[j0:j1], e.sum(dim=1, keepdim=True)
            w = fault[3] if (hit and kind == "merge" and r == fault[2]) else 1.0
            new = torch.maximum(mn, m)
            ca, cb = torch.exp2(mn - new), torch.exp2(m - new)
            o = o * ca + orun * cb * w
            l = l * ca + lrun * cb * w
            mn = new
        O[bh] = bf16(o / l)
        L[bh] = (mn.squeeze(1) * LN2 + torch.log(l.squeeze(1))).float().double()
        # backward, with the simulated lse and bf16 O
        s = (q @ kk.T).float().double()
        P = torch.exp2(s - LOG2E * L[bh].unsqueeze(1)).float().double()
        delta = (dh[bh] * O[bh]).sum(dim=1, keepdim=True).float().double()
        if hit and kind == "delta":
            delta = delta * 1.01
        dS = bf16(P * (kd * (dh[bh] @ vv.T) - delta))
        dQ[bh] = bf16(scale * (dS @ kk))
        dK[bh] = bf16(LN2 * (dS.T @ q))
        dV[bh] = bf16(bf16(P * kd).T @ dh[bh])
    return dict(o=unheads(O, B, H), lse=L, dq=unheads(dQ, B, H), dk=unheads(dK, B, H), dv=unheads(dV, B, H))
