"""Head-averaged attention maps (test reference, float64 torch): the need_weights branch of the reference's
MultiHeadAttention.call (detr_tf/networks/transformer.py:285-286, 349-354) restated, the whole-model reference built on
oracle.detr_ref / padding_ref by import, and the reference plus PER-ELEMENT bound for the kernel csrc/attention_weights.hip
(detr_hip_attention_weights) in the manner of oracle/attn_bounds.py."""
import math

import numpy as np
import torch

import padding_ref as PR
from oracle import detr_ref as R
from oracle.attn_bounds import F, HD, LN2, LOG2E, TINY, U, heads

ENC_SITE = "transformer/encoder/layer_{}/self_attn"
DEC_SELF_SITE = "transformer/decoder/layer_{}/self_attn"
DEC_CROSS_SITE = "transformer/decoder/layer_{}/multihead_attn"


def site_names(num_enc=6, num_dec=6):
    out = [ENC_SITE.format(i) for i in range(num_enc)]
    for i in range(num_dec):
        out += [DEC_SELF_SITE.format(i), DEC_CROSS_SITE.format(i)]
    return out


def head_mean_weights(q, k, H, scale, key_pad=None):
    """q [B, T, H*hd], k [B, S, H*hd] (the projected, UNSCALED query and key), key_pad bool [B, S] (True = masked key) ->
    [B, T, S].  transformer.py:307 (q * scale), :317 (q k^T per head), :322-337 as padding_ref enables it (-inf at masked keys),
    :340 (softmax over the keys), :349-354 (reshape [B*H, T, S] -> [B, H, T, S], sum over the heads / H)."""
    B, T, D = q.shape
    S = k.shape[1]
    hd = D // H
    qh = (q * scale).reshape(B, T, H, hd).permute(0, 2, 1, 3).reshape(B * H, T, hd)
    kh = k.reshape(B, S, H, hd).permute(0, 2, 1, 3).reshape(B * H, S, hd)
    s = qh @ kh.transpose(1, 2)                                                   # :317
    if key_pad is not None:
        kp = torch.as_tensor(key_pad).bool()[:, None, :].expand(B, H, S).reshape(B * H, 1, S)
        s = s.masked_fill(kp, float("-inf"))                                      # :322-337
    w = torch.softmax(s, dim=-1)                                                  # :340
    return w.reshape(B, H, T, S).sum(dim=1) / H                                   # :349-354


def _recording(orig, rec, masked):
    def mha(query, key, value, P, p, num_heads=8, drop=None, seed=0, **kw):
        T, B, D = query.shape
        W, b = P[f"{p}/in_proj_kernel"], P[f"{p}/in_proj_bias"]
        WQ = (query @ W[:D].t() + b[:D]).transpose(0, 1).double()
        WK = (key @ W[D:2 * D].t() + b[D:2 * D]).transpose(0, 1).double()
        rec[p] = head_mean_weights(WQ.detach(), WK.detach(), num_heads, float(D // num_heads) ** -0.5,
                                   kw.get("key_padding_mask") if masked else None)
        return orig(query, key, value, P, p, num_heads=num_heads, drop=drop, seed=seed, **kw)
    return mha


def detr_attention_maps(images, masks, P, sites, num_enc=6, num_dec=6, with_outputs=False):
    """The whole-model reference: {site: [B, T, S] float64} for the requested parameter paths.  Runs padding_ref.detr_forward (masks
    given) or oracle.detr_ref.detr_forward with their `multi_head_attention` substituted by a recording wrapper for the duration of
    the call (the module attribute is restored afterwards): the wrapper restates the site's projections, stores
    head_mean_weights(...) under the site's parameter path and then calls the original function with the original arguments, so
    the forward itself is untouched."""
    mod = R if masks is None else PR
    orig, rec = mod.multi_head_attention, {}
    mod.multi_head_attention = _recording(orig, rec, masks is not None)
    try:
        Pd = {n: t.double() for n, t in P.items()}
        x = torch.as_tensor(images).double()
        out = R.detr_forward(x, Pd, num_enc=num_enc, num_dec=num_dec) if masks is None else \
            PR.detr_forward(x, masks, Pd, num_enc=num_enc, num_dec=num_dec)
    finally:
        mod.multi_head_attention = orig
    missing = [s for s in sites if s not in rec]
    if missing:
        raise ValueError(f"unknown attention site(s) {missing}")
    maps = {s: rec[s] for s in sites}
    return (maps, out) if with_outputs else maps


def _kernel_terms(q, k, lse_in, H, io16, key_valid, scale):
    """Per (batch, head): exact log2-unit scores s, L = lse_in log2(e), sum_d |q_d k_d| in log2 units; masked K rows zeroed first."""
    B, T, _ = q.shape
    S = k.shape[1]
    q, k = q.double(), k.double()
    kv = None
    if key_valid is not None:
        kv = torch.as_tensor(np.asarray(key_valid)).bool()
        assert tuple(kv.shape) == (B, S)
        k = torch.where(kv.unsqueeze(2), k, torch.zeros_like(k))      # garbage (NaN, inf) in a masked row reaches nothing
    c = 1.0 if io16 else scale * LOG2E
    qh, kh = heads(q, H) * c, heads(k, H)
    s = qh @ kh.transpose(1, 2)                                       # [B*H, T, S]
    a = qh.abs() @ kh.abs().transpose(1, 2)
    L = (lse_in.double().reshape(B * H, T) * LOG2E).unsqueeze(2)
    return s, a, L, kv


def kernel_reference_and_bound(q, k, lse_in, H, io16, key_valid=None, scale=HD ** -0.5):
    """Reference W [B, T, S] and per-element bound B_w of detr_hip_attention_weights, both float64, defined from the kernel's OWN
    inputs: q, k [B, T|S, H*32] (io16: bf16 values, q the stored query that already carries scale * log2(e); otherwise fp32 values
    and the unscaled query), lse_in [B*H, T] the fp32 natural-log lse as given, key_valid bool [B, S] (True = valid) or None:
        W = (1/H) sum_h exp2(s_h - L_h),   s_h = the exact score in log2 units,   L_h = lse_in_h log2(e).
    Units as in oracle/attn_bounds.py: F = 2^-23 per fp32 operation (two unit roundoffs), every constant a count of roundings.
    Where the kernel rounds (csrc/attention_weights.hip):
      * L' = fp32(lse_in * fp32(log2 e)): the constant and the product, half an F each: F |L|.
      * score, bf16 operands: s' = fp32(-L' + sum_32 q_d k_d) inside two MFMAs, the products exact in fp32:
            E_s = 34 F (sum_d |q_d k_d| + |L|) + F |L|                                              (n_s = 34, as attn_bounds)
      * score, fp32 operands: the kernel folds scale * log2(e) into q FIRST, as attention_f32.hip does -- q' = fp32(q * qmul),
        qmul = fp32(fp32(scale) * fp32(log2 e)): four half-F roundings = 2 F on every product -- then 32 rounded products and 32
        adds (the first onto -L'):
            E_s = 66 F (sum_d |q_d k_d| + |L|) + F |L|                                              (n_s = 32 + 32 + 2)
        (the issue's count was 66 + 1 with the scale applied to the finished score; folding it into q costs 2 instead of 1, and
        the count here already includes it.)
      * both forms are in log2 units, so an exponential has relative error e = ln2 E_s + F (v_exp_f32);
      * the head sum is H fp32 adds and the product with 1/H (exact for H a power of two; one more F otherwise, counted):
            B_w = (1 + 2U) ((1/H) sum_h P_h e_h + (H + 1) F W) + TINY,       exactly 0 at a masked key.
    (1 + 2U) covers the second-order terms as in attn_bounds (asserted: ln2 E_s <= 2U); TINY = 2^-120 covers the flush of
    exponentials below the fp32 normal range."""
    B, T, _ = q.shape
    S = k.shape[1]
    s, a, L, kv = _kernel_terms(q, k, lse_in, H, io16, key_valid, scale)
    n_s = 34.0 if io16 else 66.0
    Es = n_s * F * (a + L.abs()) + F * L.abs()
    e = LN2 * Es + F
    P = torch.exp2(s - L)
    if kv is not None:
        valid = kv[:, None, None, :].expand(B, H, 1, S).reshape(B * H, 1, S)
        P = torch.where(valid, P, torch.zeros_like(P))
        assert float((LN2 * Es * valid).max()) <= 2 * U
    else:
        assert float((LN2 * Es).max()) <= 2 * U
    W = P.reshape(B, H, T, S).sum(dim=1) / H
    Bw = (1 + 2 * U) * ((P * e).reshape(B, H, T, S).sum(dim=1) / H + (H + 1) * F * W) + TINY
    if kv is not None:
        Bw = torch.where(kv.unsqueeze(1), Bw, torch.zeros_like(Bw))
    return W, Bw


def lse_of(q, k, H, io16, key_valid=None, scale=HD ** -0.5):
    """fp32 of the fp64 natural-log log-sum-exp of every score row over the valid keys: [B*H, T]."""
    B = q.shape[0]
    s, _, _, kv = _kernel_terms(q, k, torch.zeros(B * H, q.shape[1]), H, io16, key_valid, scale)
    if kv is not None:
        s = s.masked_fill(~kv[:, None, None, :].expand(B, H, 1, k.shape[1]).reshape(B * H, 1, -1), -math.inf)
    return (torch.logsumexp(s * LN2, dim=2)).float()


FAULTS = ["skip_head", "no_div_h", "lse_next_head", "mask_of_entry0", "scale_twice", "bf16_p"]


def simulate(q, k, lse_in, H, io16, key_valid=None, scale=HD ** -0.5, fault=None):
    """One admissible execution of the kernel's roundings on the CPU (fp32 q' = q * qmul, fp32 score accumulation onto -L', fp32
    exp2, fp32 head sum, * 1/H), optionally with one of FAULTS:
        skip_head        the last head left out of the sum            no_div_h         the division by H forgotten
        lse_next_head    head h uses the lse of head h + 1            mask_of_entry0   batch entry 1 uses the mask of entry 0
        scale_twice      the scale applied a second time              bf16_p           each head's probability rounded to bf16"""
    B, T, _ = q.shape
    S = k.shape[1]
    f32 = torch.float32
    kv = None if key_valid is None else torch.as_tensor(np.asarray(key_valid)).bool().clone()
    if kv is not None and fault == "mask_of_entry0":
        assert B > 1 and not torch.equal(kv[0], kv[1])
        kv[1] = kv[0]
    kk = k.double()
    if kv is not None:
        kk = torch.where(kv.unsqueeze(2), kk, torch.zeros_like(kk))
    if io16:
        qq = q.double() * (scale if fault == "scale_twice" else 1.0)
        dot = (heads(qq, H) @ heads(kk, H).transpose(1, 2))                     # bf16 products: exact in fp32, summed below
    else:
        qmul = (torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32))
        if fault == "scale_twice":
            qmul = qmul * torch.tensor(scale, dtype=f32)
        qq = (q.to(f32) * qmul)
        dot = (heads(qq, H) @ heads(kk.to(f32), H).transpose(1, 2)).double()     # fp32 products and adds
    lse = lse_in.reshape(B, H, T)
    if fault == "lse_next_head":
        lse = torch.roll(lse, -1, dims=1)
    Lp = (lse.reshape(B * H, T).to(f32) * torch.tensor(LOG2E, dtype=f32)).double().unsqueeze(2)
    sc = (dot - Lp).to(f32)
    P = torch.exp2(sc)
    if fault == "bf16_p":
        P = P.to(torch.bfloat16).to(f32)
    P = P.reshape(B, H, T, S)
    nh = H - 1 if fault == "skip_head" else H
    acc = torch.zeros(B, T, S, dtype=f32)
    for h in range(nh):
        acc = acc + P[:, h]
    w = acc if fault == "no_div_h" else acc * torch.tensor(1.0 / H, dtype=f32)
    if kv is not None:
        w = torch.where(kv.unsqueeze(1), w, torch.zeros_like(w))
    return w
