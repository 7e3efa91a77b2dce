"""GPU tests of the head-averaged attention maps: the kernel csrc/attention_weights.hip against the per-element bound of
tests/attn_weights_ref.py, and the model surface (engine.forward(attn_sites=...), model(..., need_weights=...),
inference.get_attention_maps) against the fp64 restatement (reference lines: transformer.py:285-286, 349-354)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, HD = 8, 32
D = H * HD
SCALE = HD ** -0.5
SENT = -1234.0
from test_attn_weights_cpu import GRID, SHAPES, kernel_inputs  # noqa: E402  (shapes and operands shared with the CPU self-test)


def _dev_operand(x, io16, col):
    """x [B, N, 256] -> a column block (at `col`) of a packed [B*N, 768] device buffer, the rest NaN."""
    dt = torch.bfloat16 if io16 else torch.float32
    buf = torch.full((x.shape[0] * x.shape[1], 3 * D), float("nan"), dtype=dt, device=DEV)
    buf[:, col:col + D] = x.reshape(-1, D).to(dt).to(DEV)
    return buf[:, col:col + D]


def _words(hip, kv):
    return None if kv is None else torch.from_numpy(hip.keymask_words_from_valid(np.asarray(kv))).reshape(-1).to(DEV)


def _launch(hip, qd, kd, lse, kv_words, B, T, S, pad=0):
    w = torch.full((B, T, S + pad), SENT, device=DEV)
    hip.attention_weights(qd, kd, lse.to(DEV), w, B, H, T, S, scale=SCALE, key_valid=kv_words)
    torch.cuda.synchronize()
    return w


@pytest.mark.parametrize("io16", [True, False], ids=["bf16io", "fp32"])
@pytest.mark.parametrize("kind", [None, "rect", "random"], ids=["unmasked", "rect", "random"])
@pytest.mark.parametrize("B,T,S", SHAPES)
def test_kernel_within_the_per_element_bound(hip, B, T, S, kind, io16):
    """Every element of w against W = (1/H) sum_h exp2(s_h - L_h) (fp64, from the kernel's own inputs) within B_w; packed q / k
    (column blocks of [rows, 768] buffers whose other columns are NaN) and ldw = S + 5 with sentinel columns."""
    import attn_weights_ref as AW
    from oracle.attn_bounds import ratio
    q, k, lse, kv = kernel_inputs(B, T, S, io16, kind)
    W, Bw = AW.kernel_reference_and_bound(q, k, lse, H, io16, key_valid=kv)
    w = _launch(hip, _dev_operand(q, io16, 0), _dev_operand(k, io16, D), lse, _words(hip, kv), B, T, S, pad=5)
    assert bool((w[:, :, S:] == SENT).all()), "columns past S were written"
    r = ratio(w[:, :, :S], W, Bw)
    print(f"B{B} T{T} S{S} io16={io16} mask={kind}: max |got - W| / B_w = {r:.4f}")
    assert r <= 1.0
    if kv is not None:
        inv = torch.from_numpy(~np.asarray(kv))[:, None, :].expand(B, T, S)
        assert bool((w[:, :, :S].cpu()[inv] == 0).all())


@pytest.mark.parametrize("io16", [True, False], ids=["bf16io", "fp32"])
def test_masked_key_content_and_all_valid_words(hip, io16):
    """Masked keys are exact zeros whatever their K rows hold (NaN, inf), bit for bit; all-valid words equal key_valid = NULL."""
    B, T, S = 2, 100, 1050
    q, k, lse, kv = kernel_inputs(B, T, S, io16, "rect")
    qd, words = _dev_operand(q, io16, 0), _words(hip, kv)
    w0 = _launch(hip, qd, _dev_operand(k, io16, D), lse, words, B, T, S)
    inv = torch.from_numpy(~np.asarray(kv))
    assert bool((w0.cpu()[inv[:, None, :].expand(B, T, S)] == 0).all()) and bool(torch.isfinite(w0).all())
    for junk in (float("nan"), float("inf"), -float("inf")):
        kg = k.clone()
        kg[inv] = junk
        assert torch.equal(_launch(hip, qd, _dev_operand(kg, io16, D), lse, words, B, T, S), w0), f"masked K rows = {junk} changed the map"
    q, k, lse, _ = kernel_inputs(B, T, S, io16, None)
    qd, kd = _dev_operand(q, io16, 0), _dev_operand(k, io16, D)
    ones = _words(hip, np.ones((B, S), bool))
    assert torch.equal(_launch(hip, qd, kd, lse, ones, B, T, S), _launch(hip, qd, kd, lse, None, B, T, S))


@pytest.mark.parametrize("io16", [True, False], ids=["bf16io", "fp32"])
@pytest.mark.parametrize("kind", [None, "rect"], ids=["unmasked", "rect"])
def test_rows_sum_to_one_with_the_forwards_own_lse(hip, io16, kind):
    """hip.attention first, then the maps kernel on the same buffers with the lse the forward wrote.  With lse' the forward's
    value, the exact sum over the keys of head h is exp(lse_h - lse'_h), so
        |rowsum(w) - 1| <= sum_s B_w[t, s] + (1/H) sum_h (exp(B_lse[h, t]) - 1).
    bf16: B_lse = oracle.attn_bounds.forward(...)["bound_lse"].  fp32 (attention_f32.hip), derived the same way: a score in log2
    units costs E_s = 66 F (sum_d |q_d k_d| + R) (32 products, 32 adds, 2 for scale * log2(e) folded into q; R = max_j |s_j| +
    log2(e) |lse| + 2 bounds the running maximum), an exponential e_j = ln2 E_s + F; l = sum_j p_j takes S adds plus, per 32-key
    tile, the lane-pair add, the rescale and the add onto the running sum: (S + 3 ntiles) F; lse' = fp32(m ln2 + logf(l)): the
    product, the logf and the add, F each on a magnitude <= R, R, |lse|:
        B_lse32 = sum_j P_j e_j + (S + 3 ntiles) F + F (3 R + |lse|)."""
    import attn_weights_ref as AW
    from oracle import attn_bounds as AB
    B, T, S = 2, 300, 333
    q, k, _, kv = kernel_inputs(B, T, S, io16, kind)
    g = torch.Generator().manual_seed(9)
    v = torch.randn(B, S, D, dtype=torch.float64, generator=g)
    v = AB.bf16(v) if io16 else v.float().double()
    dt = torch.bfloat16 if io16 else torch.float32
    qd, kd, vd = _dev_operand(q, io16, 0), _dev_operand(k, io16, D), _dev_operand(v, io16, 2 * D)
    od = torch.zeros(B * T, D, dtype=dt, device=DEV)
    lse = torch.zeros(B * H, T, device=DEV)
    words = _words(hip, kv)
    hip.attention(qd, kd, vd, od, lse, B, H, T, S, scale=SCALE, key_valid=words)
    w = _launch(hip, qd, kd, lse, words, B, T, S).cpu().double()
    _, Bw = AW.kernel_reference_and_bound(q, k, lse.cpu(), H, io16, key_valid=kv)
    if io16:
        blse = AB.forward(q, k, v, H, key_valid=kv)["bound_lse"]
    else:
        s, a, _, kvt = AW._kernel_terms(q, k, torch.zeros(B * H, T), H, False, kv, SCALE)
        if kvt is not None:
            valid = kvt[:, None, None, :].expand(B, H, 1, S).reshape(B * H, 1, S)
            s = s.masked_fill(~valid, -math.inf)
        lse64 = torch.logsumexp(s * AB.LN2, dim=2)
        P = torch.exp2(s - (lse64 * AB.LOG2E).unsqueeze(2))
        R = torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s)).max(dim=2, keepdim=True).values + AB.LOG2E * lse64.abs().unsqueeze(2) + 2.0
        e = AB.LN2 * 66.0 * AB.F * (a + R) + AB.F
        ntiles = -(-S // 32)
        blse = (P * e).sum(dim=2) + (S + 3 * ntiles) * AB.F + AB.F * (3 * R.squeeze(2) + lse64.abs())
    bound = Bw.sum(dim=2) + torch.expm1(blse.reshape(B, H, T)).mean(dim=1)
    err = (w.sum(dim=2) - 1.0).abs()
    r = float((err / bound).max())
    print(f"io16={io16} mask={kind}: max |rowsum - 1| = {float(err.max()):.3e}, max err / bound = {r:.4f}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------------
def _cfg():
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
    cfg.target_batch = None
    return cfg


def _small_inputs():
    """The tiny inputs of tests/test_gpu_padding.py."""
    images = np.random.default_rng(11).normal(size=(2, 128, 160, 3)).astype(np.float32)
    masks = np.zeros((2, 128, 160), bool)
    masks[1, 96:, :] = True
    masks[1, :, 128:] = True
    images[1][masks[1]] = 0.0
    return images, masks


def _params():
    from oracle import detr_ref as R
    return R.make_params(3)


def _model(precision, params=None, **kw):
    from detr_tf.networks.detr import get_detr_model
    model = get_detr_model(_cfg(), include_top=kw.pop("include_top", True), dropout=0.0, precision=precision, **kw)
    if params is not None:
        assert not model.load_weights(params)
    return model


_REF = {}


def _ref_maps(masked):
    import attn_weights_ref as AW
    from oracle import detr_ref as R
    if masked not in _REF:
        images, masks = _small_inputs()
        _REF[masked] = AW.detr_attention_maps(images, masks if masked else None, R.to_torch(_params()), AW.site_names())
    return _REF[masked]


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "padded"])
@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_model_maps_vs_restatement(hip, precision, masked):
    """All 18 sites of the 6 + 6 model against tests/attn_weights_ref.detr_attention_maps: max |err| / max |ref| < 2e-4, the bound
    test_masked_model_vs_restatement applies to the memory / hs taps of the same model."""
    import attn_weights_ref as AW
    ref = _ref_maps(masked)
    images, masks = _small_inputs()
    model = _model(precision, _params())
    out = model((images, masks) if masked else images, need_weights=AW.site_names())
    assert list(out["attn"]) == AW.site_names()
    worst = []
    for s, r in ref.items():
        got = out["attn"][s]
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(r.shape), (s, got.shape, r.shape)
        rel = float((got.cpu().double() - r).abs().max()) / float(r.abs().max())
        worst.append((rel, s))
    print(f"{precision} masked={masked}: " + ", ".join(f"{s.split('transformer/')[1]} {rel:.2e}" for rel, s in worst))
    bad = [(rel, s) for rel, s in worst if not rel < 2e-4]
    assert not bad, bad
    if masked:
        import padding_ref as PR
        fm = PR.downsample_masks(masks, 4, 5).reshape(2, 20)
        for s in (AW.ENC_SITE.format(5), AW.DEC_CROSS_SITE.format(5)):
            m = out["attn"][s].cpu()
            assert bool((m[fm[:, None, :].expand_as(m)] == 0).all())


def _site_buffers(eng, site, B):
    """(q, k, lse, T, S) of a site from the engine's own bf16 buffers after a forward."""
    kind, i = site.split("/")[1], int(site.split("layer_")[1].split("/")[0])
    L, Q = eng._feat_meta[3], eng.Q
    if site.endswith("multihead_attn"):
        q, k = eng._bufs[f"dec{i}:ca:Q16"], eng._bufs["dec:KV16"][:, i * D:(i + 1) * D]
        return q, k, eng._bufs[f"dec{i}:ca:lse"], Q, L
    tag, T = (f"enc{i}:sa", L) if kind == "encoder" else (f"dec{i}:sa", Q)
    qkv = eng._bufs[f"{tag}:QKV16"]
    return qkv[:, 0:D], qkv[:, D:2 * D], eng._bufs[f"{tag}:lse"], T, T


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "padded"])
def test_model_maps_bf16_within_the_kernel_bound(hip, masked):
    """precision="bf16": every returned map within the per-element kernel bound of the fp64 recomputation from the engine's OWN
    Q16 / K16 / lse buffers of that site (read back after the forward).  The distance to the fp32 model's maps is printed for
    the record, not asserted."""
    import attn_weights_ref as AW
    import padding_ref as PR
    from oracle.attn_bounds import ratio
    images, masks = _small_inputs()
    x = (images, masks) if masked else images
    params = _params()
    model = _model("bf16", params)
    model.eval_graph = False
    out = model(x, need_weights=AW.site_names())
    eng, B = model.engine, 2
    fmask = PR.downsample_masks(masks, 4, 5).reshape(B, 20)
    for s in AW.site_names():
        q, k, lse, T, S = _site_buffers(eng, s, B)
        kv = (~fmask).numpy() if (masked and not (("/decoder/" in s) and s.endswith("/self_attn"))) else None
        W, Bw = AW.kernel_reference_and_bound(q.float().cpu().double().reshape(B, T, D), k.float().cpu().double().reshape(B, S, D),
                                              lse.cpu(), H, True, key_valid=kv)
        r = ratio(out["attn"][s], W, Bw)
        assert r <= 1.0, f"{s}: max |err| / bound = {r:.3f}"
    m32 = _model("fp32", params)(x, need_weights=AW.site_names())
    dev = {}
    for s in AW.site_names():
        kind = "enc self" if "/encoder/" in s else ("dec self" if s.endswith("/self_attn") else "dec cross")
        dev[kind] = max(dev.get(kind, 0.0), float((out["attn"][s] - m32["attn"][s]).abs().max()))
    print(f"masked={masked}: max |bf16 map - fp32 map| per site kind: {dev}")


@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "bf16"])
def test_need_weights_surface_and_eval_graph(hip, precision):
    """need_weights=True returns the two documented sites; the detections are bit-identical with and without it; the eval-graph
    replay (third call of one shape) returns the maps of the first eager call bit for bit, and other sites re-record."""
    import attn_weights_ref as AW
    images, masks = _small_inputs()
    model = _model(precision, _params())
    base = model(images)
    assert "attn" not in base
    enc5, cross5, self0 = AW.ENC_SITE.format(5), AW.DEC_CROSS_SITE.format(5), AW.DEC_SELF_SITE.format(0)
    model.eval_graph = False
    want = model(images, need_weights=[self0, cross5])                          # always-eager results of the same engine
    images2 = images.copy()
    images2[0] += 0.5
    ref2 = model(images2, need_weights=[self0, cross5])
    model.eval_graph = True
    outs = [model(images, need_weights=True) for _ in range(3)]                 # eager, capture + replay, replay
    for o in outs:
        assert list(o["attn"]) == [enc5, cross5]
        assert tuple(o["attn"][enc5].shape) == (2, 20, 20) and tuple(o["attn"][cross5].shape) == (2, 100, 20)
        assert torch.equal(o["pred_logits"], base["pred_logits"]) and torch.equal(o["pred_boxes"], base["pred_boxes"])
        assert all(torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_boxes"], b["pred_boxes"])
                   for a, b in zip(o["aux"], base["aux"]))
        assert all(torch.equal(o["attn"][s], outs[0]["attn"][s]) for s in (enc5, cross5))
    assert model._eval_graph is not None and model._eval_graph["key"][-2] == (enc5, cross5)
    other = [model(images, need_weights=[self0, cross5]) for _ in range(3)]     # other sites: recorded anew, nothing stale
    for o in other:
        assert list(o["attn"]) == [self0, cross5]
        assert all(torch.equal(o["attn"][s], want["attn"][s]) for s in (self0, cross5))
    assert torch.equal(other[0]["attn"][cross5], outs[0]["attn"][cross5])
    got = model(images2, need_weights=[self0, cross5])                          # a replay computes the maps of ITS input
    assert all(torch.equal(got["attn"][s], ref2["attn"][s]) for s in (self0, cross5))
    assert not torch.equal(got["attn"][cross5], other[0]["attn"][cross5])
    again = model(images)                                                       # and without need_weights: as before
    assert "attn" not in again and torch.equal(again["pred_logits"], base["pred_logits"])
    padded = model((images, masks), need_weights=True)
    assert torch.equal(padded["pred_logits"], model((images, masks))["pred_logits"])


def test_documented_rejections(hip):
    model = _model("fp32", num_encoder_layers=1, num_decoder_layers=1)
    images, _ = _small_inputs()
    with pytest.raises(NotImplementedError, match="evaluation mode only"):
        model(images, training=True, need_weights=True)
    with pytest.raises(ValueError, match="valid names.*transformer/encoder/layer_0/self_attn"):
        model(images, need_weights=["transformer/encoder/layer_3/self_attn"])
    with pytest.raises(ValueError, match="unknown attention site"):
        model.engine.forward(torch.from_numpy(images).to(DEV), attn_sites=["nonsense"])
    headless = _model("fp32", include_top=False, num_encoder_layers=1, num_decoder_layers=1)
    assert headless.headless
    with pytest.raises(NotImplementedError, match="headless"):
        headless(images, need_weights=True)
    assert tuple(headless(images).shape) == (1, 2, 100, 256)
    assert model.engine.attn_site_names() == ["transformer/encoder/layer_0/self_attn", "transformer/decoder/layer_0/self_attn",
                                              "transformer/decoder/layer_0/multihead_attn"]


def test_get_attention_maps_shapes(hip):
    from detr_tf.inference import get_attention_maps
    import attn_weights_ref as AW
    model = _model("bf16", num_encoder_layers=1, num_decoder_layers=1)
    img = np.random.default_rng(2).normal(size=(1, 480, 640, 3)).astype(np.float32)
    out, maps = get_attention_maps(model, img)
    e, c, s = AW.ENC_SITE.format(0), AW.DEC_CROSS_SITE.format(0), AW.DEC_SELF_SITE.format(0)
    assert list(maps) == [e, c] and tuple(out["pred_logits"].shape) == (1, 100, 92)
    assert tuple(maps[e].shape) == (1, 300, 15, 20) and tuple(maps[c].shape) == (1, 100, 15, 20)
    assert float((maps[c].sum(dim=(2, 3)) - 1).abs().max()) < 1e-3
    images, masks = _small_inputs()
    out, maps = get_attention_maps(model, (images, masks), need_weights=[e, s, c])
    assert tuple(maps[e].shape) == (2, 20, 4, 5) and tuple(maps[c].shape) == (2, 100, 4, 5) and tuple(maps[s].shape) == (2, 100, 100)
    assert bool((maps[c][1, :, 3:, :] == 0).all()) and bool((maps[c][1, :, :, 4:] == 0).all()) and bool((maps[c][0] > 0).all())


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "padded"])
def test_full_size_bf16_maps(hip, masked):
    """B = 8, 800 x 1333, bf16, need_weights=True: finite, rows sum to 1 within sum_s B_w + mean_h (exp(B_lse) - 1) (see
    test_rows_sum_to_one_with_the_forwards_own_lse), computed per image from the engine's own buffers; with a mask, the columns
    of padded positions are exact zeros."""
    import attn_weights_ref as AW
    import padding_ref as PR
    from oracle import attn_bounds as AB
    B = 8
    model = _model("bf16")
    model.eval_graph = False
    images = torch.randn(B, 800, 1333, 3, generator=torch.Generator().manual_seed(4))
    masks = None
    if masked:
        masks = np.zeros((B, 800, 1333), bool)
        for b in range(1, B):
            masks[b, 800 - 60 * b:, :] = True
            masks[b, :, 1333 - 90 * b:] = True
        images[torch.from_numpy(masks)] = 0.0
    out = model((images, masks) if masked else images, need_weights=True)
    eng = model.engine
    L = 25 * 42
    enc, cross = AW.ENC_SITE.format(5), AW.DEC_CROSS_SITE.format(5)
    assert tuple(out["attn"][enc].shape) == (B, L, L) and tuple(out["attn"][cross].shape) == (B, 100, L)
    fmask = PR.downsample_masks(masks, 25, 42).reshape(B, L) if masked else None
    for s in (enc, cross):
        w = out["attn"][s]
        assert bool(torch.isfinite(w).all())
        q, k, lse, T, S = _site_buffers(eng, s, B)
        v = eng._bufs["enc5:sa:QKV16"][:, 2 * D:] if s == enc else eng._bufs["dec:KV16"][:, 11 * D:12 * D]
        f64 = lambda t, n: t.float().cpu().double().reshape(B, n, D)
        q, k, v, lse = f64(q, T), f64(k, S), f64(v, S), lse.cpu().reshape(B, H, T)
        worst = 0.0
        for b in range(B):
            kv = None if fmask is None else (~fmask[b:b + 1]).numpy()
            _, Bw = AW.kernel_reference_and_bound(q[b:b + 1], k[b:b + 1], lse[b].reshape(H, T), H, True, key_valid=kv)
            blse = AB.forward(q[b:b + 1], k[b:b + 1], v[b:b + 1], H, key_valid=kv)["bound_lse"]
            bound = Bw.sum(dim=2) + torch.expm1(blse.reshape(1, H, T)).mean(dim=1)
            err = (w[b:b + 1].cpu().double().sum(dim=2) - 1.0).abs()
            worst = max(worst, float((err / bound).max()))
            if kv is not None:
                assert bool((w[b].cpu()[:, fmask[b]] == 0).all())
        print(f"{s} masked={masked}: max |rowsum - 1| / bound = {worst:.4f}")
        assert worst <= 1.0
