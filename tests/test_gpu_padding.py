"""GPU tests of padded mixed-size batches: the key-padding-masked attention kernels (csrc/attention_dma.hip, attention_f32.hip)
against an fp64 masked reference, the mask-preparation and padded input-stage kernels (csrc/padding_mask.hip), and the whole
model with (images, masks) against the masked restatement tests/padding_ref.py (reference lines: detr.py:57-72,
position_embeddings.py:23-50 normalize=True, transformer.py:43-50,322-337)."""
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
LOG2E = 1.4426950408889634
# the reported total loss carries the set-loss sums' float-atomic last-bit noise run to run (csrc/setloss.hip); gradients do not
LOSS_NOISE = 1e-6


def close(a, b, rtol, what=""):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    scale = float(b.abs().max()) + 1e-30
    err = float((a - b).abs().max())
    assert err <= rtol * scale, f"{what}: max abs err {err:.3e} > {rtol * scale:.3e} (scale {scale:.3e})"


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# masked attention kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _key_valid(kind, B, S, rng):
    v = np.ones((B, S), bool)
    if kind == "rect":                     # 25 x 42 grid, rectangular padding per image
        g = np.zeros((B, 25, 42), bool)
        g[0, :18, :30] = True
        g[1 % B, :25, :20] = True
        v = g.reshape(B, -1)[:, :S]
    elif kind == "random":
        v = rng.random((B, S)) < 0.6
    elif kind == "tiles":                  # whole 32-key tiles masked, the first one among them
        for t in range(0, (S + 31) // 32, 2):
            v[:, 32 * t:32 * t + 32] = False
        v[:, 32] = True
    elif kind == "first_half":             # the first half of the keys: whole runs of waves without a valid key
        v[:, :S // 2 + 7] = False
    elif kind == "all":
        pass
    v[:, -1] |= ~v.any(axis=1)
    return v


def _attn_case(hip, B, T, S, p, kind, bf16, split=0, seed=0, garbage=None):
    """One masked forward + backward.  Returns the device results and the fp64 reference (o, lse, q.grad, k.grad, v.grad)."""
    from oracle import dropout_ref as DR
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    valid = _key_valid(kind, B, S, rng)
    site, step, scale = 77, 0xBEEF1234, HD ** -0.5
    if bf16:
        qs = (torch.randn(B, T, D, dtype=torch.float64) * 2.0 * (scale * LOG2E)).to(torch.bfloat16)
        q = (qs.to(torch.float64) / (scale * LOG2E)).requires_grad_(True)
        k = _bf(torch.randn(B, S, D, dtype=torch.float64)).requires_grad_(True)
        v = _bf(torch.randn(B, S, D, dtype=torch.float64)).requires_grad_(True)
        do = _bf(torch.randn(B, T, D, dtype=torch.float64))
    else:
        q = torch.randn(B, T, D, dtype=torch.float64).requires_grad_(True)
        k = torch.randn(B, S, D, dtype=torch.float64).requires_grad_(True)
        v = torch.randn(B, S, D, dtype=torch.float64).requires_grad_(True)
        do = torch.randn(B, T, D, dtype=torch.float64)
    keep = None
    if p > 0.0:
        keep = torch.from_numpy(DR.keep_mask(DR.drop_key(site, step), DR.attn_index(B * H, T, S).reshape(B, H, T, S), p))
    # fp64 reference: masked keys get -inf scores (transformer.py:322-337)
    qh, kh, vh = (t.view(B, -1, H, HD).transpose(1, 2) for t in (q, k, v))
    sc = (qh * scale) @ kh.transpose(-1, -2)
    sc = sc.masked_fill(torch.from_numpy(~valid)[:, None, None, :], float("-inf"))
    w = torch.softmax(sc, dim=-1)
    if keep is not None:
        w = torch.where(keep, w / (1.0 - p), torch.zeros_like(w))
    o_ref = (w @ vh).transpose(1, 2).reshape(B, T, D)
    o_ref.backward(do)
    lse_ref = torch.logsumexp(sc, dim=-1).detach()

    dt = torch.bfloat16 if bf16 else torch.float32
    kd = k.detach().to(dt).view(-1, D).to(DEV)
    vd = v.detach().to(dt).view(-1, D).to(DEV)
    if garbage is not None:                # masked K / V rows replaced: garbage(n) -> [n, D] (finite garbage, or zeros)
        inv = torch.from_numpy(~valid.reshape(-1)).to(DEV)
        g = garbage(int(inv.sum()))
        kd[inv] = g.to(dt).to(DEV)
        vd[inv] = (-g).to(dt).to(DEV)
    qd = (qs.view(-1, D) if bf16 else q.detach().to(dt).view(-1, D)).to(DEV)
    dod = do.to(dt).view(-1, D).to(DEV)
    od = torch.full((B * T, D), 7.0, dtype=dt, device=DEV)
    dqd, dkd, dvd = (torch.full_like(t, 3.0) for t in (qd, kd, vd))
    lse = torch.zeros(B * H, T, device=DEV)
    delta = torch.zeros(2 * B * H * T, device=DEV)
    stepd = torch.tensor([step - (1 << 32)] + [0] * 7, dtype=torch.int32, device=DEV)
    mask = None
    if bf16 and p > 0.0:
        mask = torch.zeros(hip.attention_dropmask_words(B, H, T, S), dtype=torch.int32, device=DEV)
        hip.attention_dropmask(mask, B, H, T, S, dropout_p=p, dropout_site=site, dropout_step=stepd)
    kv = torch.from_numpy(hip.keymask_words_from_valid(valid)).to(DEV)
    hip.set_tuning("DETR_HIP_ATTN_SPLIT", split if split else None)
    try:
        kw = dict(scale=scale, dropout_p=p, dropout_site=site, dropout_step=stepd, dropmask=mask, key_valid=kv, compute=0)
        hip.attention(qd, kd, vd, od, lse, B, H, T, S, **kw)
        hip.attention(qd, kd, vd, od, lse, B, H, T, S, d_o=dod, dq=dqd, dk=dkd, dv=dvd, delta=delta, **kw)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning("DETR_HIP_ATTN_SPLIT", None)
    dev = dict(o=od, lse=lse, dq=dqd, dk=dkd, dv=dvd, valid=valid)
    ref = dict(o=o_ref.detach(), lse=lse_ref, dq=q.grad, dk=k.grad, dv=v.grad)
    return dev, ref


def _check_attn(dev, ref, B, T, S, bf16, tag, p=0.0):
    if bf16:      # bounds of test_gpu_attention_dma.py
        to, tl, tg = 1.0e-2, 2e-3, 3.0e-2
    else:         # bounds of the exact-fp32 attention tests (test_gpu_kernels.py; 3e-5 on O with dropout)
        to, tl, tg = (3e-5 if p > 0.0 else 2e-5), 1e-5, 5e-5
    close(dev["o"].float().view(B, T, D), ref["o"], to, f"masked fwd {tag}")
    close(dev["lse"].view(B, H, T), ref["lse"], tl, f"masked lse {tag}")
    close(dev["dq"].float().view(B, T, D), ref["dq"], tg, f"masked dq {tag}")
    close(dev["dk"].float().view(B, S, D), ref["dk"], tg, f"masked dk {tag}")
    close(dev["dv"].float().view(B, S, D), ref["dv"], tg, f"masked dv {tag}")
    inv = torch.from_numpy(~dev["valid"].reshape(-1)).to(DEV)
    assert bool((dev["dk"].view(B * S, D)[inv] == 0).all()) and bool((dev["dv"].view(B * S, D)[inv] == 0).all()), \
        f"masked keys must get exact zeros in dK / dV ({tag})"


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16io", "fp32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,S,kind", [(2, 1050, 1050, "rect"), (2, 100, 1050, "rect"), (2, 300, 333, "random"),
                                        (1, 200, 700, "tiles"), (1, 70, 65, "random"), (2, 100, 1050, "first_half")])
def test_masked_attention_vs_fp64(hip, bf16, p, B, T, S, kind):
    dev, ref = _attn_case(hip, B, T, S, p, kind, bf16, seed=B * 31 + T + S + int(p * 10))
    _check_attn(dev, ref, B, T, S, bf16, f"B{B} T{T} S{S} {kind} p{p}", p)


@pytest.mark.parametrize("split", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["first_half", "tiles"])
def test_masked_attention_runs_without_valid_keys(hip, split, kind):
    """DETR_HIP_ATTN_SPLIT = 1..4: runs whose every key is masked merge as (m = -inf, l = 0); an all-masked first tile does not set
    the lazy softmax reference."""
    dev, ref = _attn_case(hip, 1, 200, 1050, 0.1, kind, True, split=split, seed=split)
    _check_attn(dev, ref, 1, 200, 1050, True, f"split {split} {kind}")


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16io", "fp32"])
def test_masked_attention_ignores_masked_key_content(hip, bf16):
    """Masked K / V rows filled with finite garbage (+-1e4) give bit-identical O, LSE and dQ to zero-filled rows."""
    B, T, S = 2, 300, 1050
    z, _ = _attn_case(hip, B, T, S, 0.1, "rect", bf16, seed=5, garbage=lambda n: torch.zeros(n, D, dtype=torch.float64))
    g, _ = _attn_case(hip, B, T, S, 0.1, "rect", bf16, seed=5, garbage=lambda n: torch.full((n, D), 1.0e4, dtype=torch.float64))
    r, _ = _attn_case(hip, B, T, S, 0.1, "rect", bf16, seed=5,
                      garbage=lambda n: torch.from_numpy(np.random.default_rng(0).uniform(-1e4, 1e4, (n, D))))
    for other in (g, r):
        for name in ("o", "lse", "dq"):
            assert torch.equal(z[name], other[name]), name
        for name in ("dk", "dv"):
            inv = torch.from_numpy(~z["valid"].reshape(-1)).to(DEV)
            assert bool((other[name].view(B * S, D)[inv] == 0).all())
            assert torch.equal(z[name].view(B * S, D)[~inv], other[name].view(B * S, D)[~inv]), name


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16io", "fp32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_all_valid_words_equal_the_unmasked_kernels(hip, bf16, p):
    B, T, S = 2, 300, 1050
    torch.manual_seed(1)
    dt = torch.bfloat16 if bf16 else torch.float32
    q, k, v, do = (torch.randn(B * n, D, device=DEV).to(dt) for n in (T, S, S, T))
    stepd = torch.tensor([12345] + [0] * 7, dtype=torch.int32, device=DEV)
    mask = None
    if bf16 and p > 0.0:
        mask = torch.zeros(hip.attention_dropmask_words(B, H, T, S), dtype=torch.int32, device=DEV)
        hip.attention_dropmask(mask, B, H, T, S, dropout_p=p, dropout_site=3, dropout_step=stepd)
    kv = torch.from_numpy(hip.keymask_words_from_valid(np.ones((B, S), bool))).to(DEV)
    outs = []
    for key_valid in (None, kv):
        o = torch.zeros(B * T, D, dtype=dt, device=DEV)
        lse = torch.zeros(B * H, T, device=DEV)
        dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
        delta = torch.zeros(2 * B * H * T, device=DEV)
        kw = dict(scale=HD ** -0.5, dropout_p=p, dropout_site=3, dropout_step=stepd, dropmask=mask, key_valid=key_valid, compute=0)
        hip.attention(q, k, v, o, lse, B, H, T, S, **kw)
        hip.attention(q, k, v, o, lse, B, H, T, S, d_o=do, dq=dq, dk=dk, dv=dv, delta=delta, **kw)
        outs.append((o, lse, dq, dk, dv))
    torch.cuda.synchronize()
    for a, b, name in zip(outs[0], outs[1], ("o", "lse", "dq", "dk", "dv")):
        assert torch.equal(a, b), name


def test_masked_entry_rejects_bf16_compute_on_fp32_tensors(hip):
    """compute = 1 is valid only with bf16 operands (io_dtype = 1): fp32 tensors with compute = 1 are rejected by the masked and
    the unmasked entry points of both directions, before anything is launched or written."""
    from ctypes import byref
    B, T, S = 1, 64, 64
    q = torch.zeros(B * T, D, device=DEV)
    o, lse, delta = torch.full_like(q, 7.0), torch.full((B * H, T), 7.0, device=DEV), torch.full((B * H, T), 7.0, device=DEV)
    grads = [torch.full_like(q, 7.0) for _ in range(3)]
    kv = torch.from_numpy(hip.keymask_words_from_valid(np.ones((B, S), bool))).to(DEV)
    with pytest.raises(RuntimeError, match="no key-padding-masked form"):
        hip.attention(q, q, q, q.clone(), torch.zeros(B * H, T, device=DEV), B, H, T, S, compute=1, key_valid=kv)
    d = hip.AttnDesc()
    d.B, d.H, d.T, d.S, d.scale = B, H, T, S, 1.0
    d.q = d.k = d.v = d.d_o = q.data_ptr()
    d.o, d.lse, d.delta = o.data_ptr(), lse.data_ptr(), delta.data_ptr()
    d.dq, d.dk, d.dv = (t.data_ptr() for t in grads)
    d.ldq = d.ldk = d.ldv = d.ldo = d.ldd_o = d.lddq = d.lddk = d.lddv = D
    d.compute, d.io_dtype = 1, 0
    lib = hip.load()
    for name, args in (("fwd", ()), ("bwd", ()), ("fwd_masked", (kv.data_ptr(),)), ("bwd_masked", (kv.data_ptr(),))):
        fn = f"detr_hip_attention_{name}"
        with pytest.raises(RuntimeError, match=r"compute = 1 \(bf16 MFMA\) needs bf16 operands \(io_dtype = 1\)"):
            hip._check(getattr(lib, fn)(byref(d), *args, hip._stream()), fn)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in [o, lse, delta] + grads)


# ------------------------------------------------------------------------------------------------------------------------------
# mask preparation and padded input stage
# ------------------------------------------------------------------------------------------------------------------------------
def _prepare(hip, masks, Hf, Wf):
    from detr_tf.engine import position_embedding_sine_table
    B = masks.shape[0]
    L = Hf * Wf
    ty = torch.from_numpy(position_embedding_sine_table(Hf)).to(DEV)
    tx = torch.from_numpy(position_embedding_sine_table(Wf)).to(DEV)
    kv = torch.full((hip.attention_keymask_words(B, L),), -1, dtype=torch.int32, device=DEV)
    pos = torch.full((B * L, 256), 9.0, device=DEV)
    status = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    hip.padding_mask_prepare(torch.from_numpy(masks).to(DEV), Hf, Wf, ty, tx, kv, pos, status)
    torch.cuda.synchronize()
    return kv.cpu().numpy(), pos.cpu().numpy().reshape(B, Hf, Wf, 256), status.cpu().numpy(), ty.cpu().numpy(), tx.cpu().numpy()


@pytest.mark.parametrize("H_,W_,Hf,Wf", [(800, 1333, 25, 42), (128, 160, 4, 5), (97, 131, 4, 5), (40, 40, 13, 7),
                                         # the limits: 128 per side, 8192 positions (91 x 90 = 8190: a ragged last key word)
                                         (1027, 515, 128, 64), (515, 1027, 64, 128), (9, 1031, 1, 128), (1031, 9, 128, 1),
                                         (731, 725, 91, 90)])
def test_padding_mask_prepare(hip, H_, W_, Hf, Wf):
    import padding_ref as PR
    from detr_tf import _hip
    from detr_tf.engine import downsample_mask_nearest
    rng = np.random.default_rng(H_ + W_)
    B = 3
    masks = np.ones((B, H_, W_), bool)
    masks[0, :H_ * 2 // 3, :W_ // 2 + 1] = False                    # rectangular padding
    masks[1] = rng.random((H_, W_)) < 0.4                           # any pattern
    # image 2: all padding -> status 1
    kv, pos, status, ty, tx = _prepare(hip, masks, Hf, Wf)
    fm = downsample_mask_nearest(masks, Hf, Wf)
    want_kv = _hip.keymask_words_from_valid(~fm.reshape(B, -1)).reshape(-1)
    assert np.array_equal(kv, want_kv), "key_valid words"
    assert list(status) == [0, 0, 1]
    nm = ~fm
    cy, cx = np.cumsum(nm, 1), np.cumsum(nm, 2)
    ny, nx = cy[:, -1:, :].repeat(Hf, 1), cx[:, :, -1:].repeat(Wf, 2)
    host = np.concatenate([ty[ny, cy], tx[nx, cx]], axis=3)
    assert pos.tobytes() == host.astype(np.float32).tobytes(), "pos must be the host gather, bit for bit"
    ref = PR.position_embedding_sine_masked(torch.from_numpy(fm)).numpy()
    assert float(np.abs(pos - ref).max()) <= 1e-6


@pytest.mark.parametrize("Hf,Wf", [(129, 8), (8, 129), (91, 91)])
def test_padding_mask_prepare_rejects_maps_over_the_limits(hip, Hf, Wf):
    """More than 128 per side or 8192 positions (91 x 91 = 8281) raises, and nothing is written to kv, pos or status."""
    from detr_tf.engine import position_embedding_sine_table
    B, L = 2, Hf * Wf
    masks = np.zeros((B, 4 * Hf + 1, 4 * Wf + 3), bool)
    masks[1, 2 * Hf:] = True
    ty = torch.from_numpy(position_embedding_sine_table(Hf)).to(DEV)
    tx = torch.from_numpy(position_embedding_sine_table(Wf)).to(DEV)
    kv = torch.full((hip.attention_keymask_words(B, L),), -1, dtype=torch.int32, device=DEV)
    pos = torch.full((B * L, 256), 9.0, device=DEV)
    status = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    with pytest.raises((RuntimeError, ValueError), match="exceeds"):
        hip.padding_mask_prepare(torch.from_numpy(masks).to(DEV), Hf, Wf, ty, tx, kv, pos, status)
    torch.cuda.synchronize()
    assert bool((kv == -1).all()) and bool((pos == 9.0).all()) and bool((status == 7).all()), "sentinels overwritten"


def test_padding_mask_prepare_all_false_is_the_unmasked_constant(hip):
    from detr_tf.engine import position_embedding_sine_host
    for (H_, W_, Hf, Wf) in ((128, 160, 4, 5), (800, 1333, 25, 42)):
        kv, pos, status, _, _ = _prepare(hip, np.zeros((2, H_, W_), bool), Hf, Wf)
        want = position_embedding_sine_host(Hf, Wf)
        assert pos[0].reshape(-1, 256).tobytes() == want.tobytes() and pos[1].reshape(-1, 256).tobytes() == want.tobytes()
        assert list(status) == [0, 0]


def test_images_padded(hip):
    from detr_tf.data.processing import DeviceInputStage, normalization_table
    from detr_tf.training_config import TrainingConfig
    rng = np.random.default_rng(3)
    sizes = [(37, 50), (64, 21), (5, 64)]
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    for method in ("torch_resnet", "tf_resnet"):
        cfg = TrainingConfig()
        cfg.normalized_method = method
        st = DeviceInputStage(cfg)
        x, m = st.images_padded(imgs)
        torch.cuda.synchronize()
        assert x.shape == (3, 64, 64, 3) and m.shape == (3, 64, 64) and m.dtype == torch.bool
        lut, perm = normalization_table(method)
        x, m = x.cpu().numpy(), m.cpu().numpy()
        for b, (im, (h, w)) in enumerate(zip(imgs, sizes)):
            want = np.stack([lut[c][im[..., perm[c]]] for c in range(3)], axis=-1)
            assert x[b, :h, :w].tobytes() == want.astype(np.float32).tobytes()
            assert not m[b, :h, :w].any() and m[b, h:].all() and m[b, :, w:].all()
            assert (x[b, h:] == 0.0).all() and (x[b, :, w:] == 0.0).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the model with (images, masks)
# ------------------------------------------------------------------------------------------------------------------------------
def _cfg():
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
    cfg.target_batch = None
    return cfg


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)


def _grad_rows(engine, P_ref):
    """test_gpu_model._grad_report's per-tensor criterion (relative L2 <= 1e-2, max abs <= 3e-2 of the tensor max)."""
    gmax = max(float(P_ref[n].grad.abs().max()) for n in engine.P.gviews)
    rows = []
    for name, gv in engine.P.gviews.items():
        ref = P_ref[name].grad.double()
        d = gv.detach().cpu().double() - ref
        err = float(d.abs().max())
        l2 = float(d.norm()) / (float(ref.norm()) + 1e-6 * gmax * math.sqrt(ref.numel()))
        tol = 3e-2 * float(ref.abs().max()) + 1e-6 * gmax
        rows.append((max(err / tol, l2 / 1e-2), name, err, float(ref.abs().max()), l2))
    rows.sort(reverse=True)
    return rows


def _small_inputs():
    from oracle import set_loss_ref as L
    images = np.random.default_rng(11).normal(size=(2, 128, 160, 3)).astype(np.float32)
    masks = np.zeros((2, 128, 160), bool)
    masks[1, 96:, :] = True
    masks[1, :, 128:] = True
    images[1][masks[1]] = 0.0
    t_bbox, t_class = L.make_targets(2, seed=21, force_full=False)
    return images, masks, t_bbox, t_class


def _model(precision, params):
    from detr_tf.networks.detr import get_detr_model
    model = get_detr_model(_cfg(), include_top=True, dropout=0.0, precision=precision)
    assert not model.load_weights(params)
    return model


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_masked_model_vs_restatement(hip, precision):
    """Forward taps, loss and every gradient of a padded batch (image 1: 96 x 128 valid of 128 x 160) against the masked
    restatement's autograd, at the bounds of test_gpu_model.py."""
    import padding_ref as PR
    from detr_tf import training
    from detr_tf.loss.loss import get_losses
    from detr_tf.optimizers import setup_optimizers
    from oracle import detr_ref as R, set_loss_ref as L
    params = R.make_params(3)
    images, masks, t_bbox, t_class = _small_inputs()
    P = R.to_torch(params, requires_grad=True)
    taps = {}
    ref = PR.detr_forward(torch.from_numpy(images), masks, P, taps=taps)
    ref_total, ref_log = L.get_losses(ref, torch.from_numpy(t_bbox), torch.from_numpy(t_class), 91)
    ref_total.backward()
    model = _model(precision, params)
    cfg = _cfg()
    out = model((images, masks))
    eng = model.engine
    B, L_ = 2, taps["memory"].shape[0]
    assert _rel(eng.pos.view(B, L_, 256), taps["pos"].reshape(B, L_, 256)) < 1e-5
    assert _rel(eng._bufs["enc5:x2"].view(B, L_, 256), taps["memory"].transpose(0, 1)) < 2e-4
    assert _rel(eng._bufs["dec:hs"].view(6, B, 100, 256), taps["hs"]) < 2e-4
    assert _rel(out["pred_logits"], ref["pred_logits"]) < 2e-4
    assert _rel(out["pred_boxes"], ref["pred_boxes"]) < 2e-4
    total, log = get_losses(out, t_bbox, t_class, cfg)
    assert abs(float(total) - float(ref_total)) <= 1e-3 * abs(float(ref_total))
    opt = setup_optimizers(model, cfg)
    training.run_train_step(model, (images, masks), t_bbox, t_class, opt, cfg)
    torch.cuda.synchronize()
    bad = [r for r in _grad_rows(eng, P) if r[0] > 1.0]
    assert not bad, f"gradient mismatch (err/tol, tensor, abs err, ref scale): {bad[:12]}"


def test_masked_bf16_step_deviation_from_masked_fp32(hip):
    """precision="bf16" on a padded batch: loss within 2e-2 of the masked fp32 step (test_bf16_compute_mode_deviation_from_fp32_oracle)."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    from oracle import detr_ref as R
    params = R.make_params(3)
    images, masks, t_bbox, t_class = _small_inputs()
    totals = {}
    for precision in ("fp32", "bf16"):
        model = _model(precision, params)
        opt = setup_optimizers(model, _cfg())
        _, total, _, _ = training.run_train_step(model, (images, masks), t_bbox, t_class, opt, _cfg())
        totals[precision] = float(total)
    assert abs(totals["bf16"] - totals["fp32"]) <= 2e-2 * abs(totals["fp32"]), totals


@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "bf16"])
def test_all_false_masks_are_bit_identical_to_unmasked(hip, precision):
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    from oracle import detr_ref as R
    params = R.make_params(3)
    images, _, t_bbox, t_class = _small_inputs()
    model = _model(precision, params)
    model.eval_graph = False
    cfg = _cfg()
    opt = setup_optimizers(model, cfg)
    res = []
    for inp in (images, (images, np.zeros(images.shape[:3], bool)), (images, torch.zeros(images.shape[:3], dtype=torch.bool, device=DEV))):
        out = model(inp)
        lg, bx = out["pred_logits"].clone(), out["pred_boxes"].clone()
        out, total, _, _ = training.run_train_step(model, inp, t_bbox, t_class, opt, cfg)
        torch.cuda.synchronize()
        res.append((lg, bx, out["pred_logits"].clone(), float(total), {n: g.clone() for n, g in model.engine.P.gviews.items()}))
    for other in res[1:]:
        assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1]) and torch.equal(res[0][2], other[2])
        assert abs(res[0][3] - other[3]) <= LOSS_NOISE * abs(res[0][3])
        for n in res[0][4]:
            assert torch.equal(res[0][4][n], other[4][n]), n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_batch_isolation(hip, precision):
    """Changing image 1's pixels or padding leaves image 0's outputs bit-identical."""
    from oracle import detr_ref as R
    model = _model(precision, R.make_params(3))
    model.eval_graph = False
    images, masks, _, _ = _small_inputs()
    base = model((images, masks))
    lg0, bx0 = base["pred_logits"][0].clone(), base["pred_boxes"][0].clone()
    im2, m2 = images.copy(), masks.copy()
    im2[1] = np.random.default_rng(99).normal(size=im2[1].shape)
    m2[1, :, :] = False
    m2[1, 64:, 96:] = True
    for im, m in ((im2, masks), (images, m2), (im2, m2)):
        out = model((im, m))
        assert torch.equal(out["pred_logits"][0], lg0) and torch.equal(out["pred_boxes"][0], bx0)
        assert not torch.equal(out["pred_logits"][1], base["pred_logits"][1])


def test_eval_graph_with_masks(hip):
    """The eval hipGraph of a masked batch equals the eager forward, and a new mask copied in before a replay takes effect."""
    from oracle import detr_ref as R
    images, masks, _, _ = _small_inputs()
    model = _model("bf16", R.make_params(3))
    masks_d = torch.from_numpy(masks).to(DEV)
    m2 = masks.copy()
    m2[0, 64:, :] = True                  # (rows 64 and 96 are the ones the 4-row feature map samples)
    m2_d = torch.from_numpy(m2).to(DEV)
    model.eval_graph = False
    eager1 = model((images, masks_d))["pred_logits"].clone()
    eager2 = model((images, m2_d))["pred_logits"].clone()
    model.eval_graph = True
    for _ in range(3):                    # eager (first sighting), capture, replay
        g1 = model((images, masks_d))["pred_logits"]
        assert torch.equal(g1, eager1)
    assert model._eval_graph is not None and model._eval_graph["key"][-1] is True
    g2 = model((images, m2_d))["pred_logits"]
    assert torch.equal(g2, eager2) and not torch.equal(g2, eager1)
    unmasked = model(images)["pred_logits"]           # the graph key tells masked from unmasked
    model.eval_graph = False
    assert torch.equal(unmasked, model(images)["pred_logits"])


def test_graphed_train_step_with_masks_equals_eager(hip):
    """One masked train step replayed from a hipGraph is bit-identical to the eager step; the next replay reads a new mask."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    from oracle import detr_ref as R
    images, masks, t_bbox, t_class = _small_inputs()
    m2 = masks.copy()
    m2[0, :, 96:] = True                  # (columns 96 and 128 are sampled by the 5-column feature map)
    params = R.make_params(3)
    results = {}
    for launch in ("eager", "graph"):
        model = _model("bf16", params)
        cfg = _cfg()
        opt = setup_optimizers(model, cfg)
        stepper = training.GraphedTrainStep(model, opt, cfg, eager_steps=1, launch=launch)
        losses = []
        for i, m in enumerate((masks, masks, m2)):
            _, total, _ = stepper((images, m), t_bbox, t_class, i)
            losses.append(float(total))
        torch.cuda.synchronize()
        results[launch] = (losses, {n: v.detach().clone() for n, v in model.engine.P.views.items()})
        if launch == "graph":
            assert stepper.step_graph is not None
    for n, v in results["eager"][1].items():
        assert torch.equal(v, results["graph"][1][n]), n
    for a, b in zip(results["eager"][0], results["graph"][0]):
        assert abs(a - b) <= LOSS_NOISE * abs(a), results


def test_invalid_masks_raise(hip):
    from oracle import detr_ref as R
    model = _model("bf16", R.make_params(3))
    images, masks, _, _ = _small_inputs()
    bad = masks.copy()
    bad[1] = True
    with pytest.raises(ValueError, match="no valid"):
        model((images, bad))
    model((images, torch.from_numpy(bad).to(DEV)))           # device mask: flagged on the device, read where the caller syncs
    with pytest.raises(ValueError, match="no valid"):
        model.engine.check_mask_status()
    model((images, torch.from_numpy(masks).to(DEV)))
    model.engine.check_mask_status()


def test_full_size_bf16_step_is_finite_and_deterministic(hip):
    """B = 8 on an 800 x 1333 canvas with mixed landscape / portrait extents: one bf16 training step, twice, bit-identical."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    from oracle import detr_ref as R, set_loss_ref as L
    B, Hc, Wc = 8, 800, 1333
    rng = np.random.default_rng(8)
    extents = [(800, 1333), (800, 533), (600, 800), (800, 1200), (533, 800), (750, 1000), (800, 600), (480, 1333)]
    images = rng.normal(size=(B, Hc, Wc, 3)).astype(np.float32)
    masks = np.ones((B, Hc, Wc), bool)
    for b, (h, w) in enumerate(extents):
        masks[b, :h, :w] = False
    images[masks] = 0.0
    t_bbox, t_class = L.make_targets(B, seed=3, force_full=False)
    model = _model("bf16", R.make_params(1))
    cfg = _cfg()
    opt = setup_optimizers(model, cfg)
    images_d, masks_d = torch.from_numpy(images).to(DEV), torch.from_numpy(masks).to(DEV)
    runs = []
    for _ in range(2):
        out, total, _, _ = training.run_train_step(model, (images_d, masks_d), t_bbox, t_class, opt, cfg)
        torch.cuda.synchronize()
        runs.append((float(total), out["pred_logits"].clone(), {n: g.clone() for n, g in model.engine.P.gviews.items()}))
    assert math.isfinite(runs[0][0]) and bool(torch.isfinite(runs[0][1]).all())
    assert all(bool(torch.isfinite(g).all()) for g in runs[0][2].values())
    assert abs(runs[0][0] - runs[1][0]) <= LOSS_NOISE * abs(runs[0][0]) and torch.equal(runs[0][1], runs[1][1])
    for n in runs[0][2]:
        assert torch.equal(runs[0][2][n], runs[1][2][n]), n
