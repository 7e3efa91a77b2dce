"""DC5 backbones on the GPU: the dilation-2 3x3 convolution (csrc/conv_dilated.hip) against fp64 torch conv2d(dilation=2, padding=2)
and its autograd, and the tiny model with dilated stages against tests/dc5_ref.py.

Tolerances are those of the dense kernel's tests -- the arithmetic is the same, only the addressing differs:
  * compute 0 (exact fp32 MFMA): tests/test_gpu_kernels.py:400,408,411 (test_conv3x3_all_modes) -- forward / input gradient 2e-5,
    weight gradient 5e-5 of the reference's largest magnitude;
  * compute 2 (fp32x3): tests/test_gpu_f32x3.py:183,190,196 (test_conv3x3_all_modes_f32x3) -- the same 2e-5 / 2e-5 / 5e-5;
  * compute 1 (bf16 tensors): tests/test_gpu_kernels.py:1160 (test_conv3x3_halo_staged_kernel) -- forward / input gradient within one
    bf16 rounding (2^-8 * 1.1 of |ref| + 1e-2 * scale) of fp64 on the same bf16 operands; weight gradient (fp32) 2e-5 of the scale,
    tests/test_gpu_kernels.py:1108 (test_conv3x3_bf16_activation_storage).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def g(t):
    return t.to(DEV).contiguous()


def _bf(t):
    return t.to(torch.bfloat16).double()


def close(a, b, rtol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = float(b.abs().max()) + 1e-30
    err = float((a - b).abs().max())
    print(f"{what}: max abs err {err:.3e}, bound {rtol * scale:.3e} (scale {scale:.3e})")
    assert err <= rtol * scale, f"{what}: max abs err {err:.3e} > {rtol * scale:.3e} (scale {scale:.3e})"


def one_bf16_rounding(a, ref, what):
    a, ref = a.detach().float().cpu().double(), ref.double()
    scale = float(ref.abs().max())
    assert scale > 0
    rel = float(((a - ref).abs() / (ref.abs() + 1e-2 * scale)).max())
    print(f"{what}: max relative err {rel:.3e}, bound {2.0 ** -8 * 1.1:.3e}")
    assert rel < 2.0 ** -8 * 1.1, f"{what}: more than one bf16 rounding from fp64 ({rel:.3e})"


SHAPES = [(5, 7), (6, 8), (1, 3), (2, 2), (13, 21)]
CASES = [(H, W, C) for (H, W) in SHAPES for C in (64, 128)] + [(5, 7, 512), (13, 21, 512)]
_REF = {}


def _reference(H, W, C):
    """fp64 conv2d(dilation=2, padding=2) and its autograd on bf16-representable operands, computed once per shape."""
    key = (H, W, C)
    if key not in _REF:
        N = 2
        gen = torch.Generator().manual_seed(1000 * H + 10 * W + C)
        x = _bf(torch.randn(N, H, W, C, generator=gen)).requires_grad_(True)
        w = _bf(torch.randn(3, 3, C, C, generator=gen) / (3 * C ** 0.5)).requires_grad_(True)      # (the BN-folded kernel)
        bias = torch.randn(C, generator=gen).double()
        scale = (torch.rand(C, generator=gen) + 0.5).double()
        dy = _bf(torch.randn(N, H, W, C, generator=gen))
        msk = _bf(torch.randn(N, H, W, C, generator=gen))
        z = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), None, stride=1, padding=2, dilation=2).permute(0, 2, 3, 1)
        y = torch.relu(z + bias).detach()
        z.backward(dy)
        _REF[key] = dict(N=N, x=x.detach(), w=w.detach(), bias=bias, scale=scale, dy=dy, msk=msk, y=y,
                         dx=(x.grad * (msk > 0)).detach(), dw=(w.grad * scale).detach())
    return _REF[key]


def _run_modes(hip, r, H, W, C, compute):
    N = r["N"]
    st = torch.bfloat16 if compute == 1 else torch.float32
    xd, wd, dyd, md = (g(r[k].float()).to(st) for k in ("x", "w", "dy", "msk"))
    bias, scale = g(r["bias"].float()), g(r["scale"].float())
    y = torch.full((N, H, W, C), 7.0, device=DEV, dtype=st)
    bits = torch.full((N, H, W, C // 8), 0xAA, device=DEV, dtype=torch.uint8) if compute == 1 else None
    hip.conv3x3(0, xd, wd, y, N, H, W, C, H, W, C, 1, pad=2, bias=bias, act=1, compute=compute, maskbits_out=bits, dilation=2)
    dx = torch.full((N, H, W, C), 7.0, device=DEV, dtype=st)
    hip.conv3x3(1, dyd, wd, dx, N, H, W, C, H, W, C, 1, pad=2, mask=md, compute=compute, dilation=2)
    dw = torch.zeros(3, 3, C, C, device=DEV)
    hip.conv3x3(2, xd, dyd, dw, N, H, W, C, H, W, C, 1, pad=2, scale=scale, compute=compute, dilation=2)
    torch.cuda.synchronize()
    return y, dx, dw, bits


@pytest.mark.parametrize("compute", [0, 1, 2])
@pytest.mark.parametrize("H,W,C", CASES)
def test_conv3x3_dilated_all_modes(hip, H, W, C, compute):
    """Modes 0 / 1 / 2 with the engine's epilogues (folded-BN kernel + bias + ReLU [+ mask bits in bf16]; ReLU mask; per-channel scale):
    5x7 has planes of 3x4, 3x3, 2x4 and 2x3 pixels, 1x3 an empty plane and 2x2 single-pixel planes, 13x21 more than one (ragged) 4-row
    tile per plane; 64 / 128 / 512 channels are the bf16 dispatch's halo<64>, LDS-DMA and layer4 routes.  Two runs are bit-identical."""
    hip.ensure_workspace(DEV)
    r = _reference(H, W, C)
    y, dx, dw, bits = _run_modes(hip, r, H, W, C, compute)
    if compute == 1:
        one_bf16_rounding(y, r["y"], f"dilated fwd bf16 {H}x{W}x{C}")
        one_bf16_rounding(dx, r["dx"], f"dilated dgrad bf16 {H}x{W}x{C}")
        close(dw, r["dw"], 2e-5, f"dilated wgrad bf16 {H}x{W}x{C}")
        want = ((y.float() > 0).view(r["N"], H, W, C // 8, 8).to(torch.int32) << torch.arange(8, device=DEV, dtype=torch.int32)).sum(-1)
        assert torch.equal(bits.to(torch.int32), want), "maskbits_out is not (y > 0)"
    else:
        what = "fp32" if compute == 0 else "fp32x3"
        close(y, r["y"], 2e-5, f"dilated fwd {what} {H}x{W}x{C}")
        close(dx, r["dx"], 2e-5, f"dilated dgrad {what} {H}x{W}x{C}")
        close(dw, r["dw"], 5e-5, f"dilated wgrad {what} {H}x{W}x{C}")
    y2, dx2, dw2, bits2 = _run_modes(hip, r, H, W, C, compute)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dw, dw2), "two runs differ"
    if bits is not None:
        assert torch.equal(bits, bits2)


# ------------------------------------------------------------------------------------------
# tiny model: the configuration of tests/golden/tiny_r50_e1d2_64x96.npz (ResNet-50, 1 encoder, 2 decoder layers), freshly seeded
# ------------------------------------------------------------------------------------------
DC5 = (False, False, True)
TH, TW = 72, 104                  # -> 5 x 7 feature map with layer4 dilated (odd x odd)


def _tiny(precision="fp32", flags=DC5, seed=7, **kw):
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.training_config import TrainingConfig
    from oracle import detr_ref as R
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
    cfg.target_batch = None
    model = get_detr_model(cfg, include_top=True, num_encoder_layers=1, num_decoder_layers=2, device="cuda:0", precision=precision,
                           replace_stride_with_dilation=flags, **kw)
    params = R.make_params(seed, num_enc=1, num_dec=2)
    model.load_weights(params)
    return model, cfg, params


def _images(B=2, H=TH, W=TW, seed=0):
    return np.random.default_rng(seed).normal(size=(B, H, W, 3)).astype(np.float32)


_ORACLE = {}


def _oracle(flags):
    """dc5_ref forward (float32 torch on the CPU, as test_forward_taps_vs_oracle runs the oracle) with taps, once per flag set."""
    import dc5_ref
    from oracle import detr_ref as R
    if flags not in _ORACLE:
        params = R.make_params(7, num_enc=1, num_dec=2)
        taps = {}
        out = dc5_ref.detr_forward_dc5(torch.from_numpy(_images()), R.to_torch(params), flags=flags, num_enc=1, num_dec=2, taps=taps)
        _ORACLE[flags] = (out, taps)
    return _ORACLE[flags]


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
@pytest.mark.parametrize("flags", [DC5, (True, True, True)])
def test_dc5_forward_taps_vs_ref(hip, precision, flags):
    """layer4 output, memory, logits and boxes against dc5_ref at the bounds of tests/test_gpu_model.py:86,90,92-93
    (test_forward_taps_vs_oracle: backbone taps 1e-4, memory / logits / boxes 2e-4 of the reference's largest magnitude);
    [True, True, True] runs the 128- and 256-channel dilated stages in a model."""
    model, _, _ = _tiny(precision, flags)
    out = model(torch.from_numpy(_images()).cuda(), training=False)
    ref, taps = _oracle(flags)
    eng = model.engine
    feat, Hf, Wf, L = eng._feat_meta
    assert tuple(taps["layer4"].shape[1:3]) == (Hf, Wf)
    if flags == DC5:
        assert (Hf, Wf) == (5, 7)
    for name, got, want, tol in (("layer4", eng._bufs["backbone/layer4/2:out"], taps["layer4"], 1e-4),
                                 ("memory", eng._bufs["enc0:x2"].view(2, L, 256), taps["memory"].transpose(0, 1), 2e-4),
                                 ("logits", out["pred_logits"], ref["pred_logits"], 2e-4),
                                 ("boxes", out["pred_boxes"], ref["pred_boxes"], 2e-4)):
        err = _rel(got, want)
        print(f"{precision} {flags} {name}: rel err {err:.3e} (bound {tol:.1e})")
        assert err < tol, (name, err)


def test_dc5_backward_vs_ref_autograd(hip):
    """Every gradient tensor against dc5_ref autograd in fp32, by the criterion of tests/test_gpu_model.py::test_backward_vs_oracle_autograd
    (its _grad_report: per tensor relative L2 <= 1e-2 and max-abs <= 3e-2 of the tensor's max)."""
    import math
    import dc5_ref
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    from oracle import detr_ref as R, set_loss_ref as Ls
    model, cfg, params = _tiny("fp32", dropout=0.0)
    images = _images()
    t_bbox, t_class = Ls.make_targets(2, seed=5, force_full=False)
    P = R.to_torch(params, requires_grad=True)
    ref_out = dc5_ref.detr_forward_dc5(torch.from_numpy(images), P, flags=DC5, num_enc=1, num_dec=2)
    ref_total, _ = Ls.get_losses(ref_out, torch.from_numpy(t_bbox), torch.from_numpy(t_class), 91)
    ref_total.backward()
    opt = setup_optimizers(model, cfg)
    _, total, _, _ = training.run_train_step(model, images, t_bbox, t_class, opt, cfg)
    torch.cuda.synchronize()
    assert abs(float(total) - float(ref_total)) <= 1e-3 * abs(float(ref_total))
    gmax = max(float(P[n].grad.abs().max()) for n in model.engine.P.gviews)
    bad = []
    for name, gv in model.engine.P.gviews.items():
        ref = P[name].grad.double()
        d = gv.detach().cpu().double() - ref
        l2 = float(d.norm()) / (float(ref.norm()) + 1e-6 * gmax * math.sqrt(ref.numel()))
        tol = 3e-2 * float(ref.abs().max()) + 1e-6 * gmax
        if float(d.abs().max()) > tol or l2 > 1e-2:
            bad.append((name, float(d.abs().max()), tol, l2))
    assert not bad, bad[:12]


def test_dc5_bf16_vs_fp32(hip):
    """bf16 against the fp32 run of the same model, at the project's bf16 model bound (tests/test_gpu_model.py:318,
    test_bf16_compute_mode_deviation_from_fp32_oracle: 3e-2 of the outputs' largest magnitude)."""
    imgs = torch.from_numpy(_images()).cuda()
    m32, _, _ = _tiny("fp32")
    o32 = {k: m32(imgs, training=False)[k].clone() for k in ("pred_logits", "pred_boxes")}
    m16, _, _ = _tiny("bf16")
    o16 = m16(imgs, training=False)
    for k in ("pred_logits", "pred_boxes"):
        err = _rel(o16[k], o32[k])
        print(f"bf16 vs fp32 {k}: rel err {err:.3e}")
        assert err < 3e-2, (k, err)


def test_dc5_defaults_untouched(hip):
    """replace_stride_with_dilation=None and [False] * 3 build the model that is built today: bit-identical outputs."""
    imgs = torch.from_numpy(_images()).cuda()
    a, _, _ = _tiny("fp32", None)
    oa = a(imgs, training=False)["pred_logits"].clone()
    b, _, _ = _tiny("fp32", [False] * 3)
    ob = b(imgs, training=False)["pred_logits"].clone()
    assert torch.equal(oa, ob)
    assert a.engine._feat_meta[1:3] == (3, 4)


def test_dc5_need_weights(hip):
    from detr_tf.inference import get_attention_maps
    model, _, _ = _tiny("fp32")
    _, maps = get_attention_maps(model, torch.from_numpy(_images()).cuda())
    dec = [v for k, v in maps.items() if k.endswith("/multihead_attn")]
    assert dec and all(tuple(v.shape) == (2, 100, 5, 7) for v in dec), {k: tuple(v.shape) for k, v in maps.items()}
    for v in maps.values():
        s = v.reshape(v.shape[0], v.shape[1], -1).sum(-1)
        assert float((s - 1).abs().max()) < 1e-4


def test_dc5_graphed_train_steps_equal_eager(hip):
    """Three bf16 training steps (dropout 0.1) of the layer4-dilated model: the hipGraph replay leaves every parameter bit-identical to
    the eager steps (the criterion of tests/test_gpu_padding.py::test_graphed_train_step_with_masks_equals_eager; the logged loss is a
    sum through fp32 atomics and is held to that test's LOSS_NOISE = 1e-6)."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    from oracle import set_loss_ref as Ls
    images = _images()
    t_bbox, t_class = Ls.make_targets(2, seed=5, force_full=False)
    results = {}
    for launch in ("eager", "graph"):
        model, cfg, _ = _tiny("bf16")
        opt = setup_optimizers(model, cfg)
        stepper = training.GraphedTrainStep(model, opt, cfg, eager_steps=1, launch=launch)
        losses = []
        for i in range(3):
            _, total, _ = stepper(images, t_bbox, t_class, i)
            losses.append(float(total))
        torch.cuda.synchronize()
        results[launch] = (losses, {n: v.detach().clone() for n, v in model.engine.P.views.items()})
        if launch == "graph":
            assert stepper.step_graph is not None
            assert DC5 in stepper._signature(images, t_bbox, t_class)           # the flags are part of the graph key
    print("losses", results["eager"][0], results["graph"][0])
    for n, v in results["eager"][1].items():
        assert torch.equal(v, results["graph"][1][n]), n
    for a, b in zip(results["eager"][0], results["graph"][0]):
        assert abs(a - b) <= 1e-6 * abs(a), (results["eager"][0], results["graph"][0])
    assert len(set(results["graph"][0])) == 3


def test_dc5_padded_batch(hip):
    """A 72x104 and a 56x88 image on one 72x104 canvas: the key-validity words are dc5_ref's feature mask (5 x 7, nearest), and the
    outputs equal the masked restatement on the dilated backbone at the bound of tests/test_gpu_padding.py:398-401 (2e-4).
    (The padded image is not compared with a run of the 56x88 image alone: the reference's backbone sees the zero canvas, whose
    pixels are non-zero after the stem's BN shift, so the reference itself differs between the two -- dc5_ref in fp64
    on these inputs: 4.8e-2 of the logit scale, 1.2e-2 of the box scale, far above any kernel bound.)"""
    import dc5_ref
    from detr_tf import _hip
    from oracle import detr_ref as R
    images = _images(seed=4)
    masks = np.zeros((2, TH, TW), bool)
    masks[1, 56:, :] = True
    masks[1, :, 88:] = True
    images[1][masks[1]] = 0.0
    model, _, params = _tiny("fp32", dropout=0.0)
    out = model((images, masks))
    eng = model.engine
    fm = dc5_ref.feature_mask(masks, TH, TW, DC5)
    assert tuple(fm.shape) == (2, 5, 7) and bool(fm[1].any()) and not bool(fm[0].any())
    want = _hip.keymask_words_from_valid(~fm.numpy().reshape(2, -1)).reshape(-1)
    assert np.array_equal(eng.key_valid.cpu().numpy(), want), "key_valid words differ from dc5_ref's feature mask"
    taps = {}
    ref = dc5_ref.detr_forward_dc5_masked(torch.from_numpy(images), masks, R.to_torch(params), flags=DC5, num_enc=1, num_dec=2, taps=taps)
    assert torch.equal(taps["feat_mask"], fm)
    for k in ("pred_logits", "pred_boxes"):
        err = _rel(out[k], ref[k])
        print(f"padded batch {k}: rel err {err:.3e} (bound 2.0e-04)")
        assert err < 2e-4, (k, err)


def test_dc5_full_size_bf16_vs_fp32x3(hip):
    """B = 1, 800x1333, "resnet50-dc5" (50 x 84 = 4200 keys), evaluation forward plus post-processing: bf16 logits and boxes within the
    project's bf16-vs-fp32 model bound (3e-2 of the largest magnitude, tests/test_gpu_model.py:318,760) of the fp32x3 run."""
    from detr_tf.inference import get_model_inference
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.training_config import TrainingConfig
    from oracle import detr_ref as R
    params = R.make_params(12)
    image = torch.from_numpy(_images(1, 800, 1333, seed=13)).cuda()
    outs = {}
    for precision in ("fp32x3", "bf16"):
        model = get_detr_model(TrainingConfig(), include_top=True, backbone="resnet50-dc5", precision=precision)
        assert not model.load_weights(params)
        out = model(image, training=False)
        assert model.engine._feat_meta[1:] == (50, 84, 4200)
        boxes, labels, scores = get_model_inference(out, 91, "xyxy")
        assert bool(torch.isfinite(boxes).all()) and bool(torch.isfinite(scores).all()) and boxes.shape[0] == labels.shape[0]
        outs[precision] = {k: out[k].clone() for k in ("pred_logits", "pred_boxes")}
        del model
    for k in ("pred_logits", "pred_boxes"):
        err = _rel(outs["bf16"][k], outs["fp32x3"][k])
        print(f"full size bf16 vs fp32x3 {k}: rel err {err:.3e} (bound 3.0e-02)")
        assert err < 3e-2, (k, err)
