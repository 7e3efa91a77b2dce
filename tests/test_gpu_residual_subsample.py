"""The residual row map of the GEMM epilogues (detr_gemm_desc.res_sub_*): the input gradient of a stride-2 projection shortcut
stays the compact [B, ho, wo, N] tensor and the block's last GEMM adds it at the even pixels of its [B, h, w, N] output.  The old
way -- detr_hip_subsample2_bwd_f32 into a zero-filled full-resolution tensor, then the same GEMM with a plain residual -- does
the same arithmetic on every element (x + 0.0 for the pixels in between), so every comparison here is bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FAMILY = {"tile": 0, "stream": 1, "ring": 2}          # detr_hip_gemm_family


@pytest.fixture(autouse=True)
def _reset_library_tuning():
    import os
    yield
    from detr_tf import _hip
    for k in ("DETR_HIP_GEMM_RING", "DETR_HIP_STREAM_NW"):
        if k in os.environ:
            _hip.set_tuning(k, None)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _pack_bits(t):
    """[M, N] bool -> [M, N / 8] uint8, bit (n & 7) of byte n / 8 (detr_gemm_desc.maskbits_out)."""
    M, N = t.shape
    w = (2 ** torch.arange(8, dtype=torch.int32, device=t.device)).view(1, 1, 8)
    return (t.view(M, N // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def _case(hip, route, B, h, w, K, N, mask_kind, seed):
    """One consumer GEMM both ways; returns (new, old, plain) outputs."""
    ho, wo = (h + 1) // 2, (w + 1) // 2
    M = B * h * w
    gen = torch.Generator().manual_seed(seed)
    b16 = lambda t: t.to(DEV).to(torch.bfloat16).contiguous()
    A = b16(torch.randn(M, K, generator=gen))
    Wt = b16(torch.randn(N, K, generator=gen) / K ** 0.5)                  # [n][k]: the layout of the block's last input-gradient GEMM
    dxs = b16(torch.randn(B * ho * wo, N, generator=gen))
    act = b16(torch.randn(M, N, generator=gen))                            # the saved activation whose sign masks the gradient
    mask = {"none": None, "bf16": act, "bits": _pack_bits(act.float() > 0)}[mask_kind]
    ldmask = 0 if mask is None else mask.stride(0)
    # the old way: scatter into a zero-filled tensor (the kernel copies 16-byte chunks: bf16 passes as N / 2 "floats")
    idg = torch.full((M, N), 7.0, device=DEV, dtype=torch.bfloat16)        # every element is overwritten
    hip.call("detr_hip_subsample2_bwd_f32", dxs.data_ptr(), idg.data_ptr(), B, h, w, N // 2, ho, wo)
    args = lambda C: (M, N, K, A, K, 1, Wt, K, 1, C, N)
    d, _ = hip._gemm_desc(*args(torch.empty(M, N, device=DEV, dtype=torch.bfloat16)), residual=dxs, ldr=N, mask=mask, ldmask=ldmask,
                          compute=1, res_sub=(h, w))
    assert hip.load().detr_hip_gemm_family(ctypes.byref(d)) == FAMILY[route], "the case does not reach the epilogue it is meant for"
    old = torch.full((M, N), 3.0, device=DEV, dtype=torch.bfloat16)
    new = torch.full((M, N), 5.0, device=DEV, dtype=torch.bfloat16)
    plain = torch.full((M, N), 9.0, device=DEV, dtype=torch.bfloat16)
    hip.gemm(*args(old), residual=idg, ldr=N, mask=mask, ldmask=ldmask, compute=1)
    hip.gemm(*args(new), residual=dxs, ldr=N, mask=mask, ldmask=ldmask, compute=1, res_sub=(h, w))
    hip.gemm(*args(plain), mask=mask, ldmask=ldmask, compute=1)
    torch.cuda.synchronize()
    return new, old, plain


# (route, tuning, B, h, w, K, N): the three epilogue routes at odd maps, then even maps and the degenerate one-row / one-column
# maps on each of them.  No M = B * h * w is a multiple of 32 (the strip / tile height): every case ends in a ragged strip.
CASES = [
    ("stream", {}, 2, 91, 93, 64, 64),                      # M = 16926: just over the kernel's M >= 16384 gate, odd h and w
    ("stream", {}, 2, 91, 93, 128, 256),                    # K = 128: two slice pairs per 8-wave workgroup (layer2's first block)
    ("stream", {"DETR_HIP_STREAM_NW": "1"}, 2, 91, 93, 128, 256),      # ... and one slice per wave, four slices per workgroup
    ("stream", {}, 2, 91, 93, 256, 128),                    # K = 256: two slices per wave (layer3's first block)
    ("stream", {}, 205, 8, 10, 64, 64),                     # even map, M = 16400
    ("stream", {}, 2, 1, 8197, 64, 64),                     # one-row maps
    ("stream", {}, 2, 8197, 1, 64, 64),                     # one-column maps
    ("ring", {"DETR_HIP_GEMM_RING": "1"}, 2, 13, 11, 256, 128),
    ("ring", {"DETR_HIP_GEMM_RING": "1"}, 3, 8, 10, 256, 128),
    ("ring", {"DETR_HIP_GEMM_RING": "1"}, 3, 1, 13, 256, 128),
    ("ring", {"DETR_HIP_GEMM_RING": "1"}, 3, 13, 1, 256, 128),
    ("tile", {}, 2, 7, 9, 64, 64),
    ("tile", {}, 3, 8, 10, 64, 64),
    ("tile", {}, 3, 1, 7, 64, 64),
    ("tile", {}, 3, 7, 1, 64, 64),
]


@pytest.mark.parametrize("mask_kind", ["bits", "bf16", "none"])
@pytest.mark.parametrize("route,tuning,B,h,w,K,N", CASES)
def test_mapped_residual_equals_scatter_then_plain_residual(hip, route, tuning, B, h, w, K, N, mask_kind):
    for k, v in tuning.items():
        hip.set_tuning(k, v)                                  # (re-read through the library's re-read call; reset by the fixture)
    assert (B * h * w) % 32 != 0
    new, old, plain = _case(hip, route, B, h, w, K, N, mask_kind, seed=B * 1000 + h * 10 + w + K)
    assert torch.equal(_bits(new), _bits(old)), f"{int((_bits(new) != _bits(old)).sum())} of {new.numel()} elements differ"
    # the residual did something, and only at the even pixels
    diff = (_bits(new) != _bits(plain)).view(B, h, w, N)
    assert bool(diff[:, ::2, ::2].any())
    odd = diff.clone()
    odd[:, ::2, ::2] = False
    assert not bool(odd.any())


def test_map_on_an_epilogue_without_it_is_an_error(hip):
    """fp32 C / residual (the 4-column epilogues of every compute mode), a missing residual and an inconsistent map: each is
    rejected with an error, never ignored."""
    B, h, w, K, N = 2, 7, 9, 64, 64
    M, Ms = B * h * w, B * 4 * 5
    A = torch.randn(M, K, device=DEV)
    Wt = torch.randn(N, K, device=DEV)
    C = torch.full((M, N), 3.0, device=DEV)
    dxs = torch.randn(Ms, N, device=DEV)
    for compute in (0, 1, 2):
        with pytest.raises(RuntimeError, match="residual row map"):
            hip.gemm(M, N, K, A, K, 1, Wt, K, 1, C, N, residual=dxs, ldr=N, compute=compute, res_sub=(h, w))
    A16, W16, C16, d16 = (t.to(torch.bfloat16) for t in (A, Wt, C, dxs))
    with pytest.raises(RuntimeError, match="residual row map"):           # fp32 residual next to a bf16 C
        hip.gemm(M, N, K, A16, K, 1, W16, K, 1, C16, N, residual=dxs, ldr=N, compute=1, res_sub=(h, w))
    with pytest.raises(RuntimeError, match="residual row map"):           # no residual at all
        hip.gemm(M, N, K, A16, K, 1, W16, K, 1, C16, N, compute=1, res_sub=(h, w))
    with pytest.raises(RuntimeError, match="residual row map"):           # M is not whole maps
        hip.gemm(M, N, K, A16, K, 1, W16, K, 1, C16, N, residual=d16, ldr=N, compute=1, res_sub=(h, w + 1))
    d, _ = hip._gemm_desc(M, N, K, A16, K, 1, W16, K, 1, C16, N, residual=d16, ldr=N, compute=1, res_sub=(h, w))
    d.res_sub_ho = 3                                                        # not (h + 1) / 2
    assert hip.load().detr_hip_gemm_f32(ctypes.byref(d), None) != 0
    assert "residual row map" in hip.load().detr_hip_last_error().decode()
    torch.cuda.synchronize()
    assert bool((C == 3.0).all()) and bool((C16.float() == 3.0).all())     # nothing was launched


def test_engine_strided_first_block_backward_equals_the_scatter_path(hip, monkeypatch):
    """A bf16 train step at 56 x 72: layer2's first block works on a 14 x 18 map (7 x 9 after its stride), layer3's on 7 x 9 and
    layer4's on 4 x 5.  Every GEMM the backward issues with a residual row map is recomputed by hand the old way -- its compact
    residual scattered into a zero-filled tensor, then the same GEMM with a plain residual -- from the operands it actually had."""
    from detr_tf import _hip, training
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.optimizers import setup_optimizers
    from detr_tf.training_config import TrainingConfig
    from oracle import detr_ref as R, set_loss_ref as L
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
    cfg.target_batch = None
    model = get_detr_model(cfg, include_top=True, num_encoder_layers=1, num_decoder_layers=1, dropout=0.0, precision="bf16")
    assert not model.load_weights(R.make_params(5, num_enc=1, num_dec=1))
    images = np.random.default_rng(3).normal(size=(2, 56, 72, 3)).astype(np.float32)
    t_bbox, t_class = L.make_targets(2, seed=9, force_full=False)
    seen = []
    real_gemm = _hip.gemm

    def spy(*a, **kw):
        real_gemm(*a, **kw)
        if kw.get("res_sub") is not None:
            keep = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()}
            seen.append((a[:3], a[3].clone(), a[4:6], a[6].clone(), a[7:9], a[9].clone(), a[10], keep))
    monkeypatch.setattr(_hip, "gemm", spy)
    training.run_train_step(model, images, t_bbox, t_class, setup_optimizers(model, cfg), cfg)
    torch.cuda.synchronize()
    monkeypatch.setattr(_hip, "gemm", real_gemm)
    assert sorted(kw["res_sub"] for *_, kw in seen) == [(4, 5), (7, 9), (14, 18)]
    assert not any(k.startswith("scratch:idg:") and k.split(":")[2] in ("256", "512", "1024") for k in model.engine._bufs)
    for (M, N, K), A, la, Bw, lb, C_new, ldc, kw in seen:
        h, w = kw.pop("res_sub")
        dxs = kw.pop("residual")
        assert dxs.dtype == torch.bfloat16 and dxs.shape == (2, (h + 1) // 2, (w + 1) // 2, N) and M == 2 * h * w
        idg = torch.full((M, N), 7.0, device=DEV, dtype=torch.bfloat16)
        hip.call("detr_hip_subsample2_bwd_f32", dxs.data_ptr(), idg.data_ptr(), 2, h, w, N // 2, (h + 1) // 2, (w + 1) // 2)
        C_old = torch.full_like(C_new, 3.0)
        hip.gemm(M, N, K, A, *la, Bw, *lb, C_old, ldc, residual=idg, compute=1, **kw)
        torch.cuda.synchronize()
        assert torch.equal(_bits(C_new), _bits(C_old)), (h, w)
        assert float(C_new.float().abs().max()) > 0
