"""fp64 references and the comparison of the matrix-kernel tests, shared by tests/test_gpu_guard_bands.py (operands inside NaN and
sentinel frames) and tests/test_gpu_nonfinite.py / test_nonfinite_cpu.py (NaN and Inf inside the operands): the seeded host values of a
GEMM case of tests/guard_band_cases.py and its reference in the order of the epilogue, the 3x3 convolution and stem problems with their
forward, input-gradient and weight-gradient results, and check_close, the tolerance of each kernel family's older test."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import guard_band_cases as G


def check_close(got, ref, tol, what):
    """Assertions (a) and (b).  tol: see guard_band_cases.gcase."""
    got, ref = got.detach().float().cpu().double(), ref.double()
    assert bool(torch.isfinite(got).all()), f"{what}: NaN / Inf in the output ({int((~torch.isfinite(got)).sum())} of {got.numel()} elements)"
    scale = float(ref.abs().max()) + 1e-30
    err = (got - ref).abs()
    if tol in ("b16", "b16conv"):               # one bf16 rounding (test_gemm_stream_bf16_short_k; the halo tests use 1.1)
        rel = float((err / (ref.abs() + 1e-2 * scale)).max())
        bound = 2.0 ** -8 * (1.05 if tol == "b16" else 1.1)
        assert rel < bound, f"{what}: {rel:.3e} >= {bound:.3e}: more than one bf16 rounding from fp64"
        return
    rtol = {"f32": 2e-5, "split": 5e-5, "ring32": 2.0 ** -16, "ring16": 2.0 ** -7, "stem16": 3e-3}[tol]
    assert float(err.max()) <= rtol * scale, f"{what}: max abs err {float(err.max()):.3e} > {rtol * scale:.3e} (scale {scale:.3e})"


@functools.lru_cache(maxsize=8)
def _gemm_values(M, N, K, low, add_rows):
    """Host values of every operand a case on this shape may take (one draw order, so that the variants of a shape share them).
    low: bf16-representable values (bf16 compute / storage: the fp64 reference is then on the same stored values)."""
    gen = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    r = lambda *s: torch.randn(*s, generator=gen)
    q = G.bf if low else (lambda t: t)
    v = dict(A=q(r(M, K)), B=q(r(K, N) / K ** 0.5), bias=r(N), scale=torch.rand(N, generator=gen) + 0.5, residual=q(r(M, N)), mask=q(r(M, N)),
             ln_gamma=torch.rand(N, generator=gen) + 0.5, ln_beta=r(N))
    v["maskbits"] = G.pack_bits(r(M, (N + 7) // 8 * 8) > 0)
    if add_rows:
        v["ln_add"] = r(add_rows, N)
    return v


def gemm_values(c):
    v = dict(_gemm_values(c["M"], c["N"], c["K"], c["compute"] == 1, c["ln"]["add_rows"] if c["ln"] and c["ln"]["add"] else 0))
    if not c["ak"]:
        v["A"] = v["A"].t().contiguous()
    if c["bk"]:
        v["B"] = v["B"].t().contiguous()
    if c["mask"] == "bits":
        v["mask"] = v["maskbits"]
    return v


def gemm_reference(c, v):
    """fp64, in the order of gemm_core.h epi_one: (acc * scale + bias) * alpha, dropout (in front of a residual), + residual,
    activation, dropout (without a residual), mask."""
    from oracle import dropout_ref as DR
    M, N = c["M"], c["N"]
    A, B = v["A"].double(), v["B"].double()
    acc = (A if c["ak"] else A.t()) @ (B.t() if c["bk"] else B)
    sc = v["scale"].double() if c["scale"] else 1.0
    if c["split"] > 1:
        return C0 + c["alpha"] * acc * sc
    x = (acc * sc + (v["bias"].double() if c["bias"] else 0.0)) * c["alpha"]
    keep = None
    if c["p"] > 0.0:
        keep = torch.from_numpy(DR.keep_mask(DR.drop_key(G.DROP_SITE, G.DROP_STEP), np.arange(M * N).reshape(M, N), c["p"]))
    if keep is not None and c["res"]:
        x = torch.where(keep, x / (1.0 - c["p"]), torch.zeros_like(x))
    if c["res"]:
        x = x + v["residual"].double()
    if c["act"] == 1:
        x = torch.relu(x)
    elif c["act"] == 2:
        x = torch.sigmoid(x)
    if keep is not None and not c["res"]:
        x = torch.where(keep, x / (1.0 - c["p"]), torch.zeros_like(x))
    if c["mask"]:
        on = G.unpack_bits(v["mask"], N) if c["mask"] == "bits" else v["mask"] > 0
        x = torch.where(on, x, torch.zeros_like(x))
    return x


C0, RS0 = 0.25, 0.5          # what a split-K launch accumulates onto: C and the fused row sums


@functools.lru_cache(maxsize=None)
def conv_problem(N, H, W, Ci, Co, stride, dil, low):
    """Host values and fp64 results of one convolution, computed once and shared by every case on it."""
    gen = torch.Generator().manual_seed(N * 1000 + H * 100 + W + Ci + Co + stride + dil)
    r = lambda *s: torch.randn(*s, generator=gen)
    q = G.bf if low else (lambda t: t)
    Ho, Wo = (H + 2 * dil - 2 * dil - 1) // stride + 1, (W + 2 * dil - 2 * dil - 1) // stride + 1
    x, w = q(r(N, H, W, Ci)), q(r(3, 3, Ci, Co) / (3 * Ci ** 0.5))
    dy, res, msk = q(r(N, Ho, Wo, Co)), q(r(N, Ho, Wo, Co)), q(r(N, H, W, Ci))
    scale, shift = torch.rand(Co, generator=gen) + 0.5, r(Co)
    w_oihw = w.double().permute(3, 2, 0, 1).contiguous()
    z = F.conv2d(x.double().permute(0, 3, 1, 2), w_oihw, None, stride=stride, padding=dil, dilation=dil).permute(0, 2, 3, 1)
    assert z.shape == (N, Ho, Wo, Co)
    opad = (H - 1 - stride * (Ho - 1), W - 1 - stride * (Wo - 1))
    dx = F.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w_oihw, stride=stride, padding=dil, dilation=dil, output_padding=opad).permute(0, 2, 3, 1)
    assert dx.shape == (N, H, W, Ci)
    dw = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (Co, Ci, 3, 3), dy.double().permute(0, 3, 1, 2), stride=stride, padding=dil,
                                     dilation=dil).permute(2, 3, 1, 0)
    return dict(Ho=Ho, Wo=Wo, x=x, w=w, dy=dy, res=res, msk=msk, scale=scale, shift=shift, z=z, dx=dx, dw=dw)


def stem_problem(N, H, W, low):
    return _stem_problem(N, H, W, bool(low))


@functools.lru_cache(maxsize=None)
def _stem_problem(N, H, W, low):
    gen = torch.Generator().manual_seed(N + H + W)
    r = lambda *s: torch.randn(*s, generator=gen)
    q = G.bf if low else (lambda t: t)
    img, w = q(r(N, H, W, 3)), q(r(7, 7, 3, 64) / 12.0)
    scale, shift = torch.rand(64, generator=gen) + 0.5, r(64)
    z = F.conv2d(F.pad(img.double().permute(0, 3, 1, 2), (3, 3, 3, 3)), w.double().permute(3, 2, 0, 1), None, stride=2).permute(0, 2, 3, 1)
    Ho, Wo = z.shape[1], z.shape[2]
    dy = q(r(N, Ho, Wo, 64))
    cols = F.unfold(F.pad(img.double().permute(0, 3, 1, 2), (3, 3, 3, 3)), 7, stride=2).view(N, 3, 49, Ho, Wo).permute(0, 3, 4, 2, 1).reshape(N, Ho, Wo, 147)
    dw = torch.einsum("nhwk,nhwc->kc", cols, dy.double())
    return dict(Ho=Ho, Wo=Wo, img=img, w=w, scale=scale, shift=shift, z=z, dy=dy, dw=dw)
