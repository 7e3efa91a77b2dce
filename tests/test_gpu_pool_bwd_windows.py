"""maxpool_bwd_kernel enumerates the (<= 2 x 2) windows that can have selected a pixel instead of walking the nine taps: checked
bit for bit against a plain loop over the taps in NumPy (same fp32 adds in the same (kh, kw) order, one rounding to the storage
type), on odd, even and degenerate maps, for the 8- and 4-channel bf16 lane forms and fp32, with inputs that hold negatives,
exact zeros, ties inside a window and border windows won by the zero padding."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _reference(dy, am, x):
    """dx = (x > 0) * sum over the windows whose argmax is the pixel, taps in kh-major order (the forward's numbering)."""
    N, H, W, C = x.shape
    _, Ho, Wo, _ = dy.shape
    dx = np.zeros_like(x)
    for h in range(H):
        for w in range(W):
            g = np.zeros((N, C), dtype=np.float32)
            for kh in range(3):
                th = h + 1 - kh
                if th < 0 or th & 1 or th // 2 >= Ho:
                    continue
                for kw in range(3):
                    tw = w + 1 - kw
                    if tw < 0 or tw & 1 or tw // 2 >= Wo:
                        continue
                    sel = am[:, th // 2, tw // 2, :] == kh * 3 + kw
                    g = np.where(sel, g + dy[:, th // 2, tw // 2, :], g).astype(np.float32)
            dx[:, h, w, :] = np.where(x[:, h, w, :] > 0, g, np.float32(0))
    return dx


def _inputs(N, H, W, C, seed):
    gen = torch.Generator().manual_seed(seed)
    vals = torch.tensor([-2.0, -0.5, 0.0, 0.0, 0.25, 0.5, 1.0])            # exact in bf16; few values: ties and zeros everywhere
    x = vals[torch.randint(0, len(vals), (N, H, W, C), generator=gen)]
    x[..., 1] = -x[..., 1].abs()                                            # a channel whose border windows the zero padding wins
    x[:, 0, :, 2] = 0.0                                                     # all-zero border windows
    x[:, :, 0, 3] = 0.0
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    return x, torch.randn(N, Ho, Wo, C, generator=gen), Ho, Wo


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("C", [8, 12, 64])            # bf16: 8 channels per lane (8, 64) and 4 (12); fp32: 4 per lane
@pytest.mark.parametrize("H,W", [(7, 9), (8, 10), (1, 1), (2, 3), (1, 6), (5, 1)])
def test_backward_equals_the_loop_over_the_taps(hip, H, W, C, dtype):
    N = 2
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    x, dy, Ho, Wo = _inputs(N, H, W, C, seed=H * 100 + W * 10 + C)
    xd, dyd = x.to(DEV).to(td).contiguous(), dy.to(DEV).to(td).contiguous()
    y = torch.empty(N, Ho, Wo, C, device=DEV, dtype=td)
    am = torch.empty(N, Ho, Wo, C, device=DEV, dtype=torch.uint8)
    hip.call(f"detr_hip_maxpool3x3s2_fwd_{dtype}", xd.data_ptr(), y.data_ptr(), am.data_ptr(), N, H, W, C, Ho, Wo)
    dx = torch.full_like(xd, 3.0)
    hip.call(f"detr_hip_maxpool3x3s2_bwd_{dtype}", dyd.data_ptr(), am.data_ptr(), xd.data_ptr(), dx.data_ptr(), N, H, W, C, Ho, Wo)
    torch.cuda.synchronize()
    want = _reference(dyd.float().cpu().numpy(), am.cpu().numpy(), xd.float().cpu().numpy())
    want = torch.from_numpy(want).to(td)                                    # one RNE rounding, as in the kernel
    bits = lambda t: t.contiguous().view(torch.int16 if td == torch.bfloat16 else torch.int32)
    assert torch.equal(bits(dx.cpu()), bits(want))
    xf = xd.float()
    assert bool((xf < 0).any()) and bool((xf == 0).any()) and bool((y.float() == 0).any())
    if H * W > 1:
        assert bool((dx.float() != 0).any())
    # every dy term lands on at most one pixel (its window's argmax): sum |dx| <= sum |dy|, up to the bf16 rounding of dx (2^-9)
    assert float(dx.float().abs().sum()) <= float(dyd.float().abs().sum()) * (1 + 1e-2) + 1e-3
