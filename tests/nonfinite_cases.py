"""NaN and Inf INSIDE the operands of the model kernels: the case tables, the poisoned host values and their fp64 references, shared by
tests/test_gpu_nonfinite.py (device) and tests/test_nonfinite_cpu.py (the references alone: the share of non-finite elements, the
routing of the GEMM cases).

The contract ("Non-finite values"): an output element is non-finite exactly where the fp64 reference of the same operation on
the same stored values is; NaN where the reference is NaN, the same-signed Inf where it is +-Inf; every other element is finite and
within the tolerance the family's older test uses.  The fp32x3 kernels split every operand into three bf16 parts (Inf, Inf - Inf = NaN,
...), so for them the reference is computed with the +-Inf of the SPLIT operands replaced by NaN ("x3" in the tables below).

Values are each family's seeded randn (tests/matrix_refs.py), so nothing overflows by itself; one NaN, one +Inf and one -Inf are planted
at chosen places, in different rows / windows, so that no accumulation holds both infinities.  The expected non-finite set always comes
from the reference, never from the kernel, and no case leaves more than a quarter of an output to it (test_nonfinite_cpu.py)."""
import numpy as np
import torch
import torch.nn.functional as F

import guard_band_cases as G
import matrix_refs as MR

NAN, INF = float("nan"), float("inf")
CAP = 0.25                 # largest share of an output that may be non-finite in the reference


def share(ref):
    return float((~torch.isfinite(ref.double())).double().mean())


def assert_same_nonfinite(got, ref, tol_name, what, close=None):
    """The contract on one output: every NaN of the reference is a NaN, the non-finite sets are equal, the infinities carry the
    reference's signs, and the finite remainder passes `close` (default: matrix_refs.check_close at tol_name)."""
    got, ref = got.detach().float().cpu().double().reshape(-1), ref.detach().double().reshape(-1)
    assert got.shape == ref.shape, f"{what}: {tuple(got.shape)} against {tuple(ref.shape)}"
    nan_r, nan_g = torch.isnan(ref), torch.isnan(got)
    lost = nan_r & ~nan_g
    assert not bool(lost.any()), (f"{what}: {int(lost.sum())} of the reference's {int(nan_r.sum())} NaN are not NaN in the output "
                                  f"(first: index {int(lost.nonzero()[0])}, output {float(got[lost][0])})")
    nf_r, nf_g = ~torch.isfinite(ref), ~torch.isfinite(got)
    diff = nf_r != nf_g
    assert not bool(diff.any()), (f"{what}: the non-finite sets differ at {int(diff.sum())} elements (first: index {int(diff.nonzero()[0])}, "
                                  f"output {float(got[diff][0])}, reference {float(ref[diff][0])})")
    inf_r = torch.isinf(ref)
    bad = inf_r & (got != ref)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} infinities of the wrong kind (first: output {float(got[bad][0]) if bad.any() else 0}, reference {float(ref[bad][0]) if bad.any() else 0})"
    fin = ~nf_r
    assert bool(fin.any()), f"{what}: no finite element left to compare"
    (close or MR.check_close)(got[fin], ref[fin], tol_name, what + " (finite remainder)")


def inf_to_nan(t):
    return torch.where(torch.isinf(t), torch.full_like(t, NAN), t)


# ------------------------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------------------------
def _pick(cases, **want):
    env = want.pop("env", None)
    for c in cases:
        if all(c[k] == v for k, v in want.items()) and (env is None or c["env"] == env):
            return dict(c)
    raise KeyError(want)


def _stream_env(nw=1):
    return {"DETR_HIP_GEMM_STREAM": 3, "DETR_HIP_STREAM_NW": nw}


_B16_ENV = {"DETR_HIP_GEMM_RING": 2, "DETR_HIP_GEMM_STREAM": 2}


def gemm_forward_cases():
    """(case, what to poison): one case per kernel family and epilogue form, picked from G.gemm_cases() (or derived from one of its
    cases where the table has no such epilogue: stated in the tag).  Poison: "A" NaN / +Inf / -Inf in three rows of A (first tile,
    last partial row block, the middle), "B" NaN in the last column of B, "bias" NaN in one entry, "res" NaN in one element.
    The GEMM + LayerNorm cases take A and res only: a NaN column would leave no finite row of ln_y.
    x3: the fp32x3 exception, +-Inf of A and B are NaN in the reference."""
    T = G.gemm_cases()
    out = []
    add = lambda c, poison, tag=None: out.append((dict(c, tag=c["tag"] + ("-" + tag if tag else "")), poison))
    full = ("A", "B", "bias", "res")
    add(_pick(T, group="f32tile", tag="vec", ak=1, bk=1, env={}), ("A", "B"))                                   # act 0, plain store
    add(_pick(T, group="f32tile", tag="odd", ak=0, bk=0, env={"DETR_HIP_GEMM_TILE": 2}), ("A", "B"))
    for act in (0, 1, 2):                                                                                      # fp32 tile engine, full epilogue, mask as values
        add(_pick(T, group="epi", compute=0, tag=f"aligned-act{act}"), full)
    add(_pick(T, group="epi", compute=0, tag="ldc53-act1"), full)                                              # its scalar epilogue
    add(_pick(T, group="epi", compute=0, tag="aligned-drop"), full)
    for act in (0, 1, 2):                                                                                      # bf16 compute, 4-wave engine
        add(_pick(T, group="epi", compute=1, tag=f"aligned-act{act}"), full)
    add(_pick(T, group="bf16c", tag="vec", ak=1, bk=1, env={}), ("A", "B"))
    add(_pick(T, group="f32x3", tag="vec", ak=1, bk=1, env={"DETR_HIP_SPLIT3_ALL": 1}), ("A", "B"))            # x3
    add(dict(_pick(T, group="epi", compute=0, tag="aligned-act1"), compute=2, env={"DETR_HIP_SPLIT3_ALL": 1}), full, "x3")      # x3, derived: ReLU epilogue
    for M in (200, 75):                                                                                        # bf16 storage on the tile engine
        add(_pick(T, group="b16tile", M=M, bk=1, tag="wide", env=_B16_ENV), full)
    add(_pick(T, group="b16tile", M=200, bk=0, tag="narrow", env=dict(_B16_ENV, DETR_HIP_GEMM_K64=1)), full)   # _k64
    add(_pick(T, group="b16tile", M=200, bk=1, tag="wide", env=dict(_B16_ENV, DETR_HIP_EPI_WIDE=2)), full)     # wide16 epilogue
    add(_pick(T, group="b16tile", M=200, bk=1, tag="bits", env=dict(_B16_ENV, DETR_HIP_EPI_WIDE=2)), full)     # mask as bits, bits out
    add(_pick(T, group="b16tile", M=75, bk=0, tag="drop", env=_B16_ENV), full)
    s = dict(group="stream", M=16384 + 37, N=64, K=64)                                                         # streaming
    add(_pick(T, tag="res_relu", bk=1, env=_stream_env(), **s), full)
    add(_pick(T, tag="res_relu_bits", bk=0, env=_stream_env(), **s), full)
    add(_pick(T, tag="res_maskbits", bk=1, env=_stream_env(), **s), full)                                      # act 0, mask as bits
    add(_pick(T, tag="mask16", bk=1, env=_stream_env(), **s), full)                                            # act 0, mask as values
    add(dict(_pick(T, tag="mask16", bk=1, env=_stream_env(), **s), mask=None), full, "nomask")                  # act 0, derived: nothing behind the store
    add(_pick(T, group="stream", M=16384 + 37, N=256, K=128, tag="res_relu", bk=1, env=_stream_env(0)), full)   # two column groups per wave
    add(_pick(T, group="stream", tag="ext", bk=1, env=_stream_env(1)), full)                                   # alpha, dropout, ReLU
    for tag in ("auto-b16", "auto-f32", "ns2-b16", "bn128-f32"):                                               # ring, bf16 operands
        add(_pick(T, group="ring", M=33, N=256, K=192, bk=1, tag=tag), full)
    add(_pick(T, group="ring", M=600, tag="auto-b16", bk=0), full)
    add(_pick(T, group="ring", tag="drop"), full)
    for tag in ("res_mask", "bias_relu"):                                                                      # ring, fp32
        add(_pick(T, group="ring32", M=33, bk=1, tag=tag, env={"DETR_HIP_GEMM_RING": 1}), full)
    add(_pick(T, group="ring32", M=600, bk=0, tag="bias_relu", env={"DETR_HIP_GEMM_RING": 1, "DETR_HIP_RING_ROWS": 96}), full)
    for tag, K in (("a32-full", 72), ("a16-plain", 256), ("a16-full", 256)):                                   # GEMM + LayerNorm
        add(_pick(T, group="ln", M=37, K=K, tag=tag), ("A", "res"))
    return out


def _a_index(c, m, k):
    return (m, k) if c["ak"] else (k, m)


def _b_index(c, k, n):
    return (n, k) if c["bk"] else (k, n)


def gemm_poison_places(c):
    """Logical (row, k) of the three specials of A and the (k, column) of B's NaN, the bias entry and the residual element: the first
    tile; the last row (a partial 32-row block at every M of the tables), the last k (the last slab of a split) and the last column (a
    partial column block wherever N is no multiple of the tile); the middle."""
    M, N, K = c["M"], c["N"], c["K"]
    return dict(a_nan=(1, 2), a_pinf=(M - 1, K - 1), a_ninf=(M // 2, K // 2), b_nan=(3 % K, N - 1), bias=5, res=(7 % M, 9))


def gemm_poisoned(c, poison):
    """(values with the specials planted, values the reference reads): copies of matrix_refs.gemm_values."""
    v = {k: t.clone() for k, t in MR.gemm_values(c).items()}
    P = gemm_poison_places(c)
    if "A" in poison:
        v["A"][_a_index(c, *P["a_nan"])] = NAN
        v["A"][_a_index(c, *P["a_pinf"])] = INF
        v["A"][_a_index(c, *P["a_ninf"])] = -INF
    if "B" in poison:
        v["B"][_b_index(c, *P["b_nan"])] = NAN
    if "bias" in poison and c["bias"]:
        v["bias"][P["bias"]] = NAN
    if "res" in poison and c["res"]:
        v["residual"][P["res"]] = NAN
    vr = dict(v)
    if c["compute"] == 2:                      # the fp32x3 exception
        vr["A"], vr["B"] = inf_to_nan(v["A"]), inf_to_nan(v["B"])
    return v, vr


def gemm_refs(c, v, vr):
    """{output: fp64 reference} of a forward or split-K case: C, the fused row sums, the LayerNorm outputs."""
    ref = {"C": MR.gemm_reference(c, vr)}
    if c["rowsum"]:
        A = vr["A"].double()
        ref["rowsum_a"] = MR.RS0 + c["alpha"] * (A.sum(1) if c["ak"] else A.sum(0))
    if c["ln"] is not None:
        ref.update(layernorm_forward_ref(ref["C"], v["ln_gamma"], v["ln_beta"], G.LN_EPS))
        ref = {("ln_" + k if k in ("y", "mean", "rstd") else k): t for k, t in ref.items()}
        if c["ln"]["add"]:
            ref["ln_y2"] = ref["ln_y"] + v["ln_add"].double()[torch.arange(c["M"]) % c["ln"]["add_rows"]]
    return ref


def split_cases():
    """Split-K and the ring weight gradient (both operands reduction-major: A is x, B is dY): NaN / +Inf / -Inf in A and NaN in dY, the
    +Inf and dY's NaN at a k of the last slab."""
    T = G.split_cases()
    return [_pick(T, tag="f32"), _pick(T, tag="bf16c-rowsum", M=136), _pick(T, tag="f32-rowsum"), _pick(T, tag="ringwgrad", M=264),
            _pick(T, tag="ringwgrad", M=120)]


def group_members():
    """The members of test_gemm_group_shares_of_an_exactly_sized_workspace; member i gets the specials of gemm_poisoned."""
    return [G.gcase("group", 136, 72, 8 * 331, 0, 0, split=5, compute=1, scale=1, alpha=0.5, rowsum=1, lda=140, ldb=76, ldc=76, tol="split"),
            G.gcase("group", 264, 136, 2100, 0, 0, split=3, compute=1, alpha=0.5, lda=268, ldb=140, ldc=140, tol="split"),
            G.gcase("group", 64, 256, 1000, 0, 0, split=4, compute=1, scale=1, alpha=0.5, lda=68, ldb=260, ldc=260, tol="split")]


def bwd_fused_problem(M):
    """conv1x1_bwd_fused at M rows (the values of the guard-band test) with NaN, +Inf and -Inf in dy, in three rows and three columns.
    da = where(a > 0, dy w^T, 0): the NaN row is NaN where the mask is positive and 0 where it is not (both occur: asserted);
    dw = dw0 + alpha * scale * (a^T dy): the three columns."""
    gen = torch.Generator().manual_seed(M)
    d1, d2 = 64, 256
    dy, a, w = (G.bf(torch.randn(*s, generator=gen)) for s in ((M, d2), (M, d1), (d1, d2)))
    scale, dw0 = torch.rand(d2, generator=gen) + 0.5, torch.randn(d1, d2, generator=gen)
    dy[1, 2], dy[M - 1, d2 - 1], dy[M // 2, 100] = NAN, INF, -INF
    da = torch.where(a > 0, dy.double() @ w.double().t(), torch.zeros(M, d1, dtype=torch.float64))
    dw = dw0.double() + 0.5 * scale.double()[None, :] * (a.double().t() @ dy.double())
    assert bool(torch.isnan(da[1]).any()) and bool((da[1] == 0).any())
    return dict(dy=dy, a=a, w=w, scale=scale, dw0=dw0, da=da, dw=dw)


# ------------------------------------------------------------------------------------------------------------------------
# 3x3 convolutions and the stem
# ------------------------------------------------------------------------------------------------------------------------
CONV_SHAPE = (2, 9, 11)        # the smallest of G.CONV_SHAPES with an interior pixel (2 x 5 x 33 and 3 x 2 x 3 have too few rows for one
#                                whose window and whose neighbours' windows stay off the padding)


def conv_cases():
    """One case per 3x3 kernel from G.conv_cases(): fp32 tile, bf16 tile, f32x3 (x3), halo-staged, LDS-DMA, stride 2 (tile and the
    halo kernel's class form), dilation 2 (tile and halo planes)."""
    T = G.conv_cases()
    ids = ["f32tile0-16x32-s1", "f32tile0-64x64-s2", "b16tile3-64x64-s1", "b16tile1-128x128-s2", "x3t1-64x64-s1", "x3t3-128x128-s2", "halo3-64x64-s1",
           "halo4-128x128-s1", "dma-128x128-s1", "s2halo-128x128-s2", "dil2-f32-64x64-s1", "dil2-b16-halo-64x64-s1"]
    by = {c["id"]: c for c in T}
    return [by[i] for i in ids]


def wgrad_cases():
    T = {c["id"]: c for c in G.wgrad_cases()}
    return [T[i] for i in ("f32-64x64-s1-k5", "fused16-64x64-s1-k5", "pertap16-64x64-s2-k7", "fused16s2-64x64-s2-k5", "x3-64x64-s2-k7", "dil2-64x64-s1-k5")]


def conv_poisoned(c, shape=CONV_SHAPE):
    """The tensors of matrix_refs.conv_problem with the specials planted and the fp64 results on them.
    x: NaN at the corner pixel (0, 0, 0) -- its halo is zero padding -- and at the interior pixel (0, 4, 5), +Inf at (1, 2, 2), -Inf at
    (1, 6, 8): windows that do not meet, at dilation 2 either.  w: NaN at tap (0, 0) of the last output channel.  dy: the same four
    pixels scaled to the output map.  The weights of the input gradient stay finite: where a tap of a border pixel has no window, the
    stride-1 kernels multiply the weight with the zero padding of dy (0 * NaN) and the stride-2 class forms skip it, the exact
    gradient has no such term, and the forward of a non-finite weight has poisoned a whole channel of the loss anyway -- the contract
    leaves those border elements open.
    The reference convolves the explicitly zero-padded map, as the network does (ZeroPadding2D + a VALID convolution): a padding tap
    is a product 0 * w like any other, so the NaN weight poisons its output channel at the border pixels too.
    x3 cases: +-Inf of the split operands (x and w forward, dy and w input gradient, x and dy weight gradient) are NaN in the reference."""
    N, H, W = shape
    Ci, Co, stride, dil = c["Ci"], c["Co"], c["stride"], c["dil"]
    low = c["compute"] == 1
    P = {k: (t.clone() if torch.is_tensor(t) else t) for k, t in MR.conv_problem(N, H, W, Ci, Co, stride, dil, low).items()}
    Ho, Wo = P["Ho"], P["Wo"]
    x, w, dy = P["x"], P["w"], P["dy"]
    x[0, 0, 0, 1], x[0, 4, 5, 2], x[1, 2, 2, 0], x[1, 6, 8, 3] = NAN, NAN, INF, -INF
    w_f = w.clone()
    w_f[0, 0, 5, Co - 1] = NAN                                   # forward: one output channel
    w_b = w                                                      # input gradient: finite weights (see the docstring)
    s = lambda h, w_: (min(h // stride, Ho - 1), min(w_ // stride, Wo - 1))
    dy[(0,) + s(0, 0) + (1,)], dy[(0,) + s(4, 5) + (2,)], dy[(1,) + s(2, 2) + (0,)], dy[(1,) + s(6, 8) + (3,)] = NAN, NAN, INF, -INF
    q = inf_to_nan if c["compute"] == 2 else (lambda t: t)
    nchw = lambda t: q(t).double().permute(0, 3, 1, 2)
    oihw = lambda t: q(t).double().permute(3, 2, 0, 1).contiguous()
    z = F.conv2d(nchw(x), oihw(w_f), None, stride=stride, padding=dil, dilation=dil).permute(0, 2, 3, 1)
    opad = (H - 1 - stride * (Ho - 1), W - 1 - stride * (Wo - 1))
    dx = F.conv_transpose2d(nchw(dy), oihw(w_b), stride=stride, padding=dil, dilation=dil, output_padding=opad).permute(0, 2, 3, 1)
    dw = torch.nn.grad.conv2d_weight(nchw(x), (Co, Ci, 3, 3), nchw(dy), stride=stride, padding=dil, dilation=dil).permute(2, 3, 1, 0)
    P.update(x=x, w_f=w_f, w_b=w_b, dy=dy, z=z, dx=dx, dw=dw)
    return P


CONV_ALPHA = 0.75


def conv_refs(c, P):
    """y = relu((z * scale + shift) * alpha + residual) and dx = alpha * mask(dx) for the rich cases, y = relu(z + shift) and
    dx = mask(dx) for the others (test_conv3x3_forward_and_input_gradient_inside_frames)."""
    rich = c["rich"]
    alpha = CONV_ALPHA if rich else 1.0
    y = torch.relu((P["z"] * (P["scale"].double() if rich else 1.0) + P["shift"].double()) * alpha + (P["res"].double() if rich else 0.0))
    dx = torch.where(P["msk"] > 0, P["dx"] * alpha, torch.zeros_like(P["dx"]))
    return dict(y=y, dx=dx)


STEM_SHAPE = (2, 37, 53)       # of G.STEM_SHAPES: at 1 x 9 x 8 (5 x 4 outputs) the 7 x 7 windows of two poisoned pixels already hold 8 of the 20 output
#                                pixels, past the cap; here a pixel reaches at most 16 of 19 x 27
STEM_SHAPE_WGRAD = STEM_SHAPE   # the weight gradient: the specials go into dy (columns of the 147 x 64 gradient); one NaN pixel of the image
#                                would reach all 49 taps of its colour, a third of the rows


def stem_poisoned(shape, low, x3=False):
    """matrix_refs.stem_problem with NaN at the corner pixel (0, 0, 0), +Inf and -Inf at two pixels whose 7 x 7 / stride-2 windows do not
    meet, NaN in one weight of the last output channel; the fp64 forward on the explicitly zero-padded image."""
    N, H, W = shape
    P = {k: (t.clone() if torch.is_tensor(t) else t) for k, t in MR.stem_problem(N, H, W, low).items()}
    img, w = P["img"], P["w"]
    img[0, 0, 0, 1] = NAN
    img[N - 1, H - 1, W - 1, 0] = INF
    if H > 16:
        img[0, H // 2, W // 2, 2] = -INF
    w[3, 3, 1, 63] = NAN
    q = inf_to_nan if x3 else (lambda t: t)
    z = F.conv2d(F.pad(q(img).double().permute(0, 3, 1, 2), (3, 3, 3, 3)), q(w).double().permute(3, 2, 0, 1), None, stride=2).permute(0, 2, 3, 1)
    P.update(img=img, w=w, z=z)
    return P


def stem_wgrad_poisoned(shape, low, x3=False):
    """The stem weight gradient with the specials in dy (three output channels: three columns of the 147 x 64 gradient) and a finite image."""
    N, H, W = shape
    P = {k: (t.clone() if torch.is_tensor(t) else t) for k, t in MR.stem_problem(N, H, W, low).items()}
    dy, img = P["dy"], P["img"]
    Ho, Wo = P["Ho"], P["Wo"]
    dy[0, 0, 0, 1], dy[N - 1, Ho - 1, Wo - 1, 63], dy[0, Ho // 2, Wo // 2, 30] = NAN, INF, -INF
    q = inf_to_nan if x3 else (lambda t: t)
    cols = F.unfold(F.pad(img.double().permute(0, 3, 1, 2), (3, 3, 3, 3)), 7, stride=2).view(N, 3, 49, Ho, Wo).permute(0, 3, 4, 2, 1).reshape(N, Ho, Wo, 147)
    P.update(dy=dy, dw=torch.einsum("nhwk,nhwc->kc", cols, q(dy).double()))
    return P


# ------------------------------------------------------------------------------------------------------------------------
# max pooling and the stride-2 subsample
# ------------------------------------------------------------------------------------------------------------------------
POOL_CASES = [("f32", 4), ("bf16", 4), ("bf16", 8), ("f32", 1)]      # (storage, C): fp32 forward runs 1 channel per lane for every C and the backward 4; bf16 runs
#                                                                  4 per lane at C = 4 and 8 at C = 8; C = 1 is the forward alone (the backward needs C % 4 == 0)
POOL_HW = (2, 9, 12)           # N, H, W: odd and even extents, 5 x 6 windows per image


def pool_problem(C):
    """Integer-valued map (exact in bf16; ties in every window) with NaN at the corner pixel (its windows touch the zero padding), at an
    interior pixel of odd coordinates (one window) and at one of even coordinates (four windows), two NaN in one window, +Inf and -Inf
    (ordinary values of a maximum).  y: F.max_pool2d of the zero-padded map."""
    N, H, W = POOL_HW
    gen = torch.Generator().manual_seed(31 + C)
    x = torch.randint(-4, 5, (N, H, W, C), generator=gen, dtype=torch.int8).float()
    c = C - 1
    x[0, 0, 0, 0], x[0, 3, 5, c], x[0, 6, 8, 0] = NAN, NAN, NAN
    x[1, 4, 4, c], x[1, 4, 5, c] = NAN, NAN
    x[1, 7, 9, 0], x[1, 1, 1, c] = INF, -INF
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    dy = torch.randint(-8, 9, (N, Ho, Wo, C), generator=gen, dtype=torch.int8).float()
    y = F.max_pool2d(F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1)
    assert y.shape == (N, Ho, Wo, C)
    return dict(x=x, dy=dy, y=y, Ho=Ho, Wo=Wo)


def pool_window(x, n, ho, wo, c):
    """The nine taps of a window of the zero-padded map, in the kernel's order (kh major): tap kh * 3 + kw."""
    H, W = x.shape[1], x.shape[2]
    out = []
    for kh in range(3):
        for kw in range(3):
            hi, wi = 2 * ho - 1 + kh, 2 * wo - 1 + kw
            out.append(float(x[n, hi, wi, c]) if (0 <= hi < H and 0 <= wi < W) else 0.0)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# row ops
# ------------------------------------------------------------------------------------------------------------------------
ROW_N = 2 * 256 + 44           # a little over one block of every row-op launch (256 threads; the float4 loops: 4 per thread, so the period
#                                and column counts below keep n a multiple of 4)
ROW_OPS = ["add", "add_bcast", "axpy", "scale_cols", "scale_cols_bf16", "scale_cols_t", "colsum", "colsum_det", "colsum_scaled", "cvt_bf16",
           "dropout", "sigmoid_bwd", "relu_mask", "bn_fold"]
ROW_COLS = 12                  # 2-D ops: ROW_N / 12 = 46 rows + 4 -> rows x cols below
DROP_P, DROP_SITE, DROP_STEP = 0.1, 0xABCDE, 0x1234567


def row_problem(op):
    """Inputs (seeded randn with NaN, +Inf and -Inf at elements 3, n - 2 and n / 2 of the first operand) and the one-line fp64 form."""
    from oracle import dropout_ref as DR
    gen = torch.Generator().manual_seed(ROW_OPS.index(op))
    n = ROW_N
    rows, cols = n // ROW_COLS, ROW_COLS
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    for t in (a,):
        t[3], t[n - 2], t[n // 2] = NAN, INF, -INF
    a2 = a[:rows * cols].view(rows, cols).clone()
    a2[rows - 1, cols - 1] = INF
    sc = torch.rand(cols, generator=gen) + 0.5
    if op == "add":
        return dict(a=a, b=b, ref=a.double() + b.double())
    if op == "add_bcast":
        p = torch.randn(ROW_COLS * 4, generator=gen)
        return dict(a=a, p=p, ref=a.double() + p.double().repeat(n // p.numel() + 1)[:n])
    if op == "axpy":
        return dict(a=a, b=b, ref=b.double() + 2.0 * a.double())
    if op in ("scale_cols", "scale_cols_bf16"):
        w = G.bf(a2) if op.endswith("bf16") else a2
        return dict(w=w, sc=sc, ref=w.double() * sc.double())
    if op == "scale_cols_t":
        return dict(w=a2, sc=sc, ref=(a2.double() * sc.double()).t().contiguous())
    if op in ("colsum", "colsum_det", "colsum_scaled"):
        out0 = torch.randn(cols, generator=gen)
        rows = 64 + 6                              # a little over the 64 rows of one block of the three launches
        x = torch.randn(rows, cols, generator=gen)
        x[1, 0], x[rows - 1, 1], x[rows // 2, 2] = NAN, INF, -INF      # three of the twelve columns
        if op == "colsum_scaled":
            return dict(x=x, sc=sc, out0=out0, ref=out0.double() + sc.double() * x.double().sum(0))
        return dict(x=x, out0=out0, ref=out0.double() + 0.5 * x.double().sum(0))
    if op == "cvt_bf16":
        return dict(a=a, ref=a.bfloat16().double())
    if op == "dropout":
        a[5] = NAN                                 # two NaN: one of them is kept, one dropped, or the case is redrawn below
        keep = torch.from_numpy(DR.keep_mask(DR.drop_key(DROP_SITE, DROP_STEP), np.arange(n), DROP_P))
        drop_at = int((~keep).nonzero()[0])
        a[drop_at] = NAN                           # a dropped NaN is 0 (the oracle's where(keep, x * s, 0))
        assert bool(keep[3]) or bool(keep[5])
        return dict(a=a, keep=keep, ref=torch.where(keep, a.double() / (1.0 - DROP_P), torch.zeros((), dtype=torch.float64)))
    if op == "sigmoid_bwd":
        y = torch.sigmoid(b)
        return dict(a=a, y=y, ref=a.double() * y.double() * (1 - y.double()))
    if op == "relu_mask":                          # NaN in the gradient, at a position the (finite) mask lets through and at one it does not
        i_on, i_off = int((b > 0).nonzero()[0]), int((b <= 0).nonzero()[0])
        a[i_on], a[i_off] = NAN, NAN
        return dict(a=a, b=b, ref=torch.where(b > 0, a.double(), torch.zeros((), dtype=torch.float64)))
    if op == "bn_fold":
        C = 64
        gamma, beta, mean = (torch.randn(C, generator=gen) for _ in range(3))
        var = torch.rand(C, generator=gen) + 0.5
        gamma[3], beta[5], mean[7], var[9] = NAN, INF, -INF, NAN
        scale = gamma.double() / torch.sqrt(var.double() + 1.001e-5)
        return dict(gamma=gamma, beta=beta, mean=mean, var=var, eps=1.001e-5, ref_scale=scale, ref_shift=beta.double() - mean.double() * scale)
    raise ValueError(op)


# ------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------
LN_CASES = [(256, 37), (252, 37)]          # (C, rows): the model's width and a ragged one of test_layernorm_widths_offsets_and_row_edges
LN_EPS = 1e-5


def layernorm_forward_ref(x, gamma, beta, eps):
    x = x.double()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return dict(y=(x - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double(), mean=mean, rstd=rstd)


def layernorm_problem(C, rows, poison_dy=False):
    """x with NaN in row 1, +Inf in the last row and -Inf in a middle row (each makes its whole row of y, mean, rstd and dx NaN: the
    mean of a row with an Inf is +-Inf and x - mean is NaN); every other row stays finite.  dgamma / dbeta sum over the rows: NaN in
    every column.  poison_dy: x finite, three NaN in dy instead (rows of dx, columns of dgamma / dbeta)."""
    gen = torch.Generator().manual_seed(C + rows)
    x, dy, add = torch.randn(rows, C, generator=gen) + 0.5, torch.randn(rows, C, generator=gen), torch.randn(rows, C, generator=gen)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    if poison_dy:                              # NaN only: an Inf in dy leaves Inf - Inf to the order in which dx combines its two row means
        dy[1, 2], dy[rows - 1, C - 1], dy[rows // 2, C // 2] = NAN, NAN, NAN
    else:
        x[1, 2], x[rows - 1, C - 1], x[rows // 2, C // 2] = NAN, INF, -INF
    f = layernorm_forward_ref(x, gamma, beta, LN_EPS)
    xd, dyd, g = x.double(), dy.double(), gamma.double()
    xhat = (xd - f["mean"][:, None]) * f["rstd"][:, None]
    dxhat = dyd * g
    dx = f["rstd"][:, None] * (dxhat - dxhat.mean(1, keepdim=True) - xhat * (dxhat * xhat).mean(1, keepdim=True))
    return dict(x=x, dy=dy, add=add, gamma=gamma, beta=beta, y=f["y"], y2=f["y"] + add.double(), mean=f["mean"], rstd=f["rstd"], dx=dx,
                dgamma=(dyd * xhat).sum(0), dbeta=dyd.sum(0))


# ------------------------------------------------------------------------------------------------------------------------
# optimiser
# ------------------------------------------------------------------------------------------------------------------------
OPT_SPECIALS = [("nan", NAN), ("inf", INF)]
OPT_TENSOR = 4                 # the 4097-element tensor of test_gpu_adamw.SIZES
OPT_SIZES = [1, 5, 64, 65, 4097, 20000]
OPT_TGROUP = [0, 1, 0, 2, 1, 1]
OPT_LRS = [1e-2, 3e-3, 1e-3]
OPT_WD = 1e-2
OPT_CLIP = 0.2


def optimiser_problem(special, joint, trained=(True, True, True), seed=3):
    """One step of tests/adamw_ref.py on the tensors of test_gpu_adamw.py with one gradient element of the 4097-element tensor set to
    `special`.  Returns the host arrays and the reference's parameters, moments, G and clip factor after the step."""
    import adamw_ref as A
    rng = np.random.default_rng(seed)
    p0 = [rng.normal(size=n).astype(np.float32) for n in OPT_SIZES]
    m0 = [(rng.normal(size=n) * 1e-2).astype(np.float32) for n in OPT_SIZES]
    v0 = [(rng.random(size=n) * 1e-3).astype(np.float32) for n in OPT_SIZES]
    grads = [(rng.normal(size=n) * 1e-2).astype(np.float32) for n in OPT_SIZES]
    grads[OPT_TENSOR][1234] = special
    kw = dict(global_clipnorm=OPT_CLIP) if joint else dict(clipnorm=OPT_CLIP)
    ref = A.AdamW(dict(enumerate(OPT_LRS)), dict(enumerate(OPT_TGROUP)), weight_decay=OPT_WD, **kw)
    ref.m = {i: m0[i].astype(np.float64) for i in range(len(OPT_SIZES))}
    ref.v = {i: v0[i].astype(np.float64) for i in range(len(OPT_SIZES))}
    params = {i: p.astype(np.float64) for i, p in enumerate(p0)}
    live = [i for i in range(len(OPT_SIZES)) if trained[OPT_TGROUP[i]]]
    with np.errstate(invalid="ignore", over="ignore"):
        s = ref.step({i: grads[i] for i in live}, params)
    return dict(p0=p0, m0=m0, v0=v0, grads=grads, live=live, p=params, m=ref.m, v=ref.v, s=s, G=ref.last_norm)



# ------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------
ATT_B, ATT_T, ATT_S, ATT_H, ATT_HD = 2, 40, 70, 8, 32       # crosses the 32- and the 64-key tile
ATT_POISON = (1, 3)            # (batch element, head) that holds the special of the unmasked kinds
ATT_CASES = [("q_nan", False), ("q_nan", True), ("v_nan", False), ("v_nan", True), ("k_pinf", False), ("k_pinf", True), ("masked_k_nan", True)]


def attention_problem(case, masked):
    """Operands of tests/attn_cases.py ("ragged_max": every row's maximum in the ragged last tile; bf16 values, q small) with one special:
    q_nan         NaN in one q element: that query row of that head (o, lse, dq, the map's row), and through the row's probabilities
                  dk / dv of the (batch, head)
    v_nan         NaN in one v element: that column of every query of the (batch, head); through delta, dq / dk of the (batch, head)
    k_pinf        +Inf in one k element: queries whose score becomes +Inf get a NaN row, those whose score becomes -Inf stay finite
                  with that key at weight 0
    masked_k_nan  NaN in the k rows of masked keys: nothing (a masked key is absent: the reference zeroes its rows).
    masked: a key mask with masked keys in both 32-key tiles and the ragged tail; v of masked keys stays finite."""
    import attn_cases as AC
    B, T, S, H, HD = ATT_B, ATT_T, ATT_S, ATT_H, ATT_HD
    gen = torch.Generator().manual_seed(7)
    q, k, v, do = AC.scores_case("ragged_max", B, T, S, 0.0, 1, None, gen)
    kv = None
    if masked:
        kv = torch.ones(B, S, dtype=torch.bool)
        kv[0, 5], kv[0, 40:47], kv[1, 66:] = False, False, False
    b, h = ATT_POISON
    if case == "q_nan":
        q[b, 17, h * HD + 4] = NAN
    elif case == "v_nan":
        v[b, 33, h * HD + 9] = NAN
    elif case == "k_pinf":
        # (a column where 5 .. 15 of the 40 queries are positive: the rows with a +Inf score stay under the cap in the head-averaged map)
        c = next(c for c in range(1, HD) if 5 <= int((q[b, :, h * HD + c] > 0).sum()) <= 15)
        k[b, 33, h * HD + c] = INF
    elif case == "masked_k_nan":
        k[0, 44, h * HD + 2] = NAN
        k[1, 68, 5] = NAN
    else:
        raise ValueError(case)
    return q, k, v, do, kv


def attention_reference(q, k, v, do, kv, mult):
    """fp64 autograd of softmax(mult * q k^T) v per head over the valid keys (masked keys absent: their k / v rows zeroed, their
    weight, dk and dv exactly 0).  mult: the scale for raw queries, ln 2 for stored bf16 queries (scores in log2 units).
    dq is the gradient with respect to the q given."""
    B, T, S, H, HD = ATT_B, ATT_T, ATT_S, ATT_H, ATT_HD
    absent = (lambda x: x) if kv is None else (lambda x: torch.where(kv.unsqueeze(2), x, torch.zeros_like(x)))
    qq, kk, vv = q.clone().requires_grad_(True), absent(k).clone().requires_grad_(True), absent(v).clone().requires_grad_(True)
    qh, kh, vh = (t.view(B, -1, H, HD).transpose(1, 2) for t in (qq, kk, vv))
    sc = (qh * mult) @ kh.transpose(-1, -2)
    if kv is not None:
        sc = sc.masked_fill(~kv[:, None, None, :], float("-inf"))
    w = torch.softmax(sc, dim=-1)
    o = (w @ vh).transpose(1, 2).reshape(B, T, H * HD)
    o.backward(do)
    dk, dv, wm = kk.grad, vv.grad, w.detach().mean(1)
    if kv is not None:
        dk, dv, wm = absent(dk), absent(dv), torch.where(kv[:, None, :], wm, torch.zeros_like(wm))
    return dict(o=o.detach(), lse=torch.logsumexp(sc, dim=-1).detach(), dq=qq.grad, dk=dk, dv=dv, w=wm)


def finite_copy(t):
    return torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)
