"""NaN and Inf INSIDE the operands of the model kernels ("Non-finite values"): every GEMM family and epilogue form, the ReLU
mask forms and the fused 1x1 backward, split-K and the ring weight gradient, the 3x3 / dilated / stem convolutions, max pooling, the row
ops, LayerNorm, the two attention cores with attention_weights, and the optimiser, each against the fp64 reference of the same operation on the same poisoned values
(tests/nonfinite_cases.py), and whole training steps from one non-finite weight or pixel.

Every case asserts, through nonfinite_cases.assert_same_nonfinite: each NaN of the reference is a NaN of the output, the two non-finite sets
are equal, infinities carry the reference's sign, and the finite remainder keeps the tolerance of the family's older test.  The expected
set comes from the reference alone.  tests/test_nonfinite_cpu.py shows on the CPU that no reference is more than a quarter non-finite
and that every GEMM case reaches the kernel family it states.

The rules themselves, and what is left open, are in DESIGN.md."""
import ctypes
import gc
import math

import numpy as np
import pytest
import torch

import guard_band_cases as G
import nonfinite_cases as NF
from nonfinite_cases import assert_same_nonfinite
from test_gpu_guard_bands import (B16, DEV, F32, U8, _reset_library_tuning, big_ws, conv_in, conv_out, gemm_launch, guarded_scratch,  # noqa: F401
                                  pack_pixels, stem_image, vec_in, with_workspace)

pytestmark = pytest.mark.gpu


def g(t):
    return t.to(DEV).contiguous()


def close_tensor(rtol):
    """max |got - ref| <= rtol * max |ref|: the per-tensor metric of tests/test_gpu_kernels.py::close, as a `close` of assert_same_nonfinite."""
    def check(got, ref, _tol, what):
        err, scale = float((got - ref).abs().max()), float(ref.abs().max()) + 1e-30
        assert err <= rtol * scale, f"{what}: max abs err {err:.3e} > {rtol * scale:.3e} (scale {scale:.3e})"
    return check


def exact(got, ref, _tol, what):
    assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} elements differ"


# ------------------------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------------------------
def gemm_outputs_check(c, v, t, ref):
    """gemm_check of the guard-band tests with assert_same_nonfinite in the place of check_close."""
    what = G.case_id(c)
    C = t["C"][0]
    assert_same_nonfinite(C, ref["C"], c["tol"], what)
    for name, (shape, dtype, lead, pitch, is_out) in G.operands(c).items():
        if is_out:
            assert G.frame_intact(t[name][1], t[name][0]), f"{what}: the launch wrote outside {name}"
    if c["bits_out"]:                          # (y > 0) of the finite outputs; the bit of a NaN output is left open, like a NaN in a mask operand
        fin = torch.isfinite(ref["C"])
        got, want = G.unpack_bits(t["maskbits_out"][0].cpu(), c["N"]), C.float().cpu() > 0
        assert torch.equal(got[fin], want[fin]), f"{what}: mask bits out"
    if c["rowsum"]:
        assert_same_nonfinite(t["rowsum_a"][0], ref["rowsum_a"], "f32", what + " row sums")
    if c["ln"] is not None:
        # rows whose C is finite: the older test's reference (LayerNorm of the kernel's own C); the others: the fp64 reference's NaN
        Cd = C.cpu().double()
        rows = torch.isfinite(ref["C"]).all(1)
        own = NF.layernorm_forward_ref(torch.where(rows[:, None], Cd, torch.zeros_like(Cd)), v["ln_gamma"], v["ln_beta"], G.LN_EPS)
        for k in ("y", "mean", "rstd"):
            r = ref["ln_" + k]
            sel = rows[:, None] if r.dim() == 2 else rows
            assert bool((torch.isfinite(r) == sel.expand_as(r)).all()), f"{what}: the case is about whole rows"
            assert_same_nonfinite(t["ln_" + k][0], torch.where(sel, own[k], r), "f32", f"{what} ln_{k}")
        y = t["ln_y"][0].cpu()
        if c["ln"]["add"]:
            add = v["ln_add"][torch.arange(c["M"]) % c["ln"]["add_rows"]]
            assert_same_nonfinite(t["ln_y2"][0], (y + add).double(), "f32", what + " ln_y2", close=exact)
            assert_same_nonfinite(t["ln_y2"][0], ref["ln_y2"], "f32", what + " ln_y2 against fp64", close=close_tensor(2e-5))
        if c["ln"]["y16"]:
            assert_same_nonfinite(t["ln_y16"][0], y.to(B16).double(), "f32", what + " ln_y16", close=exact)


_FWD = NF.gemm_forward_cases()


@pytest.mark.parametrize("c,poison", _FWD, ids=[G.case_id(c) for c, _ in _FWD])
def test_gemm_forward_forms_propagate_nan_and_inf(hip, c, poison):
    """NaN / +Inf / -Inf in three rows of A, NaN in a column of B, in a bias entry and in a residual element, through every GEMM family
    (asserted with detr_hip_gemm_family) with act 0, 1 (ReLU) and 2 (sigmoid: sigmoid(+-Inf) is the finite 1 / 0), masks as values
    and as bits (a masked-out NaN is 0 in the kernel and in the reference), dropout, and the fused LayerNorm."""
    v, vr = NF.gemm_poisoned(c, poison)
    ref = NF.gemm_refs(c, v, vr)
    with G.tuning(hip, c["env"]):
        t, _ = gemm_launch(hip, c, v)
    gemm_outputs_check(c, v, t, ref)


@pytest.mark.parametrize("c", NF.split_cases(), ids=G.case_id)
def test_split_k_propagates_nan_and_inf_and_stays_inside_its_scratch(hip, c):
    """Split-K and the ring weight gradient with the specials in x (A) and dY (B), +Inf and dY's NaN at a k of the last slab, through
    scratch of exactly detr_hip_workspace_bytes_gemm bytes in front of a sentinel guard: the reduced C (and the fused row sums) obey
    the contract, nothing behind the reported size is touched."""
    v, vr = NF.gemm_poisoned(c, ("A", "B"))
    ref = NF.gemm_refs(c, v, vr)
    lib = hip.load()
    with G.tuning(hip, c["env"]):
        probe = G.fill_desc(hip, c, G.placeholder_ptrs(c))
        query = int(lib.detr_hip_workspace_bytes_gemm(ctypes.byref(probe)))
        ws, ws_buf = guarded_scratch(query)
        t, d = gemm_launch(hip, c, v, workspace=ws.data_ptr(), workspace_bytes=query)
    assert G.frame_intact(ws_buf, ws), f"{G.case_id(c)}: wrote past the {query} bytes of scratch"
    gemm_outputs_check(c, v, t, ref)


def test_gemm_group_members_propagate_nan_and_inf(hip, big_ws):
    """Three weight gradients through gemm_group, each with the specials in its x and dY: every member obeys the contract by itself."""
    members = NF.group_members()
    built = []
    for c in members:
        v, vr = NF.gemm_poisoned(c, ("A", "B"))
        t = {}
        for name, (shape, dtype, lead, pitch, is_out) in G.operands(c).items():
            if is_out:
                t[name] = G.sentinel_framed(shape, dtype, lead, pitch, device=DEV)
                t[name][0].fill_(NF.MR.C0 if name == "C" else NF.MR.RS0)
            else:
                t[name] = G.nan_framed(v[name].to(dtype), lead, pitch, device=DEV)
        args = (c["M"], c["N"], c["K"], t["A"][0], c["lda"], 0, t["B"][0], c["ldb"], 0, t["C"][0], c["ldc"])
        kw = dict(alpha=c["alpha"], split_k=c["split"], compute=1, scale=t["scale"][0] if c["scale"] else None,
                  rowsum_a=t["rowsum_a"][0] if c["rowsum"] else None, rowsum_alpha=c["alpha"])
        built.append((c, v, vr, t, args, kw))
    old = hip.WORKSPACE
    try:
        hip.WORKSPACE = big_ws
        hip.gemm_group([(args, kw) for *_, args, kw in built])
        torch.cuda.synchronize()
    finally:
        hip.WORKSPACE = old
    for c, v, vr, t, _, _ in built:
        gemm_outputs_check(c, v, t, NF.gemm_refs(c, v, vr))


def test_conv1x1_backward_fused_propagates_nan_and_inf(hip, big_ws):
    """NaN, +Inf and -Inf in dy: da = where(a > 0, dy w^T, 0) -- the NaN row is NaN where the stored mask is positive and 0 where it
    is not -- at one bf16 rounding, dw's three columns at the bound of test_conv1x1_backward_fused_reads_dy_once."""
    M, pad = 33, 8
    P = NF.bwd_fused_problem(M)
    dyd, ad, wd = (G.nan_framed(P[k].to(B16), 32, P[k].shape[1] + pad, device=DEV)[0] for k in ("dy", "a", "w"))
    sc = vec_in(P["scale"])[0]
    da, da_buf = G.sentinel_framed((M, 64), B16, 32, 64 + pad, device=DEV)
    dw, dw_buf = G.sentinel_framed((64, 256), F32, 16, 256 + pad, device=DEV)
    dw.copy_(P["dw0"])
    hip.conv1x1_bwd_fused(dyd, ad, wd, da, dw, big_ws, scale=sc, use_mask=True, alpha=0.5)
    torch.cuda.synchronize()
    assert G.frame_intact(da_buf, da) and G.frame_intact(dw_buf, dw)
    assert_same_nonfinite(da, P["da"], "b16", "fused 1x1 backward: da")
    fin = torch.isfinite(P["dy"])
    bound = 2e-6 * float((P["a"].double().abs().t() @ torch.where(fin, P["dy"], torch.zeros(())).double().abs()).max()) + 1e-6

    def dw_close(got, ref, _tol, what):
        assert float((got - ref).abs().max()) <= bound, what
    assert_same_nonfinite(dw, P["dw"], None, "fused 1x1 backward: dw", close=dw_close)


# ------------------------------------------------------------------------------------------------------------------------
# 3x3 convolutions and the stem
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", NF.conv_cases(), ids=lambda c: c["id"])
def test_conv3x3_forward_and_input_gradient_propagate_nan_and_inf(hip, c):
    """Forward with ReLU and input gradient with the ReLU mask on every 3x3 route at N = 2, 9 x 11: a NaN pixel (the corner one, whose halo
    is zero padding, and an interior one) poisons the output pixels whose window holds it, across all channels; +-Inf pixels give
    +-Inf by the sign of the weight (0 behind the ReLU where negative; NaN on the f32x3 routes); a NaN weight poisons its channel."""
    N, H, W = NF.CONV_SHAPE
    Ci, Co, stride, dil, s16, rich, bits = c["Ci"], c["Co"], c["stride"], c["dil"], c["s16"], c["rich"], c["bits"]
    P = NF.conv_poisoned(c)
    R = NF.conv_refs(c, P)
    Ho, Wo = P["Ho"], P["Wo"]
    dt = B16 if s16 else F32
    tol = "b16conv" if s16 else "f32"
    alpha = NF.CONV_ALPHA if rich else 1.0
    msk = pack_pixels(P["msk"] > 0) if bits else P["msk"]
    with G.tuning(hip, c["env"]):
        x, wf, wb, dy = conv_in(P["x"], dt), conv_in(P["w_f"], dt), conv_in(P["w_b"], dt), conv_in(P["dy"], dt)
        res, mk = conv_in(P["res"], dt), conv_in(msk, U8 if bits else dt)
        scale, shift = vec_in(P["scale"]), vec_in(P["shift"])
        y, dx = conv_out((N, Ho, Wo, Co), dt), conv_out((N, H, W, Ci), dt)
        yb = conv_out((N, Ho, Wo, Co // 8), U8) if bits else None
        kw = dict(scale=scale[0], residual=res[0], alpha=alpha) if rich else {}
        hip.conv3x3(0, x[0], wf[0], y[0], N, H, W, Ci, Ho, Wo, Co, stride, pad=dil, bias=shift[0], act=1, compute=c["compute"], dilation=dil,
                    maskbits_out=yb[0] if bits else None, **kw)
        hip.conv3x3(1, dy[0], wb[0], dx[0], N, H, W, Ci, Ho, Wo, Co, stride, pad=dil, alpha=alpha, mask=mk[0], compute=c["compute"], dilation=dil)
        torch.cuda.synchronize()
    assert G.frame_intact(y[1], y[0]) and G.frame_intact(dx[1], dx[0]), c["id"] + ": wrote outside y / dx"
    assert_same_nonfinite(y[0], R["y"], tol, c["id"] + " forward")
    assert_same_nonfinite(dx[0], R["dx"], tol, c["id"] + " input gradient")
    if bits:
        fin = torch.isfinite(R["y"])
        got = G.unpack_bits(yb[0].cpu().reshape(N * Ho * Wo, Co // 8), Co).reshape(N, Ho, Wo, Co)
        assert torch.equal(got[fin], (y[0].float().cpu() > 0)[fin]), c["id"] + ": mask bits out"


@pytest.mark.parametrize("c", NF.wgrad_cases(), ids=lambda c: c["id"])
def test_conv3x3_weight_gradient_propagates_nan_and_inf(hip, big_ws, c):
    """3x3 weight gradients (split-K through the workspace) with the specials in x and dy: the taps and channels the reference poisons."""
    N, H, W = NF.CONV_SHAPE
    Ci, Co, stride, dil, s16 = c["Ci"], c["Co"], c["stride"], c["dil"], c["s16"]
    P = NF.conv_poisoned(c)
    dt = B16 if s16 else F32
    with G.tuning(hip, c["env"]):
        x, dy, scale = conv_in(P["x"], dt), conv_in(P["dy"], dt), vec_in(P["scale"])
        dw, dw_buf = G.sentinel_framed((3, 3, Ci, Co), F32, 64, None, device=DEV)
        dw.fill_(0.0)
        with_workspace(hip, big_ws, lambda: hip.conv3x3(2, x[0], dy[0], dw, N, H, W, Ci, P["Ho"], P["Wo"], Co, stride, pad=dil, scale=scale[0],
                                                        split=c["split"], compute=c["compute"], dilation=dil))
    assert G.frame_intact(dw_buf, dw), c["id"] + ": wrote outside dw"
    assert_same_nonfinite(dw, P["dw"] * P["scale"].double(), "split", c["id"])


STEM_FWD = [("f32", {}, 0, F32, "f32", True, False), ("f32x3", {"DETR_HIP_SPLIT3_ALL": 1}, 2, F32, "f32", True, True),
            ("rows16", {}, 1, B16, "b16conv", False, False), ("gather16", {"DETR_HIP_STEM_ROWS": 2}, 1, B16, "b16conv", False, False)]


@pytest.mark.parametrize("name,env,compute,y_dtype,tol,use_scale,x3", STEM_FWD, ids=[s[0] for s in STEM_FWD])
def test_stem_forward_propagates_nan_and_inf(hip, name, env, compute, y_dtype, tol, use_scale, x3):
    """Stem forward with the BN scale / shift and ReLU: fp32, f32x3 (x3: +-Inf of image and weights are NaN in the reference) and the
    two bf16-output kernels, NaN at the corner pixel, +-Inf at two others, NaN in one weight."""
    N, H, W = NF.STEM_SHAPE
    P = NF.stem_poisoned(NF.STEM_SHAPE, compute == 1, x3=x3)
    Ho, Wo = P["Ho"], P["Wo"]
    ref = torch.relu(P["z"] * (P["scale"].double() if use_scale else 1.0) + P["shift"].double())
    with G.tuning(hip, env):
        img, shift, scale = stem_image(P["img"]), vec_in(P["shift"]), vec_in(P["scale"])
        w, _ = G.nan_framed(P["w"].reshape(147, 64), 64, None, device=DEV)
        y, y_buf = conv_out((N, Ho, Wo, 64), y_dtype)
        hip.stem_conv(0, img[0], w, y, N, H, W, Ho, Wo, scale=scale[0] if use_scale else None, bias=shift[0], act=1, compute=compute)
        torch.cuda.synchronize()
    assert G.frame_intact(y_buf, y)
    assert_same_nonfinite(y, ref, tol, f"stem forward {name}")


STEM_WGRAD = [("f32", {}, 0, F32, "split", False), ("f32x3", {"DETR_HIP_SPLIT3_ALL": 1}, 2, F32, "split", True), ("bf16c", {}, 1, F32, "split", False),
              ("rows16", {}, 1, B16, "stem16", False), ("gather16", {"DETR_HIP_STEM_ROWS": 2}, 1, B16, "stem16", False)]


@pytest.mark.parametrize("name,env,compute,dy_dtype,tol,x3", STEM_WGRAD, ids=[s[0] for s in STEM_WGRAD])
def test_stem_weight_gradient_propagates_nan_and_inf(hip, big_ws, name, env, compute, dy_dtype, tol, x3):
    """Stem weight gradient (split 7) with NaN, +Inf and -Inf in dy: three columns of the 147 x 64 gradient."""
    N, H, W = NF.STEM_SHAPE_WGRAD
    P = NF.stem_wgrad_poisoned(NF.STEM_SHAPE_WGRAD, compute == 1, x3=x3)
    with G.tuning(hip, env):
        img, dy, scale = stem_image(P["img"]), conv_in(P["dy"], dy_dtype), vec_in(P["scale"])
        dw, dw_buf = G.sentinel_framed((147, 64), F32, 64, None, device=DEV)
        dw.fill_(0.0)
        with_workspace(hip, big_ws, lambda: hip.stem_conv(2, img[0], dy[0], dw, N, H, W, P["Ho"], P["Wo"], scale=scale[0], split=7, compute=compute))
    assert G.frame_intact(dw_buf, dw)
    assert_same_nonfinite(dw, P["dw"] * P["scale"].double(), tol, f"stem weight gradient {name}")


# ------------------------------------------------------------------------------------------------------------------------
# max pooling, subsample
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,C", NF.POOL_CASES)
def test_maxpool_selects_a_nan_tap_and_routes_its_gradient_there(hip, kind, C):
    """Forward: y equals F.max_pool2d of the zero-padded map (NaN where a window holds one, windows on the padding and off it; +Inf is
    an ordinary maximum, -Inf never wins), the argmax byte of a NaN window names a tap that holds a NaN, and the byte of every other
    window is the first maximal tap.  Backward from the kernel's own bytes: the gradient of a NaN window lands on that one tap and
    nowhere else, so the sum over the window is preserved (the pixel's own ReLU mask lets a NaN pixel through, as the oracle's does)."""
    import test_launch_edges_cpu as E
    N, H, W = NF.POOL_HW
    P = NF.pool_problem(C)
    Ho, Wo = P["Ho"], P["Wo"]
    td = torch.bfloat16 if kind == "bf16" else torch.float32
    xd = g(P["x"]).to(td)
    y = torch.full((N, Ho, Wo, C), G.SENT, dtype=td, device=DEV)
    am = torch.full((N, Ho, Wo, C), 0xEE, dtype=torch.uint8, device=DEV)
    hip.call(f"detr_hip_maxpool3x3s2_fwd_{kind}", xd.data_ptr(), y.data_ptr(), am.data_ptr(), N, H, W, C, Ho, Wo)
    assert_same_nonfinite(y, P["y"], None, f"max pool forward {kind} C{C}", close=exact)
    amh = am.cpu()
    _, am_finite = E.pool_fwd_taps(torch.where(torch.isnan(P["x"]), torch.full((), -NF.INF), P["x"]).numpy())
    nan_w = torch.isnan(P["y"])
    assert torch.equal(amh[~nan_w], torch.from_numpy(am_finite)[~nan_w]), "first maximal tap of the windows without a NaN"
    for n, ho, wo, c in nan_w.nonzero().tolist():
        tap = int(amh[n, ho, wo, c])
        assert tap < 9 and math.isnan(NF.pool_window(P["x"], n, ho, wo, c)[tap]), f"window {(n, ho, wo, c)}: argmax byte {tap} names no NaN tap"
    if C % 4:
        return
    dyd = g(P["dy"]).to(td)
    dx = torch.full((N, H, W, C), G.SENT, dtype=td, device=DEV)
    hip.call(f"detr_hip_maxpool3x3s2_bwd_{kind}", dyd.data_ptr(), am.data_ptr(), xd.data_ptr(), dx.data_ptr(), N, H, W, C, Ho, Wo)
    want = torch.zeros(N, H, W, C, dtype=torch.float64)
    for n, ho, wo, c in torch.ones(N, Ho, Wo, C).nonzero().tolist():
        kh, kw = divmod(int(amh[n, ho, wo, c]), 3)
        hi, wi = 2 * ho - 1 + kh, 2 * wo - 1 + kw
        if 0 <= hi < H and 0 <= wi < W:
            want[n, hi, wi, c] += float(P["dy"][n, ho, wo, c])
    want = torch.where(P["x"] <= 0, torch.zeros((), dtype=torch.float64), want)
    assert torch.equal(dx.float().cpu().double(), want), f"max pool backward {kind} C{C}"
    for n, ho, wo, c in nan_w.nonzero().tolist():          # (every NaN tap of these maps belongs to NaN windows only: nothing else adds to it)
        kh, kw = divmod(int(amh[n, ho, wo, c]), 3)
        assert math.isnan(float(P["x"][n, 2 * ho - 1 + kh, 2 * wo - 1 + kw, c]))


def test_subsample_copies_nan_and_inf(hip):
    N, H, W = NF.POOL_HW
    x = NF.pool_problem(8)["x"]
    x[0, 2, 4, 3], x[1, 8, 10, 5] = NF.NAN, -NF.INF
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.full((N, Ho, Wo, 8), G.SENT, device=DEV)
    xd = g(x)
    hip.call("detr_hip_subsample2_fwd_f32", xd.data_ptr(), y.data_ptr(), N, H, W, 8, Ho, Wo)
    want = x[:, ::2, ::2, :].double()
    assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any())
    assert_same_nonfinite(y, want, None, "subsample forward", close=exact)
    dx = torch.full((N, H, W, 8), G.SENT, device=DEV)
    hip.call("detr_hip_subsample2_bwd_f32", y.data_ptr(), dx.data_ptr(), N, H, W, 8, Ho, Wo)
    back = torch.zeros(N, H, W, 8, dtype=torch.float64)
    back[:, ::2, ::2, :] = want
    assert_same_nonfinite(dx, back, None, "subsample backward", close=exact)


# ------------------------------------------------------------------------------------------------------------------------
# row ops
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", NF.ROW_OPS)
def test_row_ops_propagate_nan_and_inf(hip, op):
    """Each row op at a little over one block against its one-line fp64 form.  Exact ops (add, add_bcast, scale_cols*, cvt_bf16,
    dropout, relu_mask) must equal the reference rounded to the output type; the others keep 1e-6 of the largest value (colsum:
    the 5e-5 of the bias-gradient tests)."""
    P = NF.row_problem(op)
    n = NF.ROW_N
    dev = {k: g(t) for k, t in P.items() if torch.is_tensor(t) and not k.startswith("ref") and t.dtype != torch.bool}      # held until the test ends
    out = torch.full((n,), G.SENT, device=DEV)
    f32 = lambda t: t.float().double()
    if op == "add":
        hip.call("detr_hip_add_f32", dev["a"].data_ptr(), dev["b"].data_ptr(), out.data_ptr(), n)
        assert_same_nonfinite(out, f32(P["ref"]), None, op, close=exact)
    elif op == "add_bcast":
        hip.call("detr_hip_add_bcast_f32", dev["a"].data_ptr(), dev["p"].data_ptr(), out.data_ptr(), n, P["p"].numel())
        assert_same_nonfinite(out, f32(P["ref"]), None, op, close=exact)
    elif op == "axpy":
        out.copy_(dev["b"])
        hip.call("detr_hip_axpy_f32", out.data_ptr(), dev["a"].data_ptr(), ctypes.c_float(2.0), n)
        assert_same_nonfinite(out, P["ref"], None, op, close=close_tensor(1e-6))
    elif op in ("scale_cols", "scale_cols_bf16", "scale_cols_t"):
        rows, cols = P["w"].shape
        o = torch.full((rows * cols,), G.SENT, dtype=B16 if op == "scale_cols_bf16" else F32, device=DEV)
        hip.call(f"detr_hip_{op}" + ("" if op == "scale_cols_bf16" else "_f32"), dev["w"].data_ptr(), dev["sc"].data_ptr(), o.data_ptr(), rows, cols)
        want = P["ref"].float()
        assert_same_nonfinite(o, (want.bfloat16() if op == "scale_cols_bf16" else want).double(), None, op, close=exact)
    elif op in ("colsum", "colsum_det", "colsum_scaled"):
        rows, cols = P["x"].shape
        o, xd = dev["out0"], dev["x"]
        if op == "colsum":
            hip.call("detr_hip_colsum_f32", xd.data_ptr(), o.data_ptr(), rows, cols, cols, ctypes.c_float(0.5))
        elif op == "colsum_det":
            ns = int(hip.load().detr_hip_colsum_det_scratch_floats(rows, cols))
            scr = torch.zeros(ns, device=DEV)
            hip.call("detr_hip_colsum_det_f32", xd.data_ptr(), o.data_ptr(), rows, cols, cols, ctypes.c_float(0.5), scr.data_ptr(), ns)
        else:
            hip.call("detr_hip_colsum_scaled", xd.data_ptr(), 0, rows, cols, cols, dev["sc"].data_ptr(), o.data_ptr())
        assert_same_nonfinite(o, P["ref"], None, op, close=close_tensor(5e-5))
    elif op == "cvt_bf16":
        o = torch.full((n,), G.SENT, dtype=B16, device=DEV)
        hip.call("detr_hip_cvt_bf16", dev["a"].data_ptr(), o.data_ptr(), n)
        assert_same_nonfinite(o, P["ref"], None, op, close=exact)
    elif op == "dropout":
        stepd = torch.tensor([NF.DROP_STEP] + [0] * 7, dtype=torch.int32, device=DEV)
        hip.call("detr_hip_dropout_f32", dev["a"].data_ptr(), out.data_ptr(), n, ctypes.c_float(NF.DROP_P), NF.DROP_SITE, stepd.data_ptr())
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(NF.DROP_P)))
        want = torch.where(P["keep"], P["a"] * scale, torch.zeros(()))
        assert torch.equal(torch.isfinite(want), torch.isfinite(P["ref"]))
        assert_same_nonfinite(out, want.double(), None, op, close=exact)
    elif op == "sigmoid_bwd":
        hip.call("detr_hip_sigmoid_bwd_f32", dev["a"].data_ptr(), dev["y"].data_ptr(), out.data_ptr(), n)
        assert_same_nonfinite(out, P["ref"], None, op, close=close_tensor(1e-6))
    elif op == "relu_mask":
        hip.call("detr_hip_relu_mask_f32", dev["a"].data_ptr(), dev["b"].data_ptr(), out.data_ptr(), n)
        assert_same_nonfinite(out, f32(P["ref"]), None, op, close=exact)
    elif op == "bn_fold":
        C = P["gamma"].numel()
        sc, sh = torch.full((C,), G.SENT, device=DEV), torch.full((C,), G.SENT, device=DEV)
        hip.call("detr_hip_bn_fold_f32", dev["gamma"].data_ptr(), dev["beta"].data_ptr(), dev["mean"].data_ptr(), dev["var"].data_ptr(),
                 sc.data_ptr(), sh.data_ptr(), C, ctypes.c_float(P["eps"]))
        assert_same_nonfinite(sc, P["ref_scale"], None, "bn_fold scale", close=close_tensor(1e-5))
        assert_same_nonfinite(sh, P["ref_shift"], None, "bn_fold shift", close=close_tensor(1e-5))
    else:
        raise ValueError(op)


# ------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,rows", NF.LN_CASES)
def test_layernorm_poisons_whole_rows_and_no_others(hip, C, rows):
    """NaN, +Inf and -Inf in three rows of x: those rows of y, y2 (the `add` form), y16, mean, rstd and dx are NaN (mean is +-Inf for
    the rows with an Inf: the one output where an Inf survives), every other row keeps the tolerances of
    test_layernorm_fwd_bwd (1e-5 forward, 2e-5 dx, 5e-5 dgamma / dbeta, per tensor); dgamma is NaN in every column and dbeta, which
    does not read x, is finite.  With three NaN in dy instead: three rows of dx, three columns of dgamma and dbeta."""
    P = NF.layernorm_problem(C, rows)
    xd, gd, bd, addd = g(P["x"]), g(P["gamma"]), g(P["beta"]), g(P["add"])
    new = lambda *s, dt=F32: torch.full(s, G.SENT, dtype=dt, device=DEV)
    y, y2, y16, mean, rstd = new(rows, C), new(rows, C), new(rows, C, dt=B16), new(rows), new(rows)
    hip.layernorm_fwd(xd, gd, bd, y, mean, rstd, NF.LN_EPS, add=addd, y2=y2, y16=y16)
    assert_same_nonfinite(y, P["y"], None, "layernorm y", close=close_tensor(1e-5))
    assert_same_nonfinite(y2, P["y2"], None, "layernorm y2", close=close_tensor(1e-5))
    assert_same_nonfinite(y16, y.cpu().to(B16).double(), None, "layernorm y16", close=exact)
    assert_same_nonfinite(rstd, P["rstd"], None, "layernorm rstd", close=close_tensor(1e-5))
    assert_same_nonfinite(mean, P["mean"], None, "layernorm mean", close=close_tensor(1e-5))      # (+-Inf for the rows that hold an Inf)
    for poison_dy in (False, True):
        Q = NF.layernorm_problem(C, rows, poison_dy=poison_dy) if poison_dy else P
        if poison_dy:
            xd = g(Q["x"])
            hip.layernorm_fwd(xd, gd, bd, y, mean, rstd, NF.LN_EPS)
        dx, dg, db = new(rows, C), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dyd = g(Q["dy"])
        hip.layernorm_bwd(dyd, xd, gd, mean, rstd, dx, dg, db)
        torch.cuda.synchronize()
        assert_same_nonfinite(dx, Q["dx"], None, f"layernorm dx (dy poisoned: {poison_dy})", close=close_tensor(2e-5))
        if poison_dy:
            assert_same_nonfinite(dg, Q["dgamma"], None, "layernorm dgamma", close=close_tensor(5e-5))
            assert_same_nonfinite(db, Q["dbeta"], None, "layernorm dbeta", close=close_tensor(5e-5))
        else:
            assert bool(torch.isnan(dg).all()), "dgamma sums over the poisoned rows: NaN in every column"
            assert_same_nonfinite(torch.cat([db.cpu(), torch.tensor([NF.NAN])]), torch.cat([Q["dbeta"], torch.tensor([NF.NAN], dtype=torch.float64)]),
                                  None, "layernorm dbeta", close=close_tensor(5e-5))


# ------------------------------------------------------------------------------------------------------------------------
# optimiser
# ------------------------------------------------------------------------------------------------------------------------
def _opt_device(P, packed):
    from test_gpu_adamw import KCHUNK, _flatten, _tables
    offs, total, ct, cs = _tables(packed)
    flat, m, v, gr = (g(torch.tensor(_flatten(a, offs, total))) for a in (P["p0"], P["m0"], P["v0"], P["grads"]))
    ctd, csd = g(torch.tensor(ct, dtype=torch.int32)), g(torch.tensor(cs, dtype=torch.int64))
    sed = g(torch.tensor([o + n for o, n in zip(offs, NF.OPT_SIZES)], dtype=torch.int64))
    tgd = g(torch.tensor(NF.OPT_TGROUP, dtype=torch.int32))
    sumsq = torch.zeros(len(ct), device=DEV)
    return dict(offs=offs, total=total, n=len(ct), chunk=KCHUNK, flat=flat, m=m, v=v, g=gr, ct=ctd, cs=csd, se=sed, tg=tgd, sumsq=sumsq)


def _opt_check(P, D, what):
    """Parameters, m and v after the step: adamw_ref's for the trained tensors (non-finite sets equal, the rest at the 1e-5 of
    test_joint_adamw_kernels_vs_ref), the initial bits for the others."""
    for arr, refd, init, name in ((D["flat"], P["p"], P["p0"], "parameters"), (D["m"], P["m"], P["m0"], "m"), (D["v"], P["v"], P["v0"], "v")):
        want = np.zeros(D["total"])
        for i, (o, n_) in enumerate(zip(D["offs"], NF.OPT_SIZES)):
            want[o:o + n_] = refd[i] if i in P["live"] else init[i]
        # (one finite element appended: with every group trained and no gaps, a NaN factor leaves nothing finite in the buffer itself)
        assert_same_nonfinite(torch.cat([arr.cpu(), torch.ones(1)]), torch.cat([torch.from_numpy(want), torch.ones(1, dtype=torch.float64)]), None,
                              f"{what} {name}", close=close_tensor(1e-5))
    for i in range(len(NF.OPT_SIZES)):
        if i not in P["live"]:                 # untrained: bit-identical
            sl = slice(D["offs"][i], D["offs"][i] + NF.OPT_SIZES[i])
            assert torch.equal(D["flat"][sl].cpu(), torch.tensor(P["p0"][i])) and torch.equal(D["m"][sl].cpu(), torch.tensor(P["m0"][i]))
            assert torch.equal(D["v"][sl].cpu(), torch.tensor(P["v0"][i]))


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("trained", [(True, True, True), (True, False, True)])
@pytest.mark.parametrize("special", [s for s, _ in NF.OPT_SPECIALS])
def test_joint_clip_poisons_what_the_reference_poisons(hip, special, trained, packed):
    """sumsq_segments -> global_clip_scale -> adamw with one NaN (Inf) gradient element in the 4097-element tensor: G and the factor
    are NaN (Inf and 0) as adamw_ref's, and after the step the non-finite parameters, m and v are the reference's -- every trained
    tensor for the NaN, the one element for the Inf (0 * Inf); with the tensor's group untrained nothing is non-finite and the group
    keeps its bits."""
    from test_gpu_adamw import _hyper16
    P = NF.optimiser_problem(dict(NF.OPT_SPECIALS)[special], joint=True, trained=trained)
    D = _opt_device(P, packed)
    hyper, scale = torch.zeros(16, device=DEV), torch.zeros(2, device=DEV)
    _hyper16(hip, hyper, 1, NF.OPT_CLIP, trained, wd=NF.OPT_WD)
    hip.call("detr_hip_sumsq_segments_f32", D["g"].data_ptr(), D["ct"].data_ptr(), D["cs"].data_ptr(), D["se"].data_ptr(), D["n"], D["chunk"], D["sumsq"].data_ptr())
    hip.call("detr_hip_global_clip_scale_f32", D["sumsq"].data_ptr(), D["ct"].data_ptr(), D["tg"].data_ptr(), hyper.data_ptr(), D["n"], scale.data_ptr())
    hip.call("detr_hip_adamw_f32", D["flat"].data_ptr(), D["g"].data_ptr(), D["m"].data_ptr(), D["v"].data_ptr(), D["ct"].data_ptr(), D["cs"].data_ptr(),
             D["se"].data_ptr(), D["tg"].data_ptr(), D["sumsq"].data_ptr(), hyper.data_ptr(), scale.data_ptr(), D["n"], D["chunk"])
    s_dev, G_dev = (float(x) for x in scale.cpu())
    assert_same_nonfinite(torch.tensor([s_dev, G_dev, 1.0]), torch.tensor([P["s"], P["G"], 1.0], dtype=torch.float64), None, "scale[0], G",
                          close=close_tensor(1e-5))
    _opt_check(P, D, f"joint {special}")


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("special", [s for s, _ in NF.OPT_SPECIALS])
@pytest.mark.parametrize("entry", ["adamw", "clip_adam"])
def test_per_tensor_clip_poisons_the_whole_tensor(hip, entry, special, packed):
    """The per-tensor clip of detr_hip_adamw_f32 (no joint scale) and of detr_hip_clip_adam_f32: a NaN gradient element makes the norm
    of its tensor NaN and with it every element of that tensor's parameters, m and v, as in the reference formula
    clip / max(norm, clip); the other tensors are updated as usual.  An Inf element gives the factor 0 and one NaN (0 * Inf)."""
    import adamw_ref as A
    wd = NF.OPT_WD if entry == "adamw" else 0.0
    P = NF.optimiser_problem(dict(NF.OPT_SPECIALS)[special], joint=False)
    if entry == "clip_adam":                   # no decay: the reference step again with weight_decay 0
        ref = A.AdamW(dict(enumerate(NF.OPT_LRS)), dict(enumerate(NF.OPT_TGROUP)), weight_decay=0.0, clipnorm=NF.OPT_CLIP)
        ref.m = {i: P["m0"][i].astype(np.float64) for i in range(len(NF.OPT_SIZES))}
        ref.v = {i: P["v0"][i].astype(np.float64) for i in range(len(NF.OPT_SIZES))}
        params = {i: p.astype(np.float64) for i, p in enumerate(P["p0"])}
        with np.errstate(invalid="ignore", over="ignore"):
            ref.step(dict(enumerate(P["grads"])), params)
        P = dict(P, p=params, m=ref.m, v=ref.v)
    D = _opt_device(P, packed)
    hip.call("detr_hip_sumsq_segments_f32", D["g"].data_ptr(), D["ct"].data_ptr(), D["cs"].data_ptr(), D["se"].data_ptr(), D["n"], D["chunk"], D["sumsq"].data_ptr())
    if entry == "adamw":
        from test_gpu_adamw import _hyper16
        hyper = torch.zeros(16, device=DEV)
        _hyper16(hip, hyper, 1, NF.OPT_CLIP, (True, True, True), wd=wd)
        hip.call("detr_hip_adamw_f32", D["flat"].data_ptr(), D["g"].data_ptr(), D["m"].data_ptr(), D["v"].data_ptr(), D["ct"].data_ptr(), D["cs"].data_ptr(),
                 D["se"].data_ptr(), D["tg"].data_ptr(), D["sumsq"].data_ptr(), hyper.data_ptr(), None, D["n"], D["chunk"])
    else:
        lr_t = [lr * math.sqrt(1 - 0.999) / (1 - 0.9) for lr in NF.OPT_LRS]
        hyper = torch.tensor(lr_t + [NF.OPT_CLIP, 0.9, 0.999, 1e-7, 0.0], dtype=torch.float32, device=DEV)
        hip.call("detr_hip_clip_adam_f32", D["flat"].data_ptr(), D["g"].data_ptr(), D["m"].data_ptr(), D["v"].data_ptr(), D["ct"].data_ptr(), D["cs"].data_ptr(),
                 D["se"].data_ptr(), D["tg"].data_ptr(), D["sumsq"].data_ptr(), hyper.data_ptr(), D["n"], D["chunk"])
    _opt_check(P, D, f"{entry} {special}")


def test_ema_poisons_one_shadow_element(hip):
    """detr_hip_ema_f32 with one NaN and one Inf parameter: those two shadow elements, nothing else (bit-equal to ema_ref elsewhere)."""
    import ema_ref as E
    from test_gpu_adamw import KCHUNK, SIZES, _tables
    offs, total, ct, cs = _tables(False)
    rng = np.random.default_rng(5)
    s_host, p_host = rng.normal(size=total).astype(np.float32), rng.normal(size=total).astype(np.float32)
    i_nan, i_inf = offs[4] + 1234, offs[5] + 77
    p_host[i_nan], p_host[i_inf] = np.nan, np.inf
    shadow, param = g(torch.from_numpy(s_host)), g(torch.from_numpy(p_host))
    hyper = torch.zeros(8, device=DEV)
    omd = E.omd_of(0.9998)
    hip.call("detr_hip_set_floats8_f32", hyper.data_ptr(), float(omd), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    ctd, csd = g(torch.tensor(ct, dtype=torch.int32)), g(torch.tensor(cs, dtype=torch.int64))
    sed = g(torch.tensor([o + n for o, n in zip(offs, SIZES)], dtype=torch.int64))
    hip.call("detr_hip_ema_f32", shadow.data_ptr(), param.data_ptr(), ctd.data_ptr(), csd.data_ptr(), sed.data_ptr(), hyper.data_ptr(), len(ct), KCHUNK)
    torch.cuda.synchronize()
    mask = np.zeros(total, bool)
    for o, n in zip(offs, SIZES):
        mask[o:o + n] = True
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.where(mask, E.update(s_host, p_host, omd), s_host)
    assert np.isnan(want[i_nan]) and np.isinf(want[i_inf]) and int((~np.isfinite(want)).sum()) == 2
    assert_same_nonfinite(shadow, torch.from_numpy(want).double(), None, "ema shadow", close=exact)


# ------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------
E2E_WEIGHTS = ["backbone/layer1/0/conv2/kernel", "backbone/conv1/kernel", "backbone/layer4/2/conv1/kernel", "transformer/encoder/layer_0/linear1/bias",
               "class_embed/kernel"]
E2E_GROUPS = ("backbone", "transformers", "nlayers")


@pytest.fixture(scope="module")
def e2e():
    """One model + optimisers per precision (the model of test_gpu_training.py: one encoder and two decoder layers, dropout 0), built on
    first use and put back to its initial weights and zero moments in front of every case."""
    from detr_tf.optimizers import setup_optimizers
    from test_gpu_training import _cfg, _model
    built = {}

    def get(precision):
        if precision not in built:
            cfg = _cfg()
            cfg.use_graph = False
            cfg.global_clipnorm, cfg.weight_decay = 0.1, 1e-4
            model = _model(cfg, dropout=0.0, precision=precision)
            opt = setup_optimizers(model, cfg)
            built[precision] = (cfg, model, opt, model.engine.P.flat.clone())
        cfg, model, opt, flat0 = built[precision]
        st = model.engine.P
        st.flat.copy_(flat0)
        st.adam_m.zero_(), st.adam_v.zero_()
        for n in E2E_GROUPS:
            opt[f"{n}_optimizer"].iterations = 0
            opt.pop(f"{n}_gradients", None)
        opt.pop("_joint_gradients", None)
        model.engine.bump_weights_version()
        return cfg, model, opt
    yield get
    built.clear()
    gc.collect()


def _step(cfg, model, opt, images, tb, tc):
    from detr_tf import training
    out, total, log, steps = training.run_train_step(model, images, tb, tc, opt, cfg)
    logits, boxes = out["pred_logits"].float().cpu(), out["pred_boxes"].float().cpu()
    for name in steps:
        training.aggregate_grad_and_apply(name, opt, steps[name]["gradients"], 0, cfg)
    torch.cuda.synchronize()
    return logits, boxes, float(total)


def _probe_class_head_input(model, images, index):
    """h_j of every query at every decoder level, for the class-head weight at flat index `index`: the difference of two finite
    forwards (training mode, dropout 0) whose only difference is 1.0 added to that weight."""
    st = model.engine.P

    def all_logits():
        out = model(images, training=True)
        levels = [out["pred_logits"]] + [a["pred_logits"] for a in out.get("aux", [])]
        return torch.stack([l.float().cpu() for l in levels])
    base = all_logits()
    keep = st.flat[index].clone()
    st.flat[index] = keep + 1.0
    model.engine.bump_weights_version()
    moved = all_logits()
    st.flat[index] = keep
    model.engine.bump_weights_version()
    d = (moved - base).abs().amax(dim=(0, 1, 2))
    c = int(d.argmax())                        # the one class whose logit moved
    return (moved - base)[..., c]


@pytest.mark.parametrize("special", ["nan", "inf"])
@pytest.mark.parametrize("name", E2E_WEIGHTS)
@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "bf16"])
def test_one_nonfinite_weight_poisons_the_step(hip, e2e, precision, name, special):
    """One weight element NaN (+Inf) in front of an eager training step (B = 2, 96 x 128) with the joint clip: a layer1 3x3 kernel,
    the stem kernel, a layer4 1x1 kernel, an encoder linear1 bias, the class-head kernel.  Logits and boxes (the class-head case: the logits) are non-finite, the loss
    is NaN, and after the step every trained parameter is non-finite: the joint norm holds the NaN gradient, so the factor and with
    it the whole update are NaN, as tests/adamw_ref.py and oracle/optim_ref.py's clip / max(norm, clip) make them."""
    from test_gpu_training import _batches
    cfg, model, opt = e2e(precision)
    st = model.engine.P
    (im, tb, tc), = _batches(1, seed=11)
    o, n = st.offsets[name]
    hj = None
    if special == "inf" and name == "class_embed/kernel":
        hj = _probe_class_head_input(model, im, o + n // 2)
    st.flat[o + n // 2] = dict(NF.OPT_SPECIALS)[special]
    model.engine.bump_weights_version()
    logits, boxes, total = _step(cfg, model, opt, im, tb, tc)
    assert not bool(torch.isfinite(logits).all()), f"{precision} {name}: the logits are finite"
    if name != "class_embed/kernel":             # (the boxes come from the other head: with a poisoned class head they stay finite, in the oracle too)
        assert not bool(torch.isfinite(boxes).all()), f"{precision} {name}: the boxes are finite"
    if special == "inf" and name == "class_embed/kernel":
        # +Inf in W[c, j] of the class head gives each query the logit sign(h_j) * Inf.  The signs come from a FINITE probe, not from the
        # poisoned run: the logits with W[c, j] + 1 minus the logits with W[c, j] are h_j, at every decoder level.  One +Inf logit makes
        # the softmax, and the loss, NaN; where every h_j is negative the class has probability 0 and the loss is finite in exact
        # arithmetic too (the expected outcome is then `finite`, fixed before the poisoned run is looked at).
        assert hj is not None
        if not bool((hj >= 0).any()):
            assert not bool((logits == NF.INF).any()) and not bool(torch.isnan(logits).any()) and math.isfinite(total), (precision, total)
            return
        assert bool((logits == NF.INF).any()) or bool(torch.isnan(logits).any())
    assert math.isnan(total), f"{precision} {name}: the loss is {total}"
    s, G_ = (float(x) for x in opt["_joint"].scale.cpu())
    assert math.isnan(G_) and math.isnan(s), f"joint norm {G_}, factor {s}"
    flat = st.flat.cpu()
    trained = torch.zeros(st.total, dtype=torch.bool)
    for grp in E2E_GROUPS:
        for k in opt[f"{grp}_optimizer"].names:
            o, n = st.offsets[k]
            trained[o:o + n] = True
    assert bool(trained.any()) and not bool(torch.isfinite(flat[trained]).any()), \
        f"{int(torch.isfinite(flat[trained]).sum())} of {int(trained.sum())} trained parameters stayed finite"


@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "bf16"])
def test_an_inf_pixel_makes_the_loss_nan(hip, e2e, precision):
    """All weights finite, one +Inf pixel in a float image: the loss of the step is NaN."""
    from test_gpu_training import _batches
    cfg, model, opt = e2e(precision)
    (im, tb, tc), = _batches(1, seed=12)
    im = im.copy()
    im[1, 40, 60, 1] = np.inf
    _, _, total = _step(cfg, model, opt, im, tb, tc)
    assert math.isnan(total), f"{precision}: the loss is {total}"



# ------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------
ATT_IDS = [f"{c}-{'masked' if m else 'unmasked'}" for c, m in NF.ATT_CASES]


@pytest.mark.parametrize("case,masked", NF.ATT_CASES, ids=ATT_IDS)
def test_attention_fp32_propagates_nan_and_inf(hip, case, masked):
    """The fp32 attention core, forward, backward and attention_weights at T = 40, S = 70, B = 2 against fp64 autograd on the same
    poisoned operands (nonfinite_cases.attention_problem), per batch element at the tolerances of test_masked_fp32_vs_fp64 (O 2e-5,
    lse 1e-5, gradients 5e-5; the maps 2e-5).  A masked key is absent: NaN in its k row poisons nothing, its weight, dk and dv are
    exactly 0.  lse is non-finite where the reference's is (logsumexp of a row with a +Inf score is +Inf, the kernel's running sum
    NaN: either poisons the row)."""
    B, T, S, H, HD = NF.ATT_B, NF.ATT_T, NF.ATT_S, NF.ATT_H, NF.ATT_HD
    D = H * HD
    scale = HD ** -0.5
    q, k, v, do, kv = NF.attention_problem(case, masked)
    ref = NF.attention_reference(q, k, v, do, kv, scale)
    d = lambda t: t.float().reshape(-1, D).to(DEV)
    q_, k_, v_, do_ = d(q), d(k), d(v), d(do)
    new = lambda rows: torch.full((rows, D), G.SENT, device=DEV)
    o, dq, dk, dv = new(B * T), new(B * T), new(B * S), new(B * S)
    lse, delta = torch.full((B * H * T,), G.SENT, device=DEV), torch.full((2 * B * H * T,), G.SENT, device=DEV)
    stepd = torch.tensor([12345] + [0] * 7, dtype=torch.int32, device=DEV)
    kw = dict(scale=scale, dropout_p=0.0, dropout_site=5, dropout_step=stepd, compute=0)
    words = None
    if kv is not None:
        words = torch.from_numpy(hip.keymask_words_from_valid(kv.numpy())).reshape(-1).to(DEV)
        kw["key_valid"] = words
    hip.attention(q_, k_, v_, o, lse, B, H, T, S, **kw)
    hip.attention(q_, k_, v_, o, lse, B, H, T, S, d_o=do_, dq=dq, dk=dk, dv=dv, delta=delta, **kw)
    wmap = torch.full((B, T, S), G.SENT, device=DEV)
    hip.attention_weights(q_, k_, lse, wmap, B, H, T, S, scale=scale, key_valid=words)
    torch.cuda.synchronize()
    got = dict(o=o.view(B, T, D), dq=dq.view(B, T, D), dk=dk.view(B, S, D), dv=dv.view(B, S, D), w=wmap)
    for name, rtol in (("o", 2e-5), ("dq", 5e-5), ("dk", 5e-5), ("dv", 5e-5), ("w", 2e-5)):
        for b in range(B):
            assert_same_nonfinite(got[name][b], ref[name][b], None, f"fp32 {case} {name} (batch element {b})", close=close_tensor(rtol))
    l, lr = lse.view(B, H, T).cpu().double(), ref["lse"]
    assert torch.equal(torch.isfinite(l), torch.isfinite(lr)), f"{case}: lse is non-finite at other rows than the reference's"
    fin = torch.isfinite(lr)
    assert float((l[fin] - lr[fin]).abs().max()) <= 1e-5 * float(lr[fin].abs().max())
    if kv is not None:
        inv = (~kv).to(DEV)
        assert bool((got["dk"][inv] == 0).all()) and bool((got["dv"][inv] == 0).all()) and bool((wmap.cpu()[(~kv)[:, None, :].expand(B, T, S)] == 0).all())


@pytest.mark.parametrize("case,masked", NF.ATT_CASES, ids=ATT_IDS)
def test_attention_bf16_propagates_nan_and_inf(hip, case, masked):
    """The all-bf16 attention core (csrc/attention_dma.hip) and attention_weights on bf16 operands, same cases.  The non-finite sets of
    O, lse, dQ, dK, dV and the map are those of fp64 autograd on the poisoned operands (scores in log2 units of the stored query).
    The finite remainder is held to the per-element bounds of test_gpu_masked_bounds.py (oracle/attn_bounds.py, tests/attn_weights_ref.py)
    computed on the operands with the special replaced by 0: an element the reference leaves finite does not depend on the special,
    except in the (batch, head) of the +Inf key.  There the queries whose score is -Inf see that key at weight 0, which is the same
    problem with the key marked invalid: a second set of references with that key masked for the batch element gives their O, lse,
    dQ (but the column of the Inf element, 0 * Inf = NaN in the reference too) and the map's other columns, at the same bounds; the
    map's column of the key itself is the first reference minus that head's term.  dK / dV of the (batch, head) are NaN throughout
    (every key's sum runs over the NaN rows): asserted."""
    import attn_cases as AC
    import attn_weights_ref as AW
    from oracle import attn_bounds as AB
    B, T, S, H, HD = NF.ATT_B, NF.ATT_T, NF.ATT_S, NF.ATT_H, NF.ATT_HD
    D = H * HD
    q, k, v, do, kv = NF.attention_problem(case, masked)
    true = NF.attention_reference(q, k, v, do, kv, math.log(2.0))
    dev = AC.device_operands(hip, q, k, v, do, B, T, S, 0.0, extra=8, key_valid=kv)
    AC.fwd(hip, dev, B, T, S, 0)
    AC.bwd(hip, dev, B, T, S, 0, dev["o"], dev["lse"])
    wmap = torch.full((B, T, S), G.SENT, device=DEV)
    hip.attention_weights(dev["q"], dev["k"], dev["lse"][:B * H * T].contiguous(), wmap, B, H, T, S, scale=HD ** -0.5, key_valid=dev["kw"].get("key_valid"))
    torch.cuda.synchronize()
    for n, rows in (("o", B * T), ("dq", B * T), ("dk", B * S), ("dv", B * S)):
        assert bool((dev[n][rows:] == -1234.0).all()), f"{n}: sentinel rows overwritten"
    got = dict(o=dev["o"][:B * T].float().view(B, T, D), dq=dev["dq"][:B * T].float().view(B, T, D), dk=dev["dk"][:B * S].float().view(B, S, D),
               dv=dev["dv"][:B * S].float().view(B, S, D), w=wmap, lse=dev["lse"][:B * H * T].view(B, H, T))
    qc, kc, vc = NF.finite_copy(q), NF.finite_copy(k), NF.finite_copy(v)
    fw = AB.forward(qc, kc, vc, H, None, 0.0, key_valid=kv)
    o_stored = NF.finite_copy(got["o"].double().cpu())
    bw = AB.backward(qc, kc, vc, do, o_stored, H, None, 0.0, key_valid=kv)
    lse_clean = NF.finite_copy(got["lse"].cpu().double()).reshape(B * H, T).float()
    W, Bw = AW.kernel_reference_and_bound(qc, kc, lse_clean, H, True, key_valid=kv)
    bp, hp = NF.ATT_POISON
    region = torch.ones(B, 1, D, dtype=torch.bool)
    wregion = torch.ones(B, 1, 1, dtype=torch.bool)
    if case == "k_pinf":
        region[bp, 0, hp * HD:(hp + 1) * HD] = False
        wregion[bp] = False
    refs = dict(o=(fw["o"], fw["bound_o"], region), dq=(bw["dq"], bw["bound_dq"], region), dk=(bw["dk"], bw["bound_dk"], region),
                dv=(bw["dv"], bw["bound_dv"], region), w=(W, Bw, wregion))
    for name, (r, bound, reg) in refs.items():
        t = true[name]
        # (dq: the kernel's is with respect to the unscaled query, a positive multiple of the reference's -- the same non-finite set)
        assert_same_nonfinite(got[name], t, None, f"bf16 {case} {name}", close=lambda *a: None)
        sel = torch.isfinite(t) & reg.expand_as(t)
        assert bool(sel.any())
        ratio = AB.ratio(got[name].cpu()[sel], r[sel], bound[sel])
        assert ratio <= 1.0, f"bf16 {case} {name}: max |err| / bound = {ratio:.3f} on the finite remainder"
    l, lt = got["lse"].cpu().double(), true["lse"]
    assert torch.equal(torch.isfinite(l), torch.isfinite(lt)), f"bf16 {case}: lse is non-finite at other rows than the reference's"
    sel = torch.isfinite(lt) & region[:, :, ::HD].transpose(1, 2).expand(B, H, T)
    assert AB.ratio(l[sel], fw["lse"].view(B, H, T)[sel], fw["bound_lse"].view(B, H, T)[sel]) <= 1.0, f"bf16 {case}: lse"
    if case == "k_pinf":
        # the (batch, head) of the +Inf key: rows with a -Inf score, against the references with that key marked invalid
        bI, sI, colI = (int(x) for x in torch.isinf(k).nonzero()[0])
        assert (bI, colI // HD) == (bp, hp)
        kv2 = kv.clone() if kv is not None else torch.ones(B, S, dtype=torch.bool)
        assert bool(kv2[bI, sI])
        kv2[bI, sI] = False
        fw2 = AB.forward(qc, kc, vc, H, None, 0.0, key_valid=kv2)
        bw2 = AB.backward(qc, kc, vc, do, o_stored, H, None, 0.0, key_valid=kv2)
        W2, Bw2 = AW.kernel_reference_and_bound(qc, kc, lse_clean, H, True, key_valid=kv2)
        blk = slice(hp * HD, (hp + 1) * HD)
        rows = torch.isfinite(true["o"][bp, :, hp * HD])          # the queries whose score is -Inf
        assert bool(rows.any()) and bool((~rows).any())
        assert bool((torch.isfinite(true["w"][bp]).all(-1) == rows).all())
        for name, r2, b2 in (("o", fw2["o"], fw2["bound_o"]), ("dq", bw2["dq"], bw2["bound_dq"])):
            sel = torch.zeros(B, T, D, dtype=torch.bool)
            sel[bp, :, blk] = rows[:, None]
            if name == "dq":
                sel[bp, :, colI] = False
            assert bool(torch.isfinite(true[name])[sel].all()) and int(sel.sum()) >= 5 * (HD - 1)
            ratio = AB.ratio(got[name].cpu()[sel], r2[sel], b2[sel])
            assert ratio <= 1.0, f"bf16 k_pinf {name}, rows with a -Inf score: max |err| / bound = {ratio:.3f}"
        ratio = AB.ratio(l[bp, hp][rows], fw2["lse"].view(B, H, T)[bp, hp][rows], fw2["bound_lse"].view(B, H, T)[bp, hp][rows])
        assert ratio <= 1.0, f"bf16 k_pinf lse, rows with a -Inf score: {ratio:.3f}"
        valid_keys = kv2[bp]
        assert not bool(torch.isfinite(true["dk"][bp][valid_keys][:, blk]).any()) and not bool(torch.isfinite(true["dv"][bp][valid_keys][:, blk]).any())
        # the map: every column but the key's from the second reference (its normaliser is the lse given, so masking the key only
        # removes its column) ...
        wg = got["w"].cpu().double()[bp][rows]
        cols = torch.arange(S) != sI
        ratio = AB.ratio(wg[:, cols], W2[bp][rows][:, cols], Bw2[bp][rows][:, cols])
        assert ratio <= 1.0, f"bf16 k_pinf map, rows with a -Inf score: {ratio:.3f}"
        # ... and the key's own column: the other heads' weights, this head's exactly 0 -- the first reference (the Inf element as 0)
        # minus this head's term exp2(s - L) / H, inside the first reference's bound (which still holds that term's share)
        L2 = lse_clean.double().view(B, H, T)[bp, hp][rows] * AW.LOG2E
        term = torch.exp2(qc[bp][rows][:, blk].double() @ kc[bp, sI, blk].double() - L2) / H
        ratio = AB.ratio(wg[:, sI], W[bp][rows][:, sI] - term, Bw[bp][rows][:, sI])
        assert ratio <= 1.0, f"bf16 k_pinf map, the key's column at the rows with a -Inf score: {ratio:.3f}"
        assert float(term.min()) > 4.0 * float(Bw[bp][rows][:, sI].max()), "the head's term must be visible against the bound"
    if kv is not None:
        inv = (~kv).to(DEV)
        assert bool((got["dk"][inv] == 0).all()) and bool((got["dv"][inv] == 0).all())
