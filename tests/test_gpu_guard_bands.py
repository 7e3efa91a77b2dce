"""Guard bands around the matrix kernels: the GEMM families (tile engine, streaming, ring, ring fp32, GEMM + LayerNorm, ring weight
gradient), the 3x3 convolutions (tile, f32x3, halo-staged, LDS-DMA, stride-2 classes, dilation 2), the stem and the fused 1x1 backward,
run the way the engine calls them: operands inside larger buffers, at pitches wider than their extent, next to live data.

Every input lies in a NaN-filled buffer, every output and scratch buffer in a sentinel-filled one (tests/guard_band_cases.py).  Each
case asserts (a) a finite output, (b) the fp64 reference of the same operation on the same stored values at the tolerance the older
test of that kernel family uses, (c) untouched frames and (d), where two launches are compared, identical bits: NaN padding against
zero padding on the same buffers, scratch of exactly the size the library reports against a large one.  The GEMM cases assert the
kernel family of the descriptor they launch (detr_hip_gemm_family); tests/test_guard_bands_cpu.py shows on the CPU that every case
reaches the family it states, so nothing here is skipped."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import guard_band_cases as G
from matrix_refs import C0, RS0, check_close, conv_problem, gemm_reference, gemm_values, stem_problem

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, B16, U8 = torch.float32, torch.bfloat16, torch.uint8
BIG_WS_FLOATS = 16 * 1024 * 1024


@pytest.fixture(autouse=True)
def _reset_library_tuning():
    """The library reads its DETR_HIP_* tuning variables once (at load) and on detr_hip_reload_tuning(): a test that switches
    one through hip.set_tuning() must not leak it into the next test."""
    import os
    yield
    from detr_tf import _hip
    for k in [k for k in G.TUNING_VARS if k in os.environ]:
        _hip.set_tuning(k, None)


@pytest.fixture(scope="module")
def big_ws():
    return torch.empty(BIG_WS_FLOATS, device=DEV)


def bits_of(t):
    """The stored bits of a (possibly strided) tensor, on the host."""
    t = t.contiguous().cpu()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def zero_the_frame(buf):
    """NaN padding -> zero padding, in place (the values themselves hold no NaN)."""
    buf[torch.isnan(buf)] = 0


# ------------------------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------------------------
def gemm_launch(hip, c, v, *, zero_pad=False, workspace=None, workspace_bytes=0, family=None):
    """Frames every operand of the case, asserts the family of the descriptor and launches it.  {name: (view, buffer)}."""
    t = {}
    for name, (shape, dtype, lead, pitch, is_out) in G.operands(c).items():
        if is_out:
            t[name] = G.sentinel_framed(shape, dtype, lead, pitch, device=DEV)
            if name == "C" and c["split"] > 1:
                t[name][0].fill_(C0)
            if name == "rowsum_a":
                t[name][0].fill_(RS0)
        elif dtype == U8:
            t[name] = G.bits_framed(v[name], lead, pitch, device=DEV, fill=0x00 if zero_pad else 0xFF)
        else:
            t[name] = G.nan_framed(v[name].to(dtype), lead, pitch, device=DEV)
            if zero_pad:
                zero_the_frame(t[name][1])
    step = torch.tensor([G.DROP_STEP] + [0] * 7, dtype=torch.int32, device=DEV)
    d = G.fill_desc(hip, c, {n: vb[0].data_ptr() for n, vb in t.items()}, dropout_step=step.data_ptr(), workspace=workspace,
                    workspace_bytes=workspace_bytes)
    lib = hip.load()
    fam = lib.detr_hip_gemm_family(ctypes.byref(d))
    want = c["family"] if family is None else family
    assert fam == want, f"{G.case_id(c)}: family {fam}, the case is about family {want} ({lib.detr_hip_last_error().decode() if fam < 0 else ''})"
    hip._check(lib.detr_hip_gemm_f32(ctypes.byref(d), hip._stream()), "detr_hip_gemm_f32")
    torch.cuda.synchronize()
    return t, d


def gemm_check(c, v, t, ref):
    what = G.case_id(c)
    C = t["C"][0]
    check_close(C, ref, c["tol"], what)
    for name, (shape, dtype, lead, pitch, is_out) in G.operands(c).items():
        if is_out:
            assert G.frame_intact(t[name][1], t[name][0]), f"{what}: the launch wrote outside {name}"
    if c["bits_out"]:
        assert torch.equal(t["maskbits_out"][0].cpu(), G.pack_bits(C.float().cpu() > 0)), f"{what}: mask bits out"
    if c["rowsum"]:
        A = v["A"].double()
        check_close(t["rowsum_a"][0], RS0 + c["alpha"] * (A.sum(1) if c["ak"] else A.sum(0)), "f32", what + " row sums")
    if c["ln"] is not None:
        N = c["N"]
        Cd = C.cpu().double()
        want = F.layer_norm(Cd, (N,), v["ln_gamma"].double(), v["ln_beta"].double(), G.LN_EPS)
        y = t["ln_y"][0]
        check_close(y, want, "f32", what + " ln_y")
        check_close(t["ln_mean"][0], Cd.mean(1), "f32", what + " ln_mean")
        check_close(t["ln_rstd"][0], 1.0 / torch.sqrt(Cd.var(1, unbiased=False) + G.LN_EPS), "f32", what + " ln_rstd")
        if c["ln"]["add"]:
            rows = torch.arange(c["M"]) % c["ln"]["add_rows"]
            assert torch.equal(t["ln_y2"][0].cpu(), y.cpu() + v["ln_add"][rows]), what + " ln_y2"
        if c["ln"]["y16"]:
            assert torch.equal(bits_of(t["ln_y16"][0]), bits_of(y.to(B16))), what + " ln_y16"


@pytest.mark.parametrize("c", G.gemm_cases(), ids=G.case_id)
def test_gemm_inside_nan_and_sentinel_frames(hip, c):
    """Every GEMM family on framed operands: (a) - (c), and (d) NaN padding against zero padding."""
    v = gemm_values(c)
    ref = gemm_reference(c, v)
    with G.tuning(hip, c["env"]):
        t, _ = gemm_launch(hip, c, v)
        t0, _ = gemm_launch(hip, c, v, zero_pad=True)
    gemm_check(c, v, t, ref)
    for name, (shape, dtype, lead, pitch, is_out) in G.operands(c).items():
        if is_out:
            assert torch.equal(bits_of(t[name][0]), bits_of(t0[name][0])), f"{G.case_id(c)}: {name} depends on what the padding holds"


def guarded_scratch(nbytes):
    """(fp32 view of exactly nbytes, its buffer): the guard behind the view is at least as large as the view, so even a two-fold
    under-report stays inside this allocation."""
    assert nbytes % 4 == 0
    n = nbytes // 4
    return G.sentinel_framed((n,), F32, 64, None, tail=n + 1024, device=DEV)


@pytest.mark.parametrize("c", G.split_cases(), ids=G.case_id)
def test_split_k_stays_inside_the_scratch_it_asks_for(hip, big_ws, c):
    """Split-K through scratch of exactly detr_hip_workspace_bytes_gemm (asked on the descriptor that is launched), of exactly the
    documented floor split_k * (M * N [+ M]) * 4 (row-major slabs) and of 16M floats: the same bits, (b), guards intact."""
    v = gemm_values(c)
    ref = gemm_reference(c, v)
    lib = hip.load()
    outs = []
    with G.tuning(hip, c["env"]):
        probe = G.fill_desc(hip, c, G.placeholder_ptrs(c))
        query, floor = int(lib.detr_hip_workspace_bytes_gemm(ctypes.byref(probe))), G.split_floor_bytes(c)
        assert query >= floor > 0
        for nbytes in (query, floor, None):
            if nbytes is None:
                t, d = gemm_launch(hip, c, v, workspace=big_ws.data_ptr(), workspace_bytes=big_ws.numel() * 4)
            else:
                ws, ws_buf = guarded_scratch(nbytes)
                # (with the floor alone the ring weight gradient, which writes tile-ordered slabs, leaves the launch to the 4-wave engine)
                fam = 0 if (c["family"] == 5 and nbytes < query) else None
                t, d = gemm_launch(hip, c, v, workspace=ws.data_ptr(), workspace_bytes=nbytes, family=fam)
                assert int(lib.detr_hip_workspace_bytes_gemm(ctypes.byref(d))) == query
                assert G.frame_intact(ws_buf, ws), f"{G.case_id(c)}: wrote past {nbytes} bytes of scratch (query {query}, floor {floor})"
                assert not bool((ws == G.SENT).all()), "the scratch was not used"
            gemm_check(c, v, t, ref)
            outs.append(t)
    for t in outs[1:]:
        assert torch.equal(bits_of(t["C"][0]), bits_of(outs[0]["C"][0])), f"{G.case_id(c)}: the result depends on the scratch size"
        if c["rowsum"]:
            assert torch.equal(bits_of(t["rowsum_a"][0]), bits_of(outs[0]["rowsum_a"][0]))


def test_gemm_group_shares_of_an_exactly_sized_workspace(hip, big_ws):
    """Three weight gradients of different sizes through gemm_group on a shared workspace of exactly what the wrapper hands out: one
    equal share per member, each the largest member's 256-byte-rounded query (the wrapper cuts WORKSPACE into equal shares).  The
    wrapper did not have to grow it, nothing behind it is touched, every member equals its own launch bit for bit."""
    members = [G.gcase("group", 136, 72, 8 * 331, 0, 0, split=5, compute=1, scale=1, alpha=0.5, rowsum=1, lda=140, ldb=76, ldc=76, tol="split"),
               G.gcase("group", 264, 136, 2100, 0, 0, split=3, compute=1, alpha=0.5, lda=268, ldb=140, ldc=140, tol="split"),
               G.gcase("group", 64, 256, 1000, 0, 0, split=4, compute=1, scale=1, alpha=0.5, lda=68, ldb=260, ldc=260, tol="split")]
    lib = hip.load()
    assert hip.DEFER is None
    vals = [gemm_values(c) for c in members]

    def framed(c, v):
        t = {}
        for name, (shape, dtype, lead, pitch, is_out) in G.operands(c).items():
            if is_out:
                t[name] = G.sentinel_framed(shape, dtype, lead, pitch, device=DEV)
                t[name][0].fill_(C0 if name == "C" else RS0)
            else:
                t[name] = G.nan_framed(v[name].to(dtype), lead, pitch, device=DEV)
        args = (c["M"], c["N"], c["K"], t["A"][0], c["lda"], 0, t["B"][0], c["ldb"], 0, t["C"][0], c["ldc"])
        kw = dict(alpha=c["alpha"], split_k=c["split"], compute=1, scale=t["scale"][0] if c["scale"] else None,
                  rowsum_a=t["rowsum_a"][0] if c["rowsum"] else None, rowsum_alpha=c["alpha"])
        return t, args, kw

    single = []
    need = []
    for c, v in zip(members, vals):
        t, args, kw = framed(c, v)
        d, _ = hip._gemm_desc(*args, workspace=big_ws, **kw)
        q = int(lib.detr_hip_workspace_bytes_gemm(ctypes.byref(d)))
        assert q >= G.split_floor_bytes(c)
        need.append((q + 255) & ~255)
        hip.gemm(*args, workspace=big_ws, **kw)
        single.append(t)
    assert len(set(need)) == 3
    ws, ws_buf = guarded_scratch(len(members) * max(need))
    grouped = [framed(c, v) for c, v in zip(members, vals)]
    old = hip.WORKSPACE
    try:
        hip.WORKSPACE = ws
        hip.gemm_group([(args, kw) for _, args, kw in grouped])
        torch.cuda.synchronize()
        assert hip.WORKSPACE is ws, "the wrapper replaced a workspace that held every member's share"
    finally:
        hip.WORKSPACE = old
    assert G.frame_intact(ws_buf, ws), "a member wrote outside the shared workspace"
    for c, v, (t, _, _), t1 in zip(members, vals, grouped, single):
        gemm_check(c, v, t, gemm_reference(c, v))
        assert torch.equal(bits_of(t["C"][0]), bits_of(t1["C"][0])), G.case_id(c)
        if c["rowsum"]:
            assert torch.equal(bits_of(t["rowsum_a"][0]), bits_of(t1["rowsum_a"][0]))


@pytest.mark.parametrize("compute", [0, 1])
def test_gemm_batched_attention_layout_in_packed_buffers(hip, compute):
    """The layout of test_gemm_batched_attention_layout at B * H = 4, T = 37, S = 21: q / k / v are column blocks of packed
    [rows, 3 * D] buffers whose other blocks hold NaN, the scores are written at pitch Sp = 24 into a sentinel buffer, the
    probabilities are read at that pitch from a NaN-padded one, and the output is a column block of a packed sentinel buffer."""
    torch.manual_seed(4 + compute)
    Bn, H, T, S, hd, Sp = 2, 2, 37, 21, 32, 24
    D = H * hd
    q_ = G.bf if compute else (lambda t: t)
    q, k, v = q_(torch.randn(Bn, T, D)), q_(torch.randn(Bn, S, D)), q_(torch.randn(Bn, S, D))
    lib = hip.load()

    def block(t, which):
        """t as column block `which` of a packed [B, L, 3 D] buffer inside a NaN frame: (view, buffer)."""
        L = t.shape[1]
        packed = torch.full((Bn, L, 3 * D), float("nan"))
        packed[:, :, which * D:(which + 1) * D] = t
        view, buf = G.nan_framed(packed, 16, None, device=DEV)
        return view[:, :, which * D:(which + 1) * D], buf

    def launch(*args, **kw):
        d, _ = hip._gemm_desc(*args, compute=compute, **kw)
        assert lib.detr_hip_gemm_family(ctypes.byref(d)) == 0
        hip._check(lib.detr_hip_gemm_f32(ctypes.byref(d), hip._stream()), "detr_hip_gemm_f32")
        torch.cuda.synchronize()

    (qd, qb), (kd, kb), (vd, vb) = block(q, 1), block(k, 0), block(v, 2)
    sc, sc_buf = G.sentinel_framed((Bn * H, T, S), F32, 16, Sp, device=DEV)
    elem = lambda view, buf: (view.data_ptr() - buf.data_ptr()) // 4
    launch(T, S, hd, qb, 3 * D, 1, kb, 3 * D, 1, sc_buf, Sp, a_off=elem(qd, qb), b_off=elem(kd, kb), c_off=16, batch=Bn * H, batch_inner=H,
           sA=(T * 3 * D, hd), sB=(S * 3 * D, hd), sC=(H * T * Sp, T * Sp))
    ref = torch.einsum("bthd,bshd->bhts", q.view(Bn, T, H, hd).double(), k.view(Bn, S, H, hd).double()).reshape(Bn * H, T, S)
    check_close(sc, ref, "f32", "batched QK^T")
    assert G.frame_intact(sc_buf, sc), "batched QK^T wrote into the padding columns of the scores"
    p = q_(torch.softmax(ref, -1).float())
    pd, pb = G.nan_framed(p, 16, Sp, device=DEV)
    packed_o, o_buf = G.sentinel_framed((Bn, T, 3 * D), F32, 16, None, device=DEV)
    o = packed_o[:, :, D:2 * D]
    launch(T, hd, S, pb, Sp, 1, vb, 3 * D, 0, o_buf, 3 * D, a_off=16, b_off=elem(vd, vb), c_off=elem(o, o_buf), batch=Bn * H, batch_inner=H,
           sA=(H * T * Sp, T * Sp), sB=(S * 3 * D, hd), sC=(T * 3 * D, hd))
    oref = torch.einsum("bhts,bshd->bthd", p.double().view(Bn, H, T, S), v.view(Bn, S, H, hd).double()).reshape(Bn, T, D)
    check_close(o, oref, "f32", "batched PV")
    assert G.frame_intact(o_buf, o), "batched PV wrote outside its column block"


# ------------------------------------------------------------------------------------------------------------------------
# 3x3 convolution: forward and input gradient
# ------------------------------------------------------------------------------------------------------------------------
def image_rows(t, rows=3):
    """Elements of `rows` whole image rows of an [N, H, W, C] tensor: the lead and the tail of the conv operands, so that a halo row
    above image 0 or below image N - 1 is NaN if it is read."""
    return rows * t.shape[2] * t.shape[3]


def conv_in(t, dtype, zero_pad=False):
    if dtype == U8:
        n = (image_rows(t) + 15) // 16 * 16
        return G.bits_framed(t, n, None, tail=n, device=DEV, fill=0x00 if zero_pad else 0xFF)
    n = image_rows(t)
    view, buf = G.nan_framed(t.to(dtype), n, None, tail=n, device=DEV)
    if zero_pad:
        zero_the_frame(buf)
    return view, buf


def conv_out(shape, dtype):
    n = (3 * shape[2] * shape[3] + 15) // 16 * 16
    return G.sentinel_framed(shape, dtype, n, None, tail=n, device=DEV)


def vec_in(t, zero_pad=False):
    view, buf = G.nan_framed(t, 16, None, device=DEV)
    if zero_pad:
        zero_the_frame(buf)
    return view, buf


def pack_pixels(on):
    """[N, H, W, C] bool -> [N, H, W, C / 8] uint8."""
    N, H, W, C = on.shape
    return G.pack_bits(on.reshape(N * H * W, C)).reshape(N, H, W, C // 8)


ALPHA = 0.75


@pytest.mark.parametrize("shape", G.CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", G.conv_cases(), ids=lambda c: c["id"])
def test_conv3x3_forward_and_input_gradient_inside_frames(hip, c, shape):
    """Forward and input gradient of every 3x3 route on framed tensors.  rich cases: y = relu((z * scale + shift) * alpha + residual),
    dx = alpha * mask(dx); the others (the halo-staged kernels' epilogues): y = relu(z + shift), dx = mask(dx)."""
    N, H, W = shape
    Ci, Co, stride, dil, s16, rich, bits = c["Ci"], c["Co"], c["stride"], c["dil"], c["s16"], c["rich"], c["bits"]
    P = conv_problem(N, H, W, Ci, Co, stride, dil, c["compute"] == 1)
    Ho, Wo = P["Ho"], P["Wo"]
    dt = B16 if s16 else F32
    tol = "b16conv" if s16 else "f32"
    alpha = ALPHA if rich else 1.0
    y_ref = torch.relu((P["z"] * (P["scale"].double() if rich else 1.0) + P["shift"].double()) * alpha + (P["res"].double() if rich else 0.0))
    dx_ref = torch.where(P["msk"] > 0, P["dx"] * alpha, torch.zeros_like(P["dx"]))
    msk = pack_pixels(P["msk"] > 0) if bits else P["msk"]
    outs = []
    with G.tuning(hip, c["env"]):
        for zero_pad in (False, True):
            x, w, dy = conv_in(P["x"], dt, zero_pad), conv_in(P["w"], dt, zero_pad), conv_in(P["dy"], dt, zero_pad)
            res, mk = conv_in(P["res"], dt, zero_pad), conv_in(msk, U8 if bits else dt, zero_pad)
            scale, shift = vec_in(P["scale"], zero_pad), vec_in(P["shift"], zero_pad)
            y, dx = conv_out((N, Ho, Wo, Co), dt), conv_out((N, H, W, Ci), dt)
            yb = conv_out((N, Ho, Wo, Co // 8), U8) if bits else None
            kw = dict(scale=scale[0], residual=res[0], alpha=alpha) if rich else {}
            hip.conv3x3(0, x[0], w[0], y[0], N, H, W, Ci, Ho, Wo, Co, stride, pad=dil, bias=shift[0], act=1, compute=c["compute"], dilation=dil,
                        maskbits_out=yb[0] if bits else None, **kw)
            hip.conv3x3(1, dy[0], w[0], dx[0], N, H, W, Ci, Ho, Wo, Co, stride, pad=dil, alpha=alpha, mask=mk[0], compute=c["compute"], dilation=dil)
            torch.cuda.synchronize()
            outs.append((y, dx, yb))
    (y, dx, yb), (y0, dx0, yb0) = outs
    what = f"{c['id']} {shape}"
    check_close(y[0], y_ref, tol, what + " forward")
    check_close(dx[0], dx_ref, tol, what + " input gradient")
    assert G.frame_intact(y[1], y[0]) and G.frame_intact(dx[1], dx[0]), what + ": wrote outside y / dx"
    if bits:
        assert torch.equal(yb[0].cpu(), pack_pixels(y[0].float().cpu() > 0)) and G.frame_intact(yb[1], yb[0]), what + ": mask bits out"
        assert torch.equal(yb[0], yb0[0])
    assert torch.equal(bits_of(y[0]), bits_of(y0[0])) and torch.equal(bits_of(dx[0]), bits_of(dx0[0])), what + ": the result depends on the padding"


# ------------------------------------------------------------------------------------------------------------------------
# exactly sized scratch of the weight gradients
# ------------------------------------------------------------------------------------------------------------------------
def with_workspace(hip, ws, fn):
    """fn() with hip.WORKSPACE swapped for ws (as test_split_k_deterministic_workspace_path does); ws must still be the workspace after."""
    old = hip.WORKSPACE
    try:
        hip.WORKSPACE = ws
        fn()
        torch.cuda.synchronize()
        assert hip.WORKSPACE is ws, "the wrapper replaced a workspace of exactly the reported size: the launch asked for more"
    finally:
        hip.WORKSPACE = old


@pytest.mark.parametrize("c", G.wgrad_cases(), ids=lambda c: c["id"])
def test_conv3x3_weight_gradient_stays_inside_the_scratch_it_asks_for(hip, big_ws, c):
    """conv3x3 mode 2 at N = 2, 9 x 11 through a workspace of exactly detr_hip_workspace_bytes_conv3x3 / _dilated bytes and through a
    large one: same bits, 5e-5 of the fp64 weight gradient, the guard behind the scratch and the frame of dw intact."""
    N, H, W = 2, 9, 11
    Ci, Co, stride, dil, s16 = c["Ci"], c["Co"], c["stride"], c["dil"], c["s16"]
    P = conv_problem(N, H, W, Ci, Co, stride, dil, c["compute"] == 1)
    Ho, Wo = P["Ho"], P["Wo"]
    dt = B16 if s16 else F32
    lib = hip.load()
    with G.tuning(hip, c["env"]):
        d = hip.Conv3x3DDesc() if dil == 2 else hip.Conv3x3Desc()
        d.N, d.Hi, d.Wi, d.Ci, d.Ho, d.Wo, d.Co, d.stride, d.pad, d.split, d.compute = N, H, W, Ci, Ho, Wo, Co, stride, dil, c["split"], c["compute"]
        d.x_dtype = d.w_dtype = int(s16)
        if dil == 2:
            d.dilation = 2
        query = int(getattr(lib, "detr_hip_workspace_bytes_conv3x3_dilated" if dil == 2 else "detr_hip_workspace_bytes_conv3x3")(ctypes.byref(d), 2))
        assert query > 0, "the case does not split: no scratch to guard"
        ws, ws_buf = guarded_scratch(query)
        outs = []
        for scratch in (ws, big_ws):
            x, dy, scale = conv_in(P["x"], dt), conv_in(P["dy"], dt), vec_in(P["scale"])
            dw, dw_buf = G.sentinel_framed((3, 3, Ci, Co), F32, 64, None, device=DEV)
            dw.fill_(0.0)
            with_workspace(hip, scratch, lambda: hip.conv3x3(2, x[0], dy[0], dw, N, H, W, Ci, Ho, Wo, Co, stride, pad=dil, scale=scale[0], split=c["split"],
                                                             compute=c["compute"], dilation=dil))
            check_close(dw, P["dw"] * P["scale"].double(), "split", c["id"])
            assert G.frame_intact(dw_buf, dw), c["id"] + ": wrote outside dw"
            outs.append(dw)
    assert G.frame_intact(ws_buf, ws), f"{c['id']}: wrote past the {query} bytes of scratch the library asks for"
    assert not bool((ws == G.SENT).all()), "the scratch was not used"
    assert torch.equal(outs[0], outs[1]), c["id"] + ": the result depends on the scratch size"


STEM_WGRAD = [("f32", {}, 0, F32, "split"), ("bf16c", {}, 1, F32, "split"), ("rows16", {}, 1, B16, "stem16"),
              ("gather16", {"DETR_HIP_STEM_ROWS": 2}, 1, B16, "stem16")]


def stem_image(img, zero_pad=False):
    n = (3 * img.shape[2] * 3 + 3) // 4 * 4            # three image rows, 16-byte aligned
    view, buf = G.nan_framed(img, n, None, tail=n, device=DEV)
    if zero_pad:
        zero_the_frame(buf)
    return view, buf


@pytest.mark.parametrize("shape", G.STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name,env,compute,dy_dtype,tol", STEM_WGRAD, ids=[s[0] for s in STEM_WGRAD])
def test_stem_weight_gradient_stays_inside_the_scratch_it_asks_for(hip, big_ws, shape, name, env, compute, dy_dtype, tol):
    """stem_conv mode 2 (split 7) through a workspace of exactly detr_hip_workspace_bytes_stem bytes and through a large one."""
    N, H, W = shape
    P = stem_problem(N, H, W, compute == 1)
    Ho, Wo = P["Ho"], P["Wo"]
    lib = hip.load()
    with G.tuning(hip, env):
        d = hip.StemDesc()
        d.N, d.H, d.W, d.Ho, d.Wo, d.split, d.compute, d.w_dtype = N, H, W, Ho, Wo, 7, compute, int(dy_dtype == B16)
        query = int(lib.detr_hip_workspace_bytes_stem(ctypes.byref(d), 2))
        outs = []
        ws, ws_buf = guarded_scratch(query) if query > 0 else (None, None)
        for scratch in ((ws, big_ws) if query > 0 else (big_ws,)):
            img, dy, scale = stem_image(P["img"]), conv_in(P["dy"], dy_dtype), vec_in(P["scale"])
            dw, dw_buf = G.sentinel_framed((147, 64), F32, 64, None, device=DEV)
            dw.fill_(0.0)
            with_workspace(hip, scratch, lambda: hip.stem_conv(2, img[0], dy[0], dw, N, H, W, Ho, Wo, scale=scale[0], split=7, compute=compute))
            check_close(dw, P["dw"] * P["scale"].double(), tol, f"stem wgrad {name} {shape}")
            assert G.frame_intact(dw_buf, dw), "wrote outside dw"
            outs.append(dw)
    if query > 0:                       # (a map of 20 pixels does not split on 32-row K tiles: the launch accumulates onto dw, no scratch)
        assert G.frame_intact(ws_buf, ws), f"stem wgrad {name}: wrote past the {query} bytes of scratch the library asks for"
        assert not bool((ws == G.SENT).all()), "the scratch was not used"
        assert torch.equal(outs[0], outs[1]), "the result depends on the scratch size"


STEM_FWD = [("f32", {}, 0, F32, "f32", True), ("rows16", {}, 1, B16, "b16conv", False), ("gather16", {"DETR_HIP_STEM_ROWS": 2}, 1, B16, "b16conv", False)]


@pytest.mark.parametrize("shape", G.STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name,env,compute,y_dtype,tol,use_scale", STEM_FWD, ids=[s[0] for s in STEM_FWD])
def test_stem_forward_inside_frames(hip, shape, name, env, compute, y_dtype, tol, use_scale):
    """Stem forward, implicit-GEMM (fp32) and row-staged / gathering (bf16 output), on a NaN-framed image."""
    N, H, W = shape
    P = stem_problem(N, H, W, compute == 1)
    Ho, Wo = P["Ho"], P["Wo"]
    ref = torch.relu(P["z"] * (P["scale"].double() if use_scale else 1.0) + P["shift"].double())
    outs = []
    with G.tuning(hip, env):
        for zero_pad in (False, True):
            img, shift, scale = stem_image(P["img"], zero_pad), vec_in(P["shift"], zero_pad), vec_in(P["scale"], zero_pad)
            w, w_buf = G.nan_framed(P["w"].reshape(147, 64), 64, None, device=DEV)
            if zero_pad:
                zero_the_frame(w_buf)
            y, y_buf = conv_out((N, Ho, Wo, 64), y_dtype)
            hip.stem_conv(0, img[0], w, y, N, H, W, Ho, Wo, scale=scale[0] if use_scale else None, bias=shift[0], act=1, compute=compute)
            torch.cuda.synchronize()
            assert G.frame_intact(y_buf, y), f"stem forward {name}: wrote outside y"
            outs.append(y)
    check_close(outs[0], ref, tol, f"stem forward {name} {shape}")
    assert torch.equal(bits_of(outs[0]), bits_of(outs[1])), "the result depends on the padding"


@pytest.mark.parametrize("M", [31, 33, 4100])
def test_conv1x1_backward_fused_inside_frames_and_exact_scratch(hip, big_ws, M):
    """conv1x1_bwd_fused with scratch of exactly conv1x1_bwd_fused_scratch_floats(M) in front of a guard, dy / a / w at pitch + 8 inside
    NaN frames, da and dw inside sentinel frames: one bf16 rounding for da, the bound of test_conv1x1_backward_fused_reads_dy_once for dw,
    and the same bits as with a large scratch."""
    gen = torch.Generator().manual_seed(M)
    d1, d2, pad = 64, 256, 8
    dy, a, w = (G.bf(torch.randn(*s, generator=gen)) for s in ((M, d2), (M, d1), (d1, d2)))
    scale, dw0 = torch.rand(d2, generator=gen) + 0.5, torch.randn(d1, d2, generator=gen)
    n = hip.conv1x1_bwd_fused_scratch_floats(M)
    ws, ws_buf = guarded_scratch(n * 4)
    outs = []
    for scratch in (ws, big_ws):
        dyd, ad, wd = (G.nan_framed(t.to(B16), 32, t.shape[1] + pad, device=DEV)[0] for t in (dy, a, w))
        sc = vec_in(scale)[0]
        da, da_buf = G.sentinel_framed((M, d1), B16, 32, d1 + pad, device=DEV)
        dw, dw_buf = G.sentinel_framed((d1, d2), F32, 16, d2 + pad, device=DEV)
        dw.copy_(dw0)
        hip.conv1x1_bwd_fused(dyd, ad, wd, da, dw, scratch, scale=sc, use_mask=True, alpha=0.5)
        torch.cuda.synchronize()
        assert G.frame_intact(da_buf, da) and G.frame_intact(dw_buf, dw), "wrote outside da / dw"
        outs.append((da, dw))
    assert G.frame_intact(ws_buf, ws), f"wrote past the {n} floats of scratch the library asks for"
    da_ref = torch.where(a > 0, dy.double() @ w.double().t(), torch.zeros(M, d1, dtype=torch.float64))
    check_close(outs[0][0], da_ref, "b16", "fused 1x1 backward: da")
    dw_got = outs[0][1].cpu().double()
    assert bool(torch.isfinite(dw_got).all())
    want = dw0.double() + 0.5 * scale.double()[None, :] * (a.double().t() @ dy.double())
    assert float((dw_got - want).abs().max()) <= 2e-6 * float((a.double().abs().t() @ dy.double().abs()).max()) + 1e-6
    assert torch.equal(bits_of(outs[0][0]), bits_of(outs[1][0])) and torch.equal(bits_of(outs[0][1]), bits_of(outs[1][1])), "depends on the scratch size"
