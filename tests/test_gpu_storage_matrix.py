"""The matrix kernels on every accepted mix of fp32 and bf16 storage.  The GEMM, 3x3 convolution and stem kernels share one epilogue
(csrc/gemm_core.h) in which the storage of the output, of the residual and of the mask are three independent switches, reached
through three alignment classes (8 columns per lane, 4 columns, per element); the operands have their own switches.  The cases of
tests/guard_band_cases.py (storage_cases, conv_storage_cases, STEM_STORAGE) run the whole product inside NaN and sentinel frames and
assert what tests/test_gpu_guard_bands.py asserts per launch -- family, finite output, the fp64 reference on the stored values at
the family's own tolerance, intact frames, NaN padding against zero padding -- and then the storage identity, which needs no
tolerance: operands, residual and mask hold bf16-representable values, so every launch of a group computes the same fp32 epilogue
values; all fp32 outputs hold the same bits whatever the storage and pitch of residual and mask, and every bf16 output is those bits
rounded once (include/detr_hip.h: "the epilogue arithmetic stays fp32 and the result is rounded once").
tests/test_storage_matrix_cpu.py shows that the cases cover every form the library accepts."""
import ctypes

import pytest
import torch

import guard_band_cases as G
from matrix_refs import check_close, conv_problem, gemm_reference, gemm_values, stem_problem
from test_gpu_guard_bands import (ALPHA, B16, DEV, F32, _reset_library_tuning, bits_of, conv_in, conv_out, gemm_check, gemm_launch,  # noqa: F401
                                  stem_image, vec_in, zero_the_frame)

pytestmark = pytest.mark.gpu


def assert_storage_identity(outs, what):
    """outs: [(name, is the output bf16?, output tensor)] of one group.  Every fp32 output holds the bits of the first one, every bf16
    output those bits rounded once."""
    c32 = next((o for _, is16, o in outs if not is16), None)
    assert c32 is not None, what + ": no fp32 output in the group"
    want32, want16 = bits_of(c32), bits_of(c32.to(B16))
    for name, is16, o in outs:
        got = bits_of(o)
        want = want16 if is16 else want32
        assert torch.equal(got, want), (f"{what}: {name} differs from {'bf16(C32)' if is16 else 'the first fp32 output'} in "
                                        f"{int((got != want).sum())} of {got.numel()} elements")


# ------------------------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------------------------
def storage_values(c):
    """gemm_values with the bit-packed mask packed from the bf16 mask of the same shape."""
    v = gemm_values(c)
    if c["mask"] == "bits":
        v["mask"] = G.pack_bits(gemm_values(dict(c, mask="b16"))["mask"] > 0)
    return v


GROUPS = {}
for _c in G.storage_cases():
    GROUPS.setdefault(G.storage_group(_c), []).append(_c)


@pytest.mark.parametrize("key", list(GROUPS), ids=G.storage_group_id)
def test_gemm_storage_matrix(hip, key):
    """One shape, one epilogue content, one A / B storage: every storage of C, residual and mask on every pitch class."""
    cases = GROUPS[key]
    first = next(c for c in cases if c["mask"] != "bits")
    ref = gemm_reference(first, gemm_values(first))
    outs = {}
    with G.tuning(hip, cases[0]["env"]):
        for c in cases:
            v = storage_values(c)
            t, _ = gemm_launch(hip, c, v)
            t0, _ = gemm_launch(hip, c, v, zero_pad=True)
            gemm_check(c, v, t, ref)
            assert torch.equal(bits_of(t["C"][0]), bits_of(t0["C"][0])), f"{G.case_id(c)}: C depends on what the padding holds"
            outs[c["tag"]] = (G.case_id(c), bool(c["c16"]), t["C"][0].clone())
    assert_storage_identity(list(outs.values()), G.storage_group_id(key))
    for tag, (name, _, o) in outs.items():
        if "-mbits-" in tag:
            assert torch.equal(bits_of(o), bits_of(outs[tag.replace("-mbits-", "-mb16-")][2])), f"{name}: differs from the bf16 mask it was packed from"


def _framed(c, v):
    t = {}
    for name, (shape, dtype, lead, pitch, is_out) in G.operands(c).items():
        t[name] = G.sentinel_framed(shape, dtype, lead, pitch, device=DEV) if is_out else G.nan_framed(v[name].to(dtype), lead, pitch, device=DEV)
    args = (c["M"], c["N"], c["K"], t["A"][0], c["lda"], c["ak"], t["B"][0], c["ldb"], c["bk"], t["C"][0], c["ldc"])
    kw = dict(alpha=c["alpha"], act=c["act"], compute=c["compute"], scale=t["scale"][0] if c["scale"] else None, bias=t["bias"][0] if c["bias"] else None,
              residual=t["residual"][0] if c["res"] else None, ldr=c["ldr"], mask=t["mask"][0] if c["mask"] else None, ldmask=c["ldm"])
    return t, args, kw


def test_gemm_group_members_of_different_epilogue_storage(hip):
    """Four members of one kernel variant (K-contiguous bf16 A and B, 64 x 64 tiles) whose C / residual / mask storage and pitch class
    differ -- the 8-column form, the 4-column form with its column tail, the per-element form on odd pitches and on a shifted base --
    through one grouped launch: each member equals its own single launch bit for bit."""
    by_tag = {(c["M"], c["bk"], c["tag"]): c for c in G.storage_cases() if c["group"] == "store"}
    main, tail = G.STORE_MAIN[0], G.STORE_TAIL[0]
    members = [by_tag[(main, 1, "rich-a1b1c1-rb16-mb16-wide")], by_tag[(main, 1, "rich-a1b1c0-rb16-mf32-odd")],
               by_tag[(tail, 1, "rich-a1b1c1-rf32-mNone-vec4")], by_tag[(main, 1, "rich-a1b1c1-rNone-mf32-Coff")]]
    assert len({(c["c16"], c["res"], c["mask"]) for c in members}) == 4
    lib = hip.load()
    with G.tuning(hip, G.STORE_ENV):
        single, grouped = [], []
        for c in members:
            v = storage_values(c)
            t, args, kw = _framed(c, v)
            d, _ = hip._gemm_desc(*args, **kw)
            assert lib.detr_hip_gemm_family(ctypes.byref(d)) == 0
            hip.gemm(*args, **kw)
            single.append(t)
            grouped.append(_framed(c, v))
        hip.gemm_group([(args, kw) for _, args, kw in grouped])
        torch.cuda.synchronize()
    for c, (t, _, _), t1 in zip(members, grouped, single):
        v = storage_values(c)
        gemm_check(c, v, t, gemm_reference(c, v))
        assert torch.equal(bits_of(t["C"][0]), bits_of(t1["C"][0])), f"{G.case_id(c)}: the grouped launch differs from the single one"


# ------------------------------------------------------------------------------------------------------------------------
# 3x3 convolution
# ------------------------------------------------------------------------------------------------------------------------
DT = {0: F32, 1: B16, None: None, "f32": F32, "b16": B16}


class ConvRun:
    """One convolution problem on framed tensors: inputs are framed once per (tensor, storage, padding) and shared by the launches."""

    def __init__(self, hip, c):
        self.hip, (self.N, self.H, self.W) = hip, c["shape"]
        self.Ci, self.Co, self.stride, self.dil = c["Ci"], c["Co"], c["stride"], c["dil"]
        self.P = conv_problem(self.N, self.H, self.W, self.Ci, self.Co, self.stride, self.dil, True)
        self.cache = {}

    def tensor(self, name, dtype, zero_pad):
        key = (name, dtype, zero_pad)
        if key not in self.cache:
            self.cache[key] = (vec_in(self.P[name], zero_pad) if name in ("scale", "shift") else conv_in(self.P[name], dtype, zero_pad))[0]
        return self.cache[key]

    def reference(self, mode, aux, rich):
        P, alpha = self.P, (ALPHA if rich else 1.0)
        if mode == 0:
            return torch.relu((P["z"] * (P["scale"].double() if rich else 1.0) + P["shift"].double()) * alpha + (P["res"].double() if aux else 0.0))
        return torch.where(P["msk"] > 0, P["dx"] * alpha, torch.zeros_like(P["dx"])) if aux else P["dx"] * alpha

    def launch(self, c, zero_pad, rich=True):
        """(destination view, its buffer) of one launch of the case."""
        hip, P = self.hip, self.P
        N, H, W, Ci, Co, Ho, Wo = self.N, self.H, self.W, self.Ci, self.Co, P["Ho"], P["Wo"]
        src16, w16, dst16 = c["s16"]
        w = self.tensor("w", DT[w16], zero_pad)
        aux = self.tensor("res" if c["mode"] == 0 else "msk", DT[c["aux"]], zero_pad) if c["aux"] else None
        if c["mode"] == 0:
            y = conv_out((N, Ho, Wo, Co), DT[dst16])
            kw = dict(scale=self.tensor("scale", F32, zero_pad), alpha=ALPHA) if rich else {}
            hip.conv3x3(0, self.tensor("x", DT[src16], zero_pad), w, y[0], N, H, W, Ci, Ho, Wo, Co, self.stride, pad=self.dil,
                        bias=self.tensor("shift", F32, zero_pad), act=1, compute=1, dilation=self.dil, residual=aux, **kw)
        else:
            y = conv_out((N, H, W, Ci), DT[dst16])
            hip.conv3x3(1, self.tensor("dy", DT[src16], zero_pad), w, y[0], N, H, W, Ci, Ho, Wo, Co, self.stride, pad=self.dil,
                        alpha=ALPHA if rich else 1.0, mask=aux, compute=1, dilation=self.dil)
        torch.cuda.synchronize()
        return y


def conv_name(c):
    return f"{c['id']} mode {c['mode']} s16 {c['s16']} aux {c['aux']}"


CONV_GROUPS = {}
for _c in G.conv_storage_cases():
    if not _c["halo"]:
        CONV_GROUPS.setdefault((_c["id"], _c["s16"][0], _c["s16"][1]), []).append(_c)


@pytest.mark.parametrize("key", list(CONV_GROUPS), ids=lambda k: f"{k[0]}-src{k[1]}-w{k[2]}")
def test_conv3x3_storage_matrix(hip, key):
    """One convolution, one storage of the source and of the kernel tensor: forward and input gradient on every storage of the
    destination and of the residual / the mask."""
    cases = CONV_GROUPS[key]
    run = ConvRun(hip, cases[0])
    groups = {}
    with G.tuning(hip, cases[0]["env"]):
        for c in cases:
            what = conv_name(c)
            y, y0 = run.launch(c, False), run.launch(c, True)
            check_close(y[0], run.reference(c["mode"], c["aux"], True), "b16conv", what)
            assert G.frame_intact(y[1], y[0]), what + ": wrote outside the destination"
            assert torch.equal(bits_of(y[0]), bits_of(y0[0])), what + ": the result depends on the padding"
            groups.setdefault(G.conv_storage_group(c), []).append((what, bool(c["s16"][2]), y[0]))
    for gkey, outs in groups.items():
        assert_storage_identity(outs, str(gkey))


HALO_CASES = [c for c in G.conv_storage_cases() if c["halo"]]


@pytest.mark.parametrize("c", HALO_CASES, ids=lambda c: f"mode{c['mode']}-{''.join(map(str, c['s16']))}-{c['aux']}")
def test_conv3x3_one_fp32_tensor_leaves_the_halo_kernels(hip, c):
    """A launch the halo-staged kernels would take if every tensor were bf16 (bias + ReLU / a plain or masked input gradient), with one
    tensor in fp32: the tile kernel serves it -- the same bits as with the halo kernels switched off."""
    run = ConvRun(hip, c)
    what = conv_name(c)
    with G.tuning(hip, c["env"]):
        y, y0 = run.launch(c, False, rich=False), run.launch(c, True, rich=False)
    with G.tuning(hip, {"DETR_HIP_CONV_HALO": 2}):
        yt = run.launch(c, False, rich=False)
    check_close(y[0], run.reference(c["mode"], c["aux"], False), "b16conv", what)
    assert G.frame_intact(y[1], y[0]), what + ": wrote outside the destination"
    assert torch.equal(bits_of(y[0]), bits_of(y0[0])), what + ": the result depends on the padding"
    assert torch.equal(bits_of(y[0]), bits_of(yt[0])), what + ": not the tile kernel's bits"


# ------------------------------------------------------------------------------------------------------------------------
# stem
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name,y16,alpha", G.STEM_STORAGE, ids=[s[0] for s in G.STEM_STORAGE])
def test_stem_forward_storage(hip, shape, name, y16, alpha):
    """Stem forward under bf16 compute with scale, shift, alpha and the ReLU: an fp32 output, and a bf16 output on the gathering
    kernel's own rounding path, which equals the fp32 output of the same launch rounded once."""
    N, H, W = shape
    P = stem_problem(N, H, W, True)
    Ho, Wo = P["Ho"], P["Wo"]
    ref = torch.relu((P["z"] * P["scale"].double() + P["shift"].double()) * alpha)

    def launch(dtype, zero_pad):
        img, shift, scale = stem_image(P["img"], zero_pad), vec_in(P["shift"], zero_pad), vec_in(P["scale"], zero_pad)
        w, w_buf = G.nan_framed(P["w"].reshape(147, 64), 64, None, device=DEV)
        if zero_pad:
            zero_the_frame(w_buf)
        y, y_buf = conv_out((N, Ho, Wo, 64), dtype)
        hip.stem_conv(0, img[0], w, y, N, H, W, Ho, Wo, scale=scale[0], bias=shift[0], alpha=alpha, act=1, compute=1)
        torch.cuda.synchronize()
        assert G.frame_intact(y_buf, y), f"stem forward {name}: wrote outside y"
        return y

    y, y0 = launch(B16 if y16 else F32, False), launch(B16 if y16 else F32, True)
    check_close(y, ref, "b16conv", f"stem forward {name} {shape}")
    assert torch.equal(bits_of(y), bits_of(y0)), "the result depends on the padding"
    if y16:
        assert_storage_identity([("y32", False, launch(F32, False)), ("y16", True, y)], f"stem forward {name} {shape}")


# ------------------------------------------------------------------------------------------------------------------------
# rejections: the convolution and stem entry points have no host-side probe
# ------------------------------------------------------------------------------------------------------------------------
# (field, value, compute, mode): values the header does not document, and bf16 storage outside bf16 compute
CONV_REJECT = ([("compute", 3, 3, 0)] + [(f, 2, 1, 0) for f in ("x_dtype", "y_dtype", "r_dtype", "w_dtype")] + [("m_dtype", 3, 1, 1)] +
               [(f, 1, compute, 0) for compute in (0, 2) for f in ("x_dtype", "y_dtype", "r_dtype", "w_dtype")] +
               [("m_dtype", v, compute, 1) for compute in (0, 2) for v in (1, 2)])


def all_sentinel(buf):
    return bool((buf == G.sentinel_of(buf.dtype)).all())


@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("field,value,compute,mode", CONV_REJECT, ids=[f"{f}{v}-c{c}-mode{m}" for f, v, c, m in CONV_REJECT])
def test_conv3x3_rejects_what_the_header_does_not_document(hip, dil, field, value, compute, mode):
    """Every buffer has the size of its fp32 interpretation and holds sentinels: were the descriptor accepted, the launch would stay
    inside its allocations and the test fail on the return code."""
    N, H, W, Ci, Co = 2, 9, 11, 64, 64
    lib = hip.load()
    x, w, y = conv_out((N, H, W, Ci), F32), conv_out((3, 3, Ci, Co), F32), conv_out((N, H, W, Co), F32)
    aux, vec = conv_out((N, H, W, Co), F32), G.sentinel_framed((Co,), F32, 16, None, device=DEV)
    d = hip.Conv3x3DDesc() if dil == 2 else hip.Conv3x3Desc()
    if dil == 2:
        d.dilation = 2
    d.N, d.Hi, d.Wi, d.Ci, d.Ho, d.Wo, d.Co, d.stride, d.pad = N, H, W, Ci, H, W, Co, 1, dil
    d.x, d.w, d.y = x[0].data_ptr(), w[0].data_ptr(), y[0].data_ptr()
    d.alpha, d.compute = 1.0, compute
    if mode == 0:
        d.bias, d.residual, d.act = vec[0].data_ptr(), aux[0].data_ptr(), 1
    else:
        d.mask = aux[0].data_ptr()
    setattr(d, field, value)
    rc = getattr(lib, "detr_hip_conv3x3_dilated" if dil == 2 else "detr_hip_conv3x3_f32")(ctypes.byref(d), mode, hip._stream())
    torch.cuda.synchronize()
    assert rc == -1, f"{field} = {value} under compute {compute} was accepted"
    assert lib.detr_hip_last_error().decode()
    assert all_sentinel(y[1]) and all_sentinel(x[1]) and all_sentinel(w[1]) and all_sentinel(aux[1])


STEM_REJECT = [("compute", 3, 3, 0), ("compute", 3, 3, 2), ("y_dtype", 2, 1, 0), ("w_dtype", 2, 1, 2), ("y_dtype", 1, 0, 0), ("y_dtype", 1, 2, 0),
               ("w_dtype", 1, 0, 2), ("w_dtype", 1, 2, 2)]


@pytest.mark.parametrize("field,value,compute,mode", STEM_REJECT, ids=[f"{f}{v}-c{c}-mode{m}" for f, v, c, m in STEM_REJECT])
def test_stem_rejects_what_the_header_does_not_document(hip, field, value, compute, mode):
    N, H, W = 1, 9, 8
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    lib = hip.load()
    img = G.sentinel_framed((N, H, W, 3), F32, 16, None, device=DEV)
    act, wt = conv_out((N, Ho, Wo, 64), F32), G.sentinel_framed((147, 64), F32, 64, None, device=DEV)      # y / dy, w / dw
    ws = G.sentinel_framed((1 << 20,), F32, 64, None, device=DEV)
    d = hip.StemDesc()
    d.N, d.H, d.W, d.Ho, d.Wo = N, H, W, Ho, Wo
    d.img = img[0].data_ptr()
    d.w, d.y = (wt[0].data_ptr(), act[0].data_ptr()) if mode == 0 else (act[0].data_ptr(), wt[0].data_ptr())
    d.alpha, d.compute, d.split = 1.0, compute, 1
    d.workspace, d.workspace_bytes = ws[0].data_ptr(), ws[0].numel() * 4
    setattr(d, field, value)
    rc = lib.detr_hip_stem_conv7x7_f32(ctypes.byref(d), mode, hip._stream())
    torch.cuda.synchronize()
    assert rc == -1, f"{field} = {value} under compute {compute} was accepted"
    assert lib.detr_hip_last_error().decode()
    assert all_sentinel(act[1]) and all_sentinel(wt[1]) and all_sentinel(ws[1])
