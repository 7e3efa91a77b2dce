"""Guard-band cases of the matrix kernels (GEMM families, 3x3 convolutions, stem, fused 1x1 backward): the case tables and the
framing helpers shared by tests/test_gpu_guard_bands.py (device) and tests/test_guard_bands_cpu.py (routes, helpers, and why
the zero-padded, tight-pitch method of the older tests cannot see the faults these cases look for).  The storage-matrix lists
(storage_cases, conv_storage_cases, STEM_STORAGE: every accepted mix of fp32 and bf16 tensors) serve tests/test_gpu_storage_matrix.py
and tests/test_storage_matrix_cpu.py through the same helpers.

Rule of every case: each INPUT the kernel takes a pointer to lies inside a NaN-filled buffer (a lead in front, pad columns behind
every row, a tail), each OUTPUT and scratch buffer inside a sentinel-filled one.  A read of padding that reaches the result shows
as NaN, a write outside the extent as a changed sentinel."""
import numpy as np
import torch

SENT = -8192.0            # the sentinel of tests/test_gpu_launch_edges.py: exact in bf16
SENT_U8 = 0xEE
LEAD = 64                 # bytes in front of an aligned operand (a multiple of 16)
TAIL = 96                 # elements behind the last row


def sentinel_of(dtype):
    return SENT_U8 if dtype == torch.uint8 else SENT


def _frame(shape, dtype, lead, pitch, tail, fill, device):
    shape = tuple(int(s) for s in shape)
    cols = shape[-1]
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    pitch = cols if pitch is None else int(pitch)
    assert pitch >= cols and lead >= 0 and tail >= 0
    buf = torch.full((lead + rows * pitch + tail,), fill, dtype=dtype, device=device)
    strides = [1] * len(shape)
    if len(shape) > 1:
        strides[-2] = pitch
        for i in range(len(shape) - 3, -1, -1):
            strides[i] = strides[i + 1] * shape[i + 1]
    return buf.as_strided(shape, strides, lead), buf


def nan_framed(t, lead, pitch=None, tail=TAIL, device=None):
    """(view, buffer): the values of the host tensor t (fp32 or bf16, 1-D .. N-D) at element offset `lead` of a NaN-filled buffer,
    rows of the last axis `pitch` elements apart (None: tight), `tail` elements behind the last row.  The buffer is built on the
    host and moved to `device` once."""
    assert t.dtype in (torch.float32, torch.bfloat16)
    view, buf = _frame(t.shape, t.dtype, lead, pitch, tail, float("nan"), "cpu")
    view.copy_(t)
    if device is not None and str(device) != "cpu":
        buf = buf.to(device)
        view = buf.as_strided(view.shape, view.stride(), lead)
    return view, buf


def sentinel_framed(shape, dtype, lead, pitch=None, tail=TAIL, device="cpu"):
    """(view, buffer) of an output or scratch tensor: every element, the view's included, holds the sentinel."""
    return _frame(shape, dtype, lead, pitch, tail, sentinel_of(dtype), device)


def frame_intact(buf, view):
    """True when every element of buf outside view still holds the sentinel: the lead, the pad columns of every row, the tail."""
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    inside.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(True)
    return bool((buf[~inside] == sentinel_of(buf.dtype)).all())


def bits_framed(t, lead, pitch=None, tail=TAIL, device=None, fill=0xFF):
    """nan_framed for a bit-packed (uint8) input: bytes have no NaN, the frame holds `fill` (0xFF: every mask bit set)."""
    view, buf = _frame(t.shape, torch.uint8, lead, pitch, tail, fill, "cpu")
    view.copy_(t)
    if device is not None and str(device) != "cpu":
        buf = buf.to(device)
        view = buf.as_strided(view.shape, view.stride(), lead)
    return view, buf


class tuning:
    """The given DETR_HIP_* variables (every other one of TUNING_VARS unset) for the time of a block; whatever the process had set
    comes back afterwards."""

    def __init__(self, _hip, env):
        import os
        self.hip, self.env, self.os = _hip, env, os

    def __enter__(self):
        self.saved = {k: self.os.environ.get(k) for k in TUNING_VARS}
        for k in TUNING_VARS:
            if self.saved[k] is not None or k in self.env:
                self.hip.set_tuning(k, self.env.get(k))

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is not None or k in self.env:
                self.hip.set_tuning(k, v)


def bf(t):
    """t rounded to bf16, as fp32."""
    return t.float().bfloat16().float()


def pack_bits(t):
    """[M, N] bool -> [M, N / 8] uint8, bit (n & 7) of byte n / 8 (detr_gemm_desc.maskbits_out)."""
    M, N = t.shape
    w = (2 ** torch.arange(8, dtype=torch.int32)).view(1, 1, 8)
    return (t.reshape(M, N // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def unpack_bits(b, N):
    M = b.shape[0]
    return ((b.to(torch.int32).unsqueeze(-1) >> torch.arange(8, dtype=torch.int32)) & 1).reshape(M, -1)[:, :N].bool()


# ------------------------------------------------------------------------------------------------------------------------
# GEMM cases
# ------------------------------------------------------------------------------------------------------------------------
F32, B16, U8 = torch.float32, torch.bfloat16, torch.uint8
TUNING_VARS = ("DETR_HIP_GEMM_TILE", "DETR_HIP_GEMM_RING", "DETR_HIP_GEMM_STREAM", "DETR_HIP_GEMM_K64", "DETR_HIP_EPI_WIDE", "DETR_HIP_STREAM_NW",
               "DETR_HIP_RING_NS", "DETR_HIP_RING_BN", "DETR_HIP_RING_ROWS", "DETR_HIP_SPLIT3_ALL", "DETR_HIP_SLAB_TS", "DETR_HIP_CONV_TILE",
               "DETR_HIP_WGRAD_TILE", "DETR_HIP_X3_T192", "DETR_HIP_CONV_HALO", "DETR_HIP_CONV_DMA", "DETR_HIP_DGRAD_S2_CLASSES", "DETR_HIP_WGRAD_FUSED",
               "DETR_HIP_STEM_ROWS", "DETR_HIP_SPLIT3_T128")


def gcase(group, M, N, K, ak=1, bk=1, *, family=0, env=None, compute=0, a16=0, b16=0, c16=0, res=None, mask=None, bits_out=0, bias=0,
          scale=0, alpha=1.0, act=0, p=0.0, lda=None, ldb=None, ldc=None, ldr=None, ldm=None, off=None, tol="f32", split=1, rowsum=0,
          ln=None, tag=""):
    """One GEMM case.  res / mask: None, "f32", "b16" (mask also "bits").  off: {operand: elements of extra lead} (misaligned
    bases).  tol: "f32" 2e-5 of the output scale, "split" 5e-5, "b16" one bf16 rounding, "ring32" / "ring16" 2^-16 / 2^-7 of the scale.
    ln: None or dict(add=bool, y16=bool)."""
    ea, eb = (K if ak else M), (K if bk else N)
    c = dict(group=group, M=M, N=N, K=K, ak=ak, bk=bk, family=family, env=dict(env or {}), compute=compute, a16=a16, b16=b16, c16=c16,
             res=res, mask=mask, bits_out=bits_out, bias=bias, scale=scale, alpha=alpha, act=act, p=p,
             lda=ea if lda is None else lda, ldb=eb if ldb is None else ldb, ldc=N if ldc is None else ldc,
             ldr=N if ldr is None else ldr, ldm=(((N + 7) // 8 if mask == "bits" else N) if ldm is None else ldm),
             ldbits=(N + 7) // 8 + 3, off=dict(off or {}), tol=tol, split=split, rowsum=rowsum, ln=ln, tag=tag)
    return c


def case_id(c):
    env = ",".join(f"{k[9:]}={v}" for k, v in sorted(c["env"].items()))
    return f"{c['group']}-{c['M']}x{c['N']}x{c['K']}-ak{c['ak']}bk{c['bk']}-c{c['compute']}{'-' + c['tag'] if c['tag'] else ''}{'-' + env if env else ''}"


def operands(c):
    """{name: (shape, dtype, lead elements, pitch, is_output)} of every tensor the launch takes a pointer to (workspace excepted)."""
    M, N, K = c["M"], c["N"], c["K"]
    dt = lambda is16: B16 if is16 else F32
    sd = dict(f32=F32, b16=B16, bits=U8)
    ops = {}

    def put(name, shape, dtype, pitch, out=False):
        lead = LEAD // torch.empty((), dtype=dtype).element_size() + c["off"].get(name, 0)
        ops[name] = (shape, dtype, lead, pitch, out)

    put("A", (M, K) if c["ak"] else (K, M), dt(c["a16"]), c["lda"])
    put("B", (N, K) if c["bk"] else (K, N), dt(c["b16"]), c["ldb"])
    put("C", (M, N), dt(c["c16"]), c["ldc"], True)
    if c["res"]:
        put("residual", (M, N), sd[c["res"]], c["ldr"])
    if c["mask"]:
        put("mask", (M, (N + 7) // 8) if c["mask"] == "bits" else (M, N), sd[c["mask"]], c["ldm"])
    if c["bits_out"]:
        put("maskbits_out", (M, (N + 7) // 8), U8, c["ldbits"], True)
    if c["bias"]:
        put("bias", (N,), F32, None)
    if c["scale"]:
        put("scale", (N,), F32, None)
    if c["rowsum"]:
        put("rowsum_a", (M,), F32, None, True)
    if c["ln"] is not None:
        put("ln_gamma", (N,), F32, None)
        put("ln_beta", (N,), F32, None)
        put("ln_y", (M, N), F32, None, True)
        put("ln_mean", (M,), F32, None, True)
        put("ln_rstd", (M,), F32, None, True)
        if c["ln"]["add"]:
            put("ln_add", (c["ln"]["add_rows"], N), F32, None)
            put("ln_y2", (M, N), F32, None, True)
        if c["ln"]["y16"]:
            put("ln_y16", (M, N), B16, None, True)
    return ops


def fill_desc(_hip, c, ptrs, dropout_step=None, workspace=None, workspace_bytes=0):
    """The detr_gemm_desc of a case on the operand addresses `ptrs` (real ones on the device, placeholders of the same alignment
    on the CPU: the routing is host arithmetic on the descriptor)."""
    d = _hip.GemmDesc()
    d.M, d.N, d.K = c["M"], c["N"], c["K"]
    d.A, d.lda, d.a_kcontig, d.a_dtype = ptrs["A"], c["lda"], c["ak"], c["a16"]
    d.B, d.ldb, d.b_kcontig, d.b_dtype = ptrs["B"], c["ldb"], c["bk"], c["b16"]
    d.C, d.ldc, d.c_dtype = ptrs["C"], c["ldc"], c["c16"]
    d.batch = d.batch_inner = 1
    d.alpha, d.act, d.split_k, d.compute = c["alpha"], c["act"], c["split"], c["compute"]
    d.scale, d.bias = ptrs.get("scale"), ptrs.get("bias")
    if c["res"]:
        d.residual, d.ldr, d.r_dtype = ptrs["residual"], c["ldr"], int(c["res"] == "b16")
    if c["mask"]:
        d.mask, d.ldmask, d.m_dtype = ptrs["mask"], c["ldm"], dict(f32=0, b16=1, bits=2)[c["mask"]]
    if c["bits_out"]:
        d.maskbits_out, d.ld_maskbits_out = ptrs["maskbits_out"], c["ldbits"]
    if c["p"] > 0.0:
        d.dropout_p, d.dropout_seed, d.dropout_step = c["p"], DROP_SITE, dropout_step
    if c["rowsum"]:
        d.rowsum_a, d.rowsum_alpha = ptrs["rowsum_a"], c["alpha"]
    if c["ln"] is not None:
        d.ln_gamma, d.ln_beta, d.ln_y, d.ln_mean, d.ln_rstd, d.ln_eps = (ptrs["ln_gamma"], ptrs["ln_beta"], ptrs["ln_y"], ptrs["ln_mean"],
                                                                         ptrs["ln_rstd"], LN_EPS)
        if c["ln"]["add"]:
            d.ln_add, d.ln_add_rows, d.ln_y2 = ptrs["ln_add"], c["ln"]["add_rows"], ptrs["ln_y2"]
        if c["ln"]["y16"]:
            d.ln_y16 = ptrs["ln_y16"]
    d.workspace, d.workspace_bytes = workspace, workspace_bytes
    return d


DROP_SITE, DROP_STEP, LN_EPS = 0xABCDE, 0x1234567, 1e-5


def placeholder_ptrs(c):
    """Made-up addresses with the alignment the case states (never dereferenced)."""
    out = {}
    for i, (name, (shape, dtype, lead, pitch, is_out)) in enumerate(operands(c).items()):
        out[name] = 0x10000000 * (i + 1) + lead * torch.empty((), dtype=dtype).element_size()
    return out


def split_floor_bytes(c):
    """The documented floor of the split-K scratch: row-major slabs."""
    return c["split"] * (c["M"] * c["N"] + (c["M"] if c["rowsum"] else 0)) * 4


LAYOUTS = ((1, 1), (1, 0), (0, 1), (0, 0))
up4 = lambda n: (n + 3) // 4 * 4
odd = lambda n: n + 4 if n % 2 else n + 5


def _fp32_operand_cases(group, compute, env, family=0):
    """The two fp32-storage groups of the tile engine: vector loads (132, 72, 40) and scalar loads (77, 40, 33)."""
    out = []
    for ak, bk in LAYOUTS:
        M, N, K = 132, 72, 40
        ea, eb = (K if ak else M), (K if bk else N)
        out.append(gcase(group, M, N, K, ak, bk, family=family, env=env, compute=compute, lda=ea + 4, ldb=eb + 4, ldc=N + 4, tag="vec"))
        M, N, K = 77, 40, 33
        ea, eb = (K if ak else M), (K if bk else N)
        out.append(gcase(group, M, N, K, ak, bk, family=family, env=env, compute=compute, lda=odd(ea), ldb=odd(eb), ldc=odd(N), tag="odd"))
        for name in ("A", "B"):          # aligned pitches, the base one float off: the !aligned16 branch of a_vec / b_vec
            for M, N, K in ((77, 40, 33), (132, 72, 40)):
                ea, eb = (K if ak else M), (K if bk else N)
                out.append(gcase(group, M, N, K, ak, bk, family=family, env=env, compute=compute, lda=up4(ea) + 4, ldb=up4(eb) + 4, ldc=N + 4,
                                 off={name: 1}, tag=f"{name}off"))
    return out


def _tile_envs(extra=None):
    return [dict(extra or {}, **({"DETR_HIP_GEMM_TILE": t} if t else {})) for t in (None, 1, 2, 3)]


def gemm_cases():
    out = []
    # fp32 tile engine, vector and scalar loads, every forced tile
    for env in _tile_envs():
        out += _fp32_operand_cases("f32tile", 0, env)
    # bf16 compute (1) and f32x3 (2) on fp32 storage: the same operands
    for env in _tile_envs():
        out += _fp32_operand_cases("bf16c", 1, env)
    for env in _tile_envs({"DETR_HIP_SPLIT3_ALL": 1}):
        out += _fp32_operand_cases("f32x3", 2, env)
    # scalar epilogue with epilogue work, and the vector epilogue on the same operands
    M, N, K = 77, 50, 33
    variants = {"ldc53": dict(ldc=53), "Coff": dict(off={"C": 1}), "ldr51": dict(ldr=51), "ldm55": dict(ldm=55), "biasoff": dict(off={"bias": 1}),
                "aligned": {}}
    for compute in (0, 1):
        for name, v in variants.items():
            kw = dict(lda=37, ldb=37, ldc=52, ldr=52, ldm=56)
            kw.update(v)
            for act in (0, 1, 2):
                out.append(gcase("epi", M, N, K, compute=compute, scale=1, alpha=0.75, bias=1, res="f32", mask="f32", act=act, tag=f"{name}-act{act}", **kw))
            kw.pop("ldm")
            out.append(gcase("epi", M, N, K, compute=compute, bias=1, res="f32", p=0.1, tag=f"{name}-drop", **kw))
    # bf16 storage on the tile engine
    for M, N, K in ((200, 136, 72), (75, 264, 96)):
        for bk in (1, 0):
            for k64 in (None, 1):
                for wide in (None, 2):
                    env = {"DETR_HIP_GEMM_RING": 2, "DETR_HIP_GEMM_STREAM": 2}
                    if k64:
                        env["DETR_HIP_GEMM_K64"] = k64
                    if wide:
                        env["DETR_HIP_EPI_WIDE"] = wide
                    kw = dict(env=env, compute=1, a16=1, b16=1, c16=1, lda=K + 8, ldb=(K if bk else N) + 8, tol="b16")
                    out.append(gcase("b16tile", M, N, K, 1, bk, bias=1, res="b16", mask="b16", act=1, ldc=N + 8, ldr=N + 16, ldm=N + 24, tag="wide", **kw))
                    out.append(gcase("b16tile", M, N, K, 1, bk, bias=1, res="b16", mask="b16", act=1, ldc=N + 4, ldr=N + 16, ldm=N + 24, tag="narrow", **kw))
                    out.append(gcase("b16tile", M, N, K, 1, bk, bias=1, res="b16", mask="bits", act=1, bits_out=1, ldc=N + 8, ldr=N + 16, ldm=N // 8 + 3,
                                     tag="bits", **kw))
                    out.append(gcase("b16tile", M, N, K, 1, bk, bias=1, res="b16", p=0.1, ldc=N + 8, ldr=N + 16, tag="drop", **kw))
    # streaming kernel
    for M, N, K in ((16384 + 37, 64, 64), (16384 + 37, 256, 128), (16384 + 37, 128, 256)):
        two = (K == 256 and N % 128 == 0) or (K == 128 and N % 256 == 0)
        for nw in ((1, 0) if two else (1,)):
            for bk in (1, 0):
                env = {"DETR_HIP_GEMM_STREAM": 3, "DETR_HIP_STREAM_NW": nw}
                kw = dict(family=1, env=env, compute=1, a16=1, b16=1, c16=1, lda=K + 8, ldb=(K if bk else N) + 8, ldc=N + 8, ldr=N + 16, tol="b16")
                out.append(gcase("stream", M, N, K, 1, bk, bias=1, res="b16", act=1, bits_out=int(not bk), tag="res_relu" + ("_bits" if not bk else ""), **kw))
                out.append(gcase("stream", M, N, K, 1, bk, res="b16", mask="bits", ldm=N // 8 + 3, tag="res_maskbits", **kw))
                out.append(gcase("stream", M, N, K, 1, bk, bias=1, mask="b16", ldm=N + 24, tag="mask16", **kw))
    for nw in (1, 0):
        for bk in (1, 0):
            M, N, K = 4096 + 5, 1024, 256
            env = {"DETR_HIP_GEMM_STREAM": 3, "DETR_HIP_STREAM_NW": nw}
            out.append(gcase("stream", M, N, K, 1, bk, family=1, env=env, compute=1, a16=1, b16=1, c16=1, lda=K + 8, ldb=(K if bk else N) + 8, ldc=N + 8,
                             bias=1, alpha=0.5, p=0.25, act=1, tol="b16", tag="ext"))
    # ring, bf16 operands
    for M, N, K in ((33, 256, 192), (8, 136, 128), (600, 256, 128)):
        for bk in (1, 0):
            for vname, venv in (("auto", {}), ("ns2", {"DETR_HIP_RING_NS": 2}), ("bn128", {"DETR_HIP_RING_BN": 128})):
                env = dict({"DETR_HIP_GEMM_RING": 1, "DETR_HIP_GEMM_STREAM": 2}, **venv)
                for f32 in (0, 1):
                    kw = dict(family=2, env=env, compute=1, a16=1, b16=1, c16=1 - f32, lda=K + 8, ldb=(K if bk else N) + 8, ldc=N + 8, ldr=N + 8,
                              tol="ring32" if f32 else "ring16")
                    out.append(gcase("ring", M, N, K, 1, bk, bias=1, res="f32" if f32 else "b16", act=1, tag=f"{vname}-{'f32' if f32 else 'b16'}", **kw))
    out.append(gcase("ring", 600, 256, 128, 1, 1, family=2, env={"DETR_HIP_GEMM_RING": 1, "DETR_HIP_GEMM_STREAM": 2}, compute=1, a16=1, b16=1, c16=1,
                     lda=136, ldb=136, ldc=264, ldr=264, res="b16", p=0.1, tol="ring16", tag="drop"))
    # ring, fp32
    for M, N, K in ((600, 256, 128), (33, 136, 96)):
        for bk in (1, 0):
            for rows in (None, 96):
                env = {"DETR_HIP_GEMM_RING": 1}
                if rows:
                    env["DETR_HIP_RING_ROWS"] = rows
                kw = dict(family=3, env=env, lda=K + 4, ldb=(K if bk else N) + 4, ldc=N + 4, ldr=N + 4, ldm=N + 8)
                out.append(gcase("ring32", M, N, K, 1, bk, res="f32", mask="f32", tag="res_mask", **kw))
                out.append(gcase("ring32", M, N, K, 1, bk, bias=1, act=1, tag="bias_relu", **kw))
    # GEMM + LayerNorm
    for M in (37, 800):
        for K in (256, 72):
            for a16 in (0, 1):
                for full in (0, 1):
                    out.append(gcase("ln", M, 256, K, 1, 1, family=4, compute=1, a16=a16, b16=1, lda=K + 8, ldb=K + 8, bias=1,
                                     res="f32" if full else None, ldr=260, p=0.1 if full else 0.0,
                                     ln=dict(add=bool(full), y16=bool(full), add_rows=100 if M % 100 == 0 else M),
                                     tag=("a16" if a16 else "a32") + ("-full" if full else "-plain")))
    return out


def split_cases():
    """Split-K cases of the exact-scratch runs: weight-gradient layout (both operands reduction-major)."""
    out = [gcase("split", 147, 64, 3000, 0, 0, split=7, scale=1, alpha=0.5, lda=147 + 13, tol="split", tag="f32")]
    for M, N, K, s in ((136, 72, 8 * 331, 5), (264, 136, 2100, 3)):
        for rowsum in (0, 1):
            out.append(gcase("split", M, N, K, 0, 0, split=s, compute=1, scale=1, alpha=0.5, rowsum=rowsum, lda=M + 4, ldb=N + 4, tol="split",
                             tag="bf16c" + ("-rowsum" if rowsum else "")))
    out.append(gcase("split", 100, 92, 2048, 0, 0, split=5, rowsum=1, scale=1, alpha=0.5, tol="split", tag="f32-rowsum"))
    # the ring weight gradient (family 5): bf16-stored MN-contiguous operands
    for M, N, K, s, env in RING_WGRAD_SHAPES:
        out.append(gcase("split", M, N, K, 0, 0, family=5, env=env, split=s, compute=1, a16=1, b16=1, alpha=0.75, lda=M + 8, ldb=N + 8, ldc=N + 4,
                         tol="split", tag="ringwgrad"))
    return out


# (the kernel runs on 128 x 128 tiles: the tile rule picks them from 512 x 512 x 4096 on, DETR_HIP_GEMM_TILE=1 forces them on small outputs)
RING_WGRAD_SHAPES = [(264, 136, 2100, 3, {"DETR_HIP_GEMM_TILE": 1}), (120, 128, 1000, 4, {"DETR_HIP_GEMM_TILE": 1}), (512, 512, 4096 + 8, 4, {})]


# ------------------------------------------------------------------------------------------------------------------------
# storage matrix: every accepted mix of fp32 and bf16 A / B / C / residual / mask (tests/test_gpu_storage_matrix.py,
# tests/test_storage_matrix_cpu.py)
# ------------------------------------------------------------------------------------------------------------------------
STORE_ENV = {"DETR_HIP_GEMM_TILE": 3, "DETR_HIP_GEMM_RING": 2, "DETR_HIP_GEMM_STREAM": 2}
STORE_MAIN, STORE_TAIL = (75, 136, 96), (77, 50, 40)
RES_STORES, MASK_STORES = (None, "f32", "b16"), (None, "f32", "b16", "bits")
PITCH_CLASSES = ("wide", "vec4", "odd", "Coff", "Roff")
up8 = lambda n: (n + 7) // 8 * 8


def storage_pitches(N, cls, mask=None):
    """ldc / ldr / ldm / off of a pitch class: three pairwise different pitches.  wide: all % 8 == 0; vec4: % 4 == 0 but not % 8;
    odd: odd; Coff / Roff: the wide pitches with the base of C / the residual one element off.  A bit-packed mask has its own
    pitch in bytes."""
    n8 = up8(N)
    ldc, ldr, ldm = {"vec4": (n8 + 4, n8 + 12, n8 + 20), "odd": (n8 + 5, n8 + 7, n8 + 9)}.get(cls, (n8 + 8, n8 + 16, n8 + 24))
    if mask == "bits":
        ldm = (N + 7) // 8 + 3
    return dict(ldc=ldc, ldr=ldr, ldm=ldm, off={"Coff": {"C": 1}, "Roff": {"residual": 1}}.get(cls, {}))


def storage_key(c):
    """The storage form of a GEMM case: what the completeness probe of tests/test_storage_matrix_cpu.py enumerates."""
    return (c["compute"], c["a16"], c["b16"], c["c16"], c["res"], c["mask"])


def storage_group(c):
    """Cases with the same key compute the same fp32 epilogue values from the same A / B through the same kernel: their fp32 outputs
    hold the same bits, their bf16 outputs those bits rounded once."""
    return (c["group"], c["M"], c["N"], c["K"], c["ak"], c["bk"], c["compute"], c["a16"], c["b16"], c["res"] is not None, c["mask"] is not None,
            c["act"], c["p"] > 0.0, tuple(sorted(c["env"].items())))


def storage_group_id(key):
    group, M, N, K, ak, bk, compute, a16, b16, res, mask, act, drop, env = key
    return f"{group}-{M}x{N}x{K}-bk{bk}-c{compute}-a{a16}b{b16}-{'res' if res else 'nores'}-{'mask' if mask else 'nomask'}-act{act}{'-drop' if drop else ''}"


def _content(name, res, mask):
    if name == "rich":
        return dict(scale=1, bias=1, alpha=0.75, act=1, res=res, mask=mask)
    return dict(bias=1, res=res, p=0.1)


def bits_accepted(c16, res, cls, N):
    """Where the library takes a bit-packed mask: the all-bf16 8-column epilogue."""
    return bool(c16) and res in (None, "b16") and cls == "wide" and N % 8 == 0


def storage_cases():
    out = []
    # tile engine (family 0), bf16 compute on one pinned tile: the full product of storage forms on every pitch class
    shapes = [(STORE_MAIN, 1), (STORE_MAIN, 0), (STORE_TAIL, 1)]
    for (M, N, K), bk in shapes:
        for a16 in (0, 1):
            for b16 in (0, 1):
                kw = dict(env=STORE_ENV, compute=1, a16=a16, b16=b16, lda=K + 8, ldb=(K if bk else N) + 8)
                for c16 in (0, 1):
                    for res in RES_STORES:
                        for cls in PITCH_CLASSES:
                            if cls == "Roff" and res is None:
                                continue
                            for mask in MASK_STORES:
                                if mask == "bits" and not bits_accepted(c16, res, cls, N):
                                    continue
                                tag = f"a{a16}b{b16}c{c16}-r{res}-m{mask}-{cls}"
                                out.append(gcase("store", M, N, K, 1, bk, c16=c16, tol="b16" if c16 else "f32", tag="rich-" + tag,
                                                 **_content("rich", res, mask), **storage_pitches(N, cls, mask), **kw))
                                if mask is None and res is not None:
                                    out.append(gcase("store", M, N, K, 1, bk, c16=c16, tol="b16" if c16 else "f32", tag="drop-" + tag,
                                                     **_content("drop", res, None), **storage_pitches(N, cls), **kw))
    # the sigmoid in front of a bf16 C (and its fp32 twin)
    M, N, K = STORE_MAIN
    for c16 in (0, 1):
        out.append(gcase("store", M, N, K, 1, 1, env=STORE_ENV, compute=1, a16=1, b16=1, c16=c16, bias=1, res="f32", act=2, lda=K + 8, ldb=K + 8,
                         tol="b16" if c16 else "f32", tag=f"act2-c{c16}", **storage_pitches(N, "vec4")))
    # fp32 storage under exact fp32 and f32x3: the forms those modes accept
    for compute, env in ((0, STORE_ENV), (2, dict(STORE_ENV, DETR_HIP_SPLIT3_ALL=1))):
        for res in (None, "f32"):
            for mask in (None, "f32"):
                for cls in ("vec4", "odd"):
                    out.append(gcase("store32", M, N, K, 1, 1, env=env, compute=compute, lda=K + 4, ldb=K + 4, tag=f"r{res}-m{mask}-{cls}",
                                     **_content("rich", res, mask), **storage_pitches(N, cls)))
    # ring (family 2)
    M, N, K = 33, 256, 192
    env = {"DETR_HIP_GEMM_RING": 1, "DETR_HIP_GEMM_STREAM": 2}
    for c16 in (0, 1):
        for res in RES_STORES:
            for cls in ("wide", "vec4"):
                for mask in MASK_STORES:
                    if mask == "bits" and not bits_accepted(c16, res, cls, N):
                        continue
                    out.append(gcase("storering", M, N, K, 1, 1, family=2, env=env, compute=1, a16=1, b16=1, c16=c16, lda=K + 8, ldb=K + 8,
                                     tol="ring16" if c16 else "ring32", tag=f"c{c16}-r{res}-m{mask}-{cls}", **_content("rich", res, mask),
                                     **storage_pitches(N, cls, mask)))
    # streaming shapes the streaming kernel cannot serve because one tensor is fp32: the tile engine takes them
    for M, N, K in ((16384 + 37, 64, 64), (16384 + 37, 256, 128)):
        for name, c16, res, mask in (("res32", 1, "f32", "b16"), ("mask32", 1, "b16", "f32"), ("c32", 0, "b16", "b16")):
            out.append(gcase("storefall", M, N, K, 1, 1, family=0, env={"DETR_HIP_GEMM_STREAM": 3}, compute=1, a16=1, b16=1, c16=c16, bias=1, res=res,
                             mask=mask, act=1, lda=K + 8, ldb=K + 8, tol="b16" if c16 else "f32", tag=name, **storage_pitches(N, "wide")))
    return out


def storage_probe_case(compute, a16, b16, c16, res, mask):
    """The main shape on all-aligned placements in one storage form, for the completeness probe."""
    M, N, K = STORE_MAIN
    return gcase("probe", M, N, K, 1, 1, env=STORE_ENV, compute=compute, a16=a16, b16=b16, c16=c16, lda=K + 8, ldb=K + 8,
                 **_content("rich", res, mask), **storage_pitches(N, "wide", mask))


# ------------------------------------------------------------------------------------------------------------------------
# 3x3 convolution and stem cases
# ------------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = ((2, 9, 11), (2, 5, 33), (3, 2, 3))


def conv_cases():
    """Forward / input-gradient cases; each runs on every shape of CONV_SHAPES.  s16: all tensors stored in bf16.  rich: the epilogue
    carries scale, alpha and a residual (the tile kernels; the halo-staged kernels have bias / ReLU / mask only and would hand such a
    launch to the tile kernel).  bits: the ReLU mask goes in (and comes out) bit-packed."""
    out = []

    def add(name, env, compute, s16, ci, co, stride=1, dil=1, bits=0, rich=1):
        out.append(dict(id=f"{name}-{ci}x{co}-s{stride}", env=env, compute=compute, s16=s16, Ci=ci, Co=co, stride=stride, dil=dil, bits=bits, rich=rich))

    for tile in (None, 1):                                    # fp32 tile kernel, 64 x 64 and 128 x 128 tiles
        env = {"DETR_HIP_CONV_TILE": tile} if tile else {}
        for ci, co in ((16, 32), (64, 64), (128, 256)):
            for stride in (1, 2):
                add(f"f32tile{tile or 0}", env, 0, 0, ci, co, stride)
    for tile in (3, 1):                                       # bf16 tile kernel on 64 / 128 tiles (the epilogue keeps it off the halo kernels)
        for ci, co in ((64, 64), (128, 128), (192, 192), (128, 256)):
            for stride in (1, 2):
                add(f"b16tile{tile}", {"DETR_HIP_CONV_TILE": tile, "DETR_HIP_DGRAD_S2_CLASSES": 3}, 1, 1, ci, co, stride, bits=int(ci == 128 and co == 128))
    for mode in (1, 3):                                       # f32x3 forms (128-row tiles from one tile on)
        env = {"DETR_HIP_SPLIT3_ALL": 1, "DETR_HIP_SPLIT3_T128": 1, "DETR_HIP_X3_T192": mode}
        for ci, co in ((64, 64), (128, 128), (192, 192), (128, 256)):
            add(f"x3t{mode}", env, 2, 0, ci, co, 1)
        add(f"x3t{mode}", env, 2, 0, 128, 128, 2)
    for rows in (3, 4):                                       # halo-staged kernel, 64- and 128-channel tiles
        for ci, co in ((64, 64), (128, 128), (192, 192), (128, 256)):
            add(f"halo{rows}", {"DETR_HIP_CONV_HALO": rows, "DETR_HIP_CONV_DMA": 2}, 1, 1, ci, co, 1, bits=int(ci == co == 128), rich=0)
    for dma in (None, 2):                                     # LDS-DMA halo kernel and its off switch
        for ci, co in ((128, 128), (128, 256)):
            add("dma" if dma is None else "dmaoff", {} if dma is None else {"DETR_HIP_CONV_DMA": dma}, 1, 1, ci, co, 1, rich=0)
    for ci, co in ((64, 64), (128, 128), (192, 192), (128, 256)):      # stride-2 input gradient: class form on the halo kernel
        add("s2halo", {}, 1, 1, ci, co, 2, bits=int(ci == co == 128), rich=0)
    for compute, s16, rich in ((0, 0, 1), (1, 1, 0), (1, 1, 1)):      # dilation 2: tile bodies, halo planes
        for ci, co in ((64, 64), (192, 192), (128, 256)):
            add("dil2-" + ("b16" if s16 else "f32") + ("" if rich else "-halo"), {}, compute, s16, ci, co, 1, dil=2, rich=rich)
    return out


def wgrad_cases():
    """3x3 weight gradients through an exactly sized workspace: (id, env, compute, storage bf16?, Ci, Co, stride, dilation, split)."""
    out = []
    add = lambda name, env, compute, s16, ci, co, stride, split, dil=1: out.append(
        dict(id=f"{name}-{ci}x{co}-s{stride}-k{split}", env=env, compute=compute, s16=s16, Ci=ci, Co=co, stride=stride, dil=dil, split=split))
    for ci, co in ((64, 64), (128, 128), (192, 64)):
        for split, ts in ((5, None), (7, None), (7, 2)):
            env = {"DETR_HIP_SLAB_TS": ts} if ts else {}
            add("f32" + ("-rm" if ts else ""), env, 0, 0, ci, co, 1, split)
            add("fused16" + ("-rm" if ts else ""), env, 1, 1, ci, co, 1, split)
    add("pertap16", {}, 1, 0, 128, 128, 2, 5)           # bf16 compute on fp32 tensors at stride 2: the per-tap kernel, 128 and 64 tiles
    add("pertap16", {}, 1, 0, 64, 64, 2, 7)
    add("fused16s2", {"DETR_HIP_WGRAD_FUSED": 4}, 1, 1, 64, 64, 2, 5)
    add("fused16s2", {"DETR_HIP_WGRAD_FUSED": 4}, 1, 1, 128, 128, 2, 7)
    add("x3", {"DETR_HIP_SPLIT3_ALL": 1}, 2, 0, 128, 128, 1, 5)
    add("x3", {"DETR_HIP_SPLIT3_ALL": 1}, 2, 0, 64, 64, 2, 7)
    add("dil2", {}, 0, 0, 64, 64, 1, 5, dil=2)
    add("dil2-16", {}, 1, 1, 128, 128, 1, 7, dil=2)
    return out


STEM_SHAPES = ((2, 37, 53), (1, 9, 8))
# stem forward under bf16 compute: (id, y stored in bf16?, alpha); both carry scale, shift and the ReLU, so the bf16 output stays on the
# gathering kernel's own c16 path without DETR_HIP_STEM_ROWS
STEM_STORAGE = (("c1-y32", 0, 1.0), ("c1-y16-rich", 1, 0.75))


def conv_storage_cases():
    """Mixed fp32 / bf16 storage on the bf16 tile kernel, one dict per launch.  mode 0: y = relu((conv(x, w) * scale + shift) * 0.75 + residual),
    mode 1: dx = 0.75 * mask(conv^T(dy, w)); s16 = (source, kernel, destination) stored in bf16?, aux = storage of the residual (mode 0) / the mask
    (mode 1).  halo: the launch is one fp32 tensor away from the halo-staged kernels (bias + ReLU / plain input gradient)."""
    out = []
    env = {"DETR_HIP_CONV_TILE": 3, "DETR_HIP_DGRAD_S2_CLASSES": 3}

    def product(name, env, ci, co, stride, dil, shape):
        for mode in (0, 1):
            for src in (0, 1):
                for w in (0, 1):
                    for dst in (0, 1):
                        for aux in (None, "f32", "b16"):
                            out.append(dict(id=f"{name}-{ci}x{co}-s{stride}-{'x'.join(map(str, shape))}", env=env, Ci=ci, Co=co, stride=stride, dil=dil,
                                            shape=shape, mode=mode, s16=(src, w, dst), aux=aux, halo=0))

    for shape in (CONV_SHAPES[0], CONV_SHAPES[2]):
        for ci, co in ((64, 64), (128, 256)):
            for stride in (1, 2):
                product("tile", env, ci, co, stride, 1, shape)
    product("dil2", env, 128, 256, 1, 2, CONV_SHAPES[0])
    for mode in (0, 1):
        for which in range(3):
            s16 = tuple(int(i != which) for i in range(3))
            out.append(dict(id="halo-128x128-s1-2x9x11", env={}, Ci=128, Co=128, stride=1, dil=1, shape=CONV_SHAPES[0], mode=mode, s16=s16,
                            aux=None, halo=1))
    out.append(dict(id="halo-128x128-s1-2x9x11", env={}, Ci=128, Co=128, stride=1, dil=1, shape=CONV_SHAPES[0], mode=1, s16=(1, 1, 1), aux="f32", halo=1))
    return out


def conv_storage_group(c):
    """Launches that share source and kernel storage (and everything but the storage of destination, residual and mask)."""
    return (c["id"], c["mode"], c["s16"][0], c["s16"][1], c["aux"] is not None)


# ------------------------------------------------------------------------------------------------------------------------
# NumPy models of the two faults the zero-padded, tight-pitch tests cannot see
# ------------------------------------------------------------------------------------------------------------------------
def model_gemm(A, lda, B, ldb, M, N, K, wide_k_tail=False):
    """C = A B on flat k-contiguous operands (A [M, lda], B [N, ldb]) the way a tile loop does it: K in steps of 4 with a guard per
    element.  wide_k_tail: the guard is `k < ld` where `k < K` belongs."""
    a, b = np.asarray(A, dtype=np.float64).reshape(M, lda), np.asarray(B, dtype=np.float64).reshape(N, ldb)
    C = np.zeros((M, N))
    for k0 in range(0, (K + 3) // 4 * 4, 4):
        for k in range(k0, k0 + 4):
            if k < (min(lda, ldb) if wide_k_tail else K):
                C += np.outer(a[:, k], b[:, k])
    return C


def model_dropout_epilogue(acc, ldc, p, key, by_pitch=False):
    """drop(acc) of an [M, N] accumulator stored at pitch ldc; the element index of the keyed mask is row * N + col (by_pitch: the
    fault, row * ldc + col)."""
    from oracle import dropout_ref as DR
    M, N = acc.shape
    idx = np.arange(M)[:, None] * (ldc if by_pitch else N) + np.arange(N)[None, :]
    keep = DR.keep_mask(key, idx, p)
    return np.where(keep, acc / (1.0 - p), 0.0)
