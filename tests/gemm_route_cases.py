"""GEMM descriptors whose routing the library must keep: the case list behind tests/golden/gemm_routes.json (written by
scripts/record_gemm_routes.py, replayed by tests/test_gemm_routing_cpu.py).

For every case, under every tuning environment of ENVS, the fixture holds what detr_hip_gemm_family answers (the kernel family, or the
rejection) and, for split-K cases, what detr_hip_workspace_bytes_gemm asks for.  Both are host arithmetic on the descriptor: the
pointers below are made-up addresses that are never dereferenced, so the list runs without a GPU.

The list is a handful of plain nested loops; each block keeps every STRIDE-th member of its cross product (the strides are coprime
to the loop lengths, so every value of every loop survives)."""
import ctypes
import os

MS = (64, 100, 800, 8400, 33600, 133600, 534400)
NS = (32, 64, 92, 128, 256, 512, 1024, 2048)
KS = (64, 128, 256, 512, 1024, 2048, 8400, 33600)
LAYOUTS = ((1, 1), (1, 0), (0, 1), (0, 0))                      # (a_kcontig, b_kcontig)

# (compute, storage).  storage: "f32" everything fp32; "ab16" bf16 A and B, fp32 C; "all16" bf16 A, B, C, residual and mask;
# "bits" as all16 with a bit-packed mask in and mask bits out
PRECISIONS = ((0, "f32"), (2, "f32"), (1, "f32"), (1, "ab16"), (1, "all16"), (1, "bits"))

# tuning environments: "" is the default tuning; the others set ONE variable (DETR_HIP_<name>=<value>)
ENVS = ([("", None)] + [("GEMM_TILE", v) for v in (1, 2, 3, 4, 5, 6)] + [("GEMM_RING", v) for v in (1, 2, 3)] +
        [("GEMM_STREAM", v) for v in (2, 3)] + [("SLAB_TS", 2)] + [("RING_WTILE", v) for v in (1, 2)] + [("SPLIT3_ALL", 1)] +
        [("X3_T192", v) for v in (1, 2)] + [("GEMM_K64", v) for v in (1, 2)] + [("GEMM_GROUP", 2), ("RING_ROWS", 96)])
ENV_VARS = sorted({"DETR_HIP_" + k for k, _ in ENVS if k})


def env_name(env):
    return "default" if not env[0] else f"{env[0]}={env[1]}"


# made-up device addresses, 16-byte aligned and far apart
A_, B_, C_, SCALE_, BIAS_, RES_, MASK_, ROWSUM_, BITS_, WS_ = (0x10000000 * (i + 1) for i in range(10))
LN_ = 0xB0000000


def case(M, N, K, ak, bk, compute, storage, **kw):
    c = dict(M=M, N=N, K=K, ak=ak, bk=bk, compute=compute, storage=storage, split_k=1, rowsum=0, ws=0, off_a=0, off_c=0, scale=0,
             batch=1, ln=0, res_sub=None, alpha=1.0, dropout=0.0, act=0, bias=0, residual=0, mask=0)
    c.update(kw)
    return c


def cases():
    out = []
    # 1. unsplit: every shape x precision x layout
    i = 0
    for compute, storage in PRECISIONS:
        for ak, bk in LAYOUTS:
            for M in MS:
                for N in NS:
                    for K in KS:
                        i += 1
                        if i % 13 == 0:
                            out.append(case(M, N, K, ak, bk, compute, storage, residual=storage in ("all16", "bits"), mask=storage in ("all16", "bits")))
    # 2. split-K (the weight gradients: short outputs, long K) x fused bias gradient x workspace tier
    #    ws: 0 none, 1 exactly split_k * M * N * 4 bytes, 2 what detr_hip_workspace_bytes_gemm reports
    i = 0
    for compute, storage in PRECISIONS[:4]:
        for ak, bk in LAYOUTS:
            for split_k in (8, 64):
                for rowsum in (0, 1):
                    for ws in (0, 1, 2):
                        for M in MS[:4]:
                            for N in NS:
                                for K in KS[3:]:
                                    i += 1
                                    if i % 83 == 0:
                                        out.append(case(M, N, K, ak, bk, compute, storage, split_k=split_k, rowsum=rowsum, ws=ws))
    # 2b. the ring weight gradient's own corner: MN-contiguous bf16 operands, outputs from 64 x 32 to 8400 x 2048
    for split_k, ws in ((8, 1), (8, 2), (64, 2)):
        for M in (64, 800, 8400):
            for N in NS:
                for K in (2048, 33600):
                    out.append(case(M, N, K, 0, 0, 1, "ab16", split_k=split_k, ws=ws))
    # 3. alignment of A, C and scale; batch
    shapes = ((8400, 256, 256), (33600, 64, 64), (33600, 1024, 256), (800, 256, 2048), (100, 92, 64), (64, 32, 128), (133600, 128, 512), (800, 2048, 8400))
    i = 0
    for compute, storage in PRECISIONS[:4]:
        for ak, bk in LAYOUTS:
            for off_a in (0, 4):
                for off_c in (0, 4):
                    for scale in (0, 1, 2):             # none, aligned, 4-byte offset
                        for batch in (1, 8):
                            for split_k in (1, 8):
                                for M, N, K in shapes:
                                    i += 1
                                    if i % 29 == 0:
                                        out.append(case(M, N, K, ak, bk, compute, storage, off_a=off_a, off_c=off_c, scale=scale, batch=batch,
                                                        split_k=split_k, ws=2 if split_k > 1 else 0))
    # 4. epilogue extras on the shapes the streaming and ring kernels compete for
    shapes = ((33600, 64, 64), (133600, 128, 128), (33600, 256, 256), (8400, 2048, 256), (33600, 1024, 256), (8400, 256, 2048), (33600, 512, 1024),
              (800, 256, 2048), (8400, 92, 512), (534400, 64, 64))
    i = 0
    for compute, storage in ((0, "f32"), (1, "ab16"), (1, "all16"), (1, "bits")):
        for bk in (1, 0):
            for alpha in (1.0, 1.0 / 0.9):
                for dropout in (0.0, 0.1):
                    for act in (0, 1, 2):
                        for bias in (0, 1):
                            for residual in (0, 1):
                                for mask in (0, 1):
                                    for M, N, K in shapes:
                                        i += 1
                                        if i % 23 == 0:
                                            out.append(case(M, N, K, 1, bk, compute, storage, alpha=alpha, dropout=dropout, act=act, bias=bias,
                                                            residual=residual, mask=mask))
    # 5. fused LayerNorm (ln_y): the accepted form and its neighbours
    for storage in ("ab16", "all16"):
        for ak, bk in LAYOUTS[:2]:
            for M in (100, 800, 8400):
                for N in (256, 512):
                    for K in (64, 256, 2048):
                        for split_k in ((1, 8) if K == 256 else (1,)):
                            out.append(case(M, N, K, ak, bk, 1, storage, ln=1, bias=1, residual=storage != "ab16", split_k=split_k))
    out.append(case(800, 256, 256, 1, 1, 0, "f32", ln=1))
    # 6. residual row map: M whole h x w maps, the compact residual of their even pixels
    for storage in ("all16", "bits", "ab16"):
        for bk in (1, 0):
            for M, h, w in ((100, 10, 10), (800, 20, 20), (8400, 50, 84), (33600, 100, 168), (8400, 50, 85)):
                for N in (64, 256, 1024):
                    for K in (64, 256, 1024):
                        out.append(case(M, N, K, 1, bk, 1, storage, res_sub=(h, w), residual=1, mask=storage != "ab16"))
    out.append(case(8400, 256, 256, 1, 1, 1, "all16", res_sub=(50, 84), residual=1, ln=1))
    return out


def describe(c):
    """One line that names a case in a failure message."""
    dflt = case(0, 0, 0, 0, 0, 0, "")
    extra = " ".join(f"{k}={c[k]}" for k in sorted(c) if k not in ("M", "N", "K", "ak", "bk", "compute", "storage") and c[k] != dflt[k])
    return f"M{c['M']} N{c['N']} K{c['K']} ak{c['ak']} bk{c['bk']} compute={c['compute']} {c['storage']} {extra}".rstrip()


def fill(_hip, lib, c):
    """The GemmDesc of a case (and whatever it points to that must outlive the call)."""
    d = _hip.GemmDesc()
    M, N, K = c["M"], c["N"], c["K"]
    st = c["storage"]
    d.M, d.N, d.K = M, N, K
    d.A, d.lda, d.a_kcontig = A_ + c["off_a"], (K if c["ak"] else M), c["ak"]
    d.B, d.ldb, d.b_kcontig = B_, (K if c["bk"] else N), c["bk"]
    d.C, d.ldc = C_ + c["off_c"], N
    d.batch, d.batch_inner = c["batch"], 1
    if c["batch"] > 1:
        d.sA0, d.sB0, d.sC0 = M * K, K * N, M * N
    d.alpha = c["alpha"]
    d.compute = c["compute"]
    d.a_dtype = d.b_dtype = int(st != "f32")
    d.c_dtype = int(st in ("all16", "bits"))
    if c["scale"]:
        d.scale = SCALE_ + (4 if c["scale"] == 2 else 0)
    if c["bias"]:
        d.bias = BIAS_
    if c["residual"]:
        d.residual, d.ldr, d.r_dtype = RES_, N, d.c_dtype
    if c["mask"]:
        if st == "bits":
            d.mask, d.ldmask, d.m_dtype = MASK_, (N + 7) // 8, 2
        else:
            d.mask, d.ldmask, d.m_dtype = MASK_, N, d.c_dtype
    if st == "bits":
        d.maskbits_out, d.ld_maskbits_out = BITS_, (N + 7) // 8
    d.act, d.split_k = c["act"], c["split_k"]
    d.dropout_p, d.dropout_seed = c["dropout"], 7
    if c["rowsum"]:
        d.rowsum_a, d.rowsum_alpha = ROWSUM_, 1.0
    if c["ln"]:
        d.ln_gamma, d.ln_beta, d.ln_y, d.ln_mean, d.ln_rstd, d.ln_eps = LN_, LN_ + 0x1000, LN_ + 0x2000, LN_ + 0x3000, LN_ + 0x4000, 1e-5
    if c["res_sub"]:
        d.res_sub_h, d.res_sub_w = c["res_sub"]
        d.res_sub_ho, d.res_sub_wo = (d.res_sub_h + 1) // 2, (d.res_sub_w + 1) // 2
    if c["ws"] == 1:
        d.workspace, d.workspace_bytes = WS_, c["split_k"] * M * N * 4
    elif c["ws"] == 2:
        d.workspace, d.workspace_bytes = WS_, max(0, lib.detr_hip_workspace_bytes_gemm(ctypes.byref(d)))
    return d


def family_char(rc):
    """'0' .. '5' for a family, 'a' for the rejection code -1, 'b' for -2, ..."""
    return str(rc) if rc >= 0 else chr(ord("a") - 1 - rc)


def route_all(_hip, lib, case_list=None):
    """{environment name: (family string, [workspace bytes of the split-K cases])} for every tuning environment.  The process's
    own DETR_HIP_* settings of the variables in ENVS are set aside for the run and restored afterwards."""
    case_list = cases() if case_list is None else case_list
    saved = {k: os.environ.get(k) for k in ENV_VARS}
    out = {}
    try:
        for k in ENV_VARS:
            _hip.set_tuning(k, None)
        for env in ENVS:
            if env[0]:
                _hip.set_tuning("DETR_HIP_" + env[0], env[1])
            fam, ws = [], []
            for c in case_list:
                d = fill(_hip, lib, c)
                fam.append(family_char(lib.detr_hip_gemm_family(ctypes.byref(d))))
                if c["split_k"] > 1:
                    ws.append(int(lib.detr_hip_workspace_bytes_gemm(ctypes.byref(d))))
            out[env_name(env)] = ("".join(fam), ws)
            if env[0]:
                _hip.set_tuning("DETR_HIP_" + env[0], None)
    finally:
        for k, v in saved.items():
            _hip.set_tuning(k, v)
    return out
