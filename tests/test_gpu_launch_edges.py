"""The row, glue and pooling kernels past the edges of their launch geometry: the second trip of every grid-stride loop, the
rows-per-block switch of the three column-sum launches, the exports without a reference test of their own (colsum_scaled,
fma_vec_group, cvt_bf16, scale_cols_t) and LayerNorm on widths, row counts and row means the other tests do not reach.

References are plain torch / NumPy on the CPU; the assertion is equality wherever the operation is exact.  The bounds, the data
and the reference code live in tests/test_launch_edges_cpu.py, which also shows on the CPU that the bounds separate a correct
kernel from a subtly wrong one.  Every output (and every scratch buffer) has a guard region filled with a sentinel behind its
end that must come back unchanged; padding columns of inputs hold NaN, so a read outside [0, cols) poisons the result.

Sizes are the smallest that cross the edge in question: 8192 blocks x 256 threads = 2,097,152 threads for the kernels of
rowops.hip / pool.hip, 16384 blocks for the two image-input kernels (one thread per PIXEL: the batch needs more than
4,194,304 pixels to wrap, not elements), 2048 blocks for the zero fill."""
import ctypes

import numpy as np
import pytest
import torch

import test_launch_edges_cpu as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAP = 8192 * 256            # threads of a capped_grid(n, 256, 8192) launch
SENT = -8192.0           # exact in bf16 too
GUARD = 64


def g(t):
    return t.to(DEV).contiguous()


def guarded(shape, dtype=torch.float32, fill=SENT, guard=GUARD):
    """(view of `shape` at the start of a buffer, its guard tail): the buffer is filled with the sentinel."""
    n = int(np.prod(shape))
    buf = torch.full((n + guard,), fill, dtype=dtype, device=DEV)
    return buf[:n].view(*shape), buf[n:]


def intact(tail, fill=SENT):
    return bool((tail == fill).all())


def close_global(a, b, rtol, what):
    """max |a - b| <= rtol * max |b|: the per-tensor tolerance of tests/test_gpu_kernels.py::close."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err, scale = float((a - b).abs().max()), float(b.abs().max()) + 1e-30
    assert err <= rtol * scale, f"{what}: max abs err {err:.3e} > {rtol * scale:.3e}"


# ------------------------------------------------------------------------------------------------------------------------
# A. grid-stride wrap
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["add", "sigmoid_bwd", "relu_mask", "axpy", "dropout"])
def test_scalar_loop_kernels_wrap_their_grid(hip, op):
    """add / sigmoid_bwd / relu_mask / axpy / dropout at n = 2,097,152 + 257: 257 threads take a second trip of
    `i += gridDim.x * blockDim.x`.  add, relu_mask and dropout (against oracle/dropout_ref.py) are exact; axpy and sigmoid_bwd
    keep the 1e-6 per-tensor tolerance of test_small_elementwise (the compiler may contract the multiply-add).  A stride that is too
    long leaves elements unwritten (the sentinel stays).  One that is too short only computes elements twice, which a pure map
    hides; the accumulating axpy (and multi_copy in mode 1) update such an element twice and fail."""
    n = CAP + 257
    gen = torch.Generator().manual_seed(17)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    ad, bd = g(a), g(b)
    out, tail = guarded((n,))
    if op == "add":
        hip.call("detr_hip_add_f32", ad.data_ptr(), bd.data_ptr(), out.data_ptr(), n)
        assert torch.equal(out.cpu(), a + b)
    elif op == "relu_mask":
        hip.call("detr_hip_relu_mask_f32", ad.data_ptr(), bd.data_ptr(), out.data_ptr(), n)
        assert torch.equal(out.cpu(), torch.where(b > 0, a, torch.zeros(())))
    elif op == "sigmoid_bwd":
        y = torch.sigmoid(b)
        yd = g(y)
        hip.call("detr_hip_sigmoid_bwd_f32", ad.data_ptr(), yd.data_ptr(), out.data_ptr(), n)
        close_global(out, a.double() * y.double() * (1 - y.double()), 1e-6, "sigmoid_bwd")
    elif op == "axpy":
        out.copy_(bd)
        hip.call("detr_hip_axpy_f32", out.data_ptr(), ad.data_ptr(), ctypes.c_float(2.0), n)
        close_global(out, b.double() + 2 * a.double(), 1e-6, "axpy")
    else:
        from oracle import dropout_ref as DR
        p, site, step = 0.1, 0xABCDE, 0x1234567
        stepd = torch.tensor([step] + [0] * 7, dtype=torch.int32, device=DEV)
        hip.call("detr_hip_dropout_f32", ad.data_ptr(), out.data_ptr(), n, ctypes.c_float(p), site, stepd.data_ptr())
        keep = torch.from_numpy(DR.keep_mask(DR.drop_key(site, step), np.arange(n), p))
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        assert torch.equal(out.cpu(), torch.where(keep, a * float(scale), torch.zeros(())))
    assert intact(tail)


def test_scale_cols_stays_in_phase_across_the_wrap(hip):
    """scale_cols at 6,991 x 300 = 2,097,300 elements: `i % cols` of the wrapped elements with a cols that is no power of two."""
    rows, cols = 6991, 300
    assert rows * cols > CAP and CAP % cols != 0
    gen = torch.Generator().manual_seed(5)
    w, sc = torch.randn(rows, cols, generator=gen), torch.rand(cols, generator=gen) + 0.5
    wd, scd = g(w), g(sc)
    out, tail = guarded((rows, cols))
    hip.call("detr_hip_scale_cols_f32", wd.data_ptr(), scd.data_ptr(), out.data_ptr(), rows, cols)
    assert torch.equal(out.cpu(), w * sc) and intact(tail)


def test_float4_loop_kernels_wrap_their_grid(hip):
    """add_bcast and cvt_bf16 at n = 4 * (2,097,152 + 257): their loops count float4; add_bcast with a period (1200) that does not
    divide 4 * 2,097,152, so the phase of `i % period4` differs between the trips."""
    n, period = 4 * (CAP + 257), 1200
    assert (4 * CAP) % period != 0
    gen = torch.Generator().manual_seed(6)
    x, p = torch.randn(n, generator=gen), torch.randn(period, generator=gen)
    xd, pd = g(x), g(p)
    out, tail = guarded((n,))
    hip.call("detr_hip_add_bcast_f32", xd.data_ptr(), pd.data_ptr(), out.data_ptr(), n, period)
    want = x + p.repeat(n // period + 1)[:n]
    assert torch.equal(out.cpu(), want) and intact(tail)
    o16, tail16 = guarded((n,), torch.bfloat16)
    hip.call("detr_hip_cvt_bf16", xd.data_ptr(), o16.data_ptr(), n)
    assert torch.equal(E.bf16_bits(o16.cpu()), E.bf16_bits(x.to(torch.bfloat16))) and intact(tail16)


def test_multi_copy_with_one_block_per_entry(hip):
    """multi_copy with blocks_per_entry = 1: 256 16-byte units per trip, entries of 1000, 777 and 300 units in both modes."""
    gen = torch.Generator().manual_seed(7)
    a, b = torch.randn(4000, generator=gen), torch.randn(3108, generator=gen)
    c = torch.randn(2400, generator=gen).to(torch.bfloat16)
    b0 = torch.randn(3108, generator=gen)
    ad, bd, cd = g(a), g(b), g(c)
    da, ta = guarded((4000,))
    db, tb = guarded((3108,))
    dc, tc = guarded((2400,), torch.bfloat16)
    db.copy_(b0)
    table = hip.copy_table([(ad, da, 0), (bd, db, 1), (cd, dc, 0)], DEV)
    hip.multi_copy(table, 1)
    assert torch.equal(da.cpu(), a) and torch.equal(db.cpu(), b0 + b) and torch.equal(E.bf16_bits(dc.cpu()), E.bf16_bits(c))
    assert intact(ta) and intact(tb) and intact(tc)


@pytest.mark.parametrize("offset", [16, 3])
def test_zero_fill_wraps_its_grid(hip, offset):
    """detr_hip_memset_zero: zero_fill_kernel runs at most 2048 blocks of 256 16-byte units (8 MiB per trip); 8 MiB + 257 units
    + 5 tail bytes, from an aligned start and from one that needs the byte-store head."""
    nbytes = 2048 * 256 * 16 + 257 * 16 + 5
    buf = torch.full((offset + nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    hip.call("detr_hip_memset_zero", buf.data_ptr() + offset, nbytes)
    assert bool((buf[offset:offset + nbytes] == 0).all())
    assert bool((buf[:offset] == 0xAB).all()) and bool((buf[offset + nbytes:] == 0xAB).all())


POOL_SHAPE = (2, 2049, 2048, 8)        # N * Hp * Wp * C / 8 = 2 * 1025 * 1024 = 2,099,200 lanes of the 8-channel bf16 form: above the cap


@pytest.fixture(scope="module")
def pool_case():
    """One integer-valued map (exact in bf16 and fp32, ties in every window) and its references, computed once: forward and
    backward by the tap loops of test_launch_edges_cpu.py (the backward one is test_gpu_pool_bwd_windows.py's), the sums of at
    most four dy in [-8, 8] are exact in bf16."""
    N, H, W, C = POOL_SHAPE
    gen = torch.Generator().manual_seed(23)
    x = torch.randint(-4, 5, POOL_SHAPE, generator=gen, dtype=torch.int8).float()
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    assert N * Ho * Wo * (C // 8) > CAP
    dy = torch.randint(-8, 9, (N, Ho, Wo, C), generator=gen, dtype=torch.int8).float()
    y, am = E.pool_fwd_taps(x.numpy())
    dx = E.pool_bwd_taps(dy.numpy(), am, x.numpy())
    return dict(x=x, dy=dy, y=torch.from_numpy(y), am=torch.from_numpy(am), dx=torch.from_numpy(dx), Ho=Ho, Wo=Wo)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_maxpool_forward_wraps_its_grid(hip, pool_case, dtype):
    """maxpool_fwd_kernel<float, 1> (16.8M lanes, 8 trips) and <bf16, 8> (2,099,200 lanes, the second trip) on 2 x 2049 x 2048 x 8."""
    N, H, W, C = POOL_SHAPE
    Ho, Wo = pool_case["Ho"], pool_case["Wo"]
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    xd = g(pool_case["x"]).to(td)
    y, ty = guarded((N, Ho, Wo, C), td)
    am, ta = guarded((N, Ho, Wo, C), torch.uint8, fill=0xEE)
    hip.call(f"detr_hip_maxpool3x3s2_fwd_{dtype}", xd.data_ptr(), y.data_ptr(), am.data_ptr(), N, H, W, C, Ho, Wo)
    assert torch.equal(y.float().cpu(), pool_case["y"])
    assert torch.equal(am.cpu(), pool_case["am"])
    assert intact(ty) and intact(ta, 0xEE)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_maxpool_backward_wraps_its_grid(hip, pool_case, dtype):
    """maxpool_bwd_kernel<float, 4> (16.8M lanes) and <bf16, 8> (8.4M lanes) on 2 x 2049 x 2048 x 8, from the reference argmax."""
    N, H, W, C = POOL_SHAPE
    Ho, Wo = pool_case["Ho"], pool_case["Wo"]
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    xd, dyd, amd = g(pool_case["x"]).to(td), g(pool_case["dy"]).to(td), g(pool_case["am"])
    dx, tx = guarded((N, H, W, C), td)
    hip.call(f"detr_hip_maxpool3x3s2_bwd_{dtype}", dyd.data_ptr(), amd.data_ptr(), xd.data_ptr(), dx.data_ptr(), N, H, W, C, Ho, Wo)
    assert torch.equal(dx.float().cpu(), pool_case["dx"]) and intact(tx)


def test_subsample2_wraps_its_grid(hip, pool_case):
    """subsample2 forward (4.2M float4 lanes) and backward (16.8M) on 2 x 2049 x 2048 x 8."""
    N, H, W, C = POOL_SHAPE
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert N * Ho * Wo * (C // 4) > CAP
    x = pool_case["x"]
    xd = g(x)
    y, ty = guarded((N, Ho, Wo, C))
    hip.call("detr_hip_subsample2_fwd_f32", xd.data_ptr(), y.data_ptr(), N, H, W, C, Ho, Wo)
    assert torch.equal(y.cpu(), x[:, ::2, ::2, :]) and intact(ty)
    dy = pool_case["dy"][:, :Ho, :Wo, :].contiguous()
    assert dy.shape == (N, Ho, Wo, C)
    dyd = g(dy)
    dx, tx = guarded((N, H, W, C))
    hip.call("detr_hip_subsample2_bwd_f32", dyd.data_ptr(), dx.data_ptr(), N, H, W, C, Ho, Wo)
    want = torch.zeros(N, H, W, C)
    want[:, ::2, ::2, :] = dy
    assert torch.equal(dx.cpu(), want) and intact(tx)


@pytest.mark.parametrize("method", ["torch_resnet", "tf_resnet"])
def test_input_stage_wraps_its_grid(hip, method):
    """input_stage (16384 blocks, one thread per pixel) on 3 x 1201 x 1166 = 4,201,098 pixels at equal source and target size:
    bit-identical to the host pipeline normalized_images, as in tests/test_input_stage.py."""
    from detr_tf.data.processing import DeviceInputStage, normalized_images
    from detr_tf.training_config import TrainingConfig
    B, H, W = 3, 1201, 1166
    assert B * H * W > 16384 * 256
    cfg = TrainingConfig()
    cfg.normalized_method, cfg.image_size = method, (H, W)
    batch = np.random.default_rng(11).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    out, tail = guarded((B, H, W, 3))
    got = DeviceInputStage(cfg).images(batch, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), torch.from_numpy(normalized_images(batch, cfg))) and intact(tail)


def test_input_stage_padded_wraps_its_grid(hip):
    """input_stage_padded on a 3 x 1201 x 1166 canvas with three image sizes, against the lookup-table pipeline of
    tests/test_gpu_padding.py::test_images_padded."""
    from detr_tf.data.processing import normalization_table
    sizes = [(1201, 1166), (1100, 1166), (1201, 900)]
    B, H, W = 3, 1201, 1166
    rng = np.random.default_rng(12)
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    lut, perm = normalization_table("torch_resnet")
    packed = g(torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])))
    offs = np.concatenate([[0], np.cumsum([im.size for im in imgs])[:-1]]).astype(np.int64)
    off_d, hw_d, lut_d = g(torch.from_numpy(offs)), g(torch.tensor(sizes, dtype=torch.int32).reshape(-1)), g(torch.from_numpy(lut))
    dst, td = guarded((B, H, W, 3))
    mask, tm = guarded((B, H, W), torch.uint8, fill=0xEE)
    permc = (ctypes.c_int32 * 3)(*perm)
    hip.call("detr_hip_input_stage_padded", packed.data_ptr(), off_d.data_ptr(), hw_d.data_ptr(), B, H, W, lut_d.data_ptr(),
             ctypes.cast(permc, ctypes.c_void_p), dst.data_ptr(), mask.data_ptr())
    x, m = dst.cpu().numpy(), mask.cpu().numpy()
    for b, (im, (h, w)) in enumerate(zip(imgs, sizes)):
        want = np.zeros((H, W, 3), np.float32)
        want[:h, :w] = np.stack([lut[c][im[..., perm[c]]] for c in range(3)], axis=-1)
        assert x[b].tobytes() == want.tobytes()
        wm = np.ones((H, W), np.uint8)
        wm[:h, :w] = 0
        assert np.array_equal(m[b], wm)
    assert intact(td) and intact(tm, 0xEE)


# ------------------------------------------------------------------------------------------------------------------------
# B. column sums
# ------------------------------------------------------------------------------------------------------------------------
def _colsum_run(hip, kind, xd, out, rows, cols, ld, alpha, scale_d, det_scratch=None):
    if kind == "f32":
        hip.call("detr_hip_colsum_f32", xd.data_ptr(), out.data_ptr(), rows, cols, ld, ctypes.c_float(alpha))
    elif kind == "det":
        scr, n = det_scratch
        hip.call("detr_hip_colsum_det_f32", xd.data_ptr(), out.data_ptr(), rows, cols, ld, ctypes.c_float(alpha), scr.data_ptr(), n)
    else:
        hip.call("detr_hip_colsum_scaled", xd.data_ptr(), 1 if xd.dtype == torch.bfloat16 else 0, rows, cols, ld,
                 None if scale_d is None else scale_d.data_ptr(), out.data_ptr())


def _colsum_variants(kind):
    """(input dtype, scale set?) combinations of one kernel: colsum_scaled takes both dtypes and an optional scale."""
    if kind != "scaled":
        return [(torch.float32, False)]
    return [(torch.float32, False), (torch.float32, True), (torch.bfloat16, False), (torch.bfloat16, True)]


def _det_scratch(hip, rows, cols):
    n = int(hip.load().detr_hip_colsum_det_scratch_floats(rows, cols))
    rpb, chunks = E.colsum_plan("det", rows)
    assert n == chunks * cols
    scr, tail = guarded((n,))
    return (scr, n), tail


_TIER1 = [(k, r) for k in E.COLSUM_KINDS for r in E.COLSUM_SMALL_ROWS + E.COLSUM_SWITCH_ROWS[k]]


@pytest.mark.parametrize("kind,rows", _TIER1)
def test_colsum_exact_on_integers(hip, kind, rows):
    """colsum_f32, colsum_det_f32 and colsum_scaled (fp32 and bf16 input, scale NULL and set) on integers in [-8, 8] with
    power-of-two alpha / scale and an integer-valued `out` to accumulate into: every partial sum stays below 2^24 (asserted),
    so every summation order gives the same bits and the result must EQUAL the int64 reference -- one dropped or doubled row
    fails.  Rows 1..127, and each kernel's rows-per-block switch and the count above it (16,384 / 16,385 for det and scaled,
    16,641 for scaled: ceil(rows / 256) = 66; 131,072 / 131,073 for colsum_f32), with ld = cols and ld = cols + 3 (NaN in the
    padding columns).  colsum_det_f32 must also repeat its bits."""
    small = rows <= 127
    for cols in (E.COLSUM_SMALL_COLS if small else (5, 8)):
        for ld in (cols, cols + 3):
            x, out0, scale, alpha = E.colsum_int_inputs(rows, cols, ld, seed=rows * 7 + cols)
            assert rows <= E.COLSUM_MAX_EXACT_ROWS and E.colsum_int_partial_bound(rows, alpha, scale, out0) < 2 ** 24
            isum = x[:, :cols].to(torch.int64).sum(0).double()
            for dtype, use_scale in _colsum_variants(kind):
                xd = g(x.to(dtype))
                scale_d = g(scale) if use_scale else None
                factor = (scale.double() if use_scale else 1.0) if kind == "scaled" else alpha
                want = (out0.double() + factor * isum).float()
                scratch, stail = _det_scratch(hip, rows, cols) if kind == "det" else (None, None)
                runs = []
                for _ in range(2 if kind == "det" else 1):
                    out, tail = guarded((cols,))
                    out.copy_(g(out0))
                    _colsum_run(hip, kind, xd, out, rows, cols, ld, alpha, scale_d, scratch)
                    assert torch.equal(out.cpu(), want), (kind, rows, cols, ld, dtype, use_scale)
                    assert intact(tail) and (stail is None or intact(stail))
                    runs.append(out.cpu())
                assert all(torch.equal(runs[0], r) for r in runs)


@pytest.mark.parametrize("rows,cols", E.COLSUM_TIER2)
@pytest.mark.parametrize("kind", E.COLSUM_KINDS)
def test_colsum_rounding_bound(hip, kind, rows, cols):
    """randn data against fp64 sums of the same stored values, per column
        tol_c = 1.01 * (rpb + chunks + 2) * 2^-24 * (|out0_c| + |alpha * scale_c| * sum_r |x_rc|)
    with rpb and chunks from the launch rule (test_launch_edges_cpu.colsum_plan).  colsum_f32 and colsum_scaled finish with fp32
    atomics: their bits may differ from run to run, so no equality is asserted for them; colsum_det_f32 must repeat."""
    gen = torch.Generator().manual_seed(rows + cols)
    ld = cols + 3
    x = torch.full((rows, ld), float("nan"))
    x[:, :cols] = torch.randn(rows, cols, generator=gen)
    out0 = torch.randn(cols, generator=gen)
    scale = torch.rand(cols, generator=gen) + 0.5
    alpha = 0.5
    for dtype, use_scale in _colsum_variants(kind):
        xs = x.to(dtype)
        xd = g(xs)
        stored = xs[:, :cols].float()
        scale_d = g(scale) if use_scale else None
        factor = (scale.double() if use_scale else torch.ones(cols, dtype=torch.float64)) if kind == "scaled" else torch.full((cols,), alpha, dtype=torch.float64)
        ref = out0.double() + factor * stored.double().sum(0)
        tol = E.colsum_tol(kind, rows, out0, factor, stored)
        scratch, stail = _det_scratch(hip, rows, cols) if kind == "det" else (None, None)
        runs = []
        for _ in range(2 if kind == "det" else 1):
            out, tail = guarded((cols,))
            out.copy_(g(out0))
            _colsum_run(hip, kind, xd, out, rows, cols, ld, alpha, scale_d, scratch)
            ratio = float(((out.cpu().double() - ref).abs() / tol).max())
            print(f"colsum {kind} {rows}x{cols} {dtype} scale={use_scale}: err/tol {ratio:.4f}")
            assert ratio <= 1.0, (kind, dtype, use_scale, ratio)
            assert intact(tail) and (stail is None or intact(stail))
            runs.append(out.cpu())
        assert all(torch.equal(runs[0], r) for r in runs)


# ------------------------------------------------------------------------------------------------------------------------
# C. cvt_bf16, bit for bit
# ------------------------------------------------------------------------------------------------------------------------
def _cvt(hip, src):
    xd = g(src)
    out, tail = guarded((src.numel(),), torch.bfloat16)
    hip.call("detr_hip_cvt_bf16", xd.data_ptr(), out.data_ptr(), src.numel())
    assert intact(tail)
    return out.cpu()


def test_cvt_bf16_rounds_to_nearest_even(hip):
    """cvt_bf16 on the hand-made vector of test_launch_edges_cpu.BF16_TIES (exact ties with an even and an odd kept mantissa in
    both signs, one bit above / below a tie, the carry into the exponent, the largest finite fp32 -> infinity, zeros, infinities)
    against the bits worked out by hand, which torch's CPU conversion also gives; NaN stays NaN (also the signalling NaN whose
    payload sits in the dropped bits only); n = 4, the smallest legal call."""
    src = E.f32_from_bits([b for b, _ in E.BF16_TIES])
    want = E.bf16_expected([w for _, w in E.BF16_TIES])
    assert torch.equal(E.bf16_bits(src.to(torch.bfloat16)), want)
    assert torch.equal(E.bf16_bits(_cvt(hip, src)), want)
    assert bool(torch.isnan(_cvt(hip, E.f32_from_bits(E.BF16_NANS)).float()).all())
    assert torch.equal(E.bf16_bits(_cvt(hip, src[4:8])), want[4:8])


def test_cvt_bf16_denormals(hip):
    """fp32 denormals: the result must be torch's RNE value or a zero of the same sign (a conversion that flushes denormal
    inputs); the weight shadow never holds denormals, either is accepted.  The test prints which one the device gave.
    Observed on the MI355X: RNE on all eight values (0x007FFFFF -> 0x0080, 0x00018000 -> 0x0002, ...): the conversion keeps fp32
    denormals in the mode the library is compiled with."""
    src = E.f32_from_bits(E.BF16_DENORMALS)
    rne = E.bf16_bits(src.to(torch.bfloat16))
    zero = E.bf16_expected([(b >> 16) & 0x8000 for b in E.BF16_DENORMALS])
    got = E.bf16_bits(_cvt(hip, src))
    print("cvt_bf16 denormals:", "RNE" if torch.equal(got, rne) else "flushed to zero" if torch.equal(got, zero) else "mixed",
          [hex(int(v) & 0xFFFF) for v in got])
    assert bool(((got == rne) | (got == zero)).all())


def test_scale_cols_bf16_rounds_ties_like_cvt(hip):
    """scale_cols_bf16 with the ties vector as w and scale = 1: the product is exact and the same expected bits apply."""
    src = E.f32_from_bits([b for b, _ in E.BF16_TIES])
    cols = 4
    rows = src.numel() // cols
    wd, scd = g(src.view(rows, cols)), g(torch.ones(cols))
    out, tail = guarded((rows, cols), torch.bfloat16)
    hip.call("detr_hip_scale_cols_bf16", wd.data_ptr(), scd.data_ptr(), out.data_ptr(), rows, cols)
    assert torch.equal(E.bf16_bits(out.cpu()).view(-1), E.bf16_expected([w for _, w in E.BF16_TIES])) and intact(tail)


# ------------------------------------------------------------------------------------------------------------------------
# D. fma_vec_group
# ------------------------------------------------------------------------------------------------------------------------
def test_fma_vec_group(hip):
    """fma_vec_group over a device table of detr_fma_entry rows laid out as Engine._refresh_bias_shift builds it (int64
    [a, b, c, out, n]), lengths 1 .. 2048, against fp64 a * b + c with 1.01 * 2^-24 * (|a * b| + |a * b + c|) per element: the
    contracted FMA (one rounding) and the separate multiply and add (two) both fit."""
    gen = torch.Generator().manual_seed(31)
    lens = (1, 4, 255, 256, 257, 2048)
    host = [[torch.randn(n, generator=gen) for _ in range(3)] for n in lens]
    dev = [[g(t) for t in abc] for abc in host]
    outs = [guarded((n,)) for n in lens]
    table = torch.tensor([[a.data_ptr(), b.data_ptr(), c.data_ptr(), o.data_ptr(), n] for (a, b, c), (o, _), n in zip(dev, outs, lens)],
                         dtype=torch.int64).to(DEV)
    hip.call("detr_hip_fma_vec_group", table.data_ptr(), len(lens))
    for (a, b, c), (o, tail), n in zip(host, outs, lens):
        ab = a.double() * b.double()
        ref = ab + c.double()
        tol = 1.01 * E.U * (ab.abs() + ref.abs())
        assert bool(((o.cpu().double() - ref).abs() <= tol).all()), n
        assert intact(tail), n


# ------------------------------------------------------------------------------------------------------------------------
# E. scale_cols_t_f32
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_scale", [False, True])
@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (32, 32), (33, 31), (147, 64), (576, 64), (64, 300)])
def test_scale_cols_t(hip, rows, cols, use_scale):
    """scale_cols_t_f32 (32 x 32 LDS transpose with ragged edge tiles): equals (w * scale).t() exactly, scale NULL and set."""
    gen = torch.Generator().manual_seed(rows * 1000 + cols)
    w, sc = torch.randn(rows, cols, generator=gen), torch.rand(cols, generator=gen) + 0.5
    wd, scd = g(w), g(sc)
    out, tail = guarded((cols, rows))
    hip.call("detr_hip_scale_cols_t_f32", wd.data_ptr(), scd.data_ptr() if use_scale else None, out.data_ptr(), rows, cols)
    want = ((w * sc) if use_scale else w).t().contiguous()
    assert torch.equal(out.cpu(), want) and intact(tail)


# ------------------------------------------------------------------------------------------------------------------------
# F. LayerNorm widths, offsets and row edges
# ------------------------------------------------------------------------------------------------------------------------
def ln_forward_check(x, gam, bet, y, mean, rstd, eps=1e-5, what=""):
    """y / mean / rstd of a LayerNorm launch (host tensors) against test_launch_edges_cpu.ln_forward_reference."""
    R = E.ln_forward_reference(x, gam, bet, eps)
    ry = float(((y.double() - R["ref"]).abs() / R["bound"]).max())
    rm = float(((mean.double() - R["mu"]).abs() / R["mean_bound"]).max())
    rr = float(((rstd.double() / R["rs"] - 1).abs() / R["rstd_rel_bound"]).max())
    print(f"layernorm fwd {what}: y err/bound {ry:.3f}, mean {rm:.3f}, rstd {rr:.3f}")
    assert ry <= 1.0 and rm <= 1.0 and rr <= 1.0, (what, ry, rm, rr)


def _ln_forward(hip, x, gam, bet, add=None):
    rows, C = x.shape
    xd, gd, bd = g(x), g(gam), g(bet)
    y, ty = guarded((rows, C))
    mean, tm = guarded((rows,))
    rstd, tr = guarded((rows,))
    y2, t2 = guarded((rows, C)) if add is not None else (None, None)
    addd = g(add) if add is not None else None
    hip.layernorm_fwd(xd, gd, bd, y, mean, rstd, 1e-5, add=addd, y2=y2)
    torch.cuda.synchronize()
    assert intact(ty) and intact(tm) and intact(tr) and (t2 is None or intact(t2))
    return xd, gd, y, mean, rstd, y2


@pytest.mark.parametrize("rows", [1, 5, 9])
@pytest.mark.parametrize("C", E.LN_WIDTHS)
def test_layernorm_widths_offsets_and_row_edges(hip, rows, C):
    """layernorm_fwd_kernel / layernorm_bwd_kernel on widths that fill a register slot partly (4, 252, 260, 1020: the `j < nv`
    predicate) and fully, on 1, 5 and 9 rows (idle waves in a block, a second block), with three row families in one launch:
    randn * 2 + 0.3, randn + 1000 and 0.5 * randn - 3e4.  Forward: per-element bound of ln_forward_reference (fp64 statistics
    of the stored values), which E[x^2] - E[x]^2 misses by two to four orders of magnitude on the offset rows (shown on the CPU).
    Backward: dx against fp64 from the kernel's own mean / rstd with ln_backward_reference's bound, on every row; dgamma / dbeta
    with the per-tensor 5e-5 of test_layernorm_fwd_bwd on the rows of the first family."""
    x, gam, bet, fam = E.ln_inputs(rows, C, seed=rows * 4096 + C)
    xd, gd, y, mean, rstd, _ = _ln_forward(hip, x, gam, bet)
    ln_forward_check(x, gam, bet, y.cpu(), mean.cpu(), rstd.cpu(), what=f"{rows}x{C}")
    dy = torch.randn(rows, C, generator=torch.Generator().manual_seed(C + rows))
    dyd = g(dy)
    dx, tx = guarded((rows, C))
    dg, tg = guarded((C,))
    db, tb = guarded((C,))
    dg.zero_()
    db.zero_()
    hip.layernorm_bwd(dyd, xd, gd, mean, rstd, dx, dg, db)
    ref, bound = E.ln_backward_reference(dy, x, gam, mean.cpu(), rstd.cpu())
    ratio = float(((dx.cpu().double() - ref).abs() / bound).max())
    print(f"layernorm bwd {rows}x{C}: dx err/bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    assert intact(tx) and intact(tg) and intact(tb)
    # dgamma / dbeta: the rows of the first family alone, against fp64 autograd
    keep = fam == 0
    keepd = keep.to(DEV)
    x1 = x[keep].double().requires_grad_(True)
    g1, b1 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    torch.nn.functional.layer_norm(x1, (C,), g1, b1, 1e-5).backward(dy[keep].double())
    x1d, dy1d, m1, r1 = g(x[keep]), g(dy[keep]), mean[keepd].contiguous(), rstd[keepd].contiguous()
    dx1, _ = guarded((int(keep.sum()), C))
    dg.zero_()
    db.zero_()
    hip.layernorm_bwd(dy1d, x1d, gd, m1, r1, dx1, dg, db)
    close_global(dg, g1.grad, 5e-5, "layernorm dgamma")
    close_global(db, b1.grad, 5e-5, "layernorm dbeta")
    assert intact(tg) and intact(tb)


def test_layernorm_forward_row_loop_wraps(hip):
    """16,389 x 64: the forward grid is capped at 4096 blocks of 4 rows, the last 5 rows are a second trip of the row loop."""
    rows, C = 4096 * 4 + 5, 64
    x, gam, bet, _ = E.ln_inputs(rows, C, seed=99)
    _, _, y, mean, rstd, _ = _ln_forward(hip, x, gam, bet)
    ln_forward_check(x, gam, bet, y.cpu(), mean.cpu(), rstd.cpu(), what=f"{rows}x{C}")


def test_layernorm_y2_with_a_ragged_period(hip):
    """y2 = y + add[r % add_rows] with 37 rows and a period of 5 (37 is no multiple of it)."""
    rows, C, period = 37, 64, 5
    x, gam, bet, _ = E.ln_inputs(rows, C, seed=37)
    add = torch.randn(period, C, generator=torch.Generator().manual_seed(5))
    _, _, y, mean, rstd, y2 = _ln_forward(hip, x, gam, bet, add=add)
    ln_forward_check(x, gam, bet, y.cpu(), mean.cpu(), rstd.cpu(), what="y2 case")
    assert torch.equal(y2.cpu(), y.cpu() + add[torch.arange(rows) % period])
