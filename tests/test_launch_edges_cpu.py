"""References, data and error bounds of tests/test_gpu_launch_edges.py, and the proof (on the CPU, NumPy / torch only) that those
bounds have teeth and that a correct kernel stays inside them:

  * LayerNorm: the kernel's summation order (lane-strided float4 partials of a wave64, then the 6-level tree of wave_sum) is
    emulated in fp32 with the two-pass variance the kernels use and with E[x^2] - E[x]^2.  The forward bound must leave the
    two-pass form below 0.5 and be exceeded at least 10x by the one-pass form on rows with a large mean;
  * column sums: "one thread's serial sum per chunk, then the chunks in any order" in fp32 stays inside tol_c, the integer data of
    the exact tier keeps every partial sum below 2^24, and a dropped / doubled row is (or is not: see the test) outside tol_c;
  * fp32 -> bf16: torch's CPU conversion gives the bits worked out by hand for the ties vector, so the GPU test compares the
    kernel with arithmetic and not just with another implementation;
  * pooling: the tap-loop references vectorised over the pixels equal the per-pixel loop of tests/test_gpu_pool_bwd_windows.py
    bit for bit (same adds, same (kh, kw) order).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of fp32


# ------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------
LN_WIDTHS = (4, 8, 252, 256, 260, 512, 1020, 1024)
LN_FAMILIES = ((2.0, 0.3), (1.0, 1000.0), (0.5, -3e4))       # (std, mean): row r belongs to family r % 3


def ln_inputs(rows, C, seed):
    """x [rows, C] fp32 with the three row families interleaved (one launch sees all of them), gamma, beta."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=gen, dtype=torch.float64)
    fam = torch.arange(rows) % 3
    sd = torch.tensor([f[0] for f in LN_FAMILIES], dtype=torch.float64)[fam]
    off = torch.tensor([f[1] for f in LN_FAMILIES], dtype=torch.float64)[fam]
    x = (x * sd[:, None] + off[:, None]).float()
    gam = (torch.rand(C, generator=gen) + 0.5).float()
    bet = torch.randn(C, generator=gen).float()
    return x, gam, bet, fam


def ln_forward_reference(x, gam, bet, eps):
    """fp64 LayerNorm of the STORED fp32 values and the per-element bounds a two-pass fp32 kernel must meet, u = 2^-24.

    The row sum passes every term through at most 21 additions (a lane that holds 16 values adds them in 15 steps -- the
    kernels pair them, which is shorter -- then 6 cross-lane levels), so the computed mean is off by
        d_mu <= 21u * mean|x_row|                                             (bound of the saved `mean`)
    Two-pass variance: mean((x - mu_hat)^2) = var + d_mu^2 exactly, and its own rounding (subtract, square, the 21-deep sum,
    the division) is relative, <= 26u.  With rsqrt accurate to 2u the saved rstd = rsqrt(var_hat + eps) is off by
        |rstd_hat / rstd - 1| <= 0.5 * (d_mu^2 * rstd^2 + 26u) + 2u <= 0.5 * (21u * mean|x_row|)^2 * rstd^2 + 16u   (bound of `rstd`)
    The output (x - mu_hat) * rstd_hat * gamma + beta then differs from the reference by the mean's error scaled by gamma * rstd
    (first term; the 2u * max|x_row| is the rounding of x - mu_hat), a relative error of the centred value (29u: the chain of the
    variance plus the elementwise roundings), and the roundings of the last multiply-add (4u|ref| + 2u|beta|):
        |y - ref| <= |gamma| * rstd * (21u * mean|x_row| + 2u * max|x_row|) + 29u * |gamma| * |x - mu| * rstd + 4u * |ref| + 2u * |beta|
    A one-pass variance E[x^2] - E[x]^2 loses (mean/std)^2 * u relative instead and fails this by orders of magnitude once the
    mean is large (test_layernorm_bound_separates_two_pass_from_one_pass)."""
    xd, g, b = x.double(), gam.double(), bet.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    ref = (xd - mu) * rs * g + b
    absmean, absmax = xd.abs().mean(1, keepdim=True), xd.abs().max(1, keepdim=True).values
    bound = g.abs() * rs * (21 * U * absmean + 2 * U * absmax) + 29 * U * g.abs() * (xd - mu).abs() * rs + 4 * U * ref.abs() + 2 * U * b.abs()
    mean_bound = 21 * U * absmean[:, 0]
    rstd_rel_bound = 0.5 * (mean_bound * rs[:, 0]) ** 2 + 16 * U
    return dict(ref=ref, mu=mu[:, 0], rs=rs[:, 0], bound=bound, mean_bound=mean_bound, rstd_rel_bound=rstd_rel_bound)


def ln_backward_reference(dy, x, gam, mean, rstd):
    """fp64 dx from the kernel's OWN saved mean / rstd (their error is bounded by the forward check and not charged again), and
    its per-element bound.  With g = dy * gamma, xh = (x - mean) * rstd, m1 = mean(g), m2 = mean(g * xh):
        dx = rstd * (g - m1 - xh * m2)
    m1 and m2 are 21-deep row sums: |d_m1| <= 23u * mean|g| (the rounding of g, the chain, the division) and
    |d_m2| <= 26u * mean|g * xh| (g, xh twice, the product, the chain, the division).  The elementwise roundings add
    3u|g| + 2u|m1| + 4u|xh * m2| inside the bracket and 3u|dx| outside:
        |dx - ref| <= rstd * (23u * mean|g| + 26u * |xh| * mean|g * xh| + 3u|g| + 2u|m1| + 4u|xh * m2|) + 3u * |ref|"""
    dyd, xd, g64 = dy.double(), x.double(), gam.double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    g = dyd * g64
    xh = (xd - mu) * rs
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    ref = rs * (g - m1 - xh * m2)
    bound = rs * (23 * U * g.abs().mean(1, keepdim=True) + 26 * U * xh.abs() * (g * xh).abs().mean(1, keepdim=True)
                  + 3 * U * g.abs() + 2 * U * m1.abs() + 4 * U * (xh * m2).abs()) + 3 * U * ref.abs()
    return ref, bound


def _wave_row_sum32(v):
    """fp32 row sums of v [rows, C] in the order of layernorm_fwd_kernel: lane l holds float4 j = l + 64 i (i < 4), adds
    (x + y) + (z + w) of each to its partial, then wave_sum's tree over the 64 lanes (neighbouring lanes first)."""
    rows, C = v.shape
    nv = C // 4
    lane = np.zeros((rows, 64), np.float32)
    for i in range(4):
        js = np.arange(64) + 64 * i
        live = js < nv
        if not live.any():
            break
        a = np.zeros((rows, 64, 4), np.float32)
        a[:, live] = v[:, : 4 * nv].reshape(rows, nv, 4)[:, js[live]]
        lane = lane + ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3]))
    w = lane
    while w.shape[1] > 1:
        w = w[:, 1::2] + w[:, 0::2]
    assert w.dtype == np.float32
    return w[:, 0]


def ln_emulate_fp32(x, gam, bet, eps, one_pass):
    """The forward kernel in NumPy fp32 (every operation rounded once, no FMA), with the two-pass variance it uses or with
    E[x^2] - E[x]^2 on the same sums.  Returns (y, mean, rstd)."""
    x, gam, bet = x.numpy(), gam.numpy(), bet.numpy()
    C = np.float32(x.shape[1])
    mu = (_wave_row_sum32(x) / C)[:, None]
    d = x - mu
    if one_pass:
        ex2 = (_wave_row_sum32(x * x) / C)[:, None]
        var = np.maximum(ex2 - mu * mu, np.float32(0))
    else:
        var = (_wave_row_sum32(d * d) / C)[:, None]
    rs = (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)
    y = d * rs * gam + bet
    assert y.dtype == np.float32
    return torch.from_numpy(y), torch.from_numpy(mu[:, 0].copy()), torch.from_numpy(rs[:, 0].copy())


@pytest.mark.parametrize("C", LN_WIDTHS)
def test_layernorm_bound_separates_two_pass_from_one_pass(C):
    """The forward bound of ln_forward_reference on the families and widths of the GPU test (63 rows: 21 of each family): the
    two-pass emulation uses less than half of it on every element, its mean and rstd meet their own bounds, and the one-pass
    emulation exceeds it at least 10x on both families with an offset.  0.5 and 10x are conditions on the bound, not tolerances of
    a kernel."""
    x, gam, bet, fam = ln_inputs(63, C, seed=1000 + C)
    R = ln_forward_reference(x, gam, bet, 1e-5)
    y2, mu2, rs2 = ln_emulate_fp32(x, gam, bet, 1e-5, one_pass=False)
    y1, _, _ = ln_emulate_fp32(x, gam, bet, 1e-5, one_pass=True)
    r2 = ((y2.double() - R["ref"]).abs() / R["bound"]).max(1).values
    r1 = ((y1.double() - R["ref"]).abs() / R["bound"]).max(1).values
    msg = f"C={C}: two-pass err/bound per family {[float(r2[fam == f].max()) for f in range(3)]}, one-pass {[float(r1[fam == f].max()) for f in range(3)]}"
    print(msg)
    assert float(r2.max()) < 0.5, msg
    for f in (1, 2):
        assert float(r1[fam == f].max()) > 10.0, msg
    assert bool(((mu2.double() - R["mu"]).abs() <= R["mean_bound"]).all()), msg
    assert bool(((rs2.double() / R["rs"] - 1).abs() <= R["rstd_rel_bound"]).all()), msg


def test_layernorm_backward_bound_holds_for_an_fp32_evaluation():
    """dx of the backward formula evaluated in plain fp32 (torch CPU, another summation order of the same depth class) stays inside
    ln_backward_reference's bound on all three families."""
    for C in (4, 260, 1024):
        x, gam, bet, _ = ln_inputs(9, C, seed=C)
        dy = torch.randn(9, C, generator=torch.Generator().manual_seed(C + 1))
        _, mean, rstd = ln_emulate_fp32(x, gam, bet, 1e-5, one_pass=False)
        ref, bound = ln_backward_reference(dy, x, gam, mean, rstd)
        g = dy * gam
        xh = (x - mean[:, None]) * rstd[:, None]
        dx = rstd[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
        ratio = float(((dx.double() - ref).abs() / bound).max())
        print(f"C={C}: fp32 dx err/bound {ratio:.3f}")
        assert ratio < 1.0, (C, ratio)


# ------------------------------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------------------------------
COLSUM_KINDS = ("f32", "det", "scaled")
COLSUM_SMALL_ROWS = (1, 2, 63, 64, 65, 127)
COLSUM_SMALL_COLS = (1, 255, 256, 257, 300)
COLSUM_SWITCH_ROWS = {"f32": (131072, 131073), "det": (16384, 16385), "scaled": (16384, 16385, 16641)}
COLSUM_TIER2 = ((8400, 300), (40007, 64))
COLSUM_MAX_EXACT_ROWS = 150000


def colsum_plan(kind, rows):
    """(rows per block, chunks) of the three column-sum launches, restated from the rules in csrc/rowops.hip: colsum_f32 doubles
    64 until at most 2048 chunks are left, colsum_det_f32 until at most 256, colsum_scaled takes max(64, ceil(rows / 256))."""
    if kind == "scaled":
        rpb = max(64, (rows + 255) // 256)
    else:
        cap = 2048 if kind == "f32" else 256
        rpb = 64
        while (rows + rpb - 1) // rpb > cap:
            rpb *= 2
    return rpb, (rows + rpb - 1) // rpb


def colsum_tol(kind, rows, out0, factor, x):
    """tol_c = 1.01 * (rpb + chunks + 2) * 2^-24 * (|out0_c| + |alpha * scale_c| * sum_r |x_rc|): rpb + chunks is the longest chain of
    additions a term passes through (one thread's serial sum, then the atomics or the ordered finish), + 2 for the products,
    1.01 for the second-order terms.  factor = alpha * scale_c (fp64 tensor or float), x the stored values [rows, cols]."""
    rpb, chunks = colsum_plan(kind, rows)
    factor = torch.as_tensor(factor, dtype=torch.float64)
    return 1.01 * (rpb + chunks + 2) * U * (out0.double().abs() + factor.abs() * x.double().abs().sum(0))


def colsum_int_inputs(rows, cols, ld, seed):
    """Tier 1: integers in [-8, 8] (exact in bf16) in a [rows, ld] matrix whose padding columns are NaN, small integers in out,
    power-of-two alpha and scale."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.full((rows, ld), float("nan"))
    x[:, :cols] = torch.randint(-8, 9, (rows, cols), generator=gen).float()
    out0 = torch.randint(-4, 5, (cols,), generator=gen).float()
    scale = 2.0 ** torch.randint(-2, 3, (cols,), generator=gen).float()
    return x, out0, scale, 0.5


def colsum_int_partial_bound(rows, alpha, scale, out0):
    """Largest absolute value any partial sum of the tier-1 data can reach: 8 per row, the factor, the initial value."""
    return 8.0 * rows * abs(alpha) * float(scale.abs().max()) + float(out0.abs().max())


def _colsum_emulate(kind, x, out0, factor, perm):
    """fp32 emulation: each chunk summed serially by one thread (two interleaved partials for colsum_f32 / colsum_det_f32, as
    the kernels do), then the chunks combined in the order `perm`: atomically into out (f32, scaled) or summed first (det)."""
    rows, cols = x.shape
    rpb, chunks = colsum_plan(kind, rows)
    xp = np.zeros((chunks * rpb, cols), np.float32)
    xp[:rows] = x.numpy()
    xp = xp.reshape(chunks, rpb, cols)
    if kind == "scaled":
        part = np.add.accumulate(xp, axis=1, dtype=np.float32)[:, -1]
    else:
        part = np.add.accumulate(xp[:, 0::2], axis=1, dtype=np.float32)[:, -1] + np.add.accumulate(xp[:, 1::2], axis=1, dtype=np.float32)[:, -1]
    f = np.broadcast_to(np.asarray(factor, np.float32), (cols,))
    out = out0.numpy().astype(np.float32).copy()
    if kind == "det":
        s = np.zeros(cols, np.float32)
        for k in range(chunks):
            s = s + part[k]
        return torch.from_numpy(out + f * s)
    for k in perm:
        out = out + f * part[k]
    return torch.from_numpy(out)


@pytest.mark.parametrize("rows,cols", COLSUM_TIER2)
@pytest.mark.parametrize("kind", COLSUM_KINDS)
def test_colsum_bound_holds_and_sees_a_lost_row(kind, rows, cols):
    """Tier 2 (randn data, fp64 reference of the stored values): the emulated launch stays inside tol_c for two chunk orders.
    Losing one row, or adding one twice, is outside tol_c in at least one column at 8,400 x 300 for all three kernels (asserted:
    34 x tol_c in the worst column).  At 40,007 x 64 the bound has grown with the row count (about 1.3 for colsum_f32 against
    |x| < 5): only the largest entries of the row leave it (1.6 to 2.6 x tol_c in the worst column, printed, not asserted) and
    most columns hide the fault -- there the exact tier-1 cases of the GPU test are what catches a lost row."""
    gen = torch.Generator().manual_seed(rows + cols)
    x = torch.randn(rows, cols, generator=gen)
    out0 = torch.randn(cols, generator=gen)
    alpha = 0.5
    scale = (torch.rand(cols, generator=gen) + 0.5) if kind == "scaled" else torch.ones(cols)
    factor = (alpha if kind != "scaled" else 1.0) * scale
    ref = out0.double() + factor.double() * x.double().sum(0)
    tol = colsum_tol(kind, rows, out0, factor.double(), x)
    _, chunks = colsum_plan(kind, rows)
    rng = np.random.default_rng(rows)
    worst = 0.0
    for perm in (np.arange(chunks), rng.permutation(chunks)):
        got = _colsum_emulate(kind, x, out0, factor, perm)
        worst = max(worst, float(((got.double() - ref).abs() / tol).max()))
    r = rows // 2 + 1
    lost = _colsum_emulate(kind, torch.cat([x[:r], x[r + 1:]]), out0, factor, np.arange(colsum_plan(kind, rows - 1)[1]))
    twice = _colsum_emulate(kind, torch.cat([x, x[r:r + 1]]), out0, factor, np.arange(colsum_plan(kind, rows + 1)[1]))
    seen = [float(((t.double() - ref).abs() / tol).max()) for t in (lost, twice)]
    msg = f"{kind} {rows}x{cols}: emulation err/tol {worst:.3f}; row lost {seen[0]:.2f}, row twice {seen[1]:.2f} (x tol)"
    print(msg)
    assert worst < 1.0, msg
    if (rows, cols) == (8400, 300):
        assert min(seen) > 1.0, msg


def test_colsum_exact_tier_stays_below_2_to_24():
    """Every listed row count of tier 1 keeps |partial sums| < 2^24 with the largest scale (4) and alpha 0.5, so that every
    summation order gives the same fp32 bits and the GPU test may assert equality with an int64 reference."""
    for kind in COLSUM_KINDS:
        for rows in COLSUM_SMALL_ROWS + COLSUM_SWITCH_ROWS[kind]:
            assert rows <= COLSUM_MAX_EXACT_ROWS
            _, out0, scale, alpha = colsum_int_inputs(2, 8, 8, seed=rows)
            assert float(scale.max()) <= 4.0 and float(scale.min()) >= 0.25
            assert colsum_int_partial_bound(rows, alpha, torch.tensor([4.0]), out0) < 2 ** 24, (kind, rows)
    assert colsum_plan("f32", 131072) == (64, 2048) and colsum_plan("f32", 131073) == (128, 1025)
    assert colsum_plan("det", 16384) == (64, 256) and colsum_plan("det", 16385) == (128, 129)
    assert colsum_plan("scaled", 16384)[0] == 64 and colsum_plan("scaled", 16385)[0] == 65 and colsum_plan("scaled", 16641)[0] == 66


# ------------------------------------------------------------------------------------------------------------------------
# fp32 -> bf16, round to nearest even
# ------------------------------------------------------------------------------------------------------------------------
# (fp32 bits, bf16 bits worked out by hand)
BF16_TIES = (
    (0x3F808000, 0x3F80), (0xBF808000, 0xBF80),      # exact tie, kept mantissa even: stays
    (0x3F818000, 0x3F82), (0xBF818000, 0xBF82),      # exact tie, kept mantissa odd: up to the even neighbour
    (0x3F808001, 0x3F81), (0xBF808001, 0xBF81),      # one bit above a tie
    (0x3F817FFF, 0x3F81), (0xBF817FFF, 0xBF81),      # one bit below a tie
    (0x3FFFFFFF, 0x4000), (0xBFFF8000, 0xC000),      # mantissa of all ones: the carry runs into the exponent (also as a tie)
    (0x7F7FFFFF, 0x7F80), (0xFF7FFFFF, 0xFF80),      # the largest finite fp32 rounds to infinity
    (0x00000000, 0x0000), (0x80000000, 0x8000),      # signed zeros
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),      # infinities
    (0x3F800000, 0x3F80), (0xC0490FDB, 0xC049),      # 1, -pi (below the tie)
    (0x00800000, 0x0080), (0x00FF8000, 0x0100),      # the smallest normal; a tie just above it
)
BF16_NANS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF)       # 0x7F800001: truncating its low bits would give infinity
BF16_DENORMALS = (0x00000001, 0x00008000, 0x00018000, 0x00400000, 0x007FFFFF, 0x80000001, 0x80018000, 0x807FFFFF)


def f32_from_bits(bits):
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def bf16_bits(t):
    return t.contiguous().view(torch.int16)


def bf16_expected(bits):
    return torch.from_numpy(np.array(bits, dtype=np.uint16).view(np.int16).copy())


def test_bf16_ties_vector_is_what_round_to_nearest_even_gives():
    assert len(BF16_TIES) % 4 == 0 and len(BF16_NANS) % 4 == 0 and len(BF16_DENORMALS) % 4 == 0
    src, want = [b for b, _ in BF16_TIES], [w for _, w in BF16_TIES]
    rne = [((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF for b in src]           # the integer form of RNE
    assert rne == want
    assert torch.equal(bf16_bits(f32_from_bits(src).to(torch.bfloat16)), bf16_expected(want))
    assert bool(torch.isnan(f32_from_bits(BF16_NANS).to(torch.bfloat16).float()).all())
    den = f32_from_bits(BF16_DENORMALS).to(torch.bfloat16)
    assert torch.equal(bf16_bits(den), bf16_expected([((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF for b in BF16_DENORMALS]))


# ------------------------------------------------------------------------------------------------------------------------
# pooling: the tap loops, vectorised over the pixels
# ------------------------------------------------------------------------------------------------------------------------
def pool_fwd_taps(x):
    """3x3 / stride-2 max pool of the zero-padded NHWC map, the first maximal tap in (kh, kw) order wins: (y, argmax byte)."""
    N, H, W, C = x.shape
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    xp = np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, C), x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    best = np.full((N, Ho, Wo, C), -np.inf, x.dtype)
    am = np.zeros((N, Ho, Wo, C), np.uint8)
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]
            up = v > best
            best = np.where(up, v, best)
            am[up] = kh * 3 + kw
    return best, am


def pool_bwd_taps(dy, am, x):
    """tests/test_gpu_pool_bwd_windows.py::_reference with the loop over the pixels turned into slices: for every tap, in the
    same kh-major order, the windows ho = (h + 1 - kh) / 2 that exist add their dy where their argmax is that tap."""
    N, H, W, C = x.shape
    _, Ho, Wo, _ = dy.shape
    g = np.zeros_like(x)
    for kh in range(3):
        ho = np.arange(Ho)
        ho = ho[(2 * ho + kh - 1 >= 0) & (2 * ho + kh - 1 < H)]
        for kw in range(3):
            wo = np.arange(Wo)
            wo = wo[(2 * wo + kw - 1 >= 0) & (2 * wo + kw - 1 < W)]
            if len(ho) == 0 or len(wo) == 0:
                continue
            hs, ws = slice(2 * ho[0] + kh - 1, 2 * ho[-1] + kh, 2), slice(2 * wo[0] + kw - 1, 2 * wo[-1] + kw, 2)
            os_ = (slice(None), slice(ho[0], ho[-1] + 1), slice(wo[0], wo[-1] + 1))
            sel = am[os_] == kh * 3 + kw
            g[:, hs, ws] = np.where(sel, g[:, hs, ws] + dy[os_], g[:, hs, ws])
    return np.where(x > 0, g, x.dtype.type(0))


@pytest.mark.parametrize("H,W", [(7, 9), (8, 10), (1, 1), (2, 3), (1, 6), (5, 1)])
def test_vectorised_pool_references_equal_the_loops(H, W):
    from test_gpu_pool_bwd_windows import _inputs, _reference
    x, dy, Ho, Wo = _inputs(2, H, W, 8, seed=H * 10 + W)
    y, am = pool_fwd_taps(x.numpy())
    want = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1)
    assert np.array_equal(y, want.numpy())
    kh, kw = am // 3, am % 3                          # the argmax points at a tap that holds the maximum, and at the first such tap
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 2, 1, 2)).permute(0, 2, 3, 1).numpy()
    n, ho, wo, c = np.meshgrid(np.arange(2), np.arange(Ho), np.arange(Wo), np.arange(8), indexing="ij")
    assert np.array_equal(xp[n, 2 * ho + kh, 2 * wo + kw, c], y)
    for t in range(9):
        earlier = (t < am) & (xp[n, 2 * ho + t // 3, 2 * wo + t % 3, c] == y)
        assert not earlier.any()
    assert pool_bwd_taps(dy.numpy(), am, x.numpy()).tobytes() == _reference(dy.numpy(), am, x.numpy()).tobytes()
