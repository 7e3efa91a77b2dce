"""CPU self-test of oracle/attn_bounds.py, the per-element error bounds the bf16 attention GPU tests check against: a simulated kernel
that rounds where the kernels document rounding (bf16 P before PV, l from the unrounded p, per-run maxima merged, bf16 dS and outputs,
delta from the bf16 O) must be ACCEPTED, and the same simulation with one subtle fault injected must be REJECTED -- the evidence that
the bounds are tight enough to catch a dropped key tile, a leak across batch elements, a few-percent weighting error or a wrong delta."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import attn_bounds as AB
from oracle import dropout_ref as DR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as AC                    # noqa: E402

H, HD = 8, 32
D = H * HD
SCALE = HD ** -0.5
LOG2E = 1.4426950408889634


def operands(B, T, S, p, seed):
    """The distribution of tests/test_gpu_attention_dma.py::_run (stored q in log2 units, bf16 everywhere) and its keep mask."""
    g = torch.Generator().manual_seed(seed)
    qs = AB.bf16(torch.randn(B, T, D, dtype=torch.float64, generator=g) * 2.0 * (SCALE * LOG2E))
    k = AB.bf16(torch.randn(B, S, D, dtype=torch.float64, generator=g))
    v = AB.bf16(torch.randn(B, S, D, dtype=torch.float64, generator=g))
    do = AB.bf16(torch.randn(B, T, D, dtype=torch.float64, generator=g))
    keep = None
    if p > 0.0:
        keep = torch.from_numpy(DR.keep_mask(DR.drop_key(77, 0xBEEF1234), DR.attn_index(B * H, T, S), p))
    return qs, k, v, do, keep


def ratios(sim, qs, k, v, do, keep, p):
    fw = AB.forward(qs, k, v, H, keep, p)
    bw = AB.backward(qs, k, v, do, sim["o"], H, keep, p)
    return dict(o=AB.ratio(sim["o"], fw["o"], fw["bound_o"]), lse=AB.ratio(sim["lse"], fw["lse"], fw["bound_lse"]),
                dq=AB.ratio(sim["dq"], bw["dq"], bw["bound_dq"]), dk=AB.ratio(sim["dk"], bw["dk"], bw["bound_dk"]),
                dv=AB.ratio(sim["dv"], bw["dv"], bw["bound_dv"]))


_CACHE = {}


def _case(B, T, S, p, seed):
    key = (B, T, S, p, seed)
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = operands(B, T, S, p, seed)
    return _CACHE[key]


@pytest.mark.parametrize("B,T,S,p", [(2, 1050, 1050, 0.1), (2, 1050, 1050, 0.0), (2, 70, 333, 0.1)])
@pytest.mark.parametrize("split", [0, 8])
def test_bounds_accept_the_documented_roundings(B, T, S, p, split):
    qs, k, v, do, keep = _case(B, T, S, p, 3)
    parts = AB.parts_for(-(-S // 32), split)
    sim = AB.simulate(qs, k, v, do, H, keep, p, parts=parts)
    r = ratios(sim, qs, k, v, do, keep, p)
    print(f"accept B{B} T{T} S{S} p{p} parts{parts}: " + " ".join(f"{n} {x:.3f}" for n, x in r.items()))
    for n, x in r.items():
        assert x <= 1.0, f"{n}: a correctly rounded result exceeds its bound ({x:.3f})"
    # the bf16 terms carry the bound: a correctly rounded result uses a visible part of it (not a loose, vacuous bound)
    assert max(r["o"], r["dq"], r["dk"], r["dv"]) >= 0.05, r


REJECT = [
    # (name, shape, fault, outputs that must flag it)
    ("tile omitted", (2, 1050, 1050, 0.1), ("drop_tile", 3, 5), ("o", "lse")),
    ("ragged padding keys from the next batch element", (2, 70, 333, 0.1), ("pad_from_next", 2), ("o", "lse")),
    ("one 32-query chain's P x (1 + 2^-6)", (2, 1050, 1050, 0.1), ("chain_scale", 9, 32), ("o",)),
    ("delta off by 1 %", (2, 1050, 1050, 0.1), ("delta", 4), ("dq", "dk")),
    ("merged run weighted 2^(+1/16)", (2, 1050, 1050, 0.1), ("merge", 6, 1, 2.0 ** (1.0 / 16)), ("o", "lse")),
    ("merged run weighted 2^(-1/16)", (2, 1050, 1050, 0.0), ("merge", 1, 2, 2.0 ** (-1.0 / 16)), ("o", "lse")),
]


@pytest.mark.parametrize("name,shape,fault,flags", REJECT, ids=[r[0] for r in REJECT])
def test_bounds_reject_subtle_faults(name, shape, fault, flags):
    B, T, S, p = shape
    qs, k, v, do, keep = _case(B, T, S, p, 3)
    sim = AB.simulate(qs, k, v, do, H, keep, p, parts=AB.parts_for(-(-S // 32)), fault=fault)
    r = ratios(sim, qs, k, v, do, keep, p)
    print(f"reject [{name}]: " + " ".join(f"{n} {x:.3g}" for n, x in r.items()))
    for n in flags:
        assert r[n] > 1.0, f"{name}: {n} within its bound ({r[n]:.3f}) -- the check would miss this fault"


def test_bounds_uniform_scores_closed_form():
    """q = 0: O is the mean of V over the kept keys (scaled), lse = log S exactly; the reference agrees to fp64 rounding."""
    B, T, S, p = 1, 40, 333, 0.1
    _, k, v, do, keep = operands(B, T, S, p, 9)
    qs = torch.zeros(B, T, D, dtype=torch.float64)
    fw = AB.forward(qs, k, v, H, keep, p)
    assert torch.allclose(fw["lse"], torch.full_like(fw["lse"], float(np.log(S))), rtol=0, atol=1e-12)
    kh = keep.double().view(B, H, T, S)
    want = torch.einsum("bhts,bshd->bthd", kh, v.view(B, S, H, HD)).reshape(B, T, D) / (S * (1.0 - p))
    assert torch.allclose(fw["o"], want, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------------------
# key padding masks (the MASK instantiations): masked keys exactly absent, exact-zero dK / dV, faults a masked kernel could make
# ------------------------------------------------------------------------------------------------------------------------------
def _masked_ratios(sim, qs, k, v, do, keep, p, kv):
    fw = AB.forward(qs, k, v, H, keep, p, key_valid=kv)
    bw = AB.backward(qs, k, v, do, sim["o"], H, keep, p, key_valid=kv)
    return dict(o=AB.ratio(sim["o"], fw["o"], fw["bound_o"]), lse=AB.ratio(sim["lse"], fw["lse"], fw["bound_lse"]),
                dq=AB.ratio(sim["dq"], bw["dq"], bw["bound_dq"]), dk=AB.ratio(sim["dk"], bw["dk"], bw["bound_dk"]),
                dv=AB.ratio(sim["dv"], bw["dv"], bw["bound_dv"]))


@pytest.mark.parametrize("B,T,S", [(2, 1050, 1050), (2, 70, 333)])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["rect", "random"])
@pytest.mark.parametrize("split", [0, 8])
def test_masked_bounds_accept_the_documented_roundings(B, T, S, p, kind, split):
    qs, k, v, do, keep = _case(B, T, S, p, 3)
    parts = AB.parts_for(-(-S // 32), split)
    kv = torch.from_numpy(AC.key_valid(kind, B, S, parts, seed=1))
    sim = AB.simulate(qs, k, v, do, H, keep, p, parts=parts, key_valid=kv)
    for n in ("dk", "dv"):
        assert bool((sim[n][~kv] == 0).all()), f"simulated {n} not exactly 0 at masked keys"
    r = _masked_ratios(sim, qs, k, v, do, keep, p, kv)
    print(f"accept masked {kind} B{B} T{T} S{S} p{p} parts{parts}: " + " ".join(f"{n} {x:.3f}" for n, x in r.items()))
    for n, x in r.items():
        assert x <= 1.0, f"{n}: a correctly rounded masked result exceeds its bound ({x:.3f})"
    assert max(r["o"], r["dq"], r["dk"], r["dv"]) >= 0.05, r


def _partial_tiles(kv_row, S):
    """Tiles (not the ragged last one) whose word is neither all-valid nor all-masked."""
    out = []
    for t in range(S // 32):
        n = int(kv_row[32 * t:32 * t + 32].sum())
        if 0 < n < 32:
            out.append(t)
    return out


def _fault_for(name, kv, S):
    """The concrete fault of a kind, on problem bh = 3 (batch element 0, head 3), at the first tile / key where it changes something."""
    bh, row = 3, kv[0]
    tiles = _partial_tiles(row, S)
    if name == "leak_key":
        t = tiles[0]
        j = 32 * t + int((~row[32 * t:32 * t + 32]).nonzero()[0])
        return ("leak_key", bh, j)
    if name == "mask_shift":
        return ("mask_shift", bh, tiles[0])
    if name == "mask_half":
        i = torch.arange(32)
        for t in tiles:
            w = row[32 * t:32 * t + 32]
            if not torch.equal(torch.where(AB._lane_half(i) == 1, w[(i - 4) % 32], w), w):
                return ("mask_half", bh, t)
    if name == "word_from":
        t = tiles[1]
        for u in (t + 1, t - 1, t + 2):
            if not torch.equal(row[32 * t:32 * t + 32], row[32 * u:32 * u + 32]):
                return ("word_from", bh, t, u)
    if name == "masked_dkv":
        return ("masked_dkv", bh)
    raise AssertionError(name)


MASK_REJECT = [
    # (fault kind, mask kind, p, outputs that must flag it)
    ("leak_key", "rect", 0.1, ("lse",)),
    ("leak_key", "random", 0.0, ("lse",)),
    ("mask_shift", "rect", 0.1, ("o", "lse")),
    ("mask_shift", "random", 0.0, ("o", "lse")),
    ("mask_half", "rect", 0.1, ("o", "lse")),
    ("mask_half", "random", 0.0, ("o", "lse")),
    ("word_from", "rect", 0.0, ("o", "lse")),
    ("word_from", "random", 0.1, ("o", "lse")),
    ("masked_dkv", "rect", 0.1, ("dk", "dv")),
]


@pytest.mark.parametrize("name,kind,p,flags", MASK_REJECT, ids=[f"{r[0]}-{r[1]}-p{r[2]}" for r in MASK_REJECT])
def test_masked_bounds_reject_mask_faults(name, kind, p, flags):
    B, T, S = 2, 1050, 1050
    qs, k, v, do, keep = _case(B, T, S, p, 3)
    parts = AB.parts_for(-(-S // 32))
    kv = torch.from_numpy(AC.key_valid(kind, B, S, parts, seed=1))
    fault = _fault_for(name, kv, S)
    sim = AB.simulate(qs, k, v, do, H, keep, p, parts=parts, fault=fault, key_valid=kv)
    r = _masked_ratios(sim, qs, k, v, do, keep, p, kv)
    print(f"reject masked [{fault} {kind} p{p}]: " + " ".join(f"{n} {x:.3g}" for n, x in r.items()))
    for n in flags:
        assert r[n] > 1.0, f"{fault}: {n} within its bound ({r[n]:.3f}) -- the check would miss this fault"


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_masked_bounds_ignore_masked_content(p):
    """Values and bounds with +-1e4 garbage in the masked K / V rows equal, bit for bit, those with zero-filled masked rows."""
    B, T, S = 2, 70, 333
    qs, k, v, do, keep = operands(B, T, S, p, 4)
    kv = torch.from_numpy(AC.key_valid("random", B, S, seed=2))
    inv = (~kv).unsqueeze(2)
    g = torch.Generator().manual_seed(5)
    junk = lambda: AB.bf16(torch.where(torch.rand(B, S, D, dtype=torch.float64, generator=g) < 0.5, -1.0e4, 1.0e4))
    runs = []
    for kx, vx in ((k.masked_fill(inv, 0.0), v.masked_fill(inv, 0.0)), (torch.where(inv, junk(), k), torch.where(inv, junk(), v))):
        fw = AB.forward(qs, kx, vx, H, keep, p, key_valid=kv)
        bw = AB.backward(qs, kx, vx, do, AB.bf16(fw["o"]), H, keep, p, key_valid=kv)
        runs.append({**fw, **bw})
    for n, x in runs[0].items():
        assert torch.equal(x, runs[1][n]), f"{n} depends on the content of masked rows"


def test_masked_bounds_uniform_scores_closed_form():
    """q = 0 with a mask: lse = log(n_valid) of each image, O = the keep-scaled mean of its valid V."""
    B, T, S, p = 2, 40, 333, 0.1
    _, k, v, do, keep = operands(B, T, S, p, 9)
    kv = torch.from_numpy(AC.key_valid("random", B, S, seed=3))
    qs = torch.zeros(B, T, D, dtype=torch.float64)
    fw = AB.forward(qs, k, v, H, keep, p, key_valid=kv)
    n = kv.sum(dim=1).double()                                                    # [B]
    want_lse = torch.log(n).repeat_interleave(H).unsqueeze(1).expand(B * H, T)
    assert torch.allclose(fw["lse"], want_lse, rtol=0, atol=1e-12)
    kh = keep.view(B, H, T, S).double() * kv.view(B, 1, 1, S).double()
    want = torch.einsum("bhts,bshd->bthd", kh, v.view(B, S, H, HD)).reshape(B, T, D) / (n.view(B, 1, 1) * (1.0 - p))
    assert torch.allclose(fw["o"], want, rtol=0, atol=1e-12)
