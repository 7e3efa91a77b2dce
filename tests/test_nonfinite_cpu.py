"""What tests/test_gpu_nonfinite.py rests on, checked without a GPU: every case of tests/nonfinite_cases.py builds its poisoned inputs and
its fp64 reference, the reference holds the non-finite elements the case is about but never more than a quarter of an output (so the
finite remainder, which keeps the family's tolerance, is never empty), the GEMM cases reach the kernel family they state (the library's
routing is host arithmetic on the descriptor), and assert_same_nonfinite rejects each way of breaking the contract."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_band_cases as G                  # noqa: E402
import nonfinite_cases as NF                  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from detr_tf import _hip
    return _hip, _hip.load()


def capped(ref, what, need=("nan",)):
    """A reference output: holds what the case plants, at most a quarter non-finite, a finite remainder."""
    ref = ref.double()
    s = NF.share(ref)
    assert 0.0 < s <= NF.CAP, f"{what}: {s:.3f} of the reference is non-finite"
    assert bool(torch.isfinite(ref).any())
    if "nan" in need:
        assert bool(torch.isnan(ref).any()), what + ": no NaN in the reference"
    if "pinf" in need:
        assert bool((ref == NF.INF).any()), what + ": no +Inf in the reference"
    if "ninf" in need:
        assert bool((ref == -NF.INF).any()), what + ": no -Inf in the reference"


def _family(lib, c, ws_bytes=0):
    _hip, L = lib
    d = G.fill_desc(_hip, c, G.placeholder_ptrs(c), dropout_step=0xC0000000, workspace=0xD0000000 if ws_bytes else None, workspace_bytes=ws_bytes)
    fam = L.detr_hip_gemm_family(ctypes.byref(d))
    return d, fam, (L.detr_hip_last_error().decode() if fam < 0 else "")


def test_gemm_forward_cases_route_and_keep_the_cap(lib):
    cases = NF.gemm_forward_cases()
    assert {c["family"] for c, _ in cases} == {0, 1, 2, 3, 4}
    assert {c["act"] for c, _ in cases} == {0, 1, 2}
    assert len({G.case_id(c) for c, _ in cases}) == len(cases)
    for fam in range(4):                                        # every family with an activation switch runs with and without the ReLU
        assert {c["act"] for c, _ in cases if c["family"] == fam} >= {0, 1}, fam
    assert any(c["mask"] == "bits" for c, _ in cases) and any(c["mask"] in ("f32", "b16") for c, _ in cases)
    for c, poison in cases:
        with G.tuning(lib[0], c["env"]):
            _, fam, err = _family(lib, c)
        assert fam == c["family"], f"{G.case_id(c)}: family {fam}, stated {c['family']} {err}"
        v, vr = NF.gemm_poisoned(c, poison)
        for name, ref in NF.gemm_refs(c, v, vr).items():
            need = ("nan",) if (c["compute"] == 2 or c["act"] == 2 or c["ln"] is not None or name != "C") else ("nan", "pinf")
            capped(ref, f"{G.case_id(c)} {name}", need)
        if c["mask"]:                                          # the NaN row of A meets the mask on both sides, stored as values or as bits
            row = NF.gemm_poison_places(c)["a_nan"][0]
            on = G.unpack_bits(v["mask"], c["N"])[row] if c["mask"] == "bits" else v["mask"][row] > 0
            assert bool(on.any()) and bool((~on).any()), G.case_id(c)


def test_relu_cases_hold_a_nan_the_old_maximum_would_have_lost(lib):
    """In every ReLU case the reference keeps NaN behind the activation: fmaxf(NaN, 0) = 0 there is what the cases are for."""
    n = 0
    for c, poison in NF.gemm_forward_cases():
        if c["act"] == 1:
            v, vr = NF.gemm_poisoned(c, poison)
            assert bool(torch.isnan(NF.gemm_refs(c, v, vr)["C"]).any()), G.case_id(c)
            n += 1
    assert n >= 10


def test_split_cases_route_and_keep_the_cap(lib):
    _hip, L = lib
    cases = NF.split_cases()
    assert {c["family"] for c in cases} == {0, 5}
    for c in cases:
        with G.tuning(_hip, c["env"]):
            d, _, _ = _family(lib, c)
            query = int(L.detr_hip_workspace_bytes_gemm(ctypes.byref(d)))
            assert query >= G.split_floor_bytes(c) > 0
            _, fam, err = _family(lib, c, query)
            assert fam == c["family"], (G.case_id(c), fam, err)
        P = NF.gemm_poison_places(c)
        assert P["a_pinf"][1] >= c["K"] - c["K"] // c["split"] and P["b_nan"][0] < c["K"]      # +Inf at a k of the last slab
        v, vr = NF.gemm_poisoned(c, ("A", "B"))
        for name, ref in NF.gemm_refs(c, v, vr).items():
            capped(ref, f"{G.case_id(c)} {name}", ("nan", "pinf", "ninf") if name == "rowsum_a" else ("nan", "pinf"))
    for c in NF.group_members():
        v, vr = NF.gemm_poisoned(c, ("A", "B"))
        for name, ref in NF.gemm_refs(c, v, vr).items():
            capped(ref, f"group {G.case_id(c)} {name}")


def test_fused_1x1_backward_case():
    P = NF.bwd_fused_problem(33)
    capped(P["da"], "da", ("nan", "pinf", "ninf"))
    capped(P["dw"], "dw", ("nan", "pinf", "ninf"))
    assert int(torch.isnan(P["dw"]).all(0).sum()) == 1          # one whole column


@pytest.mark.parametrize("c", NF.conv_cases(), ids=lambda c: c["id"])
def test_conv_cases(c):
    P = NF.conv_poisoned(c)
    R = NF.conv_refs(c, P)
    x3 = c["compute"] == 2
    capped(R["y"], c["id"] + " y", ("nan",) if x3 else ("nan", "pinf"))
    capped(R["dx"], c["id"] + " dx")
    z = P["z"]
    N, Ho, Wo, Co = z.shape
    # the NaN weight: its whole output channel, border pixels included (0 * NaN on the explicit zero padding)
    assert bool(torch.isnan(z[..., Co - 1]).all())
    # a NaN pixel: at most 9 output pixels, across all output channels; the corner pixel fewer (its window is cut by the border)
    hit = torch.isnan(z[0, :, :, :Co - 1]).all(-1)
    assert bool((torch.isnan(z[0, :, :, :Co - 1]).any(-1) == hit).all())
    assert 2 <= int(hit.sum()) <= 9 + 4
    assert not bool(torch.isnan(z[1, :, :, :Co - 1]).any()) or x3


@pytest.mark.parametrize("c", NF.wgrad_cases(), ids=lambda c: c["id"])
def test_conv_weight_gradient_cases(c):
    P = NF.conv_poisoned(c)
    s = NF.share(P["dw"])
    assert 0.0 < s <= NF.CAP, (c["id"], s)


def test_stem_cases():
    for low in (False, True):
        P = NF.stem_poisoned(NF.STEM_SHAPE, low)
        capped(torch.relu(P["z"] + P["shift"].double()), "stem forward", ("nan", "pinf"))
        W = NF.stem_wgrad_poisoned(NF.STEM_SHAPE_WGRAD, low)
        capped(W["dw"], "stem weight gradient", ("nan", "pinf", "ninf"))
    capped(torch.relu(NF.stem_poisoned(NF.STEM_SHAPE, False, x3=True)["z"]), "stem forward x3")


@pytest.mark.parametrize("kind,C", NF.POOL_CASES)
def test_pool_cases(kind, C):
    P = NF.pool_problem(C)
    capped(P["y"], "pool", ("nan", "pinf"))
    y, x = P["y"], P["x"]
    nan_windows = [(n, ho, wo, c) for n, ho, wo, c in torch.isnan(y).nonzero().tolist()]
    touching = [w for w in nan_windows if w[1] == 0 or w[2] == 0]
    assert touching and len(touching) < len(nan_windows)        # windows that touch the zero padding and windows that do not
    for n, ho, wo, c in nan_windows:
        assert any(np.isnan(t) for t in NF.pool_window(x, n, ho, wo, c))
    assert any(sum(np.isnan(t) for t in NF.pool_window(x, *w)) == 2 for w in nan_windows)      # two NaN taps in one window


@pytest.mark.parametrize("op", NF.ROW_OPS)
def test_row_cases(op):
    P = NF.row_problem(op)
    for k in [k for k in P if k.startswith("ref")]:
        capped(P[k], f"{op} {k}", ("nan",))
    if op == "dropout":
        a, keep = P["a"], P["keep"]
        assert bool((torch.isnan(a) & ~keep).any()) and bool((torch.isnan(a) & keep).any())


@pytest.mark.parametrize("C,rows", NF.LN_CASES)
def test_layernorm_cases(C, rows):
    P = NF.layernorm_problem(C, rows)
    for k in ("y", "y2", "dx"):
        bad = torch.isnan(P[k]).all(1)
        assert int(bad.sum()) == 3 and bool((torch.isnan(P[k]).any(1) == bad).all()), k      # three whole rows, nothing else
        assert not bool(torch.isinf(P[k]).any())
    assert int(torch.isnan(P["mean"]).sum()) == 1 and int(torch.isinf(P["mean"]).sum()) == 2
    assert int(torch.isnan(P["rstd"]).sum()) == 3
    # dgamma = sum over the rows of dy * xhat: NaN in every column; dbeta = sum of dy does not read x and stays finite
    assert bool(torch.isnan(P["dgamma"]).all()) and bool(torch.isfinite(P["dbeta"]).all())
    Q = NF.layernorm_problem(C, rows, poison_dy=True)
    assert int(torch.isnan(Q["dx"]).all(1).sum()) == 3 and bool(torch.isfinite(Q["y"]).all())
    capped(Q["dbeta"], "dbeta")
    capped(Q["dgamma"], "dgamma")


@pytest.mark.parametrize("special", [s for s, _ in NF.OPT_SPECIALS])
def test_optimiser_cases(special):
    val = dict(NF.OPT_SPECIALS)[special]
    # per tensor: the whole 4097-element tensor for a NaN (its norm is NaN), one element for an Inf (the factor is 0, Inf * 0 = NaN)
    P = NF.optimiser_problem(val, joint=False)
    bad = [int((~np.isfinite(P["p"][i])).sum()) for i in range(len(NF.OPT_SIZES))]
    assert bad == [0, 0, 0, 0, 4097 if special == "nan" else 1, 0]
    # joint: every trained tensor for a NaN; with group 1 untrained the special is not part of the step at all
    P = NF.optimiser_problem(val, joint=True)
    bad = [int((~np.isfinite(P["p"][i])).sum()) for i in range(len(NF.OPT_SIZES))]
    assert bad == (list(NF.OPT_SIZES) if special == "nan" else [0, 0, 0, 0, 1, 0])
    assert np.isnan(P["s"]) == (special == "nan") and not np.isfinite(P["G"])
    P = NF.optimiser_problem(val, joint=True, trained=(True, False, True))
    assert all(np.isfinite(P["p"][i]).all() for i in range(len(NF.OPT_SIZES))) and np.isfinite(P["G"])


@pytest.mark.parametrize("case,masked", NF.ATT_CASES)
def test_attention_cases(case, masked):
    q, k, v, do, kv = NF.attention_problem(case, masked)
    for mult in (NF.ATT_HD ** -0.5, 0.6931471805599453):
        ref = NF.attention_reference(q, k, v, do, kv, mult)
        for name in ("o", "dq", "dk", "dv", "w", "lse"):
            s = NF.share(ref[name])
            assert s <= NF.CAP, (case, name, s)
            assert (s > 0.0) == (case != "masked_k_nan" and not (case == "v_nan" and name in ("dv", "w", "lse"))), (case, name, s)
        if case == "k_pinf":                   # both kinds of query row: +Inf score (NaN row) and -Inf score (finite, the key at weight 0)
            rows = torch.isnan(ref["o"][1, :, 3 * NF.ATT_HD])
            assert bool(rows.any()) and not bool(rows.all()) and bool(torch.isfinite(ref["o"][1][~rows]).all())
    if kv is not None:
        assert bool(torch.isfinite(v[~kv]).all()) and bool((v[~kv].abs().sum(1) > 0).all())


# ------------------------------------------------------------------------------------------------------------------------
# the comparison itself
# ------------------------------------------------------------------------------------------------------------------------
def test_assert_same_nonfinite_rejects_every_breach():
    ref = torch.tensor([1.0, NF.NAN, NF.INF, -NF.INF, 2.0, -3.0], dtype=torch.float64)
    NF.assert_same_nonfinite(ref.float(), ref, "f32", "identical")
    for i, val, why in ((1, 0.0, "NaN swallowed"), (1, -NF.INF, "NaN turned into -Inf"), (2, -NF.INF, "wrong sign"), (3, NF.NAN, "Inf turned into NaN"),
                        (0, NF.NAN, "a finite element poisoned"), (4, NF.INF, "a finite element overflowed"), (5, -3.01, "finite remainder off")):
        got = ref.clone().float()
        got[i] = val
        with pytest.raises(AssertionError):
            NF.assert_same_nonfinite(got, ref, "f32", why)
    with pytest.raises(AssertionError):
        NF.assert_same_nonfinite(torch.tensor([NF.NAN]), torch.tensor([NF.NAN]), "f32", "nothing finite")
