"""What tests/test_gpu_storage_matrix.py rests on, checked without a GPU: every storage case of tests/guard_band_cases.py reaches the
kernel family it states, the case lists cover EVERY storage form detr_hip_gemm_family accepts (a form the library takes and no case
runs fails here), the entry point rejects what include/detr_hip.h does not document, and NumPy models of two wrong epilogues -- a
double rounding and a residual read at C's pitch -- pass the tolerance against fp64 (or a launch with equal pitches) while the
identities and the pitches of the storage cases catch them."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_band_cases as G                  # noqa: E402
from test_guard_bands_cpu import _family, tuning          # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from detr_tf import _hip
    return _hip, _hip.load()


def test_every_storage_case_reaches_the_family_it_states(lib):
    bad = []
    cases = G.storage_cases()
    for c in cases:
        with tuning(lib[0], c["env"]):
            _, fam, err = _family(lib, c)
        if fam != c["family"]:
            bad.append(f"{G.case_id(c)}: family {fam}, stated {c['family']} {err}")
    assert not bad, f"{len(bad)} of {len(cases)}:\n" + "\n".join(bad)
    assert {c["family"] for c in cases} == {0, 2}
    assert len({G.case_id(c) for c in cases}) == len(cases)
    # the streaming shapes really are the streaming kernel's: all-bf16, the same launch is family 1
    for c in (c for c in cases if c["group"] == "storefall"):
        with tuning(lib[0], c["env"]):
            _, fam, err = _family(lib, dict(c, c16=1, res="b16", mask="b16"))
        assert fam == 1, (G.case_id(c), fam, err)


def test_the_three_pitches_of_every_storage_case_differ():
    for c in G.storage_cases():
        pitches = [c["ldc"]] + ([c["ldr"]] if c["res"] else []) + ([c["ldm"]] if c["mask"] else [])
        assert len(set(pitches)) == len(pitches), (G.case_id(c), pitches)
        assert c["ldc"] != c["N"], G.case_id(c)


def test_every_identity_group_has_an_fp32_output_to_round():
    groups = {}
    for c in G.storage_cases():
        groups.setdefault(G.storage_group(c), []).append(c)
    for key, cs in groups.items():
        assert any(not c["c16"] for c in cs), G.storage_group_id(key)
        assert len({c["family"] for c in cs}) == 1
    assert any(len({c["c16"] for c in cs}) == 2 for cs in groups.values())


def _probe_product():
    return itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1), G.RES_STORES, G.MASK_STORES)


def test_every_accepted_storage_form_has_a_case(lib):
    """detr_hip_gemm_family over compute x a16 x b16 x c16 x residual x mask at the main shape, all operands aligned."""
    covered = {G.storage_key(c) for c in G.storage_cases() + G.gemm_cases()}
    accepted, rejected, uncovered = [], [], []
    for key in _probe_product():
        c = G.storage_probe_case(*key)
        with tuning(lib[0], c["env"]):
            _, fam, err = _family(lib, c)
        if fam >= 0:
            accepted.append(key)
            if key not in covered:
                uncovered.append(key)
        else:
            rejected.append(key)
            assert err, f"{key}: rejected without an error text"
    assert not uncovered, f"accepted by the library, run by no case: {uncovered}"
    # bf16 compute: A, B, C, residual and mask are independent switches; bit-packed masks need the all-bf16 epilogue
    want = {k for k in _probe_product() if k[0] == 1 and (k[5] != "bits" or (k[3] == 1 and k[4] in (None, "b16")))}
    # exact fp32 and f32x3: fp32 tensors only
    want |= {k for k in _probe_product() if k[0] != 1 and not (k[1] or k[2] or k[3]) and k[4] in (None, "f32") and k[5] in (None, "f32")}
    assert set(accepted) == want, (sorted(set(accepted) - want, key=str), sorted(want - set(accepted), key=str))
    assert len(accepted) + len(rejected) == 3 * 8 * 3 * 4


@pytest.mark.parametrize("field,value", [("compute", -1), ("compute", 3), ("a_dtype", 2), ("b_dtype", 2), ("c_dtype", 2), ("r_dtype", 2), ("m_dtype", 3),
                                         ("a_dtype", -1), ("m_dtype", -1)])
def test_gemm_rejects_values_the_header_does_not_document(lib, field, value):
    _hip, L = lib
    c = G.storage_probe_case(1, 1, 1, 1, "b16", "b16")
    with tuning(_hip, c["env"]):
        d, fam, _ = _family(lib, c)
        assert fam == 0
        setattr(d, field, value)
        assert L.detr_hip_gemm_family(ctypes.byref(d)) == -1
        assert L.detr_hip_last_error().decode()
        assert L.detr_hip_gemm_f32(ctypes.byref(d), None) == -1, "the launch entry point goes through the same check"


@pytest.mark.parametrize("compute", [0, 2])
@pytest.mark.parametrize("field", ["c_dtype", "r_dtype", "m_dtype"])
def test_gemm_rejects_bf16_storage_outside_bf16_compute(lib, compute, field):
    _hip, L = lib
    c = G.storage_probe_case(compute, 0, 0, 0, "f32", "f32")
    with tuning(_hip, c["env"]):
        d, fam, _ = _family(lib, c)
        assert fam == 0
        for value in ((1, 2) if field == "m_dtype" else (1,)):
            setattr(d, field, value)
            assert L.detr_hip_gemm_family(ctypes.byref(d)) == -1
            assert "compute = bf16" in L.detr_hip_last_error().decode()
            assert L.detr_hip_gemm_f32(ctypes.byref(d), None) == -1


def test_conv_and_stem_case_lists():
    cases = G.conv_storage_cases()
    tile = [c for c in cases if not c["halo"]]
    assert len(tile) == 9 * 2 * 8 * 3 and len(cases) - len(tile) == 7
    assert len({(c["id"], c["mode"], c["s16"], c["aux"]) for c in cases}) == len(cases)
    for c in cases:
        if c["halo"]:
            assert sum(c["s16"]) + (c["aux"] != "f32") == 3, "one fp32 tensor away from the halo kernels"
    assert [s[1] for s in G.STEM_STORAGE] == [0, 1]


# ------------------------------------------------------------------------------------------------------------------------
# what the identities and the three pitches add: two wrong epilogues the older assertions let through
# ------------------------------------------------------------------------------------------------------------------------
def _bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).bfloat16().float().numpy()


def model_epilogue(acc, residual, ldc, ldr, c16, double_rounding=False, residual_by_ldc=False):
    """C = acc + residual the way the scalar epilogue does it: fp32 arithmetic on an fp32 accumulator, the residual read from a flat
    buffer at row * ldr + col, the result rounded once when C is bf16.  double_rounding: the accumulator is rounded to bf16 before
    the residual is added.  residual_by_ldc: the residual is read at row * ldc + col."""
    M, N = acc.shape
    flat = np.full(M * max(ldc, ldr) + N, np.nan, dtype=np.float32)
    for r in range(M):
        flat[r * ldr:r * ldr + N] = residual[r]
    idx = np.arange(M)[:, None] * (ldc if residual_by_ldc else ldr) + np.arange(N)[None, :]
    a = acc.astype(np.float32)
    if double_rounding:
        a = _bf16(a)
    out = a + flat[idx]
    return _bf16(out) if c16 else out


def _b16_close(got, ref):
    """check_close(..., "b16")."""
    scale = float(np.abs(ref).max())
    return bool(np.isfinite(got).all()) and float((np.abs(got - ref) / (np.abs(ref) + 1e-2 * scale)).max()) < 2.0 ** -8 * 1.05


def test_a_double_rounding_passes_the_bf16_tolerance_and_fails_the_identity():
    rng = np.random.default_rng(2)
    M, N = 75, 136
    # a branch output added to a larger residual stream (x + f(x)): the extra rounding of the accumulator (2^-9 of it) is far below
    # the one-rounding bound of the sum, yet it moves the sum across a rounding boundary of the bf16 output now and then
    acc = (0.1 * rng.standard_normal((M, N))).astype(np.float32)
    res = _bf16(rng.standard_normal((M, N)) * 8.0)
    ref = acc.astype(np.float64) + res.astype(np.float64)
    c32 = model_epilogue(acc, res, N + 8, N + 16, c16=False)
    good = model_epilogue(acc, res, N + 8, N + 16, c16=True)
    bad = model_epilogue(acc, res, N + 8, N + 16, c16=True, double_rounding=True)
    assert _b16_close(good, ref) and _b16_close(bad, ref), "inside one bf16 rounding of fp64: both pass assertion (b)"
    assert np.array_equal(good, _bf16(c32)), "the identity holds for the right epilogue"
    assert not np.array_equal(bad, _bf16(c32))
    assert 0.0 < float((bad != _bf16(c32)).mean()) < 0.5


def test_a_residual_read_at_the_pitch_of_c_hides_behind_equal_pitches():
    rng = np.random.default_rng(3)
    M, N = 77, 50
    acc, res = rng.standard_normal((M, N)).astype(np.float32), _bf16(rng.standard_normal((M, N)))
    ref = model_epilogue(acc, res, N + 6, N + 6, c16=False)
    assert np.array_equal(model_epilogue(acc, res, N + 6, N + 6, c16=False, residual_by_ldc=True), ref), "ldr == ldc: the fault is invisible"
    seen = set()
    for c in G.storage_cases():
        if c["res"] and (c["ldc"], c["ldr"]) not in seen and c["N"] == N:
            seen.add((c["ldc"], c["ldr"]))
            assert np.array_equal(model_epilogue(acc, res, c["ldc"], c["ldr"], c16=False), ref)
            bad = model_epilogue(acc, res, c["ldc"], c["ldr"], c16=False, residual_by_ldc=True)
            assert not np.array_equal(bad, ref) and (np.isnan(bad).any() or float((bad != ref).mean()) > 0.5), (c["ldc"], c["ldr"])
    assert len(seen) >= 3
