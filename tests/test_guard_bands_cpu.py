"""What tests/test_gpu_guard_bands.py rests on, checked without a GPU: every GEMM case of tests/guard_band_cases.py reaches the kernel
family it states (the library's routing is host arithmetic on the descriptor), the split-K scratch query is at least the documented
floor, the framing helpers build what they say, and NumPy models of a widened K tail and of a dropout index by pitch pass the
zero-padded, tight-pitch comparison of the older tests while the framed cases catch them."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_band_cases as G                  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from detr_tf import _hip
    return _hip, _hip.load()


tuning = G.tuning


def _family(lib, c, ws_bytes=0):
    _hip, L = lib
    d = G.fill_desc(_hip, c, G.placeholder_ptrs(c), dropout_step=0xC0000000, workspace=0xD0000000 if ws_bytes else None, workspace_bytes=ws_bytes)
    fam = L.detr_hip_gemm_family(ctypes.byref(d))
    return d, fam, (L.detr_hip_last_error().decode() if fam < 0 else "")


def test_every_gemm_case_reaches_the_family_it_states(lib):
    bad = []
    cases = G.gemm_cases()
    for c in cases:
        with tuning(lib[0], c["env"]):
            _, fam, err = _family(lib, c)
        if fam != c["family"]:
            bad.append(f"{G.case_id(c)}: family {fam}, stated {c['family']} {err}")
    assert not bad, f"{len(bad)} of {len(cases)}:\n" + "\n".join(bad)
    assert {c["family"] for c in cases} == {0, 1, 2, 3, 4}
    assert len({G.case_id(c) for c in cases}) == len(cases)


def test_split_cases_route_and_ask_for_at_least_the_floor(lib):
    _hip, L = lib
    larger = 0
    cases = G.split_cases()
    for c in cases:
        with tuning(_hip, c["env"]):
            d, _, _ = _family(lib, c)
            query = int(L.detr_hip_workspace_bytes_gemm(ctypes.byref(d)))
            floor = G.split_floor_bytes(c)
            assert query >= floor > 0, (G.case_id(c), query, floor)
            for ws_bytes in (query, floor, 64 << 20):
                d, fam, err = _family(lib, c, ws_bytes)
                # the ring weight gradient writes tile-ordered slabs: with the floor alone the 4-wave engine takes the launch
                want = c["family"] if not (c["family"] == 5 and ws_bytes < query) else 0
                assert fam == want, (G.case_id(c), ws_bytes, fam, err)
            larger += query > floor
    assert larger >= 1, "no case where the tile-ordered slabs need more than the floor: 'exact' and 'floor' would be one run"
    assert {c["family"] for c in cases} == {0, 5}


def test_every_output_family_has_a_lead_a_wide_pitch_and_a_tail():
    for fam in range(5):
        ok = False
        for c in G.gemm_cases():
            shape, dtype, lead, pitch, out = G.operands(c)["C"]
            ok |= c["family"] == fam and lead > 0 and G.TAIL > 0 and (pitch > shape[1] or fam == 4)      # (the LayerNorm form requires ldc == N)
        assert ok, fam


def test_layernorm_gemm_rejects_a_padded_output_pitch(lib):
    """The GEMM + LayerNorm kernel documents ldc == N == 256 (its C, ln_y, ln_y2 and ln_y16 rows are tight): a wider pitch is refused
    by the entry point before anything is launched, which is why the family-4 cases frame C with a lead and a tail only."""
    _hip, L = lib
    c = dict(next(c for c in G.gemm_cases() if c["family"] == 4), ldc=264)
    d = G.fill_desc(_hip, c, G.placeholder_ptrs(c), dropout_step=0xC0000000)
    assert L.detr_hip_gemm_f32(ctypes.byref(d), None) == -1
    assert "N = ldc = 256" in L.detr_hip_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("lead", [16, 17])
def test_nan_framed_layout(dtype, lead):
    t = torch.arange(5 * 7, dtype=torch.float32).reshape(5, 7).to(dtype)
    view, buf = G.nan_framed(t, lead, 11, 9)
    assert buf.numel() == lead + 5 * 11 + 9 and buf.dtype == dtype
    assert view.stride() == (11, 1) and view.storage_offset() == lead and torch.equal(view, t)
    assert (view.data_ptr() - buf.data_ptr()) == lead * t.element_size()
    assert ((view.data_ptr() - buf.data_ptr()) % 16 == 0) == (lead * t.element_size() % 16 == 0)
    assert int(torch.isnan(buf.float()).sum()) == buf.numel() - 35
    t4 = torch.randn(2, 3, 4, 6).to(dtype)
    v4, b4 = G.nan_framed(t4, lead, None, 9)
    assert v4.is_contiguous() and torch.equal(v4, t4) and b4.numel() == lead + t4.numel() + 9
    v4, b4 = G.nan_framed(t4, lead, 8, 9)
    assert v4.stride() == (96, 32, 8, 1) and torch.equal(v4, t4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_sentinel_frame_catches_a_planted_element(dtype):
    sent = G.sentinel_of(dtype)
    view, buf = G.sentinel_framed((6, 5), dtype, 8, 9, 12)
    assert buf.numel() == 8 + 6 * 9 + 12 and bool((buf == sent).all()) and view.stride() == (9, 1)
    assert float(torch.tensor(G.SENT).bfloat16()) == G.SENT
    view.fill_(1)
    assert G.frame_intact(buf, view)
    for where in (3, 8 + 3 * 9 + 5, 8 + 3 * 9 + 8, buf.numel() - 1, 8 + 6 * 9 - 1):      # lead, first and last pad column of a middle row, tail, last row's pad
        keep = buf[where].clone()
        buf[where] = 1
        assert not G.frame_intact(buf, view), where
        buf[where] = keep
    assert G.frame_intact(buf, view)
    for where in (8, 8 + 3 * 9 + 4, 8 + 5 * 9 + 4):                                     # inside the view: not the frame's business
        buf[where] = 2
    assert G.frame_intact(buf, view)


def test_bit_packing_round_trip():
    t = torch.rand(5, 24) > 0.5
    assert torch.equal(G.unpack_bits(G.pack_bits(t), 24), t)
    assert int(G.pack_bits(torch.tensor([[1, 0, 0, 0, 0, 0, 0, 1]]).bool())[0, 0]) == 0x81


# ------------------------------------------------------------------------------------------------------------------------
# why the zero-padded, tight-pitch method is blind
# ------------------------------------------------------------------------------------------------------------------------
def _close(got, ref, rtol=2e-5):
    return bool(np.isfinite(got).all()) and float(np.abs(got - ref).max()) <= rtol * float(np.abs(ref).max())


def test_zero_padding_hides_a_widened_k_tail_nan_padding_shows_it():
    rng = np.random.default_rng(0)
    M, N, K = 77, 40, 33
    A, B = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64).T
    ld = K + 4
    for wide in (False, True):
        # the method of test_gemm_layouts: operands in zero-filled [rows, K + 4] buffers
        Az, Bz = np.zeros((M, ld), np.float32), np.zeros((N, ld), np.float32)
        Az[:, :K], Bz[:, :K] = A, B
        assert _close(G.model_gemm(Az, ld, Bz, ld, M, N, K, wide_k_tail=wide), ref), "zero padding: both models pass"
        # the framed operands of this suite
        (Av, Ab), (Bv, Bb) = G.nan_framed(torch.from_numpy(A), 16, ld, 8), G.nan_framed(torch.from_numpy(B), 16, ld, 8)
        got = G.model_gemm(Ab[16:16 + M * ld].numpy(), ld, Bb[16:16 + N * ld].numpy(), ld, M, N, K, wide_k_tail=wide)
        assert _close(got, ref) == (not wide)
        assert bool(np.isnan(got).any()) == wide              # assertion (a) of the device cases


def test_tight_pitch_hides_a_dropout_index_by_pitch():
    from oracle import dropout_ref as DR
    rng = np.random.default_rng(1)
    M, N, p = 77, 50, 0.1
    acc = rng.standard_normal((M, N))
    key = DR.drop_key(G.DROP_SITE, G.DROP_STEP)
    ref = G.model_dropout_epilogue(acc, N, p, key)
    assert np.array_equal(G.model_dropout_epilogue(acc, N, p, key, by_pitch=True), ref), "ldc == N: the fault is invisible"
    for ldc in (53, 52, N + 8):
        assert np.array_equal(G.model_dropout_epilogue(acc, ldc, p, key), ref)
        bad = G.model_dropout_epilogue(acc, ldc, p, key, by_pitch=True)
        assert not _close(bad, ref), ldc
        assert 0.1 < float((bad != ref).mean()) < 0.25          # ~ 2 p (1 - p) of the elements change sides
