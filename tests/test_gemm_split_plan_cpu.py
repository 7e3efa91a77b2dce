"""The split-K plan of the weight-gradient GEMMs, pinned: pick_split_k asks the library (detr_hip_gemm_split_plan, beside gemm_pick_tile in
csrc/gemm_f32.hip), and what it answers on the cases of tests/gemm_split_cases.py must equal tests/golden/gemm_splits.json, which
scripts/record_gemm_splits.py recorded while the plan was still Python arithmetic in detr_tf/_hip.py.  Host arithmetic only: no GPU."""
import inspect
import json
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_split_cases as G                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_splits.json")
TUNING = ("DETR_HIP_SPLIT_TARGET", "DETR_HIP_SPLIT_TARGET64", "DETR_HIP_X3_SPLIT_TARGET", "DETR_HIP_SPLIT3_T128")


def _hip_lib():
    sys.path.insert(0, os.path.join(ROOT, "detr-tensorflow_amd"))
    from detr_tf import _hip
    if not os.path.exists(_hip.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    return _hip, _hip.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture()
def hip():
    """The binding under the default tuning of the plan: the process's own settings of its variables are set aside and restored."""
    _hip, _ = _hip_lib()
    saved = {k: os.environ.get(k) for k in TUNING}
    for k in TUNING:
        _hip.set_tuning(k, None)
    yield _hip
    for k, v in saved.items():
        _hip.set_tuning(k, v)


def cdiv(a, b):
    return -(-a // b)


def big_split(M, N, K):
    return (N >= 128 and K >= 16384) or (M >= 512 and N >= 512 and K >= 4096) or (K >= 4096 and ((M >= 256 and N >= 2048) or (M >= 2048 and N >= 256)))


def x3_shape(M, N, K):
    return N >= 128 and K >= 256 and M >= 128


def plan64(M, N, K, compute, max_split=1024, target=1024):
    """The 64 x 64 plan, restated."""
    ktiles = cdiv(K, 32 if compute == 1 else 16)
    return max(1, min(max(1, target // (cdiv(M, 64) * cdiv(N, 64))), max_split, ktiles // 8 if ktiles >= 64 else ktiles // 4))


def branch(M, N, K, compute, max_split):
    """Which branch of the plan a case takes under the default tuning (targets 256 / 1024 / 512, f32x3 threshold 192)."""
    if compute == 1 and big_split(M, N, K):
        return "bf16_128"
    if compute == 2 and x3_shape(M, N, K):
        t128, ktiles = cdiv(M, 128) * cdiv(N, 128), cdiv(K, 32)
        s128 = max(1, min(512 // t128, max_split, ktiles // 8 if ktiles >= 64 else max(1, ktiles // 4)))
        if t128 * s128 >= 192:
            return "x3_128"
        return "x3_declined_long" if cdiv(K, 16) >= 64 else "x3_declined_short"
    return "64_long" if cdiv(K, 32 if compute == 1 else 16) >= 64 else "64_short"


def test_plan_equals_the_recorded_one(hip, golden):
    cases = G.cases()
    assert len(cases) == len(golden) and os.path.getsize(GOLDEN) < 100 * 1000
    got = G.plan_all(hip, cases)
    bad = [f"M{c[0]} N{c[1]} K{c[2]} compute={c[3]} max_split={c[4]}: split {g}, recorded {w}" for c, g, w in zip(cases, got, golden) if g != w]
    assert not bad, f"{len(bad)} case(s) differ:\n" + "\n".join(bad[:20])
    assert got == golden


def test_fixture_is_not_blind(golden):
    """Every branch of the plan occurs among the cases (counted with the predicates restated above), with more than one answer."""
    cases = G.cases()
    by = {}
    for c, s in zip(cases, golden):
        by.setdefault(branch(*c), []).append(s)
    for name in ("bf16_128", "x3_128", "64_long", "64_short"):
        assert len(by.get(name, ())) >= 20 and len(set(by[name])) > 1, (name, len(by.get(name, ())))
    assert len(by.get("x3_declined_long", ())) + len(by.get("x3_declined_short", ())) >= 20      # t128 * s128 below the threshold
    assert all(isinstance(s, int) and 1 <= s <= c[4] for c, s in zip(cases, golden))
    assert any(s == c[4] for c, s in zip(cases, golden) if c[4] == 8) and any(s < 8 for c, s in zip(cases, golden) if c[4] == 8)
    for (M, N, K, compute, max_split), s in zip(cases, golden):          # whatever ends in the 64 x 64 plan is checked in full
        if branch(M, N, K, compute, max_split).startswith(("64_", "x3_declined")):
            assert s == plan64(M, N, K, compute, max_split), (M, N, K, compute, max_split)


SPOT = [(1, (256, 256, 8400), 32), (1, (64, 256, 534400), 128), (1, (2048, 256, 8400), 8), (1, (256, 1024, 33600), 16), (1, (4, 256, 4800), 18),
        (2, (128, 128, 8400), 65), (2, (256, 1024, 8400), 32), (2, (64, 256, 534400), 256), (0, (147, 64, 2134400), 341), (0, (256, 256, 8400), 64)]


@pytest.mark.parametrize("compute,shape,split", SPOT, ids=[f"c{c}-{'x'.join(map(str, s))}" for c, s, _ in SPOT])
def test_spot_values(hip, golden, compute, shape, split):
    """Values worked out on the commit before the plan moved into the library, so that a wrongly recorded fixture is caught."""
    assert hip.pick_split_k(*shape, compute=compute) == split
    case = (*shape, compute, 1024)
    cases = G.cases()
    if case in cases:
        assert golden[cases.index(case)] == split


def test_compute_none_is_the_module_default(hip):
    old = hip.COMPUTE_BF16
    try:
        for mode in (0, 1, 2):
            hip.COMPUTE_BF16 = mode
            assert hip.pick_split_k(256, 1024, 8400) == hip.pick_split_k(256, 1024, 8400, compute=mode)
        assert len({hip.pick_split_k(256, 1024, 8400, compute=m) for m in (0, 1, 2)}) > 1
    finally:
        hip.COMPUTE_BF16 = old


def test_tuning_reaches_the_plan_and_clears_the_cache(hip):
    before = {k: v for k, v in os.environ.items() if k.startswith("DETR_HIP_")}
    a, b, c = (256, 1024, 33600), (128, 128, 8400), (256, 1024, 8400)
    defaults = lambda: (hip.pick_split_k(*a, compute=1), hip.pick_split_k(*b, compute=2), hip.pick_split_k(*c, compute=2))
    assert defaults() == (16, 65, 32)
    try:
        hip.set_tuning("DETR_HIP_SPLIT_TARGET", 512)
        assert hip.pick_split_k(*a, compute=1) == 32
        hip.set_tuning("DETR_HIP_SPLIT_TARGET", None)
        assert defaults() == (16, 65, 32)
        hip.set_tuning("DETR_HIP_SPLIT3_T128", 16)           # the plan follows the tile rule's tuned threshold: 1 tile x 32 splits >= 16
        assert hip.pick_split_k(*b, compute=2) == 32
        hip.set_tuning("DETR_HIP_SPLIT3_T128", None)
        assert defaults() == (16, 65, 32)
        hip.set_tuning("DETR_HIP_X3_SPLIT_TARGET", -1)       # off: f32x3 takes the 64 x 64 plan
        assert plan64(*c, 2) == 16 and hip.pick_split_k(*c, compute=2) == plan64(*c, 2)
        hip.set_tuning("DETR_HIP_X3_SPLIT_TARGET", None)
        assert defaults() == (16, 65, 32)
        hip.set_tuning("DETR_HIP_SPLIT_TARGET64", 512)
        assert hip.pick_split_k(256, 256, 8400, compute=0) == plan64(256, 256, 8400, 0, target=512) == 32
        hip.set_tuning("DETR_HIP_SPLIT_TARGET64", None)
        assert hip.pick_split_k(256, 256, 8400, compute=0) == 64
    finally:
        for k in TUNING:
            hip.set_tuning(k, None)
    assert {k: v for k, v in os.environ.items() if k.startswith("DETR_HIP_")} == before


def test_warm_lookups_do_not_call_the_library(hip):
    lib = hip.load()
    first = hip.pick_split_k(92, 256, 4800, compute=1)
    real, calls = lib.detr_hip_gemm_split_plan, []
    lib.detr_hip_gemm_split_plan = lambda *a: calls.append(a) or real(*a)
    try:
        assert hip.pick_split_k(92, 256, 4800, compute=1) == first and not calls
        assert hip.pick_split_k(92, 256, 4801, compute=1) >= 1 and len(calls) == 1
    finally:
        lib.detr_hip_gemm_split_plan = real


@pytest.mark.parametrize("args", [(0, 64, 64, 0, 1024), (64, -1, 64, 0, 1024), (64, 64, 0, 1, 1024), (64, 64, 64, 3, 1024), (64, 64, 64, -1, 1024),
                                  (64, 64, 64, 2, 0)], ids=str)
def test_rejections(hip, args):
    lib = hip.load()
    assert lib.detr_hip_gemm_split_plan(64, 64, 64, 0, 1024) >= 1
    assert lib.detr_hip_gemm_split_plan(*args) == -1
    msg = lib.detr_hip_last_error().decode()
    assert "gemm_split_plan" in msg and any(str(v) in msg for v in args)
    M, N, K, compute, max_split = args
    with pytest.raises(RuntimeError, match="gemm_split_plan"):
        hip.pick_split_k(M, N, K, max_split, compute=compute)


def test_binding_holds_no_shape_thresholds(hip):
    src = inspect.getsource(hip.pick_split_k)
    assert not re.search(r"\b(16384|4096|2048)\b", src)
    text = open(hip.__file__).read()
    assert not re.search(r"environ[^\n]*SPLIT_TARGET", text) and "SPLIT_TARGET_128" not in text and "DEFER_WS" not in text
