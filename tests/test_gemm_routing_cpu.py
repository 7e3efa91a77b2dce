"""The GEMM dispatcher's decisions, pinned: which kernel family detr_hip_gemm_f32 launches for a descriptor (detr_hip_gemm_family)
and how much split-K scratch it asks for (detr_hip_workspace_bytes_gemm) are host arithmetic, replayed here on the cases of
tests/gemm_route_cases.py under every tuning environment and compared with tests/golden/gemm_routes.json, which
scripts/record_gemm_routes.py recorded before the host side of csrc/gemm_f32.hip was restructured.  No GPU."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_route_cases as G                  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_routes.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replay():
    from detr_tf import _hip
    cases = G.cases()
    before = {k: os.environ.get(k) for k in G.ENV_VARS}
    routes = G.route_all(_hip, _hip.load(), cases)
    assert {k: os.environ.get(k) for k in G.ENV_VARS} == before, "route_all must leave the tuning variables as it found them"
    return cases, routes


def test_fixture_covers_every_family_and_a_rejection(golden):
    """Under the default tuning every family 0 .. 5 and at least one rejection occur: a thinner list would not pin the order of the
    routing decision.  Every tuning environment of the case list is recorded."""
    fam = golden["families"]["default"]
    assert set("012345") <= set(fam), sorted(set(fam))
    assert any(ch >= "a" for ch in fam)
    assert list(golden["families"]) == [G.env_name(e) for e in G.ENVS]
    assert os.path.getsize(GOLDEN) < 100 * 1000


def test_case_list_matches_the_fixture(golden):
    cases = G.cases()
    assert len(cases) == golden["cases"] and sum(c["split_k"] > 1 for c in cases) == golden["split_cases"]
    for env in G.ENVS[1:]:
        name = G.env_name(env)
        assert len(golden["families"][name]) == len(cases) and name in golden["workspace_bytes_diff"]


@pytest.mark.parametrize("env", G.ENVS, ids=G.env_name)
def test_routes_and_workspace_bytes_equal_the_recorded_ones(golden, replay, env):
    cases, routes = replay
    name = G.env_name(env)
    fam, ws = routes[name]
    want_fam = golden["families"][name]
    want_ws = list(golden["workspace_bytes"])
    for i, w in golden["workspace_bytes_diff"].get(name, {}).items():
        want_ws[int(i)] = w
    split_cases = [c for c in cases if c["split_k"] > 1]
    bad = [f"{G.describe(c)}: family {g!r}, recorded {w!r}" for c, g, w in zip(cases, fam, want_fam) if g != w]
    bad += [f"{G.describe(c)}: workspace bytes {g}, recorded {w}" for c, g, w in zip(split_cases, ws, want_ws) if g != w]
    assert not bad, f"[{name}] {len(bad)} case(s) differ:\n" + "\n".join(bad[:20])
    assert fam == want_fam and ws == want_ws
