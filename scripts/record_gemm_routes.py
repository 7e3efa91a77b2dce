"""Record the GEMM routing of the library that is built in this tree: for every case of tests/gemm_route_cases.py, under every tuning
environment listed there, the family detr_hip_gemm_family answers (or its rejection) and, for the split-K cases, the bytes
detr_hip_workspace_bytes_gemm asks for.  Writes tests/golden/gemm_routes.json (tests/test_gemm_routing_cpu.py replays it).

Host arithmetic only: runs without a GPU.  Run it BEFORE a change to the GEMM host side (csrc/gemm_f32.hip: gemm_prepare, gemm_pick_tile,
gemm_route) that is meant to keep the routing, and commit the fixture unchanged with that change; run it again, and review the diff,
with a change that is meant to move a shape to another kernel.

    python scripts/record_gemm_routes.py [--out tests/golden/gemm_routes.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "detr-tensorflow_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def encode(routes):
    """Compact form: one family string per environment; the workspace bytes of the split-K cases in full for the default tuning and
    as {index among the split-K cases: bytes} where another environment differs from it."""
    fam = {name: f for name, (f, _) in routes.items()}
    base = routes["default"][1]
    diff = {name: {str(i): w for i, (w, b) in enumerate(zip(ws, base)) if w != b} for name, (_, ws) in routes.items() if name != "default"}
    return {"cases": len(fam["default"]), "split_cases": len(base), "families": fam, "workspace_bytes": base, "workspace_bytes_diff": diff}


def dump(enc, path):
    c = lambda v: json.dumps(v, separators=(",", ":"))
    lines = ['{"cases":%d,"split_cases":%d,' % (enc["cases"], enc["split_cases"]), '"families":{']
    lines += [",\n".join(f"{c(k)}:{c(v)}" for k, v in enc["families"].items()), "},"]
    lines += [f'"workspace_bytes":{c(enc["workspace_bytes"])},', '"workspace_bytes_diff":{']
    lines += [",\n".join(f"{c(k)}:{c(v)}" for k, v in enc["workspace_bytes_diff"].items()), "}}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gemm_routes.json"))
    args = ap.parse_args()
    import gemm_route_cases as G
    from detr_tf import _hip
    enc = encode(G.route_all(_hip, _hip.load()))
    dump(enc, args.out)
    json.load(open(args.out))
    print(f"{args.out}: {enc['cases']} cases x {len(enc['families'])} environments, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
