"""Record the split-K plan of the tree this runs in: for every case of tests/gemm_split_cases.py, what pick_split_k answers under the
default tuning.  Writes tests/golden/gemm_splits.json, a flat list of ints in case order (tests/test_gemm_split_plan_cpu.py replays it).

Host arithmetic only: runs without a GPU.  Run it BEFORE a change that is meant to keep the plan (csrc/gemm_f32.hip: gemm_split_plan and
the predicates it shares with gemm_pick_tile) and commit the fixture unchanged with that change; run it again, and review the diff,
with a change that is meant to move a shape to another split.

    python scripts/record_gemm_splits.py [--out tests/golden/gemm_splits.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "detr-tensorflow_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

TUNING = ("DETR_HIP_SPLIT_TARGET", "DETR_HIP_SPLIT_TARGET64", "DETR_HIP_X3_SPLIT_TARGET", "DETR_HIP_SPLIT3_T128")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gemm_splits.json"))
    args = ap.parse_args()
    set_ = [k for k in TUNING if k in os.environ]
    if set_:
        sys.exit(f"unset {', '.join(set_)} first: the fixture holds the plan of the default tuning")
    import gemm_split_cases as G
    from detr_tf import _hip
    splits = G.plan_all(_hip)
    with open(args.out, "w") as f:
        f.write(json.dumps(splits, separators=(",", ":")) + "\n")
    json.load(open(args.out))
    print(f"{args.out}: {len(splits)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
