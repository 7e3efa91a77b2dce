"""GEMM shapes whose split-K plan the library must keep: the case list behind tests/golden/gemm_splits.json (written by
scripts/record_gemm_splits.py, replayed by tests/test_gemm_split_plan_cpu.py).

For every case the fixture holds what pick_split_k answers under the default tuning.  The grid straddles every threshold of the two
shape predicates of the plan (gemm_big_split, gemm_x3_shape in csrc/gemm_f32.hip) and the 16 / 64 steps of its K-tile caps."""

MS = NS = (4, 63, 64, 65, 92, 127, 128, 255, 256, 511, 512, 2047, 2048)
KS = (600, 800, 2047, 2048, 4095, 4096, 8400, 16383, 16384, 33600, 133600, 534400, 2134400)
COMPUTES = (0, 1, 2)

# (M, N, K, compute, max_split) with a max_split that binds (or, on the last two, does not)
CAPPED = ((256, 256, 8400, 1, 8), (64, 256, 534400, 1, 8), (256, 1024, 8400, 2, 8), (128, 128, 8400, 2, 8), (147, 64, 2134400, 0, 8),
          (64, 64, 2048, 0, 8), (2048, 2048, 8400, 1, 8), (4, 4, 600, 0, 8))


def cases():
    """[(M, N, K, compute, max_split)]"""
    out = [(M, N, K, compute, 1024) for compute in COMPUTES for M in MS for N in NS for K in KS]
    return out + list(CAPPED)


def plan_all(_hip, case_list=None):
    return [int(_hip.pick_split_k(M, N, K, max_split, compute=compute)) for M, N, K, compute, max_split in (cases() if case_list is None else case_list)]
