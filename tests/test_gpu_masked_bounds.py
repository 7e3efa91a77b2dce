"""GPU tests of the key-padding-masked attention kernels (the MASK instantiations of csrc/attention_dma.hip and attention_f32.hip)
at the standard of the unmasked bf16 core: every element of O, lse, dQ, dK and dV against the per-element bounds of
oracle/attn_bounds.py (masked keys exactly absent; dK / dV exactly 0 there), on masks built to reach each piece of masked logic --
skipped tiles, `fresh` set by a later or partial tile, runs without a valid key, the register-to-key bit mapping, and the validity
words of tiles 64 and later, which the kernels read from memory instead of from a lane (S up to 8192: 256 key tiles).  Exact
structural checks (a prefix mask is truncation, batch elements are isolated, masked content is ignored) cover the bf16 and fp32
kernels; the fp32 kernels are compared with an fp64 masked reference at the large shapes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as AC                    # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, HD, D = AC.H, AC.HD, AC.D
X = 64                                     # sentinel rows / entries past every output and scratch buffer
SCORES4 = ["uniform", "ascending", "ragged_max", "masked_dominant"]
SCORES_FAR = ["uniform", "ascending", "descending", "masked_dominant"]
SPLIT_DEPENDENT = ("run_heads", "empty_runs_last", "empty_runs_first")


def _masked_bounds(hip, case, kind, B, T, S, p, splits, seed, grid=None):
    """The masked forward / backward under each split against the bounds; the backward of every split reads the stored O of the
    heuristic forward, the O the backward reference forms delta from.  Returns the largest ratio per output."""
    from oracle import attn_bounds as AB
    keep = AC.keep_mask(B, T, S, p)
    ntk = -(-S // 32)
    worst = dict(o=0.0, lse=0.0, dq=0.0, dk=0.0, dv=0.0)
    fw = None
    for split in splits:
        parts = AB.parts_for(ntk, split)
        if fw is None or kind in SPLIT_DEPENDENT or case == "distant_runs":
            kv = torch.from_numpy(AC.key_valid(kind, B, S, parts, seed=seed, grid=grid))
            qs, k, v, do = AC.scores_case(case, B, T, S, p, parts, keep, torch.Generator().manual_seed(seed), key_valid=kv)
            assert bool((k.view(B, S, D)[~kv].abs().sum(dim=1) > 0).all()) and bool((v[~kv].abs().sum(dim=1) > 0).all()), \
                "masked K / V rows must hold content"
            if case == "near_limit":
                print(f"near_limit {kind} B{B} T{T} S{S} p{p} parts{parts}: largest lane sum "
                      f"{AC.assert_below_sum_limit(qs, k, B, T, S, p, parts, key_valid=kv):.0f}")
            dev = AC.device_operands(hip, qs, k, v, do, B, T, S, p, extra=X, key_valid=kv)
            fw = AB.forward(qs, k, v, H, keep, p, key_valid=kv)
            o0 = torch.full_like(dev["o"], -1234.0)
            AC.fwd(hip, dev, B, T, S, 0, o=o0)
            bw = AB.backward(qs, k, v, do, o0[:B * T].double().cpu().view(B, T, D), H, keep, p, key_valid=kv)
        tag = f"{case} {kind} B{B} T{T} S{S} p{p} split{split}"
        AC.fwd(hip, dev, B, T, S, split)
        r = dict(o=AC.check(f"O ({tag})", dev["o"][:B * T].float().view(B, T, D), fw["o"], fw["bound_o"]),
                 lse=AC.check(f"lse ({tag})", dev["lse"][:B * H * T].view(B * H, T), fw["lse"], fw["bound_lse"]))
        AC.bwd(hip, dev, B, T, S, split, o0, dev["lse"])
        inv = (~kv).reshape(-1).to(DEV)
        for n in ("dk", "dv"):
            assert bool((dev[n][:B * S][inv] == 0).all()), f"{n}: masked keys must get exact zeros ({tag})"
        r["dq"] = AC.check(f"dQ ({tag})", dev["dq"][:B * T].float().view(B, T, D), bw["dq"], bw["bound_dq"])
        r["dk"] = AC.check(f"dK ({tag})", dev["dk"][:B * S].float().view(B, S, D), bw["dk"], bw["bound_dk"])
        r["dv"] = AC.check(f"dV ({tag})", dev["dv"][:B * S].float().view(B, S, D), bw["dv"], bw["bound_dv"])
        AC.sentinels_intact(dev, B, T, S, X)
        for n in worst:
            worst[n] = max(worst[n], r[n])
    return worst


def _report(label, worst):
    print(f"RATIO {label}: " + " ".join(f"{n} {x:.3g}" for n, x in worst.items()))


# rect / random on the step's shapes, every score construction (dropped_dominant needs dropout; at the largest shape one dropout
# rate per construction, alternating)
ALL_SCORES = AC.CASES + ["masked_dominant"]
ROW_A = [(c, m, B, T, S, p) for c in ALL_SCORES for m in ("rect", "random")
         for B, T, S in ((2, 1050, 1050), (2, 100, 1050), (2, 70, 333)) for p in (0.0, 0.1)
         if not (c == "dropped_dominant" and p == 0.0)
         and not (S == T == 1050 and c != "dropped_dominant" and p != (0.1 if (ALL_SCORES.index(c) + (m == "random")) % 2 else 0.0))]
# the structural masks on a one-run-per-tile-group shape and the step's shape (the latter with dropout only)
ROW_B = [(c, m, B, T, S, p) for m in ("tiles", "first_half", "run_heads", "empty_runs_last", "empty_runs_first", "single_valid")
         for c in SCORES4 for B, T, S in ((2, 1050, 1050), (1, 200, 700)) for p in (0.0, 0.1) if not (S == 1050 and p == 0.0)]
# more than 64 key tiles: a 50 x 42 and a 64 x 128 feature grid, and far-tile words
ROW_C = [(c, m, B, T, S, p) for m in ("rect", "far_tiles") for c in SCORES_FAR
         for B, T, S in ((1, 130, 2100), (1, 2100, 2100), (1, 100, 8192)) for p in (0.0, 0.1)
         if not (T == 2100 and p != (0.1 if SCORES_FAR.index(c) % 2 else 0.0))]


@pytest.mark.parametrize("case,kind,B,T,S,p", ROW_A + ROW_B)
def test_masked_bf16_within_per_element_bounds(hip, case, kind, B, T, S, p):
    """Heuristic and DETR_HIP_ATTN_SPLIT = 1, 2, 5, 8."""
    seed = 100 * ALL_SCORES.index(case) + AC.MASKS.index(kind) + T + S
    _report(f"{case} {kind} B{B} T{T} S{S} p{p}", _masked_bounds(hip, case, kind, B, T, S, p, (0, 1, 2, 5, 8), seed))


@pytest.mark.parametrize("case,kind,B,T,S,p", ROW_C)
def test_masked_bf16_past_64_key_tiles_within_per_element_bounds(hip, case, kind, B, T, S, p):
    """S = 2100 and 8192: runs of more than 64 tiles read tile words 64+ from memory.  Heuristic and splits 1, 2, 3 (at S = 8192 the
    heuristic gives exactly 64 tiles per run)."""
    seed = 100 * SCORES_FAR.index(case) + AC.MASKS.index(kind) + T + S
    _report(f"{case} {kind} B{B} T{T} S{S} p{p}", _masked_bounds(hip, case, kind, B, T, S, p, (0, 1, 2, 3), seed))


# ------------------------------------------------------------------------------------------------------------------------------
# exact structural checks
# ------------------------------------------------------------------------------------------------------------------------------
def _operands(B, T, S, seed, bf16):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    c = (2.0 * HD ** -0.5 * 1.4426950408889634) if bf16 else 1.0         # bf16: the stored query carries scale * log2 e
    return rn(B, T, D) * c, rn(B, S, D), rn(B, S, D), rn(B, T, D)


def _f32_outputs(hip, qs, k, v, do, B, T, S, p, kv, split=0):
    """fp32 masked (kv bool [B, S]) or unmasked (kv None) forward + backward; outputs with X sentinel rows."""
    d = lambda t: t.float().reshape(-1, D).to(DEV)
    q_, k_, v_, do_ = d(qs), d(k), d(v), d(do)
    sent = lambda rows: torch.full((rows + X, D), -1234.0, device=DEV)
    o, dq, dk, dv = sent(B * T), sent(B * T), sent(B * S), sent(B * S)
    lse = torch.full((B * H * T + X,), -4321.0, device=DEV)
    delta = torch.full((2 * B * H * T + X,), -4321.0, device=DEV)
    stepd = torch.tensor([12345] + [0] * 7, dtype=torch.int32, device=DEV)
    kw = dict(scale=HD ** -0.5, dropout_p=p, dropout_site=5, dropout_step=stepd, compute=0)
    if kv is not None:
        kw["key_valid"] = torch.from_numpy(hip.keymask_words_from_valid(np.asarray(kv))).reshape(-1).to(DEV)
    hip.set_tuning("DETR_HIP_ATTN_SPLIT", split if split else None)
    try:
        hip.attention(q_, k_, v_, o[:B * T], lse, B, H, T, S, **kw)
        hip.attention(q_, k_, v_, o[:B * T], lse, B, H, T, S, d_o=do_, dq=dq[:B * T], dk=dk[:B * S], dv=dv[:B * S], delta=delta, **kw)
        torch.cuda.synchronize()
    finally:
        hip.set_tuning("DETR_HIP_ATTN_SPLIT", None)
    dev = dict(o=o, dq=dq, dk=dk, dv=dv, lse=lse, delta=delta)
    AC.sentinels_intact(dev, B, T, S, X)
    return dict(o=o[:B * T].view(B, T, D), lse=lse[:B * H * T].view(B, H, T), dq=dq[:B * T].view(B, T, D),
                dk=dk[:B * S].view(B, S, D), dv=dv[:B * S].view(B, S, D))


def _bf16_outputs(hip, qs, k, v, do, B, T, S, p, kv, split):
    dev = AC.device_operands(hip, qs, k, v, do, B, T, S, p, extra=X, key_valid=kv)
    AC.all_outputs(hip, dev, B, T, S, split)
    AC.sentinels_intact(dev, B, T, S, X)
    return dict(o=dev["o"][:B * T].view(B, T, D), lse=dev["lse"][:B * H * T].view(B, H, T), dq=dev["dq"][:B * T].view(B, T, D),
                dk=dev["dk"][:B * S].view(B, S, D), dv=dev["dv"][:B * S].view(B, S, D))


def _outputs(hip, bf16, *args):
    return _bf16_outputs(hip, *args) if bf16 else _f32_outputs(hip, *args)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16io", "fp32"])
@pytest.mark.parametrize("S,ns", [(1050, (31, 33, 1000)), (2100, (2047, 2049, 2090)), (2100, (64, 1056, 2100))])
def test_masked_prefix_is_truncation(hip, bf16, S, ns):
    """Key j valid iff j < n_b (a different n_b per image, on both sides of a tile boundary and past tile 64): the masked kernels
    at p = 0 give O, lse, dQ and the dK / dV of valid keys bit-identical to the unmasked kernels run on each image's first n_b
    keys alone -- same tile sequence, ragged handling and reference.  bf16 at DETR_HIP_ATTN_SPLIT = 1 (one run: the same runs)."""
    B, T = 3, 100
    qs, k, v, do = _operands(B, T, S, 41 + S, bf16)
    kv = np.zeros((B, S), bool)
    for b, n in enumerate(ns):
        kv[b, :n] = True
    split = 1 if bf16 else 0
    got = _outputs(hip, bf16, qs, k, v, do, B, T, S, 0.0, kv, split)
    for b, n in enumerate(ns):
        one = _outputs(hip, bf16, qs[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], do[b:b + 1], 1, T, n, 0.0, None, split)
        for name in ("o", "lse", "dq"):
            assert torch.equal(got[name][b], one[name][0]), f"{name} of image {b} (n {n}, S {S}) differs from the truncated run"
        for name in ("dk", "dv"):
            assert torch.equal(got[name][b, :n], one[name][0]), f"{name} of image {b} (n {n}, S {S}) differs from the truncated run"
            assert bool((got[name][b, n:] == 0).all()), f"{name}: masked keys must get exact zeros"


@pytest.mark.parametrize("bf16,split", [(True, 0), (True, 8), (False, 0)], ids=["bf16io-heuristic", "bf16io-split8", "fp32"])
@pytest.mark.parametrize("S", [1050, 2100])
def test_masked_batch_elements_are_isolated(hip, bf16, split, S):
    """B = 3: new masks and new K / V for elements 0 and 2 leave every output of element 1 bit-identical."""
    B, T, p = 3, 200, 0.1
    qs, k, v, do = _operands(B, T, S, 61 + S, bf16)
    kv = AC.key_valid("random", B, S, seed=1)
    a = _outputs(hip, bf16, qs, k, v, do, B, T, S, p, kv, split)
    kv2 = kv.copy()
    kv2[0], kv2[2] = AC.key_valid("first_half", 3, S)[0], AC.key_valid("tiles", 3, S)[2]
    g = torch.Generator().manual_seed(62)
    for b in (0, 2):
        k[b] = torch.randn(S, D, dtype=torch.float64, generator=g) * 4.0
        v[b] = torch.randn(S, D, dtype=torch.float64, generator=g) * 50.0
    c = _outputs(hip, bf16, qs, k, v, do, B, T, S, p, kv2, split)
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(a[n][1], c[n][1]), f"{n} of batch element 1 depends on the masks / keys of elements 0 and 2"
        assert not torch.equal(a[n], c[n]), f"{n}: the replaced elements changed nothing"


GARBAGE = [(True, 1, 1050), (True, 2, 1050), (True, 8, 1050), (True, 0, 2100), (True, 1, 2100), (True, 2, 2100), (True, 8, 2100),
           (True, 0, 8192), (True, 1, 8192), (True, 3, 8192), (False, 0, 2100), (False, 0, 8192)]


@pytest.mark.parametrize("bf16,split,S", GARBAGE, ids=[f"{'bf16io' if g[0] else 'fp32'}-split{g[1]}-S{g[2]}" for g in GARBAGE])
def test_masked_content_is_ignored(hip, bf16, split, S):
    """Masked K / V rows zero-filled, filled with +-1e4 and filled with uniform garbage in +-1e4 give bit-identical outputs (dK / dV:
    exact zeros at masked keys, identical at valid ones)."""
    B, T, p = 2, 100, 0.1
    qs, k, v, do = _operands(B, T, S, 81 + S, bf16)
    kv = AC.key_valid("far_tiles" if S > 2048 else "rect", B, S)
    inv = torch.from_numpy(~kv).unsqueeze(2)
    rng = np.random.default_rng(0)
    fills = [torch.zeros(B, S, D, dtype=torch.float64), torch.full((B, S, D), 1.0e4, dtype=torch.float64),
             torch.from_numpy(rng.uniform(-1e4, 1e4, (B, S, D)))]
    outs = [_outputs(hip, bf16, qs, torch.where(inv, f, k), torch.where(inv, -f, v), do, B, T, S, p, kv, split) for f in fills]
    for other in outs[1:]:
        for n in ("o", "lse", "dq", "dk", "dv"):
            assert torch.equal(outs[0][n], other[n]), f"{n} depends on the content of masked keys (S {S}, split {split})"
    for n in ("dk", "dv"):
        assert bool((outs[0][n][torch.from_numpy(~kv).to(DEV)] == 0).all()), f"{n}: masked keys must get exact zeros"


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 masked kernels against the fp64 masked reference at the large shapes
# ------------------------------------------------------------------------------------------------------------------------------
def _close_per_element(a, b, rtol, what, floor=None):
    """|a - b| <= rtol * max |b| of the same batch element (images with few valid keys have their own O / gradient scale); floor:
    a per-element lower limit of that scale, for an output that vanishes in exact arithmetic."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    for i in range(b.shape[0]):
        scale = max(float(b[i].abs().max()), floor[i] if floor is not None else 0.0) + 1e-30
        err = float((a[i] - b[i]).abs().max())
        assert err <= rtol * scale, f"{what} (element {i}): max abs err {err:.3e} > {rtol * scale:.3e} (scale {scale:.3e})"


F32_MASKS = ["rect", "random", "tiles", "first_half", "run_heads", "empty_runs_last", "single_valid", "far_tiles"]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind", F32_MASKS)
@pytest.mark.parametrize("B,T,S", [(2, 130, 2100), (1, 100, 8192)])
def test_masked_fp32_vs_fp64(hip, B, T, S, kind, p):
    """The tolerances of test_gpu_padding._check_attn for fp32, taken per batch element."""
    from oracle import dropout_ref as DR
    from oracle import attn_bounds as AB
    site, step, scale = 5, 12345, HD ** -0.5
    qs, k, v, do = _operands(B, T, S, 91 + S + AC.MASKS.index(kind), False)
    kv = AC.key_valid(kind, B, S, AB.parts_for(-(-S // 32)), seed=4)
    got = _f32_outputs(hip, qs, k, v, do, B, T, S, p, kv)
    q, kk, vv = (t.clone().requires_grad_(True) for t in (qs, k, v))
    qh, kh, vh = (t.view(B, -1, H, HD).transpose(1, 2) for t in (q, kk, vv))
    sc = ((qh * scale) @ kh.transpose(-1, -2)).masked_fill(torch.from_numpy(~kv)[:, None, None, :], float("-inf"))
    w = torch.softmax(sc, dim=-1)
    if p > 0.0:
        keep = torch.from_numpy(DR.keep_mask(DR.drop_key(site, step), DR.attn_index(B * H, T, S).reshape(B, H, T, S), p))
        w = torch.where(keep, w / (1.0 - p), torch.zeros_like(w))
    o = (w @ vh).transpose(1, 2).reshape(B, T, D)
    o.backward(do)
    tag = f"fp32 masked {kind} B{B} T{T} S{S} p{p}"
    _close_per_element(got["o"], o, 3e-5 if p > 0.0 else 2e-5, f"O {tag}")
    _close_per_element(got["lse"], torch.logsumexp(sc, dim=-1), 1e-5, f"lse {tag}")
    # one valid key: the softmax is constant, dS = P (dP - delta) = 0 and so dQ = dK = 0 exactly; the kernel's values are the rounding
    # of dP - delta, measured against the size of the terms that cancel (scale |dP| |K_j| for dQ, scale sum_i |dP_i| |q_i| for dK)
    fq, fk = [0.0] * B, [0.0] * B
    for b in range(B):
        if int(kv[b].sum()) == 1:
            j = int(np.flatnonzero(kv[b])[0])
            dp = (do[b].view(T, H, HD) * v[b, j].view(1, H, HD)).sum(dim=2).abs()                    # [T, H]
            fq[b] = scale * float(dp.max()) * float(k[b, j].abs().max())
            fk[b] = scale * float((dp.unsqueeze(2) * qs[b].view(T, H, HD).abs()).sum(dim=0).max())
    _close_per_element(got["dq"], q.grad, 5e-5, f"dQ {tag}", fq)
    _close_per_element(got["dk"], kk.grad, 5e-5, f"dK {tag}", fk)
    _close_per_element(got["dv"], vv.grad, 5e-5, f"dV {tag}")
    inv = torch.from_numpy(~kv).to(DEV)
    assert bool((got["dk"][inv] == 0).all()) and bool((got["dv"][inv] == 0).all()), f"masked keys must get exact zeros ({tag})"


# ------------------------------------------------------------------------------------------------------------------------------
# padding_mask_prepare feeding the masked attention at its largest feature map
# ------------------------------------------------------------------------------------------------------------------------------
def test_prepared_words_drive_masked_attention_at_8192_keys(hip):
    """Key words from padding_mask_prepare at a 64 x 128 feature map (8192 positions, 256 key tiles) feed the masked bf16 attention
    at (1, 100, 8192), checked against the per-element bounds under the heuristic and splits 1, 2, 3."""
    from detr_tf.engine import position_embedding_sine_table
    from oracle import attn_bounds as AB
    Hf, Wf, B, T = 64, 128, 1, 100
    S = Hf * Wf
    masks = np.ones((B, 512, 1024), bool)
    masks[0, :389, :701] = False
    kvw = torch.full((hip.attention_keymask_words(B, S),), -1, dtype=torch.int32, device=DEV)
    pos = torch.empty(B * S, 256, device=DEV)
    status = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    hip.padding_mask_prepare(torch.from_numpy(masks).to(DEV), Hf, Wf, torch.from_numpy(position_embedding_sine_table(Hf)).to(DEV),
                             torch.from_numpy(position_embedding_sine_table(Wf)).to(DEV), kvw, pos, status)
    torch.cuda.synchronize()
    assert int(status[0]) == 0
    words = kvw.cpu().numpy().view(np.uint32).reshape(B, -1)
    kv = torch.from_numpy(((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(B, -1)[:, :S])
    assert 0 < int(kv.sum()) < S
    p = 0.1
    keep = AC.keep_mask(B, T, S, p)
    qs, k, v, do = AC.scores_case("ascending", B, T, S, p, 4, keep, torch.Generator().manual_seed(8), key_valid=kv)
    dev = AC.device_operands(hip, qs, k, v, do, B, T, S, p, extra=X, key_valid=kv)
    dev["kw"]["key_valid"] = kvw                                  # the prepared words themselves
    fw = AB.forward(qs, k, v, H, keep, p, key_valid=kv)
    o0 = torch.full_like(dev["o"], -1234.0)
    AC.fwd(hip, dev, B, T, S, 0, o=o0)
    bw = AB.backward(qs, k, v, do, o0[:B * T].double().cpu().view(B, T, D), H, keep, p, key_valid=kv)
    worst = dict(o=0.0, lse=0.0, dq=0.0, dk=0.0, dv=0.0)
    for split in (0, 1, 2, 3):
        tag = f"prepared 64x128 split{split}"
        AC.fwd(hip, dev, B, T, S, split)
        r = dict(o=AC.check(f"O ({tag})", dev["o"][:B * T].float().view(B, T, D), fw["o"], fw["bound_o"]),
                 lse=AC.check(f"lse ({tag})", dev["lse"][:B * H * T].view(B * H, T), fw["lse"], fw["bound_lse"]))
        AC.bwd(hip, dev, B, T, S, split, o0, dev["lse"])
        r["dq"] = AC.check(f"dQ ({tag})", dev["dq"][:B * T].float().view(B, T, D), bw["dq"], bw["bound_dq"])
        r["dk"] = AC.check(f"dK ({tag})", dev["dk"][:B * S].float().view(B, S, D), bw["dk"], bw["bound_dk"])
        r["dv"] = AC.check(f"dV ({tag})", dev["dv"][:B * S].float().view(B, S, D), bw["dv"], bw["bound_dv"])
        AC.sentinels_intact(dev, B, T, S, X)
        for n in worst:
            worst[n] = max(worst[n], r[n])
    _report("prepared 64x128 ascending B1 T100 S8192 p0.1", worst)
