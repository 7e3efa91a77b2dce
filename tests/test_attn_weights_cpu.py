"""Head-averaged attention maps, host side: the C entry point's symbol and argument checks (no GPU), the fp64 restatement
tests/attn_weights_ref.py (head_mean_weights, detr_attention_maps) and the discrimination of the kernel's per-element bound."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

H, HD = 8, 32
D = H * HD
SHAPES = [(2, 1050, 1050), (2, 100, 1050), (2, 300, 333), (1, 100, 100), (1, 1, 33), (2, 37, 8192)]
GRID = {1050: (25, 42), 333: (9, 37), 100: (10, 10), 33: (3, 11), 8192: (64, 128)}


def _lib():
    from detr_tf import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip, _hip.load()


def test_attention_weights_symbol_declared_exported_mirrored():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    name = "detr_hip_attention_weights"
    assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9


def test_attention_weights_rejects_bad_arguments_without_a_gpu():
    _hip, lib = _lib()
    fake = 4096                                   # never dereferenced: every call below fails its checks first

    def desc(**kw):
        d = _hip.AttnDesc()
        d.B, d.H, d.T, d.S = 2, 8, 100, 1050
        d.q, d.k, d.lse = fake, fake, fake
        d.ldq, d.ldk = 256, 768
        d.scale, d.dropout_p, d.compute, d.io_dtype = HD ** -0.5, 0.0, 0, 0
        for n, v in kw.items():
            setattr(d, n, v)
        return d

    def rejected(d, text, w=fake, ldw=1050):
        rc = lib.detr_hip_attention_weights(ctypes.byref(d) if d is not None else None, None, w, ldw, None)
        msg = lib.detr_hip_last_error().decode()
        assert rc < 0 and text in msg, (rc, msg, text)

    rejected(None, "null descriptor")
    for n in ("q", "k", "lse"):
        rejected(desc(**{n: None}), "null operand")
    rejected(desc(), "null operand", w=None)
    for kw in (dict(B=0), dict(B=-1), dict(B=70000), dict(T=0), dict(S=0), dict(S=8193)):
        rejected(desc(**kw), "bad shape")
    for h in (0, -2, 9):
        rejected(desc(H=h), "heads")
    rejected(desc(), "ldw", ldw=1049)
    rejected(desc(dropout_p=0.1), "dropout_p")
    rejected(desc(io_dtype=2), "io_dtype")
    rejected(desc(compute=1), "bf16 compute (1) needs bf16 tensors")
    rejected(desc(io_dtype=1, compute=0), "need compute = 1")
    rejected(desc(io_dtype=1, compute=1, ldq=260), "row strides")          # bf16: multiples of 8
    rejected(desc(ldk=254), "row strides")                                 # fp32: multiples of 4
    rejected(desc(ldq=128), "row strides")                                 # < heads * 32
    rejected(desc(q=fake + 4), "16-byte aligned")
    rejected(desc(scale=0.0), "scale")


def test_head_mean_weights_properties():
    import attn_weights_ref as AW
    import padding_ref as PR
    g = torch.Generator().manual_seed(5)
    B, T, S = 2, 37, 75
    q = torch.randn(B, T, D, dtype=torch.float64, generator=g) * 2.0
    k = torch.randn(B, S, D, dtype=torch.float64, generator=g)
    pad = torch.rand(B, S, generator=g) < 0.4
    pad[:, 0] = False
    scale = HD ** -0.5
    w = AW.head_mean_weights(q, k, H, scale)
    wm = AW.head_mean_weights(q, k, H, scale, key_pad=pad)
    assert w.shape == (B, T, S)
    assert float((w.sum(dim=2) - 1).abs().max()) <= 1e-12 and float((wm.sum(dim=2) - 1).abs().max()) <= 1e-12
    assert bool((wm[pad[:, None, :].expand(B, T, S)] == 0).all())
    assert torch.equal(AW.head_mean_weights(q, k, H, scale, key_pad=torch.zeros(B, S, dtype=torch.bool)), w)
    # the head mean of padding_ref.masked_attention_core's weights
    from oracle.attn_bounds import heads
    _, wc = PR.masked_attention_core(heads(q * scale, H), heads(k, H), heads(k, H), key_pad=pad.repeat_interleave(H, dim=0))
    assert float((wc.reshape(B, H, T, S).mean(dim=1) - wm).abs().max()) <= 1e-15


def test_detr_attention_maps_records_without_touching_the_forward():
    import attn_weights_ref as AW
    import padding_ref as PR
    from oracle import detr_ref as R
    P = R.to_torch(R.make_params(3, num_enc=1, num_dec=2))
    images = np.random.default_rng(11).normal(size=(2, 128, 160, 3)).astype(np.float32)       # test_gpu_padding._small_inputs
    masks = np.zeros((2, 128, 160), bool)
    masks[1, 96:, :] = True
    masks[1, :, 128:] = True
    images[1][masks[1]] = 0.0
    sites = AW.site_names(1, 2)
    Pd = {n: t.double() for n, t in P.items()}
    x = torch.from_numpy(images).double()
    L, Q = 4 * 5, 100
    shapes = {AW.ENC_SITE.format(0): (2, L, L)}
    for i in range(2):
        shapes[AW.DEC_SELF_SITE.format(i)] = (2, Q, Q)
        shapes[AW.DEC_CROSS_SITE.format(i)] = (2, Q, L)
    for m in (None, masks):
        plain = R.detr_forward(x, Pd, num_enc=1, num_dec=2) if m is None else PR.detr_forward(x, m, Pd, num_enc=1, num_dec=2)
        maps, out = AW.detr_attention_maps(images, m, P, sites, num_enc=1, num_dec=2, with_outputs=True)
        assert (R if m is None else PR).multi_head_attention.__name__ == "multi_head_attention"       # restored
        assert torch.equal(out["pred_logits"], plain["pred_logits"]) and torch.equal(out["pred_boxes"], plain["pred_boxes"])
        assert all(torch.equal(a["pred_logits"], b["pred_logits"]) for a, b in zip(out["aux"], plain["aux"]))
        assert list(maps) == sites
        for s in sites:
            assert tuple(maps[s].shape) == shapes[s], (s, maps[s].shape)
            assert float((maps[s].sum(dim=2) - 1).abs().max()) <= 1e-12
        if m is not None:
            fm = PR.downsample_masks(m, 4, 5).reshape(2, L)
            for s in (AW.ENC_SITE.format(0), AW.DEC_CROSS_SITE.format(1)):
                assert bool((maps[s][fm[:, None, :].expand_as(maps[s])] == 0).all())
            assert bool((maps[AW.DEC_SELF_SITE.format(0)] > 0).all())                                   # never masked
    with pytest.raises(ValueError):
        AW.detr_attention_maps(images, None, P, ["transformer/encoder/layer_7/self_attn"], num_enc=1, num_dec=2)


def kernel_inputs(B, T, S, io16, kind, seed=0):
    """Operands of the kernel tests (also used by tests/test_gpu_attn_weights.py): bf16 form from tests/attn_cases.py
    ("second_chain": peaked rows next to flat ones, "ragged_max" for T < 64; masked: "masked_dominant", the masked keys ~30 log2 units above the valid
    ones), fp32 form random normal with the unscaled query; key_valid of kind "rect" / "random" / None; lse_in = fp32 of the fp64
    log-sum-exp."""
    import attn_cases as AC
    import attn_weights_ref as AW
    g = torch.Generator().manual_seed(100 + seed)
    kv = None if kind is None else AC.key_valid(kind, B, S, seed=seed, grid=GRID[S])
    if io16:
        # ("second_chain" zeroes the first 32 queries of every 64: with T < 64 every row would be flat and all heads alike)
        case = "masked_dominant" if kv is not None else ("second_chain" if T >= 64 else "ragged_max")
        q, k, _, _ = AC.scores_case(case, B, T, S, 0.0, 1, None, g, key_valid=kv)
    else:
        q = (2.0 * torch.randn(B, T, D, dtype=torch.float64, generator=g)).float().double()
        k = torch.randn(B, S, D, dtype=torch.float64, generator=g).float().double()
    lse = AW.lse_of(q, k, H, io16, key_valid=kv)
    return q, k, lse, kv


@pytest.mark.parametrize("io16", [True, False], ids=["bf16io", "fp32"])
@pytest.mark.parametrize("B,T,S", SHAPES)
def test_bound_accepts_a_correct_execution_and_rejects_wrong_ones(B, T, S, io16):
    import attn_weights_ref as AW
    from oracle.attn_bounds import ratio
    kind = "random" if S in (333, 33, 8192) else "rect"
    for masked in (False, True):
        q, k, lse, kv = kernel_inputs(B, T, S, io16, kind if masked else None)
        W, Bw = AW.kernel_reference_and_bound(q, k, lse, H, io16, key_valid=kv)
        r = ratio(AW.simulate(q, k, lse, H, io16, key_valid=kv), W, Bw)
        print(f"B{B} T{T} S{S} io16={io16} masked={masked}: correct execution ratio {r:.3f}")
        assert r <= 1.0
        for fault in AW.FAULTS:
            if fault == "mask_of_entry0" and (kv is None or B < 2):
                continue
            rf = ratio(AW.simulate(q, k, lse, H, io16, key_valid=kv, fault=fault), W, Bw)
            print(f"    {fault}: ratio {rf:.3g}")
            assert rf > 1.0, f"the bound cannot tell `{fault}` from a correct execution (ratio {rf:.3f})"
