"""Padded mixed-size batches, host side: the masked fp64 restatement (tests/padding_ref.py) against the unmasked oracle and
against cropped feature maps, the host sine tables the mask-preparation kernel gathers from, the nearest-neighbour mask
downsampling rule, the key-validity word layout, and the new C-ABI entry points' exports and argument checks."""
import ctypes
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import padding_ref as PR                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("detr_hip_attention_keymask_words", "detr_hip_attention_fwd_masked", "detr_hip_attention_bwd_masked",
               "detr_hip_padding_mask_prepare", "detr_hip_input_stage_padded")


def test_all_false_mask_restatement_equals_the_oracle_exactly():
    """padding_ref.detr_forward with an all-False mask is oracle.detr_ref.detr_forward, bit for bit in fp64."""
    from oracle import detr_ref as R
    params = R.make_params(5, num_enc=1, num_dec=2)
    P = R.to_torch(params, dtype=torch.float64)
    images = torch.from_numpy(np.random.default_rng(3).normal(size=(2, 64, 96, 3)))
    ref = R.detr_forward(images, P, num_enc=1, num_dec=2)
    got = PR.detr_forward(images, np.zeros((2, 64, 96), bool), P, num_enc=1, num_dec=2)
    assert torch.equal(got["pred_logits"], ref["pred_logits"])
    assert torch.equal(got["pred_boxes"], ref["pred_boxes"])
    for a, b in zip(got["aux"], ref["aux"]):
        assert torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_boxes"], b["pred_boxes"])


def test_masked_transformer_equals_the_cropped_feature_map():
    """A top-left valid region of a padded feature map gives, at its positions, the transformer output of the cropped map run
    unmasked: masked keys contribute nothing, and the normalised encoding only counts valid positions (fp64, 1e-12)."""
    from oracle import detr_ref as R
    P = R.to_torch(R.make_params(9, num_enc=2, num_dec=2), dtype=torch.float64)
    rng = np.random.default_rng(4)
    Hf, Wf, h, w = 7, 9, 5, 6
    src = torch.from_numpy(rng.normal(size=(1, Hf, Wf, 256)))
    src[:, h:, :] = torch.from_numpy(rng.normal(size=(1, Hf - h, Wf, 256)) * 50.0)   # padding content must not matter
    src[:, :, w:] = 1e3
    fmask = torch.ones(1, Hf, Wf, dtype=torch.bool)
    fmask[:, :h, :w] = False
    taps_p, taps_c = {}, {}
    hs_p = PR.transformer(src, fmask, P["query_embed/kernel"], P, 2, 2, taps=taps_p)
    hs_c = PR.transformer(src[:, :h, :w].contiguous(), torch.zeros(1, h, w, dtype=torch.bool), P["query_embed/kernel"], P, 2, 2, taps=taps_c)
    mem_p = taps_p["memory"].reshape(Hf, Wf, 256)[:h, :w]
    mem_c = taps_c["memory"].reshape(h, w, 256)
    assert float((mem_p - mem_c).abs().max()) <= 1e-12 * float(mem_c.abs().max())
    assert float((hs_p - hs_c).abs().max()) <= 1e-12 * float(hs_c.abs().max())
    # and the restated encoding at valid positions equals the unmasked one of the cropped size
    pos_c = R.position_embedding_sine(1, h, w, dtype=torch.float64)
    assert float((taps_p["pos"][0, :h, :w] - pos_c[0]).abs().max()) <= 1e-12


def test_host_sine_tables_reproduce_the_unmasked_constant_bit_for_bit():
    from detr_tf.engine import position_embedding_sine_host, position_embedding_sine_table
    for Hf, Wf in ((4, 5), (25, 42), (42, 25), (1, 1), (13, 7)):
        ty, tx = position_embedding_sine_table(Hf), position_embedding_sine_table(Wf)
        assert ty.shape == (Hf + 1, Hf + 1, 128) and ty.dtype == np.float32
        i, j = np.meshgrid(np.arange(Hf), np.arange(Wf), indexing="ij")
        gathered = np.concatenate([ty[Hf, i + 1], tx[Wf, j + 1]], axis=2).reshape(Hf * Wf, 256)     # all valid: c = index + 1, n = side
        want = position_embedding_sine_host(Hf, Wf)
        assert gathered.tobytes() == want.tobytes(), (Hf, Wf)
        # a fully padded axis (n = 0, c = 0): sin 0 = 0, cos 0 = 1
        assert np.array_equal(ty[0, 0, 0::2], np.zeros(64, np.float32)) and np.array_equal(ty[0, 0, 1::2], np.ones(64, np.float32))


def test_host_sine_table_gather_follows_the_fp64_restatement():
    """Gathering by (cumulative count, axis total) for an arbitrary mask: within 1e-6 of the fp64 normalised encoding."""
    from detr_tf.engine import position_embedding_sine_table
    rng = np.random.default_rng(7)
    Hf, Wf = 9, 11
    mask = rng.random((2, Hf, Wf)) < 0.35
    mask[1, :, 8:] = True
    mask[1, 6:, :] = True
    ty, tx = position_embedding_sine_table(Hf), position_embedding_sine_table(Wf)
    nm = ~mask
    cy, cx = np.cumsum(nm, 1), np.cumsum(nm, 2)
    ny, nx = cy[:, -1:, :].repeat(Hf, 1), cx[:, :, -1:].repeat(Wf, 2)
    got = np.concatenate([ty[ny, cy], tx[nx, cx]], axis=3)
    want = PR.position_embedding_sine_masked(torch.from_numpy(mask)).numpy()
    assert float(np.abs(got - want).max()) <= 1e-6


def test_nearest_downsample_rule_on_odd_sizes():
    from detr_tf.engine import downsample_mask_nearest, feature_size
    rng = np.random.default_rng(1)
    for (H, W, Hf, Wf) in ((13, 17, 5, 7), (97, 131, 4, 5), (7, 7, 7, 7), (5, 3, 9, 4), (800, 1333, 25, 42)):
        m = rng.random((2, H, W)) < 0.5
        want = np.empty((2, Hf, Wf), bool)
        for i in range(Hf):
            for j in range(Wf):
                want[:, i, j] = m[:, min((i * H) // Hf, H - 1), min((j * W) // Wf, W - 1)]
        assert np.array_equal(downsample_mask_nearest(m, Hf, Wf), want)
        assert np.array_equal(PR.downsample_masks(m, Hf, Wf).numpy(), want)
    assert feature_size(800, 1333) == (25, 42) and feature_size(128, 160) == (4, 5) and feature_size(96, 128) == (3, 4)


def test_key_validity_word_layout():
    from detr_tf import _hip
    rng = np.random.default_rng(2)
    valid = rng.random((3, 77)) < 0.5
    w = _hip.keymask_words_from_valid(valid).view(np.uint32)
    assert w.shape == (3, 3)
    for b in range(3):
        for s in range(96):
            bit = (int(w[b, s // 32]) >> (s % 32)) & 1
            assert bit == (int(valid[b, s]) if s < 77 else 0)


def test_new_exports_are_declared_and_mirrored():
    from detr_tf import _hip
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    lib = _hip.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9


def test_masked_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument checks run on the host before anything touches device memory: negative code + last_error."""
    from detr_tf import _hip
    lib = _hip.load()
    assert lib.detr_hip_attention_keymask_words(2, 1050) == 2 * 33
    assert lib.detr_hip_attention_keymask_words(0, 5) < 0 and lib.detr_hip_attention_keymask_words(2, 0) < 0
    d = _hip.AttnDesc()
    d.B, d.H, d.T, d.S = 2, 8, 100, 1050
    d.io_dtype, d.compute = 0, 1
    fake = ctypes.c_void_p(4096)              # never dereferenced: every call below fails its checks first
    assert lib.detr_hip_attention_fwd_masked(ctypes.byref(d), fake, None) < 0
    assert "io_dtype = 0, compute = 1" in lib.detr_hip_last_error().decode()
    assert lib.detr_hip_attention_bwd_masked(ctypes.byref(d), fake, None) < 0
    d.compute = 0
    assert lib.detr_hip_attention_fwd_masked(ctypes.byref(d), None, None) < 0
    assert "key_valid" in lib.detr_hip_last_error().decode()
    assert lib.detr_hip_attention_fwd_masked(None, fake, None) < 0
    d.io_dtype = 2
    assert lib.detr_hip_attention_fwd_masked(ctypes.byref(d), fake, None) < 0
    assert "io_dtype" in lib.detr_hip_last_error().decode()
    # mask preparation: null operands, feature maps past the kernel's limits
    assert lib.detr_hip_padding_mask_prepare(None, 2, 64, 64, 2, 2, fake, fake, fake, fake, fake, None) < 0
    assert lib.detr_hip_padding_mask_prepare(fake, 1, 64, 64, 200, 2, fake, fake, fake, fake, fake, None) < 0
    assert "exceeds" in lib.detr_hip_last_error().decode()
    assert lib.detr_hip_padding_mask_prepare(fake, 0, 64, 64, 2, 2, fake, fake, fake, fake, fake, None) < 0
    bad_perm = (ctypes.c_int32 * 3)(0, 1, 3)
    assert lib.detr_hip_input_stage_padded(fake, fake, fake, 1, 8, 8, fake, ctypes.cast(bad_perm, ctypes.c_void_p), fake, fake, None) < 0
    assert "permutation" in lib.detr_hip_last_error().decode()
    assert lib.detr_hip_input_stage_padded(fake, fake, fake, 0, 8, 8, fake, ctypes.cast(bad_perm, ctypes.c_void_p), fake, fake, None) < 0
