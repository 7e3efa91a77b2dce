"""Masked restatement of the DETR forward for padded mixed-size batches (test reference, float64 torch).

The reference declares the padding-mask interface without using it (detr_tf/networks/detr.py:57-72 `downsample_masks` and
`x, masks = inp`, position_embeddings.py:23-50 built on `not_mask = ~mask` with normalize=True, transformer.py:322-337 the
commented-out key_padding_mask branch, fed by source_key_padding_mask / memory_key_padding_mask at :43-50).  This module
restates those lines as if enabled, on top of oracle.detr_ref's backbone, linear, layer_norm and FFN pieces:
  * masks: bool [B, H, W], True = padding;
  * downsampling: TF-legacy nearest neighbour, src = min(floor(dst * in / out), in - 1) per axis;
  * masked keys get a score of -inf before the softmax (encoder self-attention and decoder cross-attention only);
    queries are never masked.
"""
import math

import numpy as np
import torch

from oracle import detr_ref as R
from oracle.detr_ref import RESNET50_BLOCKS


def downsample_masks(masks, Hf, Wf):
    """detr.py:57-63 (tf.image.resize nearest, legacy): bool [B, H, W] -> bool [B, Hf, Wf]."""
    masks = torch.as_tensor(np.asarray(masks)).bool()
    H, W = masks.shape[1:]
    sy = torch.clamp((torch.arange(Hf) * H) // Hf, max=H - 1)
    sx = torch.clamp((torch.arange(Wf) * W) // Wf, max=W - 1)
    return masks[:, sy][:, :, sx]


def position_embedding_sine_masked(mask, num_pos_features=128, temperature=10000.0, eps=1e-6, dtype=torch.float64):
    """position_embeddings.py:23-50 with normalize=True: mask bool [B, H, W] (True = padding) -> [B, H, W, 256]."""
    not_mask = (~mask).to(dtype)
    y_embed = torch.cumsum(not_mask, 1)
    x_embed = torch.cumsum(not_mask, 2)
    scale = 2 * math.pi
    y_embed = y_embed / (y_embed[:, -1:, :] + eps) * scale
    x_embed = x_embed / (x_embed[:, :, -1:] + eps) * scale
    dim_t = torch.arange(num_pos_features, dtype=dtype)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_features)
    B, H, W = mask.shape
    pos_x = x_embed[..., None] / dim_t
    pos_y = y_embed[..., None] / dim_t
    pos_x = torch.stack([pos_x[..., 0::2].sin(), pos_x[..., 1::2].cos()], dim=4).reshape(B, H, W, -1)
    pos_y = torch.stack([pos_y[..., 0::2].sin(), pos_y[..., 1::2].cos()], dim=4).reshape(B, H, W, -1)
    return torch.cat([pos_y, pos_x], dim=3)


def masked_attention_core(q, k, v, key_pad=None):
    """softmax(q k^T + mask) v on [BH, T, hd] / [BH, S, hd]; key_pad bool [BH, S] (True = masked key -> -inf score)."""
    s = q @ k.transpose(1, 2)
    if key_pad is not None:
        s = s.masked_fill(key_pad[:, None, :], float("-inf"))
    w = torch.softmax(s, dim=-1)
    return w @ v, w


def multi_head_attention(query, key, value, P, p, num_heads=8, drop=None, seed=0, key_padding_mask=None):
    """oracle.detr_ref.multi_head_attention plus the key_padding_mask branch of transformer.py:322-337 (bool [B, S], True = pad)."""
    T, B, D = query.shape
    S = key.shape[0]
    hd = D // num_heads
    W, b = P[f"{p}/in_proj_kernel"], P[f"{p}/in_proj_bias"]
    WQ = (query @ W[:D].t() + b[:D]) * float(hd) ** -0.5
    WK = key @ W[D:2 * D].t() + b[D:2 * D]
    WV = value @ W[2 * D:].t() + b[2 * D:]
    WQ = WQ.reshape(T, B * num_heads, hd).transpose(0, 1)
    WK = WK.reshape(S, B * num_heads, hd).transpose(0, 1)
    WV = WV.reshape(S, B * num_heads, hd).transpose(0, 1)
    s = WQ @ WK.transpose(1, 2)
    if key_padding_mask is not None:
        kp = key_padding_mask[:, None, None, :].expand(B, num_heads, 1, S).reshape(B * num_heads, 1, S)
        s = s.masked_fill(kp, float("-inf"))
    w = torch.softmax(s, dim=-1)
    if drop is not None:
        w = drop(seed + 0, w, "attn")
    o = (w @ WV).transpose(0, 1).reshape(T, B, D)
    out = o @ P[f"{p}/out_proj_kernel"].t() + P[f"{p}/out_proj_bias"]
    if drop is not None:
        out = drop(seed + 1, out, "lbc")
    return out


def encoder_layer(src, pos, P, p, drop=None, seed=0, kpm=None):
    q = k = src + pos
    src = R.layer_norm(src + multi_head_attention(q, k, src, P, f"{p}/self_attn", drop=drop, seed=seed, key_padding_mask=kpm),
                       P, f"{p}/norm1")
    return R.layer_norm(src + R._ffn(src, P, p, drop, seed + 2), P, f"{p}/norm2")


def decoder_layer(tgt, memory, pos, qpos, P, p, drop=None, seed=0, kpm=None):
    q = k = tgt + qpos
    tgt = R.layer_norm(tgt + multi_head_attention(q, k, tgt, P, f"{p}/self_attn", drop=drop, seed=seed), P, f"{p}/norm1")
    tgt = R.layer_norm(tgt + multi_head_attention(tgt + qpos, memory + pos, memory, P, f"{p}/multihead_attn", drop=drop,
                                                  seed=seed + 2, key_padding_mask=kpm), P, f"{p}/norm2")
    return R.layer_norm(tgt + R._ffn(tgt, P, p, drop, seed + 4), P, f"{p}/norm3")


def transformer(src_nhwc, feat_mask, query_embed, P, num_enc=6, num_dec=6, taps=None, drop=None):
    """Transformer.call transformer.py:29-57 with source / memory key padding masks; feat_mask bool [B, Hf, Wf] (True = pad)."""
    B, H, W, D = src_nhwc.shape
    pos_nhwc = position_embedding_sine_masked(feat_mask, dtype=src_nhwc.dtype)
    src = src_nhwc.reshape(B, H * W, D).transpose(0, 1)
    pos = pos_nhwc.reshape(B, H * W, D).transpose(0, 1)
    kpm = feat_mask.reshape(B, H * W)
    qpos = query_embed[:, None, :].expand(-1, B, -1)
    x = src
    for i in range(num_enc):
        x = encoder_layer(x, pos, P, f"transformer/encoder/layer_{i}", drop, 16 * i, kpm)
    memory = x
    if taps is not None:
        taps["memory"] = memory
        taps["pos"] = pos_nhwc
    inter = []
    x = torch.zeros_like(qpos)
    for i in range(num_dec):
        x = decoder_layer(x, memory, pos, qpos, P, f"transformer/decoder/layer_{i}", drop, 16 * (32 + i), kpm)
        inter.append(R.layer_norm(x, P, "transformer/decoder/norm"))
    return torch.stack(inter, 0).transpose(1, 2)


def detr_hs(images_nhwc, masks, P, blocks=RESNET50_BLOCKS, num_enc=6, num_dec=6, taps=None, drop=None):
    x = R.backbone_tf(images_nhwc, P, blocks, taps) if "resnet50/conv1_conv/kernel" in P else R.backbone(images_nhwc, P, blocks, taps)
    B, Hf, Wf, _ = x.shape
    fmask = downsample_masks(masks, Hf, Wf)
    proj = R.conv2d_valid(x, P["input_proj/kernel"]) + P["input_proj/bias"]
    if taps is not None:
        taps["input_proj"] = proj
        taps["feat_mask"] = fmask
    return transformer(proj, fmask, P["query_embed/kernel"], P, num_enc, num_dec, taps, drop)


def detr_forward(images_nhwc, masks, P, blocks=RESNET50_BLOCKS, num_enc=6, num_dec=6, taps=None, drop=None):
    """oracle.detr_ref.detr_forward with the reference's (images, masks) input."""
    hs = detr_hs(images_nhwc, masks, P, blocks, num_enc, num_dec, taps, drop)
    if taps is not None:
        taps["hs"] = hs
    if "class_embed/kernel" in P:
        logits = R.linear(hs, P, "class_embed")
        t = torch.relu(R.linear(hs, P, "bbox_embed_0"))
        t = torch.relu(R.linear(t, P, "bbox_embed_1"))
        boxes = torch.sigmoid(R.linear(t, P, "bbox_embed_2"))
        n_aux = num_dec - 1
    else:
        logits = hs @ P["cls_layer/kernel"] + P["cls_layer/bias"]
        t = torch.relu(hs @ P["pos_layer/dense_0/kernel"] + P["pos_layer/dense_0/bias"])
        t = torch.relu(t @ P["pos_layer/dense_1/kernel"] + P["pos_layer/dense_1/bias"])
        boxes = torch.sigmoid(t @ P["pos_layer/dense_2/kernel"] + P["pos_layer/dense_2/bias"])
        n_aux = 5
    out = {"pred_logits": logits[-1], "pred_boxes": boxes[-1]}
    out["aux"] = [{"pred_logits": logits[i], "pred_boxes": boxes[i]} for i in range(n_aux)]
    return out
