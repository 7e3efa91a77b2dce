"""Dilation-aware restatement of the backbone for the DC5 models (test reference; torch on the CPU, fp64-capable, differentiable).

oracle.detr_ref.backbone hard-codes stride 2 / pad 1 for every stage; the reference's ResidualBlock (resnet_backbone.py:69-85) takes
`replace_stride_with_dilation`: a flagged stage runs at stride 1, its first block at dilation 1, every later block with
ZeroPadding2D(2) + Conv2D(3x3, dilation_rate=2) (:98,104-105).  This module restates only that, from the oracle's own pieces
(conv2d_valid already takes `dilation`; frozen_bn; the transformer and the heads through detr_forward itself).
"""
import functools
from unittest import mock

import torch
import torch.nn.functional as F

from oracle import detr_ref as R
from oracle.detr_ref import RESNET50_BLOCKS

import padding_ref as PR


def bottleneck_dc5(x, P, p, stride, downsample, dilation, taps=None):
    """BottleNeck.call resnet_backbone.py:116-137 with self.pad = ZeroPadding2D(dilation), conv2 dilation_rate = dilation."""
    y1 = torch.relu(R.frozen_bn(R.conv2d_valid(x, P[f"{p}/conv1/kernel"]), P, f"{p}/bn1"))
    y2 = torch.relu(R.frozen_bn(R.conv2d_valid(y1, P[f"{p}/conv2/kernel"], stride=stride, pad=dilation, dilation=dilation), P, f"{p}/bn2"))
    out = R.frozen_bn(R.conv2d_valid(y2, P[f"{p}/conv3/kernel"]), P, f"{p}/bn3")
    identity = R.frozen_bn(R.conv2d_valid(x, P[f"{p}/downsample_0/kernel"], stride=stride), P, f"{p}/downsample_1") if downsample else x
    return torch.relu(out + identity)


def backbone_dc5(images_nhwc, P, blocks=RESNET50_BLOCKS, flags=(False, False, False), taps=None):
    """ResNetBase.call resnet_backbone.py:20-32 over ResidualBlocks built with replace_stride_with_dilation = flags (layer2..4)."""
    flags = tuple(bool(f) for f in flags)
    assert len(flags) == 3
    x = R.conv2d_valid(images_nhwc, P["backbone/conv1/kernel"], stride=2, pad=3)
    x = torch.relu(R.frozen_bn(x, P, "backbone/bn1"))
    if taps is not None:
        taps["stem_conv"] = x
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), value=0.0)
    x = F.max_pool2d(xp, 3, 2).permute(0, 2, 3, 1)
    if taps is not None:
        taps["stem_pool"] = x
    for li, nb in enumerate(blocks):
        dilated = li > 0 and flags[li - 1]
        for b in range(nb):
            stride = 2 if (b == 0 and li > 0 and not dilated) else 1      # :74-76,80-81
            dilation = 2 if (dilated and b > 0) else 1                    # :80-85: block 0 keeps dilation 1
            x = bottleneck_dc5(x, P, f"backbone/layer{li + 1}/{b}", stride, b == 0, dilation, taps)
        if taps is not None:
            taps[f"layer{li + 1}"] = x
    return x


def _patched(flags):
    """oracle.detr_ref with its backbone() replaced by backbone_dc5(flags): detr_hs / detr_forward look it up at call time."""
    def bb(images_nhwc, P, blocks=RESNET50_BLOCKS, taps=None):
        return backbone_dc5(images_nhwc, P, blocks, flags, taps)
    return mock.patch.object(R, "backbone", bb)


def detr_forward_dc5(images_nhwc, P, blocks=RESNET50_BLOCKS, flags=(False, False, True), num_enc=6, num_dec=6, taps=None, drop=None):
    """oracle.detr_ref.detr_forward (position encoding, input_proj, transformer, heads: the oracle's own code) on backbone_dc5."""
    with _patched(flags):
        return R.detr_forward(images_nhwc, P, blocks, num_enc, num_dec, taps, drop)


def detr_forward_dc5_masked(images_nhwc, masks, P, blocks=RESNET50_BLOCKS, flags=(False, False, True), num_enc=6, num_dec=6, taps=None):
    """padding_ref.detr_forward -- the (images, masks) input of a padded batch -- on backbone_dc5: its mask helper then runs at the
    dilated model's feature size (taps["feat_mask"])."""
    with _patched(flags):
        return PR.detr_forward(images_nhwc, masks, P, blocks, num_enc, num_dec, taps)


def feature_mask(masks, H, W, flags):
    """padding_ref.downsample_masks at the feature size of an H x W input under `flags`."""
    for halves in (True, True) + tuple(not f for f in flags):
        if halves:
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return PR.downsample_masks(masks, H, W)


def conv_dilated_planes(x_nchw, w_oihw):
    """The parity-plane identity the kernel is built on: a dilation-2, pad-2, stride-1 3x3 convolution as four dense pad-1
    convolutions, one per (row parity, column parity) plane."""
    out = torch.zeros(x_nchw.shape[0], w_oihw.shape[0], x_nchw.shape[2], x_nchw.shape[3], dtype=x_nchw.dtype)
    for py in range(2):
        for px in range(2):
            plane = x_nchw[:, :, py::2, px::2]
            if plane.numel():
                out[:, :, py::2, px::2] = F.conv2d(plane, w_oihw, padding=1)
    return out
