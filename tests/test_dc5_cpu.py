"""DC5 backbones, host side: the reference's self-check, feature_size, the appended C ABI and the constructors (no GPU)."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import dc5_ref
from oracle import detr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- reference self-check ------------------------------------------------------------------
def test_dc5_ref_without_flags_is_the_oracle_backbone():
    P = R.to_torch(R.make_params(7, num_enc=1, num_dec=2))
    x = torch.randn(2, 64, 96, 3, generator=torch.Generator().manual_seed(1))
    assert torch.equal(dc5_ref.backbone_dc5(x, P, flags=(False, False, False)), R.backbone(x, P))
    a = dc5_ref.detr_forward_dc5(x, P, flags=(False, False, False), num_enc=1, num_dec=2)
    b = R.detr_forward(x, P, num_enc=1, num_dec=2)
    assert torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_boxes"], b["pred_boxes"])
    assert R.backbone.__module__ == "oracle.detr_ref"          # the patch was undone


def test_dc5_ref_feature_sizes():
    P = R.to_torch(R.make_params(7, num_enc=1, num_dec=2))
    x = torch.randn(1, 72, 104, 3, generator=torch.Generator().manual_seed(2))
    assert tuple(dc5_ref.backbone_dc5(x, P, flags=(False, False, True)).shape) == (1, 5, 7, 2048)
    assert tuple(dc5_ref.backbone_dc5(x, P, flags=(False, False, False)).shape) == (1, 3, 4, 2048)


@pytest.mark.parametrize("H,W", [(5, 7), (6, 8), (1, 3)])
def test_parity_plane_identity_fp64(H, W):
    """A dilation-2, pad-2 3x3 convolution is four dense pad-1 convolutions on the parity planes (fp64: summation order only)."""
    gen = torch.Generator().manual_seed(10 * H + W)
    x = torch.randn(2, 4, H, W, dtype=torch.float64, generator=gen)
    w = torch.randn(6, 4, 3, 3, dtype=torch.float64, generator=gen)
    ref = F.conv2d(x, w, padding=2, dilation=2)
    assert float((dc5_ref.conv_dilated_planes(x, w) - ref).abs().max()) <= 1e-13


# ---- feature_size --------------------------------------------------------------------------
def test_feature_size():
    from detr_tf.engine import feature_size
    assert feature_size(800, 1333) == (25, 42) and feature_size(72, 104) == (3, 4) and feature_size(1, 1) == (1, 1)
    assert feature_size(800, 1333, None) == (25, 42) and feature_size(800, 1333, [False] * 3) == (25, 42)
    assert feature_size(800, 1333, [False, False, True]) == (50, 84)
    assert feature_size(72, 104, [False, False, True]) == (5, 7)
    assert feature_size(72, 104, [False, True, True]) == (9, 13)          # two flags compose
    assert feature_size(72, 104, [True, True, True]) == (18, 26)
    with pytest.raises(ValueError):
        feature_size(72, 104, [True])


# ---- C ABI ---------------------------------------------------------------------------------
NEW_SYMBOLS = ("detr_hip_conv3x3_dilated", "detr_hip_workspace_bytes_conv3x3_dilated")


def test_abi_version_stays_and_the_symbols_are_appended():
    from detr_tf import _hip
    lib = _hip.load()
    assert lib.detr_hip_abi_version() == 9 == _hip.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    assert "#define DETR_HIP_ABI_VERSION 9" in header
    for name in NEW_SYMBOLS:
        assert name in header and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert header.index("detr_conv3x3d_desc;") > header.index("detr_hip_adamw_f32")          # appended, behind the newest entry
    assert [f[0] for f in _hip.Conv3x3DDesc._fields_] == [f[0] for f in _hip.Conv3x3Desc._fields_] + ["dilation"]


def test_conv3x3d_desc_size_matches_the_header(tmp_path):
    from detr_tf import _hip
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "detr_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(detr_conv3x3d_desc), offsetof(detr_conv3x3d_desc, dilation), '
                   'sizeof(detr_conv3x3_desc)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off, dense = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert size == ctypes.sizeof(_hip.Conv3x3DDesc) and off == _hip.Conv3x3DDesc.dilation.offset
    assert dense == ctypes.sizeof(_hip.Conv3x3Desc)


def _desc(**kw):
    from detr_tf import _hip
    d = _hip.Conv3x3DDesc()
    d.N, d.Hi, d.Wi, d.Ci, d.Ho, d.Wo, d.Co, d.stride, d.pad, d.dilation = 2, 5, 7, 64, 5, 7, 64, 1, 2, 2
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("bad,word", [(dict(dilation=1), "dilation"), (dict(dilation=3), "dilation"), (dict(stride=2), "stride"),
                                      (dict(pad=1), "pad"), (dict(Ho=3), "output"), (dict(Wo=4), "output")])
def test_malformed_descriptors_are_rejected_without_a_device(bad, word):
    from detr_tf import _hip
    lib = _hip.load()
    d = _desc(**bad)
    for mode in (0, 1, 2):
        assert lib.detr_hip_conv3x3_dilated(ctypes.byref(d), mode, None) == -1
        assert word in lib.detr_hip_last_error().decode()
    assert lib.detr_hip_workspace_bytes_conv3x3_dilated(ctypes.byref(d), 2) < 0


def test_null_descriptor_and_bad_mode_are_rejected():
    from detr_tf import _hip
    lib = _hip.load()
    assert lib.detr_hip_conv3x3_dilated(None, 0, None) == -1 and "null descriptor" in lib.detr_hip_last_error().decode()
    assert lib.detr_hip_workspace_bytes_conv3x3_dilated(None, 2) < 0
    d = _desc()
    assert lib.detr_hip_conv3x3_dilated(ctypes.byref(d), 3, None) == -1
    assert lib.detr_hip_conv3x3_dilated(ctypes.byref(d), 0, None) == -1 and "null operand" in lib.detr_hip_last_error().decode()


def test_workspace_query_and_the_4gb_guard():
    from detr_tf import _hip
    lib = _hip.load()
    d = _desc()
    assert lib.detr_hip_workspace_bytes_conv3x3_dilated(ctypes.byref(d), 0) == 0
    assert lib.detr_hip_workspace_bytes_conv3x3_dilated(ctypes.byref(d), 1) == 0
    big = _desc(N=8, Hi=100, Wi=167, Ho=100, Wo=167, Ci=512, Co=512, compute=1, x_dtype=1, w_dtype=1)
    n = lib.detr_hip_workspace_bytes_conv3x3_dilated(ctypes.byref(big), 2)
    assert n > 0 and n % (9 * 512 * 512 * 4) == 0                       # whole per-split slabs
    # 32-bit buffer offsets: a tensor past 4 GB is rejected, not wrapped (checked before any pointer is used)
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p).value & ~15
    huge = _desc(N=64, Hi=400, Wi=668, Ho=400, Wo=668, Ci=512, Co=512, x=p, w=p, y=p)
    assert lib.detr_hip_conv3x3_dilated(ctypes.byref(huge), 0, None) == -1
    assert "4 GB" in lib.detr_hip_last_error().decode()


def test_binding_rejects_other_dilations():
    from detr_tf import _hip
    with pytest.raises(ValueError):
        _hip.conv3x3(0, None, None, None, 1, 4, 4, 64, 4, 4, 64, 1, dilation=3)


# ---- constructors --------------------------------------------------------------------------
def test_constructors_take_the_new_arguments():
    from detr_tf.engine import DetrEngine
    from detr_tf.networks.detr import DetrModel, get_detr_model, resolve_backbone
    for fn in (get_detr_model, DetrModel.__init__, DetrEngine.__init__):
        assert "replace_stride_with_dilation" in inspect.signature(fn).parameters, fn
    assert inspect.signature(get_detr_model).parameters["replace_stride_with_dilation"].default is None
    assert resolve_backbone("resnet50")[1] == (False, False, False)
    assert resolve_backbone("resnet50-dc5")[1] == (False, False, True)
    blocks, flags = resolve_backbone("resnet101-dc5")
    assert tuple(blocks) == (3, 4, 23, 3) and flags == (False, False, True)
    assert resolve_backbone("resnet50", [True, False, True])[1] == (True, False, True)
    with pytest.raises(ValueError):
        resolve_backbone("resnet50-dc5", [True, False, False])
    with pytest.raises(ValueError):
        resolve_backbone("resnet18")


def test_tf_backbone_with_a_flag_raises_before_any_device_is_needed():
    from detr_tf.networks.detr import DetrModel, get_detr_model
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    before = cfg.normalized_method
    with pytest.raises(ValueError, match="replace_stride_with_dilation"):
        get_detr_model(cfg, include_top=True, tf_backbone=True, replace_stride_with_dilation=[False, False, True])
    assert cfg.normalized_method == before
    with pytest.raises(ValueError, match="replace_stride_with_dilation"):
        DetrModel(tf_backbone=True, replace_stride_with_dilation=[True, False, False])
    with pytest.raises(ValueError):
        DetrModel(tf_backbone=True, backbone="resnet50-dc5")
