"""DETR execution engine for MI355X: the forward and the hand-written backward of the whole
hot path (ResNet backbone -> 6+6 transformer -> heads) as an explicit sequence of launches of
the HIP kernels in libdetr_hip.so.  No autograd graph, no allocation in the step: every
activation lives in a named, cached device buffer (static memory plan, hipGraph friendly).

Internal layout: NHWC feature maps, i.e. batch-first token matrices [B*L, 256]; this is the
reference's [L, B, 256] (transformer.py:32-33) with the two transposes removed -- every op of
the transformer is row-wise except attention, which addresses (batch, head) through strides.

Reference lines implemented (paths relative to the reference root):
  backbone   detr_tf/networks/resnet_backbone.py:20-32,116-137, custom_layers.py:21-24
  pos enc    detr_tf/networks/position_embeddings.py:23-50 (constant for a zero mask, detr.py:172)
  transformer detr_tf/networks/transformer.py:29-57,157-179,207-234,285-356
  heads      detr_tf/networks/detr.py:94-114,181-204
  backward   what tape.gradient (detr_tf/optimizers.py:115) computes for the graph above
"""
import math
import os
from ctypes import byref, c_float
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _hip as hip
from .params import ParamStore, RESNET50_BLOCKS, block_names, bn_conv_pairs, stem_names
from .streams import DropMasks, SideStream

D = 256
HEADS = 8
HD = 32
FF = 2048
BN_EPS = 1e-5
KERAS_BN_EPS = 1.001e-5      # tf.keras.applications.resnet BatchNormalization(epsilon=1.001e-5) (tf_backbone=True)
LN_EPS = 1e-5
DEFER_REDUCE = os.environ.get("DETR_HIP_DEFER_REDUCE", "1") != "0"     # queue the weight gradients' split-K reductions (A/B switch)
WGRAD_STREAM = os.environ.get("DETR_HIP_WGRAD_STREAM", "1") != "0"      # backbone weight gradients on a second HIP stream (A/B switch)
BWD_FUSED = os.environ.get("DETR_HIP_BWD_FUSED", "1") != "0"            # layer1: input + weight gradient of the 64 -> 256 1x1 convolutions in one pass over dY (round 5)
# the NEXT step's keep bits generated during this step (eager launches): 2 (default) = next to the assignment kernel alone, behind the matcher's
# cost kernel (pregen_dropmasks_at_matcher: -0.05 ms per step, profiles/r06_ab_results.txt #5); 1 = from the start of the decoder forward
# (measured SLOWER, #3); 0 = at the head of their own step
DROPMASK_AHEAD = int(os.environ.get("DETR_HIP_DROPMASK_AHEAD", "2") or 0)
QK_ALPHA = float(HD) ** -0.5 * 1.4426950408889634      # what the stored bf16 query carries: softmax scale (transformer.py:307) * log2(e)


def mix32(x):
    """csrc/common.h::mix32."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def step_seed(base_seed, step_no, rank=0):
    """uint32 seed of one training step: base seed, step counter and data-parallel rank, mixed on the host (the kernels
    mix it once more with the dropout site id, csrc/common.h::drop_key)."""
    return mix32(mix32((base_seed + 0x9E3779B9 * step_no) & 0xFFFFFFFF) ^ ((rank * 0x85EBCA6B) & 0xFFFFFFFF))


def position_embedding_sine_host(H, W, num_pos_features=128, temperature=10000.0, eps=1e-6):
    """position_embeddings.py:23-50 for an all-False mask: [H*W, 256] fp32, [pos_y | pos_x]."""
    y = (np.arange(1, H + 1, dtype=np.float32) / np.float32(H + eps) * np.float32(2 * math.pi)).astype(np.float32)
    x = (np.arange(1, W + 1, dtype=np.float32) / np.float32(W + eps) * np.float32(2 * math.pi)).astype(np.float32)
    k = np.arange(num_pos_features, dtype=np.float32)
    dim_t = np.power(np.float32(temperature), (2 * np.floor(k / 2) / np.float32(num_pos_features)).astype(np.float32)).astype(np.float32)
    py = (y[:, None] / dim_t[None, :]).astype(np.float32)
    px = (x[:, None] / dim_t[None, :]).astype(np.float32)
    ey = np.empty_like(py)
    ex = np.empty_like(px)
    ey[:, 0::2], ey[:, 1::2] = np.sin(py[:, 0::2]), np.cos(py[:, 1::2])
    ex[:, 0::2], ex[:, 1::2] = np.sin(px[:, 0::2]), np.cos(px[:, 1::2])
    pos = np.concatenate([np.broadcast_to(ey[:, None, :], (H, W, num_pos_features)),
                          np.broadcast_to(ex[None, :, :], (H, W, num_pos_features))], axis=2)
    return np.ascontiguousarray(pos.reshape(H * W, 2 * num_pos_features), dtype=np.float32)


def position_embedding_sine_table(n_max, num_pos_features=128, temperature=10000.0, eps=1e-6):
    """Per-axis sine table of the masked positional encoding (position_embeddings.py:23-50, normalize=True): entry [n][c] is the
    encoding of cumulative count c on an axis with n valid positions, c / (n + eps) * 2 pi, through the float32 NumPy expressions
    of position_embedding_sine_host -- so an all-valid gather reproduces it bit for bit.  [n_max + 1, n_max + 1, 128] fp32
    (entries with c > n are never read)."""
    k = np.arange(num_pos_features, dtype=np.float32)
    dim_t = np.power(np.float32(temperature), (2 * np.floor(k / 2) / np.float32(num_pos_features)).astype(np.float32)).astype(np.float32)
    tab = np.zeros((n_max + 1, n_max + 1, num_pos_features), np.float32)
    c = np.arange(0, n_max + 1, dtype=np.float32)
    for n in range(n_max + 1):
        y = (c / np.float32(n + eps) * np.float32(2 * math.pi)).astype(np.float32)
        py = (y[:, None] / dim_t[None, :]).astype(np.float32)
        tab[n, :, 0::2], tab[n, :, 1::2] = np.sin(py[:, 0::2]), np.cos(py[:, 1::2])
    return tab


def downsample_mask_nearest(mask, Hf, Wf):
    """detr.py:57-63 downsample_masks: TF-legacy nearest neighbour (align_corners = half_pixel_centers = False),
    src = min(floor(dst * in / out), in - 1) per axis.  mask [B, H, W] bool (NumPy) -> [B, Hf, Wf]."""
    mask = np.asarray(mask)
    H, W = mask.shape[1:]
    sy = np.minimum((np.arange(Hf) * H) // Hf, H - 1)
    sx = np.minimum((np.arange(Wf) * W) // Wf, W - 1)
    return mask[:, sy][:, :, sx]


def dilation_flags(replace_stride_with_dilation):
    """replace_stride_with_dilation (None or one flag each for layer2, layer3, layer4; resnet_backbone.py:36-49) as a tuple of 3 bools."""
    if replace_stride_with_dilation is None:
        return (False, False, False)
    flags = tuple(bool(f) for f in replace_stride_with_dilation)
    if len(flags) != 3:
        raise ValueError(f"replace_stride_with_dilation: expected 3 flags (layer2, layer3, layer4), got {len(flags)}")
    return flags


def feature_size(H, W, replace_stride_with_dilation=None):
    """Feature-map size of an H x W input: stem conv, max-pool, layer2..4 each take ceil(n / 2) -- except the stages whose
    stride is replaced by dilation (resnet_backbone.py:74-76), which keep their input size."""
    for halves in (True, True) + tuple(not f for f in dilation_flags(replace_stride_with_dilation)):
        if halves:
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return H, W


def backbone_stride(replace_stride_with_dilation=None):
    """Input pixels per feature-map cell: 4 for the stem and the max-pool, times 2 for every stage of layer2..4 that keeps its stride."""
    return 4 * 2 ** sum(1 for f in dilation_flags(replace_stride_with_dilation) if not f)


class Block(NamedTuple):
    """What one bottleneck block's forward (_block_fwd) leaves for its backward (_block_bwd)."""
    p: str                                  # buffer tag of the block
    n: dict                                 # its parameter names (params.block_names)
    x: torch.Tensor                         # block input [B, h, w, cin]
    xs: torch.Tensor                        # ... at the pixels a stride-2 1x1 conv reads (= x otherwise)
    x1: torch.Tensor                        # input of conv1 (x, or xs when the stride sits on conv1: tf_backbone)
    y1: torch.Tensor                        # conv1 output [B, h1, w1, d1]
    y2: torch.Tensor                        # conv2 output [B, ho, wo, d1]
    out: torch.Tensor                       # block output [B, ho, wo, d2]
    h: int
    w: int
    ho: int
    wo: int
    h1: int
    w1: int
    M1: int                                 # rows of conv1: B * h1 * w1
    s2: int                                 # stride of the 3x3 conv
    cin: int
    d1: int
    d2: int
    stride: int                             # stride of the block
    first: bool                             # first block of its stage: projection shortcut
    out_bits: Optional[torch.Tensor]        # sign bits of `out` (the next block's ReLU mask), training + bf16 storage only
    dil: int                                # dilation (= padding) of the 3x3 conv


class DetrEngine:
    def __init__(self, device="cuda:0", blocks=RESNET50_BLOCKS, num_enc=6, num_dec=6, num_queries=100,
                 num_classes=92, nb_class=None, seed=0, tf_backbone=False, replace_stride_with_dilation=(False, False, False)):
        # replace_stride_with_dilation (resnet_backbone.py:36-49,74-85): one flag each for layer2..4.  A flagged stage keeps its input
        # size (stride 1) and the 3x3 convs of its blocks >= 1 run at dilation 2 (DETR-DC5: layer4 flagged, feature stride 16)
        self.dilate = dilation_flags(replace_stride_with_dilation)
        if tf_backbone and any(self.dilate):
            raise ValueError("replace_stride_with_dilation needs the reference backbone: tf.keras.applications.ResNet50 "
                             "(tf_backbone=True) has no such option")
        hip.load()
        self.device = torch.device(device)
        hip.ensure_workspace(self.device)
        if DEFER_REDUCE:
            hip.ensure_defer_workspace(self.device)        # allocated here, never inside a graph capture
        self.blocks = tuple(blocks)
        self.num_enc, self.num_dec, self.Q = num_enc, num_dec, num_queries
        self.nb_class = nb_class
        self.C = num_classes if nb_class is None else nb_class
        # tf_backbone=True (detr.py:146-148): tf.keras.applications ResNet50 -- ResNet v1 (the stride of a stage sits on the
        # FIRST 1x1 conv of its first block), convs with a trainable bias, BatchNormalization(eps 1.001e-5) in inference mode
        self.tf_backbone = bool(tf_backbone)
        self.bn_eps = KERAS_BN_EPS if self.tf_backbone else BN_EPS
        self.P = ParamStore(self.device, blocks, num_enc, num_dec, num_queries, num_classes, nb_class, seed, tf_backbone=tf_backbone)
        self._stem = stem_names(self.tf_backbone)
        self._pairs = bn_conv_pairs(self.blocks, self.tf_backbone)
        self._bufs = {}
        self._buf_gen = 0                # bumped whenever buf() replaces (frees) a buffer: recorded graphs of older generations are invalid
        self._pos_cache = {}
        self._pos_tables = {}
        self.key_valid = None        # key-validity words of the current masked pass (None: unmasked)
        self._attn_sites = ()        # attention sites whose head-averaged map this pass writes (forward(attn_sites=...))
        self.attn_maps = {}          # site name -> engine buffer [B, T, S] fp32 of the last pass that requested it
        self._shape = None
        self._adt = torch.float32        # storage type of the backbone activations (and their gradients) of the last forward
        self._block_recs = []            # one Block per bottleneck block of the last forward
        self._feat_meta = None           # (feat, Hf, Wf, L) of the last forward
        self._fold_table = self._shift_table = None
        self.bn_scale, self.bn_shift = {}, {}
        self._weights_version, self._built = 0, {}
        self.P.on_change = self._params_changed   # ParamStore.load / load_dict: refold the frozen BN, bump the weights version
        self.fold_bn()
        self.compute = 0                 # 0 = exact fp32 MFMA (parity mode); 1 = bf16 MFMA, fp32 storage (config C3)
        # fp32 storage mode only: the GEMMs / convolutions / stem run on the bf16 matrix pipe at fp32 accuracy (detr_gemm_desc.compute = 2,
        # csrc/gemm_core.h: mma_ktile_split3) instead of on v_mfma_f32_32x32x2_f32; everything else of the fp32 mode is unchanged
        self.f32_split = False
        self.dropout_p = 0.1             # Transformer(dropout=0.1) transformer.py:9 -- active when training=True
        self.dropout_seed = 0x5EED       # base seed; mixed with the step counter and the data-parallel rank
        self.dp_rank = 0                 # parallel.DataParallel sets it: every rank draws its own masks
        self._step_no = 0
        self._drop = (0.0, 0)
        self._step_seed = 0
        self._seed_dev = torch.zeros(8, dtype=torch.int32, device=self.device)   # [0] = uint32 seed of the current training step
        self._cross = {}
        self._graph_replay = False       # True while a captured step is being recorded / replayed (training.GraphedTrainStep)
        self.phase_events = None         # list of (name, torch.cuda.Event) while a caller times the phases of a step (bench.py --phase-events)
        self.side = SideStream(self.device)          # second launch stream (streams.SideStream)
        self.masks = DropMasks(self, HEADS)          # dropout keep bits and their stream (streams.DropMasks)

    # Derived weight copies (BN-folded kernels, the bf16 shadow, the gathered cross-attention weights) are stamped with the
    # weights version they were built from.  EVERY mutation of the parameters bumps the version -- the optimiser after an
    # apply, fold_bn, and ParamStore.load / load_dict themselves (through the store's on_change hook), so a direct
    # `engine.P.load(...)` cannot leave a recorded eval graph or a bf16 shadow stale -- and a copy is rebuilt exactly when
    # it is next needed, also when fp32 and bf16 passes are interleaved.
    @property
    def gemm_mode(self):
        """detr_gemm_desc.compute of this pass's GEMM / conv / stem launches: 1 = bf16 MFMA, 0 = exact fp32 MFMA, 2 = f32x3."""
        return 1 if self.compute == 1 else (2 if self.f32_split else 0)

    def bump_weights_version(self):
        self._weights_version += 1

    def _stale(self, key):
        if self._built.get(key) == self._weights_version:
            return False
        self._built[key] = self._weights_version
        return True

    def seed_of_step(self, step_no):
        return step_seed(self.dropout_seed, step_no, self.dp_rank)

    def advance_dropout_step(self):
        """Next training step: a new uint32 step seed (base seed, step counter, DP rank) is written to DEVICE memory; every
        dropout site derives its key from it inside the kernels, so a captured hipGraph sees the new masks on replay."""
        self._step_no += 1
        self._step_seed = self.seed_of_step(self._step_no)
        # slot 1: the seed of the step after this one (the keep bits of the next step's attention sites are generated while this
        # step's decoder / matcher leave most of the chip idle, DropMasks.pregen) -- a generation ahead that is still queued
        # reads the slot this write replaces: behind it (never inside a capture: GraphedTrainStep calls this before the replay)
        self.masks.settle()
        hip.call("detr_hip_set_u32x8", self._seed_dev.data_ptr(), self._step_seed, self.seed_of_step(self._step_no + 1),
                 0, 0, 0, 0, 0, 0)
        self._drop = (float(self.dropout_p), self._step_seed)
        return self._step_seed

    def phase(self, name):
        """Phase marker of the launch sequence: a timing event on the current stream when `phase_events` is a list (measurement only)."""
        if self.phase_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.phase_events.append((name, ev))

    # ---- buffers ------------------------------------------------------------------------------
    def buf(self, name, shape, dtype=torch.float32):
        """Named device buffer of the static memory plan.  A request with another shape / dtype REPLACES the buffer (the
        old storage is freed: alternating train / validation shapes do not add up) and bumps `buf_generation`; every
        recorded hipGraph remembers the generation it was captured at and is dropped when it no longer matches
        (training.GraphedTrainStep, DetrModel._eval_forward) -- a replay would write through the freed addresses."""
        key = name
        t = self._bufs.get(key)
        shape = tuple(int(s) for s in shape)
        if t is None or tuple(t.shape) != shape or t.dtype != dtype:
            if t is not None:
                self._buf_gen += 1
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._bufs[key] = t
        return t

    @property
    def buf_generation(self):
        """Changes whenever device memory a recorded hipGraph may address has been replaced: an engine buffer (buf) or the
        binding's shared split-reduction scratch (hip.need_workspace)."""
        return self._buf_gen + hip.WS_GENERATION

    def buffer_bytes(self):
        """Bytes held by the named buffers (activations, scratch, derived weight copies)."""
        return sum(t.numel() * t.element_size() for t in self._bufs.values())

    def fold_bn(self):
        """custom_layers.py:21-23: scale = w * rsqrt(var + eps), shift = b - mean * scale (frozen)."""
        for p, c in self.P.bn.items():
            raw = self.P.bn_raw[p]
            sc = self.buf(f"bnscale:{p}", (c,))
            sh = self.buf(f"bnshift:{p}", (c,))
            hip.call("detr_hip_bn_fold_f32", raw[0].data_ptr(), raw[1].data_ptr(), raw[2].data_ptr(), raw[3].data_ptr(),
                     sc.data_ptr(), sh.data_ptr(), c, c_float(self.bn_eps))
            self.bn_scale[p] = sc
            # a conv bias under the frozen BN moves into the shift: scale*(conv + b) + shift0 (rebuilt by _refresh_bias_shift)
            self.bn_shift[p] = self.buf(f"bnshift_eff:{p}", (c,)) if self.tf_backbone else sh
        self.bump_weights_version()
        self._fold_table = None
        self._shift_table = None

    def _refresh_bias_shift(self):
        """tf_backbone=True: effective shift = bias * scale + (beta - mean * scale) for every conv, one launch."""
        if self._shift_table is None:
            rows = []
            for bn_name, conv_name in self._pairs:
                c = self.P.bn[bn_name]
                rows.append([self.P.views[f"{conv_name}/bias"].data_ptr(), self.bn_scale[bn_name].data_ptr(),
                             self._bufs[f"bnshift:{bn_name}"].data_ptr(), self.bn_shift[bn_name].data_ptr(), c])
            self._shift_table = torch.tensor(rows, dtype=torch.int64).to(self.device)
        hip.call("detr_hip_fma_vec_group", self._shift_table.data_ptr(), self._shift_table.shape[0])

    def _params_changed(self):
        self.fold_bn()

    def load_params(self, params):
        return self.P.load_dict(params)       # (the store's on_change hook refolds the frozen BN and bumps the weights version)

    def _w(self, name):
        """Weight OPERAND of a GEMM: the fp32 tensor, or -- while the bf16-compute kernels are active -- its bf16 shadow
        (half the bytes, no conversion in the kernel).  Biases, LayerNorm vectors and gradients stay fp32."""
        if self.compute == 1 and self.P.views16 is not None:
            return self.P.views16[name]
        return self.P.views[name]

    def _refresh_shadow(self):
        """bf16 compute mode: one flat fp32 -> bf16 conversion of all parameters per optimiser step (~60 us)."""
        flat16 = self.P.shadow16()
        hip.call("detr_hip_cvt_bf16", self.P.flat.data_ptr(), flat16.data_ptr(), self.P.flat.numel())
        self._refold_group()

    def _refold_group(self):
        """Frozen-BN fold of every bf16 conv kernel (all but the stem) in one launch: a device table of
        (kernel, bn scale, bf16 out, n/4, cols/4) entries, built once -- the tensors it points at never move."""
        if self._fold_table is None:
            rows = []
            for bn_name, conv in self._pairs[1:]:               # (the stem kernel takes the fp32 copy)
                conv_name = f"{conv}/kernel"
                w = self.P.views[conv_name]
                co = w.shape[-1]
                ws16 = self.buf(f"ws16:{conv_name}", w.shape, torch.bfloat16)
                rows.append([w.data_ptr(), self.bn_scale[bn_name].data_ptr(), ws16.data_ptr(), w.numel() // 4, co // 4])
            self._fold_table = torch.tensor(rows, dtype=torch.int64).to(self.device)
            self._fold_keep = [self.bn_scale, self._bufs]
        hip.call("detr_hip_scale_cols_bf16_group", self._fold_table.data_ptr(), self._fold_table.shape[0])

    def _scaled_kernel(self, conv_name, bn_name):
        """kernel * bn scale per output channel (the frozen-BN fold into the conv); bf16 compute mode: the bf16 copy."""
        w = self.P.views[conv_name]
        co = w.shape[-1]
        if self.compute == 1 and conv_name != f"{self._stem['conv']}/kernel":      # (the stem kernel takes the fp32 copy)
            return self.buf(f"ws16:{conv_name}", w.shape, torch.bfloat16)     # filled by _refold_group()
        ws = self.buf(f"ws:{conv_name}", w.shape)
        if self._stale(f"ws:{conv_name}"):
            hip.call("detr_hip_scale_cols_f32", w.data_ptr(), self.bn_scale[bn_name].data_ptr(), ws.data_ptr(),
                     w.numel() // co, co)
        return ws

    def _conv1x1_fwd(self, x, M, cin, cout, conv_name, bn_name, out, residual=None, act=1, maskbits_out=None):
        """1x1 conv + frozen BN (+ residual) (+ ReLU) as one GEMM (resnet_backbone.py:119-121,128-135).
        B = scaled kernel [cin][cout] (N contiguous; in bf16 mode it is staged as a transpose-read LDS image, which
        made the former transposed weight copy unnecessary).  maskbits_out: also emit (out > 0) as one byte per 8 channels."""
        ws = self._scaled_kernel(conv_name, bn_name)
        shift = self.bn_shift[bn_name]
        ldr = cout if residual is not None else 0
        hip.gemm(M, cout, cin, x, cin, 1, ws, cout, 0, out, cout, bias=shift, residual=residual, ldr=ldr, act=act,
                 maskbits_out=maskbits_out)

    # ---- small helpers ----------------------------------------------------------------------------
    @staticmethod
    def _wgrad(M_out, N_out, K_red, A, lda, Bm, ldb, C, ldc, scale=None, alpha=1.0, compute=None):
        """C[M_out,N_out] += alpha * scale[n] * A'^T-style reduction (both operands reduction-major)."""
        args, kwargs = hip.wgrad_call(M_out, N_out, K_red, A, lda, Bm, ldb, C, ldc, scale=scale, alpha=alpha, compute=compute)
        hip.gemm(*args, **kwargs)

    def _a16(self, base):
        """(buffer name, dtype) of an attention operand: bf16 compute mode stores them in bf16 under the name `base`16."""
        return (f"{base}16", torch.bfloat16) if self.compute == 1 else (base, torch.float32)

    def _colsum(self, x2d, out, alpha=1.0):
        """out += alpha * column sums of x2d, in a FIXED order (round 5: the atomic form made input_proj/bias the one gradient of
        the step that differed between two runs, scripts/experiments/determinism_full.py)."""
        rows, cols = x2d.shape
        n = int(hip.load().detr_hip_colsum_det_scratch_floats(rows, cols))
        scratch = self.buf(f"colsum:{rows}x{cols}", (n,))
        hip.call("detr_hip_colsum_det_f32", x2d.data_ptr(), out.data_ptr(), rows, cols, x2d.stride(0), c_float(alpha),
                 scratch.data_ptr(), n)

    def _ln_fwd(self, x, pfx, y, tag, add=None, y2=None, y16=None):
        """LayerNormalization(eps 1e-5) transformer.py:151-152; optional fused y2 = y + add[r % rows(add)] -- the
        `+ pos` / `+ query_pos` operand of the next attention block (transformer.py:161-163,209,219); optional bf16 twin."""
        rows = x.shape[0]
        mean = self.buf(f"{tag}:mean", (rows,))
        rstd = self.buf(f"{tag}:rstd", (rows,))
        hip.layernorm_fwd(x, self.P.views[f"{pfx}/gamma"], self.P.views[f"{pfx}/beta"], y, mean, rstd, LN_EPS, add=add, y2=y2,
                          y16=y16)

    def _ln_spec(self, rows, pfx, y, tag, add=None, y2=None, y16=None, ffn=False):
        """The same LayerNorm as an epilogue of the GEMM that produces its input (hip.linear_fwd(..., ln=spec)); None when this
        pass runs them as two launches.  Only bf16 compute mode fuses, and only behind the attention out-projections (row-complete
        32 x 256 tiles, same bits as the two launches).  Measured, same box: 16.53 / 16.56 ms fused there vs 16.53 / 16.61 unfused
        vs 16.85 / 16.96 also behind the FFN's second Linear -- the K = 256 launches absorb their LayerNorm at equal time (18
        launches fewer per step), the K = 2048 ones lose 0.35 ms: a 32-row tile walks 64 K tiles behind one barrier each."""
        if self.compute != 1 or ffn:
            return None
        return dict(gamma=self.P.views[f"{pfx}/gamma"], beta=self.P.views[f"{pfx}/beta"], y=y, mean=self.buf(f"{tag}:mean", (rows,)),
                    rstd=self.buf(f"{tag}:rstd", (rows,)), eps=LN_EPS, add=add, y2=y2, y16=y16)

    def _ln_bwd(self, dy, x, pfx, dx, tag, dx_add=None, drop_site=None, want16=False, dy_add=None):
        """Backward of _ln_fwd w.r.t. x (+ dx_add); the incoming gradient is dy (+ dy_add).  drop_site: also return dropout_bwd(dx)
        -- the gradient through the Dropout in front of the residual add that feeds this LayerNorm -- as a second output of the
        same launch.  want16: that second output as bf16 (it only feeds GEMM operands of the bf16-compute FFN backward)."""
        dp, _ = self._drop
        dx_drop = dx_drop16 = None
        if drop_site is not None:
            if want16:
                dx_drop16 = self.buf(f"scratch:drop16:{dx.shape[0]}{self.side.suffix(tag)}", dx.shape, torch.bfloat16)
            elif dp > 0.0:
                dx_drop = self.buf(f"scratch:drop:{dx.shape[0]}{self.side.suffix(tag)}", dx.shape)
        hip.layernorm_bwd(dy, x, self.P.views[f"{pfx}/gamma"], self._bufs[f"{tag}:mean"], self._bufs[f"{tag}:rstd"], dx,
                          self.P.gviews[f"{pfx}/gamma"], self.P.gviews[f"{pfx}/beta"], dx_add=dx_add, dx_drop=dx_drop,
                          dropout_p=dp, dropout_site=(drop_site or 0), dropout_step=self._seed_dev, dx_drop16=dx_drop16,
                          dy_add=dy_add)
        if dx_drop16 is not None:
            return dx_drop16
        return dx if dx_drop is None else dx_drop

    def _add_bcast(self, x, p, out):
        hip.call("detr_hip_add_bcast_f32", x.data_ptr(), p.data_ptr(), out.data_ptr(), x.numel(), p.numel())

    # ---- attention --------------------------------------------------------------------------------
    # MultiHeadAttention.call transformer.py:285-356.  The three projections write column blocks of ONE packed buffer
    # QKV [rows, 768] = [Q | K | V]; q and k share their input (src + pos / tgt + query_pos), so Q and K are ONE GEMM
    # with N = 512 against rows 0..511 of in_proj_kernel.  The query scaling head_dim**-0.5 (:307) is folded into the
    # attention kernels (detr_attn_desc.scale).  In the backward the packed dQKV buffer turns the three data gradients
    # and the three residual-style adds into ONE GEMM with K = 768:  d_x = dQKV @ in_proj_kernel + d_residual.
    # bf16 compute mode: the attention operands Q / K / V / O / dO / dQ / dK / dV are STORED in bf16 (the projection GEMMs write
    # them, Q with scale * log2(e) as its alpha) and the attention core is csrc/attention_dma.hip (LDS-DMA K / V rings per wave,
    # dropout keep flags as bits generated once per step).
    @property
    def attn16(self):
        return self.compute == 1

    def pregen_dropmasks_at_matcher(self):
        """The set loss calls this between its cost and assignment kernels (training.run_train_step passes it to get_losses): the next step's
        keep bits, when DROPMASK_AHEAD = 2 deferred them to here (DropMasks.pregen)."""
        self.masks.at_matcher()

    def _self_attn_fwd(self, tag, pfx, qk_in, v_in, B, T, out, site, ln=None, key_valid=None):
        W, bias = self._w(f"{pfx}/in_proj_kernel"), self.P.views[f"{pfx}/in_proj_bias"]
        dp, _ = self._drop
        lse = self.buf(f"{tag}:lse", (B * HEADS, T))
        if self.attn16:
            # bf16 operands: three members of one grouped launch (Q alone carries the alpha), bf16 O straight into the out-projection
            QKV = self.buf(f"{tag}:QKV16", (B * T, 3 * D), torch.bfloat16)
            hip.gemm_group([hip.linear_fwd_call(qk_in, W[0:D], bias[0:D], QKV[:, 0:D], alpha=QK_ALPHA),          # :294-300, :307
                            hip.linear_fwd_call(qk_in, W[D:2 * D], bias[D:2 * D], QKV[:, D:2 * D]),
                            hip.linear_fwd_call(v_in, W[2 * D:], bias[2 * D:], QKV[:, 2 * D:])])                  # :302-304
            O = self.buf(f"{tag}:O16", (B * T, D), torch.bfloat16)
            self.masks.join()
            hip.attention(QKV[:, 0:D], QKV[:, D:2 * D], QKV[:, 2 * D:], O, lse, B, HEADS, T, T, scale=float(HD) ** -0.5, dropout_p=dp,
                          dropout_site=site, dropout_step=self._seed_dev, dropmask=self.masks.mask(site, B, T, T) if dp > 0.0 else None,
                          key_valid=key_valid)
        else:
            QKV = self.buf(f"{tag}:QKV", (B * T, 3 * D))
            hip.gemm_group([hip.linear_fwd_call(qk_in, W[0:2 * D], bias[0:2 * D], QKV[:, 0:2 * D]),        # :294-300
                            hip.linear_fwd_call(v_in, W[2 * D:], bias[2 * D:], QKV[:, 2 * D:])])          # :302-304
            O = self.buf(f"{tag}:O", (B * T, D))
            hip.attention(QKV[:, 0:D], QKV[:, D:2 * D], QKV[:, 2 * D:], O, lse, B, HEADS, T, T, scale=float(HD) ** -0.5,
                          dropout_p=dp, dropout_site=site, dropout_step=self._seed_dev, key_valid=key_valid)     # :307-345
        if pfx in self._attn_sites:
            self._attn_map(pfx, QKV[:, 0:D], QKV[:, D:2 * D], lse, B, T, T, key_valid)
        hip.linear_fwd(O, self._w(f"{pfx}/out_proj_kernel"), self.P.views[f"{pfx}/out_proj_bias"], out, residual=v_in,
                       dropout_p=dp, dropout_seed=site + 1, dropout_step=self._seed_dev, ln=ln)        # :346-347 + :169 (+ the LayerNorm behind it)

    def attn_site_names(self):
        """The attention sites of this model, by the parameter paths of the weight files, in launch order."""
        names = [f"transformer/encoder/layer_{i}/self_attn" for i in range(self.num_enc)]
        for i in range(self.num_dec):
            names += [f"transformer/decoder/layer_{i}/self_attn", f"transformer/decoder/layer_{i}/multihead_attn"]
        return names

    def _check_attn_sites(self, attn_sites, training):
        if not attn_sites:
            return ()
        if isinstance(attn_sites, str):
            attn_sites = (attn_sites,)
        sites, valid = tuple(dict.fromkeys(attn_sites)), self.attn_site_names()
        unknown = [s for s in sites if s not in valid]
        if unknown:
            raise ValueError(f"attn_sites: unknown attention site(s) {unknown}; valid names: {valid}")
        if training:
            # the reference averages the weights AFTER the attention dropout there (transformer.py:341, 349-354)
            raise NotImplementedError("attention maps (attn_sites / need_weights) are returned in evaluation mode only: with training=True "
                                      "the reference averages the weights after their dropout, which the maps kernel does not apply")
        return sites

    def _attn_map(self, site, q, k, lse, B, T, S, key_valid):
        """The head-averaged map of `site` right behind its attention launch (same stream, same q / k / lse / key_valid), :349-354."""
        w = self.buf(f"attnw:{site}", (B, T, S))
        hip.attention_weights(q, k, lse, w, B, HEADS, T, S, scale=float(HD) ** -0.5, key_valid=key_valid)
        self.attn_maps[site] = w

    def _self_attn_bwd(self, tag, pfx, d_out, d_res, qk_in, v_in, B, T, d_x, site, acc_qk=None, key_valid=None):
        """d_out: gradient of the out-projection output (dropout backward already applied), d_res: gradient of the
        block output (residual path).  Writes d_x = gradient w.r.t. v_in, including the q / k branch when qk_in is
        v_in + const (d_x = None: not needed).  acc_qk: buffer that ACCUMULATES the gradient of the q / k input alone
        (the decoder's query_pos gradient)."""
        G = self.P.gviews
        W, gW, gb = self._w(f"{pfx}/in_proj_kernel"), G[f"{pfx}/in_proj_kernel"], G[f"{pfx}/in_proj_bias"]
        a16 = self.attn16
        (qkv, adt), (o, _) = self._a16(f"{tag}:QKV"), self._a16(f"{tag}:O")
        QKV, O = self._bufs[qkv], self._bufs[o]
        dO = self.buf(f"scratch:dO:{B * T}:{int(a16)}", (B * T, D), adt)
        hip.linear_dgrad(d_out, self._w(f"{pfx}/out_proj_kernel"), dO)
        dQKV = self.buf(f"scratch:dQKV:{B * T}:{int(a16)}{self.side.suffix(tag)}", (B * T, 3 * D), adt)
        delta = self.buf(f"scratch:delta:{B * T}", (2 * B * HEADS, T))       # (bf16 operands: delta / scale | lse * log2 e - log2 scale)
        dp, _ = self._drop
        hip.attention(QKV[:, 0:D], QKV[:, D:2 * D], QKV[:, 2 * D:], O, self._bufs[f"{tag}:lse"], B, HEADS, T, T,
                      scale=float(HD) ** -0.5, dropout_p=dp, dropout_site=site, dropout_step=self._seed_dev,
                      d_o=dO, dq=dQKV[:, 0:D], dk=dQKV[:, D:2 * D], dv=dQKV[:, 2 * D:], delta=delta,
                      dropmask=self.masks.mask(site, B, T, T) if (a16 and dp > 0.0) else None, key_valid=key_valid)
        # weight gradients (bias gradients fused: row sums of dy^T), one grouped launch (bf16 operands: the out-projection's pair has
        # other storage types than the in-projections' and is a launch of its own)
        wg_out = hip.linear_wgrad_call(d_out, O, G[f"{pfx}/out_proj_kernel"], bias_grad=G[f"{pfx}/out_proj_bias"])
        wg_in = [hip.linear_wgrad_call(dQKV[:, 0:2 * D], qk_in, gW[0:2 * D], bias_grad=gb[0:2 * D]),
                 hip.linear_wgrad_call(dQKV[:, 2 * D:], v_in, gW[2 * D:], bias_grad=gb[2 * D:])]
        if a16:
            self.side.run(lambda: (hip.gemm(*wg_out[0], **wg_out[1]), hip.gemm_group(wg_in)))
        else:
            self.side.run(lambda: hip.gemm_group([wg_out] + wg_in))
        calls = []
        if acc_qk is not None:
            calls.append(hip.linear_dgrad_call(dQKV[:, 0:2 * D], W[0:2 * D], acc_qk, residual=acc_qk))
        if d_x is not None:
            calls.append(hip.linear_dgrad_call(dQKV, W, d_x, residual=d_res))
        if len(calls) == 1:
            hip.gemm(*calls[0][0], **calls[0][1])
        elif calls:
            hip.gemm_group(calls)

    # bf16 compute mode: the tensors that ONLY feed GEMM operands of the FFN -- its input twin x16 (written by the LayerNorm
    # that produces x), the hidden activation h, its gradient dh and the incoming gradient twin d_y16 (written by the
    # LayerNorm backward) -- are STORED in bf16: the loaders would round them anyway (bit-identical products), the two
    # [rows, 2048] tensors move half the bytes, and both weight gradients become one grouped launch of the all-bf16 variant.
    @property
    def ffn16(self):
        return self.compute == 1

    def _ffn_fwd(self, tag, pfx, x, out_pre_ln, seed=0, x16=None, ln=None):
        V = self.P.views
        dp, _ = self._drop
        h = self.buf(f"{tag}:h", (x.shape[0], FF), torch.bfloat16 if self.ffn16 else torch.float32)
        hip.linear_fwd(x16 if x16 is not None else x, self._w(f"{pfx}/linear1/kernel"), V[f"{pfx}/linear1/bias"], h, act=1,
                       dropout_p=dp, dropout_seed=seed, dropout_step=self._seed_dev)    # :172-174
        hip.linear_fwd(h, self._w(f"{pfx}/linear2/kernel"), V[f"{pfx}/linear2/bias"], out_pre_ln, residual=x, dropout_p=dp,
                       dropout_seed=seed + 1, dropout_step=self._seed_dev, ln=ln)      # :175-176 (+ the LayerNorm behind it)

    def _ffn_bwd(self, tag, pfx, d_y, d_f, x, dx, x16=None):
        """d_f: grad of (drop(linear2(drop(relu(linear1(x))))) + x); d_y = dropout_bwd(d_f) (from the LayerNorm backward
        launch; bf16 in bf16 compute mode); dx = full gradient w.r.t. x."""
        G = self.P.gviews
        h = self._bufs[f"{tag}:h"]                 # post-ReLU, post-dropout hidden activation
        dp, _ = self._drop
        dh = self.buf(f"scratch:dh:{h.shape[0]}:{int(self.ffn16)}{self.side.suffix(tag)}", h.shape,
                      torch.bfloat16 if self.ffn16 else torch.float32)
        # (h > 0) is both the ReLU and the keep mask of the hidden dropout; its 1/(1-p) scale goes in alpha
        hip.linear_dgrad(d_y, self._w(f"{pfx}/linear2/kernel"), dh, mask=h, alpha=(1.0 / (1.0 - dp)) if dp > 0.0 else 1.0)
        self.side.run(lambda: hip.gemm_group([
            hip.linear_wgrad_call(d_y, h, G[f"{pfx}/linear2/kernel"], bias_grad=G[f"{pfx}/linear2/bias"]),
            hip.linear_wgrad_call(dh, x16 if x16 is not None else x, G[f"{pfx}/linear1/kernel"],
                                  bias_grad=G[f"{pfx}/linear1/bias"])]))
        hip.linear_dgrad(dh, self._w(f"{pfx}/linear1/kernel"), dx, residual=d_f)

    # ---- layer-invariant decoder cross-attention K / V (transformer.py:221-223: memory is the same for every layer) ------
    def _cross_tables(self):
        """Wkv [2*nd*256, 256] = [Wk_0 .. Wk_nd-1 ; Wv_0 .. Wv_nd-1] (rows 256..767 of every multihead_attn in_proj_kernel) and
        its bias: a derived weight copy like the BN-folded conv kernels, gathered by ONE multi-copy launch per weights
        version; the gradient of the copy is scattered back by one more."""
        nd = self.num_dec
        key = ("cross", self.compute)
        if key not in self._cross:
            wdt = torch.bfloat16 if self.compute == 1 else torch.float32
            Wkv = self.buf(f"cross:Wkv:{self.compute}", (2 * nd * D, D), wdt)
            bkv = self.buf("cross:bkv", (2 * nd * D,))
            gW = self.buf("cross:gWkv", (2 * nd * D, D))
            gb = self.buf("cross:gbkv", (2 * nd * D,))
            gather, scatter = [], []
            src_views = self.P.views16 if self.compute == 1 else self.P.views
            for i in range(nd):
                pfx = f"transformer/decoder/layer_{i}/multihead_attn"
                w, b = src_views[f"{pfx}/in_proj_kernel"], self.P.views[f"{pfx}/in_proj_bias"]
                g, gbias = self.P.gviews[f"{pfx}/in_proj_kernel"], self.P.gviews[f"{pfx}/in_proj_bias"]
                for part, row0 in ((0, i * D), (1, (nd + i) * D)):             # part 0 = K rows, 1 = V rows
                    lo = (1 + part) * D
                    gather.append((w[lo:lo + D], Wkv[row0:row0 + D], 0))
                    gather.append((b[lo:lo + D], bkv[row0:row0 + D], 0))
                    scatter.append((gW[row0:row0 + D], g[lo:lo + D], 1))
                    scatter.append((gb[row0:row0 + D], gbias[lo:lo + D], 1))
            self._cross[key] = dict(Wkv=Wkv, bkv=bkv, gW=gW, gb=gb, gather=hip.copy_table(gather, self.device),
                                    scatter=hip.copy_table(scatter, self.device))
        return self._cross[key]

    # ---- forward ----------------------------------------------------------------------------------
    def forward(self, images, training=False, masks=None, attn_sites=None):
        """See _forward_impl.  GEMM / conv compute mode: self.compute (0 = exact fp32, 1 = bf16 MFMA).
        attn_sites: iterable of attention site names (attn_site_names(): the parameter paths `transformer/encoder/layer_{i}/self_attn`,
        `transformer/decoder/layer_{i}/self_attn`, `transformer/decoder/layer_{i}/multihead_attn`).  For each, one extra launch
        behind that site's attention launch writes the head-averaged attention map [B, T, S] (fp32, transformer.py:349-354) into
        self.attn_maps[name]; evaluation mode only.  None / empty: the launch sequence is unchanged.
        masks: optional padding mask [B, H, W] (True = padding, detr.py:65-72) as a device uint8 / bool tensor or a host array
        (validated on the host: an image without a valid feature position raises ValueError).  A device mask is validated on
        the device: check_mask_status() reads the result where the caller synchronises anyway."""
        self._attn_sites = self._check_attn_sites(attn_sites, training)
        self.attn_maps = {}
        hip.COMPUTE_BF16 = self.gemm_mode
        if self.compute == 1 and (self._stale("shadow16") or self.P.views16 is None):
            self._refresh_shadow()
        if self.tf_backbone and self._stale("bias_shift"):
            self._refresh_bias_shift()
        if masks is not None and not (torch.is_tensor(masks) and masks.is_cuda):
            masks = self._host_masks(masks, tuple(images.shape[:3]))        # validated before any launch
        self.side.begin(WGRAD_STREAM and images.is_cuda)
        try:
            return self._forward_impl(images, training, masks)
        finally:
            try:
                self.side.end()
            finally:
                hip.COMPUTE_BF16 = 0

    def backward(self, d_logits, d_boxes, backbone=True, on_bucket=None):
        hip.COMPUTE_BF16 = self.gemm_mode
        cb = on_bucket
        if DEFER_REDUCE:
            # the weight gradients are only read by the bucket exchange / the optimiser: their split-K reductions are queued
            # and run 16 per launch (hip.flush_reduces) instead of one ~9 us latency-bound launch behind every GEMM
            hip.begin_deferred_reduces(self.device)
            if on_bucket:
                def cb(i):
                    self.side.join()
                    hip.flush_reduces()
                    on_bucket(i)
        elif on_bucket:
            def cb(i):
                self.side.join()
                on_bucket(i)
        # (immediate split-K reductions share ONE slab workspace between all launches: single stream then)
        self.side.begin(WGRAD_STREAM and DEFER_REDUCE and d_logits.is_cuda)
        try:
            return self._backward_impl(d_logits, d_boxes, backbone, cb)
        finally:
            try:
                self.side.end()
                hip.flush_reduces(end=True)
            finally:
                hip.COMPUTE_BF16 = 0

    def _prepare_masks(self, masks, B, H, W, Hf, Wf):
        """Padding mask -> self.key_valid words, per-image pos [B*L, 256] and the status words, one launch
        (detr_hip_padding_mask_prepare).  Returns pos."""
        L = Hf * Wf
        if tuple(masks.shape) != (B, H, W) or masks.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"masks: expected a uint8 / bool tensor of shape {(B, H, W)}, got {masks.dtype} {tuple(masks.shape)}")
        key = (Hf, Wf)
        if key not in self._pos_tables:
            self._pos_tables[key] = (torch.from_numpy(position_embedding_sine_table(Hf)).to(self.device),
                                     torch.from_numpy(position_embedding_sine_table(Wf)).to(self.device))
        tab_y, tab_x = self._pos_tables[key]
        kv = self.buf("mask:key_valid", (B * ((L + 31) // 32),), torch.int32)
        pos = self.buf("mask:pos", (B * L, D))
        status = self.buf("mask:status", (B,), torch.int32)
        hip.padding_mask_prepare(masks, Hf, Wf, tab_y, tab_x, kv, pos, status)
        self.key_valid = kv
        return pos

    def _host_masks(self, masks, shape):
        """A host mask (NumPy / CPU tensor, True = padding): validated on the host, then copied to the device as uint8."""
        host = np.asarray(masks.cpu() if torch.is_tensor(masks) else masks).astype(bool)
        if host.shape != shape:
            raise ValueError(f"masks: expected shape {shape}, got {host.shape}")
        Hf, Wf = feature_size(shape[1], shape[2], self.dilate)
        empty = [b for b in range(shape[0]) if downsample_mask_nearest(host[b:b + 1], Hf, Wf).all()]
        if empty:
            raise ValueError(f"masks: image(s) {empty} have no valid (unpadded) position on the {Hf} x {Wf} feature map")
        return torch.from_numpy(host.view(np.uint8)).to(self.device)

    def check_mask_status(self):
        """Raise ValueError when an image of the last masked pass had no valid feature position (reads the device status
        words: call it where the step synchronises anyway).  No-op after an unmasked pass."""
        if self.key_valid is None:
            return
        st = self._bufs["mask:status"].cpu()
        bad = [int(b) for b in torch.nonzero(st).flatten()]
        if bad:
            raise ValueError(f"masks: image(s) {bad} have no valid (unpadded) position on the feature map")

    # ---- the two passes: a sequence of stages ---------------------------------------------------------
    def _forward_impl(self, images, training=False, masks=None):
        """images: CUDA fp32 NHWC [B,H,W,3] (already normalised, processing.py:12-16).
        Returns (logits [Lv,B,Q,C], boxes [Lv,B,Q,4]) views of engine buffers."""
        assert images.is_cuda and images.dtype == torch.float32 and images.dim() == 4 and images.shape[3] == 3
        images = images.contiguous()
        if training and self.dropout_p > 0.0:
            if not self._graph_replay:          # a captured step is fed its seed by training.GraphedTrainStep before every replay
                self.advance_dropout_step()
            self._drop = (float(self.dropout_p), self._step_seed)
        else:
            self._drop = (0.0, 0)
        B, H, W, _ = images.shape
        self._shape = (B, H, W)
        if self._drop[0] > 0.0:
            hf, wf = feature_size(H, W, self.dilate)        # stem conv, max-pool, layer2..4: each ceil(n / 2) unless dilated
            self.masks.gen(B, hf * wf)
        self.images = images
        self.phase("fwd backbone")
        x, h, w = self._stem_fwd(images, B, H, W)
        cin = 64
        self._block_recs = []
        for li, nb in enumerate(self.blocks):               # residual stages (resnet_backbone.py:116-137)
            for b in range(nb):
                m = self._block_fwd(li, b, x, h, w, cin, B, training)
                self._block_recs.append(m)
                x, h, w, cin = m.out, m.ho, m.wo, m.d2
        L = h * w
        self._feat_meta = (x, h, w, L)
        self.phase("fwd encoder")
        x, pos = self._input_proj_fwd(x, masks, B, L)
        qk = self.buf("enc0:qk", (B * L, D))
        self._add_bcast(x, pos, qk)                              # src + pos (:161-163); later layers get it from LayerNorm 2
        for i in range(self.num_enc):
            x, qk = self._encoder_layer_fwd(i, x, qk, pos, B, L)
        self.phase("fwd decoder")
        if training:
            self.masks.pregen(B, L, DROPMASK_AHEAD)
        # ---------------- decoder (transformer.py:207-234, :104-133) ----------------
        Q, nd = self.Q, self.num_dec
        qpos = self.P.views["query_embed/kernel"]
        tgt = self.buf("dec:tgt0", (B * Q, D))
        hip.zero_(tgt)                                           # transformer.py:45
        hs = self.buf("dec:hs", (nd, B * Q, D))
        t3all = self.buf("dec:t3all", (nd, B * Q, D))           # the layer outputs, contiguous: ONE final-norm launch over all levels
        KV = self._cross_kv_fwd(x, qk, B, L)                     # memory = x, memory + pos = qk (src + pos without an encoder)
        qin = self.buf("dec0:qin", (B * Q, D))
        self._add_bcast(tgt, qpos, qin)                          # tgt + query_pos (:209); later layers: from LayerNorm 3
        for i in range(nd):
            tgt, qin = self._decoder_layer_fwd(i, tgt, qin, qpos, KV, t3all[i], B, L)
        # the shared decoder norm of every level (:121-125) in one launch (round 4: it was one 800-row launch per layer, forward and backward)
        self._ln_fwd(t3all.view(nd * B * Q, D), "transformer/decoder/norm", hs.view(nd * B * Q, D), "dec:lnf")
        self.phase("fwd heads")
        logits, boxes = self._heads_fwd(hs.view(nd * B * Q, D))
        self.phase("set loss")
        return logits.view(nd, B, Q, self.C), boxes.view(nd, B, Q, 4)

    def zero_grad(self):
        hip.zero_(self.P.grad)

    def _backward_impl(self, d_logits, d_boxes, backbone=True, on_bucket=None):
        """d_logits [Lv,B,Q,C], d_boxes [Lv,B,Q,4] (contiguous CUDA fp32): gradients of the scalar
        loss w.r.t. the head outputs.  Parameter gradients are ACCUMULATED into P.grad.
        on_bucket(i) is called when gradient bucket i (ParamStore.bucket_bounds) is final."""
        B = self._shape[0]
        feat, _, _, L = self._feat_meta
        nd, BQ = self.num_dec, B * self.Q
        R = nd * BQ
        self.phase("bwd heads")
        d_hs = self._heads_bwd(d_logits.reshape(R, self.C), d_boxes.reshape(R, 4))
        self.phase("bwd decoder")
        memory = self._bufs[f"enc{self.num_enc - 1}:x2"] if self.num_enc > 0 else self._bufs["enc:src0"]
        mem_pos = self._bufs["dec:mem_pos"] if self.num_enc > 0 else self._bufs["enc0:qk"]
        KV = self._bufs[self._a16("dec:KV")[0]]
        dKV = self.buf(f"scratch:dKV:{int(self.attn16)}", KV.shape, KV.dtype)      # every column block is written by its layer's attention backward
        acc_qpos = self.buf("scratch:acc_qpos", (BQ, D))             # sum over layers / sites of d(tgt + query_pos): query_pos gradient
        hip.zero_(acc_qpos)
        # the shared decoder norm, all levels at once: d_t3n[i] = gradient of level i's head input w.r.t. t3 of layer i
        d_t3n = self.buf("scratch:d_t3n", (nd, BQ, D))
        self._ln_bwd(d_hs, self._bufs["dec:t3all"].view(R, D), "transformer/decoder/norm", d_t3n.view(R, D), "dec:lnf")
        d_next = None                       # gradient flowing into t3 of layer i from layer i+1
        for i in reversed(range(nd)):
            d_next = self._decoder_layer_bwd(i, d_t3n[i], d_next, KV, dKV, acc_qpos, B, L)
        self._colsum(acc_qpos.view(B, self.Q * D), self.P.gviews["query_embed/kernel"].view(self.Q * D))      # d query_pos (sum over the batch)
        d_x = self._cross_kv_bwd(dKV, memory, mem_pos, B, L)
        self.phase("bwd encoder")
        for i in reversed(range(self.num_enc)):
            d_x = self._encoder_layer_bwd(i, d_x, B, L)
        if on_bucket:
            on_bucket(0)
        self.phase("bwd backbone")
        g = self._input_proj_bwd(d_x, feat, B, L, want_dx=backbone)
        if not backbone:
            if on_bucket:
                for i in (1, 2, 3):
                    on_bucket(i)
            return
        bucket_at = {block_names(3, 0, self.tf_backbone)["tag"]: 1, block_names(2, 0, self.tf_backbone)["tag"]: 2}
        for bi in reversed(range(len(self._block_recs))):
            g = self._block_bwd(bi, g, B)
            if on_bucket and self._block_recs[bi].p in bucket_at:
                on_bucket(bucket_at[self._block_recs[bi].p])
        self.side.join()
        self._stem_bwd(g, B)
        if on_bucket:
            on_bucket(3)

    # ---- stem (resnet_backbone.py:11-26) --------------------------------------------------------------
    def _pool_fn(self, which):
        return f"detr_hip_maxpool3x3s2_{which}_{'bf16' if self._adt == torch.bfloat16 else 'f32'}"

    def _chunks(self, c):
        """The subsample kernels copy 16-byte chunks: a bf16 tensor passes as c / 2 "float" channels."""
        return c // 2 if self._adt == torch.bfloat16 else c

    def _bias_grad(self, conv, bn, dz, rows, cols):
        """tf_backbone: db = scale * column sums of the gradient at the conv + BN output (the folded BN scales the bias)."""
        if self.tf_backbone:
            hip.call("detr_hip_colsum_scaled", dz.data_ptr(), 1 if dz.dtype == torch.bfloat16 else 0, rows, cols, cols,
                     self.bn_scale[bn].data_ptr(), self.P.gviews[f"{conv}/bias"].data_ptr())

    def _stem_fwd(self, images, B, H, W):
        """7x7 / 2 conv + frozen BN + ReLU, 3x3 / 2 max pool.  Returns (pool, H2, W2)."""
        H1, W1 = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        ws = self._scaled_kernel(f"{self._stem['conv']}/kernel", self._stem["bn"])
        adt = self._adt = torch.bfloat16 if self.compute == 1 else torch.float32      # storage type of backbone activations (and their gradients)
        stem = self.buf("stem:out", (B, H1, W1, 64), adt)
        # implicit GEMM: the 7x7x3 patches are gathered from the image by the A loader (stem_conv.hip), no im2col buffer
        hip.stem_conv(0, images, ws, stem, B, H, W, H1, W1, bias=self.bn_shift[self._stem["bn"]], act=1)
        H2, W2 = (H1 + 2 - 3) // 2 + 1, (W1 + 2 - 3) // 2 + 1
        pool = self.buf("stem:pool", (B, H2, W2, 64), adt)
        amax = self.buf("stem:amax", (B, H2, W2, 64), torch.uint8)
        hip.call(self._pool_fn("fwd"), stem.data_ptr(), pool.data_ptr(), amax.data_ptr(), B, H1, W1, 64, H2, W2)
        return pool, H2, W2

    def _stem_bwd(self, g, B):
        stem, pool, amax = (self._bufs[f"stem:{n}"] for n in ("out", "pool", "amax"))
        (H1, W1), (H2, W2) = stem.shape[1:3], pool.shape[1:3]
        d_stem = self.buf("scratch:d_stem", stem.shape, self._adt)
        hip.call(self._pool_fn("bwd"), g.data_ptr(), amax.data_ptr(), stem.data_ptr(), d_stem.data_ptr(), B, H1, W1, 64, H2, W2)
        M1 = B * H1 * W1
        hip.stem_conv(2, self.images, d_stem, self.P.gviews[f"{self._stem['conv']}/kernel"], B, self._shape[1], self._shape[2], H1, W1,
                      scale=self.bn_scale[self._stem["bn"]], split=max(1, min(512, M1 // 4096)))
        self._bias_grad(self._stem["conv"], self._stem["bn"], d_stem, M1, 64)

    # ---- one bottleneck block (resnet_backbone.py:116-137) ----------------------------------------------
    def _block_fwd(self, li, b, x, h, w, cin, B, training):
        """Block b of stage li on x [B, h, w, cin].  Returns its Block record (.out: the output)."""
        adt, nb = self._adt, self.blocks[li]
        d1, d2 = 64 * 2 ** li, 256 * 2 ** li
        n = block_names(li, b, self.tf_backbone)
        p = n["tag"]
        dilated = li > 0 and self.dilate[li - 1]         # the stage trades its stride for dilation (resnet_backbone.py:74-85)
        stride = 2 if (b == 0 and li > 0 and not dilated) else 1
        dil = 2 if (dilated and b > 0) else 1            # the stage's first block keeps dilation 1
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        M_in, M_out = B * h * w, B * ho * wo
        xs = x
        if stride == 2 and (b == 0):
            # stride-2 1x1 convs read every second pixel: gather them once (a plain 16-byte-chunk copy)
            xs = self.buf(f"{p}:xs", (B, ho, wo, cin), adt)
            hip.call("detr_hip_subsample2_fwd_f32", x.data_ptr(), xs.data_ptr(), B, h, w, self._chunks(cin), ho, wo)
        if self.tf_backbone:            # ResNet v1 (keras.applications): the stride sits on the FIRST 1x1 conv
            x1, M1, h1, w1, s2 = xs, M_out, ho, wo, 1
        else:                           # reference backbone (resnet_backbone.py:104-105): on the 3x3 conv
            x1, M1, h1, w1, s2 = x, M_in, h, w, stride
        if b == 0:
            # the projection shortcut only meets the main branch at conv3's residual operand: second stream
            # (an HBM-bound 1x1 GEMM next to the MFMA-bound 3x3 conv)
            idn = self.buf(f"{p}:idn", (B, ho, wo, d2), adt)
            self.side.run(lambda: self._conv1x1_fwd(xs, M_out, cin, d2, f"{n['down']}/kernel", n["bnd"], idn, act=0))
        else:
            idn = x
        y1 = self.buf(f"{p}:y1", (B, h1, w1, d1), adt)
        self._conv1x1_fwd(x1, M1, cin, d1, f"{n['conv1']}/kernel", n["bn1"], y1)
        y2 = self.buf(f"{p}:y2", (B, ho, wo, d1), adt)
        hip.conv3x3(0, y1, self._scaled_kernel(f"{n['conv2']}/kernel", n["bn2"]), y2, B, h1, w1, d1, ho, wo, d1,
                    s2, bias=self.bn_shift[n["bn2"]], act=1, pad=dil, dilation=dil)
        if b == 0:
            self.side.join()
        out = self.buf(f"{p}:out", (B, ho, wo, d2), adt)
        # training, bf16 activation storage: the block output's ReLU mask as BITS (1 byte per 8 channels) next to the tensor --
        # the backward only needs the sign, and the GEMMs that apply it are HBM streams (1/16 of the mask bytes)
        # (only where the consumer is the STREAMING kernel -- the conv1 input gradient of a following block of layer1-3: there the
        #  mask stream is a third of the bytes; in the tile engine's / the 3x3 kernels' epilogues the byte loads measured 2-9 %
        #  SLOWER than the 16-byte mask loads, so y1 / y2 and the layer4 blocks keep their bf16 masks)
        nxt_d1 = 64 * 2 ** (li if b + 1 < nb else li + 1)        # d1 of the next block
        last = (li + 1 == len(self.blocks)) and (b + 1 == nb)
        obits = self.buf(f"{p}:out_bits", (M_out, d2 // 8), torch.uint8) \
            if (training and adt == torch.bfloat16 and not last and nxt_d1 <= 256) else None
        self._conv1x1_fwd(y2, M_out, d1, d2, f"{n['conv3']}/kernel", n["bn3"], out, residual=idn, maskbits_out=obits)
        return Block(p=p, n=n, x=x, xs=xs, x1=x1, y1=y1, y2=y2, out=out, h=h, w=w, ho=ho, wo=wo, h1=h1, w1=w1, M1=M1, s2=s2,
                     cin=cin, d1=d1, d2=d2, stride=stride, first=(b == 0), out_bits=obits, dil=dil)

    def _ws(self, conv):
        """Scaled kernel of `conv` as the forward used it (the bf16 copy in bf16 mode)."""
        return self._bufs[f"{'ws16' if self.compute == 1 else 'ws'}:{conv}/kernel"]

    def _bwd_fused(self, m):
        """(conv3, shortcut): which of layer1's 64 -> 256 convolutions on bf16 tensors take input AND weight gradient from one
        pass over dY (csrc/bwd_fused.hip) -- dY (274 MB at B = 8, 800 x 1333) is read once per convolution, not twice."""
        ok = BWD_FUSED and self.compute == 1 and self._adt == torch.bfloat16 and m.d2 == 256
        return ok and m.d1 == 64, ok and m.first and m.stride == 1 and m.cin == 64

    def _shortcut_dgrad(self, m, g, B):
        """Data gradient of the block's shortcut: (idg, idg_sub, ready).  idg is the residual operand of the block's last GEMM
        (g itself for an identity shortcut), idg_sub = (h, w) when idg is the COMPACT [B, ho, wo, cin] gradient of a stride-2
        projection (bf16 tensors: the GEMM's residual row map, detr_gemm_desc.res_sub_*, adds it at the even pixels -- no
        zero-filled full-resolution copy is written or read), ready = the side-stream event behind it (None: nothing to wait
        for).  The tf backbone's strided blocks fold the shortcut into their own last GEMMs (_block_bwd)."""
        strided = m.first and m.stride == 2
        if not m.first or (self.tf_backbone and strided):
            return g, None, None
        adt, cin, d2, ho, wo, M_out = self._adt, m.cin, m.d2, m.ho, m.wo, B * m.ho * m.wo
        wsd, n = self._ws(m.n["down"]), m.n
        compact = strided and adt == torch.bfloat16
        fuse_down = self._bwd_fused(m)[1]
        idg = self.buf(f"scratch:dxs:{cin}:{ho}", (B, ho, wo, cin), adt) if compact else self.buf(f"scratch:idg:{cin}:{m.h}", (B, m.h, m.w, cin), adt)

        def dgrad():
            if strided and not compact:         # fp32 tensors: scattered into the zero-filled full-resolution gradient
                dxs = self.buf(f"scratch:dxs:{cin}:{ho}", (B, ho, wo, cin), adt)
                hip.gemm(M_out, cin, d2, g, d2, 1, wsd, d2, 1, dxs, cin)
                hip.call("detr_hip_subsample2_bwd_f32", dxs.data_ptr(), idg.data_ptr(), B, m.h, m.w, self._chunks(cin), ho, wo)
            elif fuse_down:                     # with the shortcut's weight gradient (_wg3 skips it)
                hip.conv1x1_bwd_fused(g.view(M_out, d2), m.xs.view(M_out, cin), wsd.view(cin, d2), idg.view(M_out, cin),
                                      self.P.gviews[f"{n['down']}/kernel"].view(cin, d2),
                                      self.buf(f"bwdfused:slabs:down:{M_out}", (hip.conv1x1_bwd_fused_scratch_floats(M_out),)),
                                      scale=self.bn_scale[n["bnd"]], use_mask=False)
            else:
                hip.gemm(M_out, cin, d2, g, d2, 1, wsd, d2, 1, idg, cin)
        self.side.run(dgrad)
        return idg, ((m.h, m.w) if compact else None), self.side.event()

    # Weight gradients of a block do not feed the data-gradient chain (g -> dz2 -> dz1 -> gx): _block_bwd issues each group
    # through side.run, behind an event of the main stream that follows its producer, so a chip-filling but HBM-bound
    # data-gradient GEMM and an MFMA/LDS-bound weight gradient share the CUs.
    def _wg3(self, m, g, M_out, fuse3, fuse_down):
        """conv3 and the projection shortcut (both read g)."""
        n, G = m.n, self.P.gviews
        if not fuse3:
            self._wgrad(m.d1, m.d2, M_out, m.y2, m.d1, g, m.d2, G[f"{n['conv3']}/kernel"], m.d2, scale=self.bn_scale[n["bn3"]])
        self._bias_grad(n["conv3"], n["bn3"], g, M_out, m.d2)
        if m.first:
            if not fuse_down:
                self._wgrad(m.cin, m.d2, M_out, m.xs, m.cin, g, m.d2, G[f"{n['down']}/kernel"], m.d2, scale=self.bn_scale[n["bnd"]])
            self._bias_grad(n["down"], n["bnd"], g, M_out, m.d2)

    def _wg2(self, m, dz2, B):
        n, d1 = m.n, m.d1
        hip.conv3x3(2, m.y1, dz2, self.P.gviews[f"{n['conv2']}/kernel"], B, m.h1, m.w1, d1, m.ho, m.wo, d1, m.s2,
                    scale=self.bn_scale[n["bn2"]], pad=m.dil, dilation=m.dil)
        self._bias_grad(n["conv2"], n["bn2"], dz2, B * m.ho * m.wo, d1)

    def _wg1(self, m, dz1):
        n = m.n
        self._wgrad(m.cin, m.d1, m.M1, m.x1, m.cin, dz1, m.d1, self.P.gviews[f"{n['conv1']}/kernel"], m.d1, scale=self.bn_scale[n["bn1"]])
        self._bias_grad(n["conv1"], n["bn1"], dz1, m.M1, m.d1)

    def _block_bwd(self, bi, g, B):
        """g: gradient w.r.t. the output of block bi (= bn3(conv3(y2)) + shortcut), already ReLU-masked.  Returns the gradient
        w.r.t. its input, masked by the previous block's ReLU.  The scratch tensors the side stream reads (dz2, dz1: double-buffered
        by block parity; gx) are only overwritten after the side work that read them has been waited for (side.mark / wait)."""
        m, side, adt = self._block_recs[bi], self.side, self._adt
        n, cin, d1, d2, ho, wo = m.n, m.cin, m.d1, m.d2, m.ho, m.wo
        M_in, M_out = B * m.h * m.w, B * ho * wo
        side.wait(bi + 2)
        par = side.suffix(bi & 1)
        fuse3, fuse_down = self._bwd_fused(m)
        idg, idg_sub, idg_ready = self._shortcut_dgrad(m, g, B)
        # conv3 (1x1)
        side.run(lambda: self._wg3(m, g, M_out, fuse3, fuse_down))
        dz2 = self.buf(f"scratch:dz2:{d1}:{ho}{par}", (B, ho, wo, d1), adt)
        ws3 = self._ws(n["conv3"])
        if fuse3:
            hip.conv1x1_bwd_fused(g.view(M_out, d2), m.y2.view(M_out, d1), ws3.view(d1, d2), dz2.view(M_out, d1),
                                  self.P.gviews[f"{n['conv3']}/kernel"].view(d1, d2),
                                  self.buf(f"bwdfused:slabs:{M_out}", (hip.conv1x1_bwd_fused_scratch_floats(M_out),)),
                                  scale=self.bn_scale[n["bn3"]], use_mask=True)
        else:
            hip.gemm(M_out, d1, d2, g, d2, 1, ws3, d2, 1, dz2, d1, mask=m.y2, ldmask=d1)
        # conv2 (3x3)
        side.run(lambda: self._wg2(m, dz2, B))
        dz1 = self.buf(f"scratch:dz1:{d1}:{m.h1}{par}", (B, m.h1, m.w1, d1), adt)
        hip.conv3x3(1, dz2, self._ws(n["conv2"]), dz1, B, m.h1, m.w1, d1, ho, wo, d1, m.s2, mask=m.y1, pad=m.dil, dilation=m.dil)
        # conv1 (1x1)
        side.run(lambda: self._wg1(m, dz1))
        side.mark(bi)
        side.wait(bi + 1)               # gx of this parity was read (as g) by the side work of block bi + 1
        gx = self.buf(f"scratch:gx:{cin}:{m.h}:{bi & 1}", (B, m.h, m.w, cin), adt)
        ws1 = self._ws(n["conv1"])
        if self.tf_backbone and m.first and m.stride == 2:
            # both branches read the subsampled input: d_xs = g @ Wd^T + dz1 @ W1^T (ReLU-masked at the sampled pixels),
            # scattered back into the zero-filled full-resolution gradient
            dxs = self.buf(f"scratch:dxs:{cin}:{ho}", (B, ho, wo, cin), adt)
            hip.gemm(M_out, cin, d2, g, d2, 1, self._ws(n["down"]), d2, 1, dxs, cin)
            hip.gemm(M_out, cin, d1, dz1, d1, 1, ws1, d1, 1, dxs, cin, residual=dxs, ldr=cin,
                     mask=(m.xs if bi > 0 else None), ldmask=(cin if bi > 0 else 0))
            hip.call("detr_hip_subsample2_bwd_f32", dxs.data_ptr(), gx.data_ptr(), B, m.h, m.w, self._chunks(cin), ho, wo)
        else:
            if idg_ready is not None:
                side.main.wait_event(idg_ready)
            mask, ldmask = None, 0
            if bi > 0:                  # x = ReLU output of the previous block: masked by it, or by its sign bits where the forward kept them
                bits = self._block_recs[bi - 1].out_bits
                mask, ldmask = (m.x, cin) if bits is None else (bits, bits.stride(0))
            hip.gemm(M_in, cin, d1, dz1, d1, 1, ws1, d1, 1, gx, cin, residual=idg, ldr=cin, mask=mask, ldmask=ldmask, res_sub=idg_sub)
        return gx

    # ---- input_proj + positional encoding (detr.py:172-175) ---------------------------------------------
    def _input_proj_fwd(self, feat, masks, B, L):
        """Returns (src [B*L, 256], pos)."""
        _, H, W = self._shape
        _, Hf, Wf, _ = self._feat_meta
        src = self.buf("enc:src0", (B * L, D))
        hip.gemm(B * L, D, 2048, feat, 2048, 1, self._w("input_proj/kernel"), D, 0, src, D, bias=self.P.views["input_proj/bias"])
        if masks is None:
            self.key_valid = None
            if (Hf, Wf) not in self._pos_cache:
                self._pos_cache[(Hf, Wf)] = torch.from_numpy(position_embedding_sine_host(Hf, Wf)).to(self.device)
            pos = self._pos_cache[(Hf, Wf)]
        else:
            # padded batch: per-image encoding [B*L, 256] (add_bcast / the LayerNorm's add[r % rows] take it as they take the
            # [L, 256] constant) and the key padding mask of the encoder self-attention and every decoder cross-attention
            pos = self._prepare_masks(masks, B, H, W, Hf, Wf)
        self.pos = pos
        return src, pos

    def _input_proj_bwd(self, d_x, feat, B, L, want_dx=True):
        """Returns the gradient w.r.t. the backbone's feature map (ReLU-masked), None unless want_dx."""
        G = self.P.gviews
        self._wgrad(2048, D, B * L, feat, 2048, d_x, D, G["input_proj/kernel"], D)
        self._colsum(d_x, G["input_proj/bias"])
        if not want_dx:
            return None
        g = self.buf("scratch:g_feat", feat.shape, self._adt)
        hip.gemm(B * L, 2048, D, d_x, D, 1, self._w("input_proj/kernel"), D, 1, g, 2048, mask=feat, ldmask=2048)
        return g

    # ---- encoder layer (transformer.py:157-179) -------------------------------------------------------------
    def _encoder_layer_fwd(self, i, x, qk, pos, B, L):
        """x: layer input, qk = x + pos.  Returns (output, output + pos)."""
        pfx, tag = f"transformer/encoder/layer_{i}", f"enc{i}"
        a = self.buf(f"{tag}:a", (B * L, D))
        x1 = self.buf(f"{tag}:x1", (B * L, D))
        x1h = self.buf(f"{tag}:x1h", (B * L, D), torch.bfloat16) if self.ffn16 else None
        ln1 = self._ln_spec(B * L, f"{pfx}/norm1", x1, f"{tag}:ln1", y16=x1h)
        self._self_attn_fwd(f"{tag}:sa", f"{pfx}/self_attn", qk, x, B, L, a, site=16 * i, ln=ln1, key_valid=self.key_valid)
        if ln1 is None:
            self._ln_fwd(a, f"{pfx}/norm1", x1, f"{tag}:ln1", y16=x1h)
        f = self.buf(f"{tag}:f", (B * L, D))
        x2 = self.buf(f"{tag}:x2", (B * L, D))
        # x2 + pos = the q / k input of the next layer, or `memory + pos` of the decoder (:219), in the same launch
        qk = self.buf(f"enc{i + 1}:qk" if i + 1 < self.num_enc else "dec:mem_pos", (B * L, D))
        ln2 = self._ln_spec(B * L, f"{pfx}/norm2", x2, f"{tag}:ln2", add=pos, y2=qk, ffn=True)
        self._ffn_fwd(tag, pfx, x1, f, seed=16 * i + 2, x16=x1h, ln=ln2)
        if ln2 is None:
            self._ln_fwd(f, f"{pfx}/norm2", x2, f"{tag}:ln2", add=pos, y2=qk)
        return x2, qk

    def _encoder_layer_bwd(self, i, d_x, B, L):
        """d_x: gradient w.r.t. the layer's output.  Returns the gradient w.r.t. its input."""
        pfx, tag = f"transformer/encoder/layer_{i}", f"enc{i}"
        x_in = self._bufs[f"enc{i - 1}:x2"] if i > 0 else self._bufs["enc:src0"]
        qk, a, x1, f = (self._bufs[f"{tag}:{n}"] for n in ("qk", "a", "x1", "f"))
        d_f = self.buf(f"scratch:e_d_f{self.side.suffix(tag)}", (B * L, D))
        d_y = self._ln_bwd(d_x, f, f"{pfx}/norm2", d_f, f"{tag}:ln2", drop_site=16 * i + 3, want16=self.ffn16)
        d_x1 = self.buf("scratch:e_d_x1", (B * L, D))
        self._ffn_bwd(tag, pfx, d_y, d_f, x1, d_x1, x16=self._bufs.get(f"{tag}:x1h") if self.ffn16 else None)
        d_a = self.buf(f"scratch:e_d_a{self.side.suffix(tag)}", (B * L, D))
        d_out = self._ln_bwd(d_x1, a, f"{pfx}/norm1", d_a, f"{tag}:ln1", drop_site=16 * i + 1)
        d_xn = self.buf(f"scratch:e_d_x{i & 1}", (B * L, D))
        self._self_attn_bwd(f"{tag}:sa", f"{pfx}/self_attn", d_out, d_a, qk, x_in, B, L, d_xn, site=16 * i, key_valid=self.key_valid)
        return d_xn

    # ---- decoder cross attention: Q from its layer, K / V column blocks of the shared projection buffer (_cross_kv_*) -----
    def _cross_attn_fwd(self, tag, pfx, i, q_in, res, KV, B, L, out, site, ln=None):
        """Cross attention of decoder layer i (tag = its buffer tag `dec{i}`); res: the residual operand of the out-projection."""
        V, Q, nd = self.P.views, self.Q, self.num_dec
        dp, _ = self._drop
        a16 = self.attn16
        W, bias = self._w(f"{pfx}/in_proj_kernel"), V[f"{pfx}/in_proj_bias"]
        (q_name, adt), (o_name, _) = self._a16(f"{tag}:ca:Q"), self._a16(f"{tag}:ca:O")
        Qc = self.buf(q_name, (B * Q, D), adt)
        hip.linear_fwd(q_in, W[0:D], bias[0:D], Qc, alpha=QK_ALPHA if a16 else 1.0)
        if i == 0:
            self.side.join()                                 # K / V of all layers
        Oc = self.buf(o_name, (B * Q, D), adt)
        lse = self.buf(f"{tag}:ca:lse", (B * HEADS, Q))
        K = KV[:, i * D:(i + 1) * D]
        hip.attention(Qc, K, KV[:, (nd + i) * D:(nd + i + 1) * D], Oc, lse, B, HEADS, Q, L,
                      scale=float(HD) ** -0.5, dropout_p=dp, dropout_site=site, dropout_step=self._seed_dev,
                      dropmask=self.masks.mask(site, B, Q, L) if (a16 and dp > 0.0) else None, key_valid=self.key_valid)
        if pfx in self._attn_sites:
            self._attn_map(pfx, Qc, K, lse, B, Q, L, self.key_valid)
        hip.linear_fwd(Oc, self._w(f"{pfx}/out_proj_kernel"), V[f"{pfx}/out_proj_bias"], out, residual=res, dropout_p=dp,
                       dropout_seed=site + 1, dropout_step=self._seed_dev, ln=ln)      # :226 (+ the LayerNorm behind it)

    def _cross_attn_bwd(self, tag, pfx, i, d_out, d_res, q_in, KV, dKV, B, L, d_x, site, acc_q):
        """d_out: gradient of the out-projection output (dropout backward already applied), d_res: gradient of the block output
        (residual path).  Writes d_x = gradient w.r.t. the residual input t1 (q_in = t1 + query_pos: the q gradient goes there too),
        column blocks i of dKV, and ACCUMULATES the q gradient into acc_q (the query_pos sum)."""
        G, Q, nd = self.P.gviews, self.Q, self.num_dec
        dp, _ = self._drop
        a16 = self.attn16
        W = self._w(f"{pfx}/in_proj_kernel")
        (q_name, adt), (o_name, _) = self._a16(f"{tag}:ca:Q"), self._a16(f"{tag}:ca:O")
        Qc, Oc = self._bufs[q_name], self._bufs[o_name]
        dO = self.buf(f"scratch:dO:{B * Q}:{int(a16)}", (B * Q, D), adt)
        hip.linear_dgrad(d_out, self._w(f"{pfx}/out_proj_kernel"), dO)
        dQc = self.buf(f"scratch:dQc:{int(a16)}{self.side.suffix(tag)}", (B * Q, D), adt)
        delta = self.buf(f"scratch:delta:{B * Q}", (2 * B * HEADS, Q))
        kc, vc = slice(i * D, (i + 1) * D), slice((nd + i) * D, (nd + i + 1) * D)
        hip.attention(Qc, KV[:, kc], KV[:, vc], Oc, self._bufs[f"{tag}:ca:lse"], B, HEADS, Q, L, scale=float(HD) ** -0.5,
                      dropout_p=dp, dropout_site=site, dropout_step=self._seed_dev, d_o=dO, dq=dQc, dk=dKV[:, kc], dv=dKV[:, vc],
                      delta=delta, dropmask=self.masks.mask(site, B, Q, L) if (a16 and dp > 0.0) else None, key_valid=self.key_valid)
        self.side.run(lambda: hip.gemm_group([
            hip.linear_wgrad_call(d_out, Oc, G[f"{pfx}/out_proj_kernel"], bias_grad=G[f"{pfx}/out_proj_bias"]),
            hip.linear_wgrad_call(dQc, q_in, G[f"{pfx}/in_proj_kernel"][0:D], bias_grad=G[f"{pfx}/in_proj_bias"][0:D])]))
        hip.gemm_group([hip.linear_dgrad_call(dQc, W[0:D], acc_q, residual=acc_q),
                        hip.linear_dgrad_call(dQc, W[0:D], d_x, residual=d_res)])

    # ---- layer-invariant cross-attention K / V (transformer.py:221-223: memory is the same for every layer) --------------
    def _cross_kv_fwd(self, memory, mem_pos, B, L):
        """K / V projections of `memory` for ALL decoder layers at once, on the second stream: the first decoder self-attention
        block -- 800-row kernels -- does not need them (_cross_attn_fwd of layer 0 joins)."""
        nd = self.num_dec
        ct = self._cross_tables()
        if self._stale(f"cross:{self.compute}"):
            hip.multi_copy(ct["gather"])
        name, adt = self._a16("dec:KV")
        KV = self.buf(name, (B * L, 2 * nd * D), adt)
        self.side.run(lambda: hip.gemm_group([hip.linear_fwd_call(mem_pos, ct["Wkv"][0:nd * D], ct["bkv"][0:nd * D], KV[:, 0:nd * D]),
                                              hip.linear_fwd_call(memory, ct["Wkv"][nd * D:], ct["bkv"][nd * D:], KV[:, nd * D:])]))
        return KV

    def _cross_kv_bwd(self, dKV, memory, mem_pos, B, L):
        """Weight gradient of the gathered copy (scattered back into the per-layer in_proj gradients by one launch) and ONE data
        gradient GEMM with K = 2*nd*256.  Returns d_mem."""
        nd = self.num_dec
        ct = self._cross_tables()
        hip.zero_(ct["gW"])
        hip.zero_(ct["gb"])
        hip.gemm_group([hip.linear_wgrad_call(dKV[:, 0:nd * D], mem_pos, ct["gW"][0:nd * D], bias_grad=ct["gb"][0:nd * D]),
                        hip.linear_wgrad_call(dKV[:, nd * D:], memory, ct["gW"][nd * D:], bias_grad=ct["gb"][nd * D:])])
        self.side.join()
        hip.flush_reduces()                            # the scatter reads the gathered gradient
        hip.multi_copy(ct["scatter"])
        d_mem = self.buf("scratch:d_mem", (B * L, D))
        hip.linear_dgrad(dKV, ct["Wkv"], d_mem)        # d(memory + pos) through K and d(memory) through V land on the same tensor
        return d_mem

    # ---- decoder layer (transformer.py:207-234) -----------------------------------------------------------------
    def _decoder_layer_fwd(self, i, tgt, qin, qpos, KV, t3, B, L):
        """tgt: layer input, qin = tgt + query_pos; t3: where the output goes.  Returns (t3, t3 + query_pos; None behind the last layer)."""
        pfx, tag = f"transformer/decoder/layer_{i}", f"dec{i}"
        Q, ds = self.Q, 16 * (32 + i)
        a1 = self.buf(f"{tag}:a1", (B * Q, D))
        t1 = self.buf(f"{tag}:t1", (B * Q, D))
        q2 = self.buf(f"{tag}:q2", (B * Q, D))
        ln1 = self._ln_spec(B * Q, f"{pfx}/norm1", t1, f"{tag}:ln1", add=qpos, y2=q2)
        self._self_attn_fwd(f"{tag}:sa", f"{pfx}/self_attn", qin, tgt, B, Q, a1, site=ds, ln=ln1)
        if ln1 is None:
            self._ln_fwd(a1, f"{pfx}/norm1", t1, f"{tag}:ln1", add=qpos, y2=q2)      # q2 = t1 + query_pos (:219)
        a2 = self.buf(f"{tag}:a2", (B * Q, D))
        t2 = self.buf(f"{tag}:t2", (B * Q, D))
        t2h = self.buf(f"{tag}:t2h", (B * Q, D), torch.bfloat16) if self.ffn16 else None
        ln2 = self._ln_spec(B * Q, f"{pfx}/norm2", t2, f"{tag}:ln2", y16=t2h)
        self._cross_attn_fwd(tag, f"{pfx}/multihead_attn", i, q2, t1, KV, B, L, a2, site=ds + 2, ln=ln2)
        if ln2 is None:
            self._ln_fwd(a2, f"{pfx}/norm2", t2, f"{tag}:ln2", y16=t2h)
        f = self.buf(f"{tag}:f", (B * Q, D))
        self._bufs[f"{tag}:t3"] = t3
        qin = self.buf(f"dec{i + 1}:qin", (B * Q, D)) if i + 1 < self.num_dec else None        # next layer's tgt + query_pos
        ln3 = self._ln_spec(B * Q, f"{pfx}/norm3", t3, f"{tag}:ln3", add=qpos if qin is not None else None, y2=qin, ffn=True)
        self._ffn_fwd(tag, pfx, t2, f, seed=ds + 4, x16=t2h, ln=ln3)
        if ln3 is None:
            self._ln_fwd(f, f"{pfx}/norm3", t3, f"{tag}:ln3", add=qpos if qin is not None else None, y2=qin)
        return t3, qin

    def _decoder_layer_bwd(self, i, d_t3n, d_next, KV, dKV, acc_qpos, B, L):
        """d_t3n: gradient of this level's head input w.r.t. t3, d_next: the gradient the layer above sends into t3 (None above
        the last layer).  Returns the gradient w.r.t. the layer's input (None for layer 0: the constant zero target)."""
        pfx, tag = f"transformer/decoder/layer_{i}", f"dec{i}"
        BQ, ds, sx = B * self.Q, 16 * (32 + i), self.side.suffix(tag)
        t1, t2, a1, a2, f, qin, q2 = (self._bufs[f"{tag}:{n}"] for n in ("t1", "t2", "a1", "a2", "f", "qin", "q2"))
        tgt = self._bufs[f"dec{i - 1}:t3"] if i > 0 else self._bufs["dec:tgt0"]
        d_f = self.buf(f"scratch:d_f{sx}", (BQ, D))
        # d_t3 = d_t3n + d_next: the two branches are summed by the norm3 backward itself
        d_y = self._ln_bwd(d_t3n, f, f"{pfx}/norm3", d_f, f"{tag}:ln3", drop_site=ds + 5, want16=self.ffn16, dy_add=d_next)
        d_t2 = self.buf("scratch:d_t2", (BQ, D))
        self._ffn_bwd(tag, pfx, d_y, d_f, t2, d_t2, x16=self._bufs.get(f"{tag}:t2h") if self.ffn16 else None)
        d_a2 = self.buf(f"scratch:d_a2{sx}", (BQ, D))
        d_out = self._ln_bwd(d_t2, a2, f"{pfx}/norm2", d_a2, f"{tag}:ln2", drop_site=ds + 3)
        d_t1 = self.buf("scratch:d_t1", (BQ, D))
        # q2 = t1 + query_pos ; a2 = attn + t1: the q gradient goes to t1 (with the residual path) and to the query_pos sum
        self._cross_attn_bwd(tag, f"{pfx}/multihead_attn", i, d_out, d_a2, q2, KV, dKV, B, L, d_t1, site=ds + 2, acc_q=acc_qpos)
        d_a1 = self.buf(f"scratch:d_a1{sx}", (BQ, D))
        d_out = self._ln_bwd(d_t1, a1, f"{pfx}/norm1", d_a1, f"{tag}:ln1", drop_site=ds + 1)
        # self attention: qin = tgt + query_pos feeds q and k, tgt feeds v and the residual
        d_tgt = self.buf(f"scratch:d_tgt{i & 1}", (BQ, D)) if i > 0 else None
        self._self_attn_bwd(f"{tag}:sa", f"{pfx}/self_attn", d_out, d_a1, qin, tgt, B, self.Q, d_tgt, site=ds, acc_qk=acc_qpos)
        return d_tgt

    # ---- heads (detr.py:181-204 / :94-114): always exact fp32 (compute=0), like LayerNorm / softmax / the set loss -----------
    def _head_layers(self):
        """(parameter name, kernel stored as (in, out)) of the class Linear and the three of the box MLP: the reference's Linear
        kernels are (out, in), the Keras Dense kernels of the nb_class heads (in, out)."""
        if self.nb_class is None:
            return [("class_embed", False)] + [(f"bbox_embed_{j}", False) for j in range(3)]
        return [("cls_layer", True)] + [(f"pos_layer/dense_{j}", True) for j in range(3)]

    def _dense(self, x, layer, out, act=0):
        name, in_out = layer
        k = self.P.views[f"{name}/kernel"]
        hip.gemm(x.shape[0], k.shape[1 if in_out else 0], x.shape[1], x, x.stride(0), 1, k, k.stride(0), 0 if in_out else 1,
                 out, out.stride(0), bias=self.P.views[f"{name}/bias"], act=act, compute=0)

    def _dense_bwd(self, dy, x, layer, dx, mask=None, residual=None):
        """Weight and bias gradient of one head Linear, then dx = dy @ W^T (+ residual) (masked by mask > 0)."""
        name, in_out = layer
        k, gk, gb = self.P.views[f"{name}/kernel"], self.P.gviews[f"{name}/kernel"], self.P.gviews[f"{name}/bias"]
        if in_out:      # dW (in, out) = x^T dy: dy is the B operand, its column sums are a launch of their own
            n_in, n_out = k.shape
            self._wgrad(n_in, n_out, x.shape[0], x, x.stride(0), dy, dy.stride(0), gk, n_out, compute=0)
            self._colsum(dy, gb)
        else:           # dW (out, in) = dy^T x, the bias gradient as the row sums of its A operand
            n_out, n_in = k.shape
            hip.linear_wgrad(dy, x, gk, bias_grad=gb, compute=0)
        hip.gemm(dy.shape[0], n_in, n_out, dy, dy.stride(0), 1, k, k.stride(0), 1 if in_out else 0, dx, dx.stride(0), residual=residual,
                 ldr=(dx.stride(0) if residual is not None else 0), mask=mask, ldmask=(mask.stride(0) if mask is not None else 0), compute=0)

    def _heads_fwd(self, hs2):
        """hs2 [R, 256]: every decoder level's normalised output.  Returns (logits [R, C], boxes [R, 4])."""
        R = hs2.shape[0]
        cls, mlp0, mlp1, mlp2 = self._head_layers()
        logits = self.buf("head:logits", (R, self.C))
        boxes = self.buf("head:boxes", (R, 4))
        t_a, t_b = self.buf("head:t1", (R, D)), self.buf("head:t2", (R, D))
        self._dense(hs2, cls, logits)
        self._dense(hs2, mlp0, t_a, act=1)
        self._dense(t_a, mlp1, t_b, act=1)
        self._dense(t_b, mlp2, boxes, act=2)
        return logits, boxes

    def _heads_bwd(self, dl, db):
        """dl [R, C], db [R, 4]: gradients w.r.t. logits and (sigmoid) boxes.  Returns d_hs [R, 256]."""
        R = dl.shape[0]
        cls, mlp0, mlp1, mlp2 = self._head_layers()
        hs2 = self._bufs["dec:hs"].view(R, D)
        boxes, t_a, t_b = self._bufs["head:boxes"], self._bufs["head:t1"], self._bufs["head:t2"]
        dz3 = self.buf("scratch:dz3", (R, 4))
        hip.call("detr_hip_sigmoid_bwd_f32", db.data_ptr(), boxes.data_ptr(), dz3.data_ptr(), R * 4)
        d_hs = self.buf("scratch:d_hs", (R, D))
        dt_b, dt_a = self.buf("scratch:dt_b", (R, D)), self.buf("scratch:dt_a", (R, D))
        self._dense_bwd(dz3, t_b, mlp2, dt_b, mask=t_b)
        self._dense_bwd(dt_b, t_a, mlp1, dt_a, mask=t_a)
        self._dense_bwd(dt_a, hs2, mlp0, d_hs)
        self._dense_bwd(dl, hs2, cls, d_hs, residual=d_hs)
        return d_hs
