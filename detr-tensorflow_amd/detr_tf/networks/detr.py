"""Model factory of the drop-in API: `get_detr_model(...)` (reference detr_tf/networks/detr.py:116-204).

The returned object is callable like the reference's Keras model -- `model(images, training=bool)`
with fp32 NHWC images -- and returns the same output structure
`{"pred_logits": [B,Q,C], "pred_boxes": [B,Q,4], "aux": [{...}] * (levels-1)}` (detr.py:190-204);
underneath every layer is a HIP kernel launch of `engine.DetrEngine`.
"""
import os

import numpy as np
import torch

from ..engine import DetrEngine, dilation_flags
from ..params import RESNET50_BLOCKS, RESNET101_BLOCKS


class DetrOutputs(dict):
    """Output dict + handles used by get_losses / run_train_step (levels tensors, loss state)."""
    levels_logits = None
    levels_boxes = None
    set_loss = None
    reduce_sums = None
    model = None


class _Layer:
    def __init__(self, name, variables):
        self.name = name
        self.trainable_variables = variables


BACKBONES = {"resnet50": RESNET50_BLOCKS, "resnet101": RESNET101_BLOCKS}


def resolve_backbone(backbone, replace_stride_with_dilation=None, tf_backbone=False):
    """(blocks, dilation flags) of a backbone name.  "resnet50-dc5" / "resnet101-dc5" name replace_stride_with_dilation =
    [False, False, True] (DETR-DC5: layer4 at stride 1, dilation 2 -- feature stride 16; resnet_backbone.py:36-85).  Pure host
    code: raises ValueError for an unknown name, contradicting arguments, or flags together with tf_backbone=True."""
    base, dc5 = (backbone[:-4], True) if isinstance(backbone, str) and backbone.endswith("-dc5") else (backbone, False)
    if base not in BACKBONES:
        raise ValueError(f"backbone must be one of {sorted(BACKBONES)} or their '-dc5' variants, got {backbone!r}")
    flags = dilation_flags(replace_stride_with_dilation)
    if dc5:
        if replace_stride_with_dilation is not None and flags != (False, False, True):
            raise ValueError(f"backbone={backbone!r} means replace_stride_with_dilation=[False, False, True], got {list(flags)}")
        flags = (False, False, True)
    if tf_backbone and any(flags):
        raise ValueError("replace_stride_with_dilation needs the reference backbone: tf.keras.applications.ResNet50 "
                         "(tf_backbone=True) has no such option")
    return BACKBONES[base], flags


class DetrModel:
    def __init__(self, include_top=True, nb_class=None, num_decoder_layers=6, num_encoder_layers=6, num_queries=100,
                 backbone="resnet50", device=None, seed=0, dropout=0.1, precision="fp32", tf_backbone=False,
                 replace_stride_with_dilation=None):
        blocks, dilate = resolve_backbone(backbone, replace_stride_with_dilation, tf_backbone)      # argument errors before any device is needed
        device = device or (f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else None)
        if device is None:
            raise RuntimeError("DETR HIP model needs a GPU: the hot path has no CPU fallback")
        self.include_top = include_top
        self.headless = (not include_top) and nb_class is None
        self.name = "detr" if self.headless else "detr_finetuning"
        self.tf_backbone = bool(tf_backbone)
        self.eval_graph, self._eval_graph, self._eval_seen = True, None, None     # hipGraph replay of the eval forward (_eval_forward)
        self.engine = DetrEngine(device, blocks, num_encoder_layers, num_decoder_layers, num_queries, 92, nb_class, seed,
                                 tf_backbone=tf_backbone, replace_stride_with_dilation=dilate)
        self.backbone = backbone
        self.replace_stride_with_dilation = dilate
        if precision not in ("fp32", "bf16", "fp32x3"):
            raise ValueError("precision must be 'fp32' (exact fp32 MFMA, parity mode), 'fp32x3' (fp32 storage and accuracy on the bf16 matrix "
                             "pipe: 3-way operand split, detr_gemm_desc.compute = 2) or 'bf16' (bf16 MFMA, fp32 accumulate)")
        self.engine.compute = 1 if precision == "bf16" else 0
        self.engine.f32_split = precision == "fp32x3"
        self.precision = precision
        self.engine.dropout_p = float(dropout)  # Transformer(dropout=0.1), applied when called with training=True
        self.dp = None                        # parallel.DataParallel when training on several GPUs
        self.device = self.engine.device

    # ---- Keras-like surface used by the reference's scripts / optimizers.py ----------------
    @property
    def trainable_variables(self):
        return list(self.engine.P.views.values())

    @property
    def layers(self):
        tops = []
        for k in self.engine.P.shapes:
            t = k.split("/", 1)[0]
            if t not in tops:
                tops.append(t)
        return [_Layer(t, [v for k, v in self.engine.P.views.items() if k.split("/", 1)[0] == t]) for t in tops]

    def get_layer(self, name):
        for l in self.layers:
            if l.name == name:
                return l
        raise ValueError(f"No such layer: {name}")

    def summary(self):
        P = self.engine.P
        n_train = sum(n for _, n in P.offsets.values())
        n_frozen = sum(4 * c for c in P.bn.values())
        print(f'Model: "{self.name}"  trainable params: {n_train:,}  non-trainable (frozen BN): {n_frozen:,}')
        dilate = self.replace_stride_with_dilation
        variant = "plain (feature stride 32)" if not any(dilate) else \
            ("DC5 (layer4 dilated, feature stride 16)" if dilate == (False, False, True) else
             "dilated " + "+".join(f"layer{i + 2}" for i, f in enumerate(dilate) if f) + f" (feature stride {32 >> sum(dilate)})")
        print(f"  backbone: {self.backbone}, {variant}, replace_stride_with_dilation={list(dilate)}")
        for l in self.layers:
            print(f"  {l.name:28s} {sum(v.numel() for v in l.trainable_variables):>12,}")

    @staticmethod
    def _npz(path):
        return path if path.endswith(".npz") else path + ".npz"      # np.savez appends the suffix: keep save / load symmetric

    def wanted_shapes(self):
        """{parameter name: shape} of everything a weight file may provide (trainable tensors + frozen-BN vectors)."""
        P = self.engine.P
        out = dict(P.shapes)
        for p, c in P.bn.items():
            for leaf in P.bn_leaves:
                out[f"{p}/{leaf}"] = (c,)
        return out

    def load_weights(self, path_or_dict):
        """A parameter dict, this package's `.npz` file, or a TensorFlow checkpoint prefix (`x.ckpt` with `x.ckpt.index` next to
        it: the reference's own weight files, weights.py:33 -- read without TensorFlow).  Returns the names left unset."""
        # (ParamStore.load / load_dict notify the engine: frozen-BN refold + weights-version bump)
        if isinstance(path_or_dict, str) and os.path.exists(path_or_dict + ".index"):
            from .weights import load_tf_checkpoint_params
            params, unused = load_tf_checkpoint_params(path_or_dict, self.wanted_shapes())
            missing = self.engine.load_params(params)
            # `.expect_partial()` of the reference (weights.py:35) covers the fine-tuning heads only: everything else of the
            # network must come out of the file, or the model silently keeps its random initialisation
            heads = ("class_embed", "bbox_embed", "cls_layer", "pos_layer")
            lost = sorted(n for n in (missing or ()) if not n.startswith(heads))
            self.last_load_report = dict(missing=sorted(missing or ()), unused=sorted(unused))
            if lost:
                shown = ", ".join(lost[:8]) + (" ..." if len(lost) > 8 else "")
                extra = ", ".join(sorted(unused)[:8]) + (" ..." if len(unused) > 8 else "")
                raise ValueError(f"{path_or_dict}: {len(lost)} network parameters were not found in the checkpoint ({shown}); "
                                 f"{len(unused)} checkpoint variables matched no parameter by name and shape ({extra})")
            if unused:
                import warnings
                warnings.warn(f"{path_or_dict}: {len(unused)} checkpoint variables were not used: " +
                              ", ".join(sorted(unused)[:8]) + (" ..." if len(unused) > 8 else ""))
            return missing
        return self.engine.P.load(self._npz(path_or_dict)) if isinstance(path_or_dict, str) else self.engine.load_params(path_or_dict)

    def save_weights(self, path, weights="model"):
        """weights="ema": the averaged weights kept by config.ema_decay (optimizers.WeightEMA) under the normal parameter
        names, with the frozen-BN vectors: `load_weights(path)` into a fresh model gives the deployable averaged model."""
        self.engine.P.save(self._npz(path), weights=weights)

    def set_class_prior(self, prior=0.01):
        """Focal-loss initialisation of the class head (Lin et al., section 4.1): every bias becomes -log((1 - prior) / prior), so a
        fresh head scores every class at sigmoid = `prior` and the focal loss of the many unmatched queries starts small (without it
        a fresh head starts with a label_cost in the hundreds).  Written through load_weights' path: the bf16 shadow, the recorded
        graphs and a weight average follow.  Returns the bias value."""
        import math
        prior = float(prior)
        if not (math.isfinite(prior) and 0.0 < prior < 1.0):
            raise ValueError(f"set_class_prior: prior = {prior}: expected a value inside (0, 1)")
        if self.headless:
            raise ValueError("set_class_prior: this model has no class head (include_top=False without nb_class)")
        name = self.engine._head_layers()[0][0] + "/bias"
        value = -math.log((1.0 - prior) / prior)
        self.engine.load_params({name: np.full(tuple(self.engine.P.shapes[name]), value, np.float32)})
        return value

    # ---- forward ----------------------------------------------------------------------------
    def _eval_forward(self, images, masks=None, attn_sites=()):
        """Eval-mode forward.  The launch sequence of a fixed input shape is static, so the second call with the same shape
        (and the same weights version) records it as a hipGraph and later calls replay it: a single 480x640 image is ~300
        launches whose host cost (ctypes, ~10 us each) exceeds their GPU time.  DETR_HIP_GRAPH=0 / model.eval_graph = False:
        always eager.  Outputs are views of the engine's buffers either way (the caller clones).  attn_sites: the attention maps this
        call also writes (engine.attn_maps); they are part of the graph key, and a replay refills the same buffers."""
        eng = self.engine
        if masks is not None and not (torch.is_tensor(masks) and masks.is_cuda):
            masks = eng._host_masks(masks, tuple(images.shape[:3]))      # validated on the host, then a device input like any other
        if not (self.eval_graph and os.environ.get("DETR_HIP_GRAPH", "1") != "0" and images.is_cuda):
            return eng.forward(images, training=False, masks=masks, attn_sites=attn_sites)
        key = (tuple(images.shape), eng._weights_version, eng.compute, tuple(eng.dilate), tuple(attn_sites), masks is not None)
        g = self._eval_graph
        # a graph addresses the engine's buffers as they were at capture: any later re-allocation (a forward of another
        # shape in between) makes it unusable -- engine.buf_generation tells
        if g is not None and g["key"] == key and g["gen"] == eng.buf_generation:
            g["static"].copy_(images)
            if masks is not None:
                g["static_mask"].copy_(masks)
            g["graph"].replay()
            eng.attn_maps = dict(g["maps"])
            return g["out"]
        if g is not None and g["gen"] != eng.buf_generation:
            self._eval_graph = g = None
        if self._eval_seen != (key, eng.buf_generation):
            # first sighting of this shape with these buffers: eager (allocates the buffers, refreshes derived weight copies)
            out = eng.forward(images, training=False, masks=masks, attn_sites=attn_sites)
            self._eval_seen = (key, eng.buf_generation)
            return out
        static = g["static"] if g is not None and g["static"].shape == images.shape else torch.empty_like(images)
        static.copy_(images)
        static_mask = None
        if masks is not None:          # the mask is a static input like the images: copied in before every replay
            static_mask = torch.empty_like(masks)
            static_mask.copy_(masks)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):       # (see training._Segments.begin)
            out = eng.forward(static, training=False, masks=static_mask, attn_sites=attn_sites)
        self._eval_graph = dict(key=key, static=static, static_mask=static_mask, graph=graph, out=out, gen=eng.buf_generation,
                                maps=dict(eng.attn_maps))
        graph.replay()
        return out

    def __call__(self, images, training=False, masks=None, need_weights=None, return_embeddings=False):
        """images: [B, H, W, 3] float32, or the reference's `(images, masks)` pair (detr.py:65-72); masks: [B, H, W] bool, True =
        padding (a padded mixed-size batch).  Host masks are validated here (ValueError for an image without a
        valid feature position); device masks on the device (engine.check_mask_status).
        need_weights (the reference's MultiHeadAttention need_weights, transformer.py:285-286, 349-354; evaluation mode only): True
        = the head-averaged maps of the last encoder layer's self-attention [B, L, L] and of the last decoder layer's
        cross-attention [B, Q, L] (L = Hf * Wf); an iterable of site names (engine.attn_site_names()) = those.  The result gains
        out["attn"] = {site name: fp32 tensor [B, T, S]}.
        return_embeddings (evaluation mode only, a model with a head): the result gains out["embed"], fp32 [B, Q, 256]: the last
        decoder layer's normalised hidden state of every object query -- what the headless mode returns as hs[-1] --, the default
        appearance descriptor of inference.Tracker(embed_dim=256).  A copy of the engine's buffer taken after the forward (or the
        graph replay): no kernel of the model is added and the captured graph is the same one."""
        sites = self._need_weights_sites(need_weights, training)
        if return_embeddings:
            if training:
                raise NotImplementedError("return_embeddings: the embeddings are returned in evaluation mode only; with training=True "
                                          "the outputs are views of the engine's buffers")
            if self.headless:
                raise NotImplementedError("return_embeddings: the headless mode (include_top=False, nb_class=None) already returns the "
                                          "hidden states themselves: take hs[-1]")
        if isinstance(images, (tuple, list)):
            if masks is not None or len(images) != 2:
                raise TypeError("model((images, masks)): pass the mask once, either in the tuple or as masks=")
            images, masks = images
        if isinstance(images, np.ndarray):
            images = torch.from_numpy(images)
        images = images.to(device=self.device, dtype=torch.float32)
        if masks is not None and torch.is_tensor(masks) and masks.is_cuda:
            if masks.dtype not in (torch.bool, torch.uint8):
                masks = masks != 0
            masks = masks.contiguous()
        logits, boxes = self.engine.forward(images, training=True, masks=masks) if training else self._eval_forward(images, masks, sites)
        if self.headless:
            hs = self.engine._bufs["dec:hs"].view(self.engine.num_dec, images.shape[0], self.engine.Q, 256)
            return hs if training else hs.clone()
        if not training:
            # inference outputs are often kept across calls (predictions accumulated for mAP, train vs val outputs): hand out
            # fresh tensors like Keras does.  Training outputs stay views of the engine's buffers (consumed by get_losses
            # before the next forward; no allocation in the step).
            logits, boxes = logits.clone(), boxes.clone()
        out = DetrOutputs()
        out["pred_logits"], out["pred_boxes"] = logits[-1], boxes[-1]
        out["aux"] = [{"pred_logits": logits[i], "pred_boxes": boxes[i]} for i in range(logits.shape[0] - 1)]
        out.levels_logits, out.levels_boxes, out.model = logits, boxes, self
        if sites:
            out["attn"] = {name: self.engine.attn_maps[name].clone() for name in sites}
        if return_embeddings:
            eng = self.engine
            out["embed"] = eng._bufs["dec:hs"][eng.num_dec - 1].view(images.shape[0], eng.Q, 256).clone()
        if self.dp is not None:
            out.reduce_sums = self.dp.reduce_sums
        return out

    def default_attn_sites(self):
        """The two maps of need_weights=True: last encoder self-attention, last decoder cross-attention."""
        eng = self.engine
        sites = [f"transformer/encoder/layer_{eng.num_enc - 1}/self_attn"] if eng.num_enc > 0 else []
        if eng.num_dec > 0:
            sites.append(f"transformer/decoder/layer_{eng.num_dec - 1}/multihead_attn")
        return tuple(sites)

    def _need_weights_sites(self, need_weights, training):
        if need_weights is None or need_weights is False:
            return ()
        sites = self.default_attn_sites() if need_weights is True else need_weights
        sites = self.engine._check_attn_sites(sites, training)          # unknown names, training=True: rejected here
        if sites and self.headless:
            raise NotImplementedError("need_weights: the headless mode (include_top=False, nb_class=None) returns a bare tensor and "
                                      "cannot carry attention maps; build the model with a head")
        return sites


def get_detr_model(config, include_top=False, nb_class=None, weights=None, tf_backbone=False, num_decoder_layers=6,
                   num_encoder_layers=6, num_queries=100, backbone="resnet50", device=None, seed=0, dropout=0.1,
                   precision="fp32", replace_stride_with_dilation=None):
    """Same arguments and three output modes as the reference (detr.py:116-204); `num_queries`,
    `backbone` ("resnet50" | "resnet101", resnet_backbone.py:35-66), `device` and `seed` are
    extensions (the reference never exposes num_queries / ResNet101); `dropout` is the
    transformer dropout rate of training mode (the reference hard-codes 0.1, transformer.py:9).
    `replace_stride_with_dilation` (one flag each for layer2..4, resnet_backbone.py:36-85) or the backbone names
    "resnet50-dc5" / "resnet101-dc5" (= [False, False, True]) build the dilated variants.  A DC5 checkpoint has the same
    variable names and shapes as a plain one: it loads into either model, so the flag must be given with it."""
    resolve_backbone(backbone, replace_stride_with_dilation, tf_backbone)      # argument errors first: before the config is touched
    if tf_backbone:
        # detr.py:146-148: the backbone becomes tf.keras.applications.ResNet50 (ResNet v1, conv biases, BatchNormalization in
        # inference mode) and the data pipeline switches to the caffe-style BGR mean subtraction.  (The reference also
        # downloads the ImageNet weights; here the backbone starts from the seeded random init unless `weights` is given.)
        if backbone != "resnet50":
            raise ValueError("tf_backbone=True is tf.keras.applications.ResNet50")
        config.normalized_method = "tf_resnet"
    model = DetrModel(include_top=include_top, nb_class=nb_class, num_decoder_layers=num_decoder_layers,
                      num_encoder_layers=num_encoder_layers, num_queries=num_queries, backbone=backbone, device=device,
                      seed=seed, dropout=dropout, precision=precision, tf_backbone=tf_backbone,
                      replace_stride_with_dilation=replace_stride_with_dilation)
    if weights is not None:
        if isinstance(weights, str) and weights == "detr":
            # the reference downloads three files from GCS into weights/detr/ (weights.py:5-11,24-32) and loads
            # weights/detr/detr.ckpt; there is no network here, but files placed there are read (networks/tf_checkpoint.py)
            weights = os.path.join("weights", "detr", "detr.ckpt")
            if not os.path.exists(weights + ".index"):
                raise FileNotFoundError(
                    f'weights="detr": {weights}.index not found.  The reference fetches checkpoint / detr.ckpt.index / '
                    "detr.ckpt.data-00000-of-00001 from https://storage.googleapis.com/visualbehavior-publicweights/detr/ "
                    "(weights.py:5-11); put them under weights/detr/, or convert the original PyTorch detr-r50 state-dict with "
                    "`python -m detr_tf.networks.weights in.pth out.npz` and pass the .npz path")
            model.load_weights(weights)          # (`.expect_partial()`, weights.py:35: fine-tuning heads are not in the file)
            weights = None
    if weights is not None:
        model.load_weights(weights)
    if include_top is False and nb_class is not None:
        config.add_nlayers([_Layer("cls_layer", None), _Layer("pos_layer", None)])      # detr.py:103
    return model
