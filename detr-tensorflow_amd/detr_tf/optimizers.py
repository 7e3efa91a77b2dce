"""Optimiser side of the drop-in API (reference detr_tf/optimizers.py:10-163).

Three Adam(clipnorm) optimisers -- backbone / transformers / nlayers -- over disjoint groups of a
flat fp32 parameter buffer; per-TENSOR clip-by-norm and the Adam update are two HIP launches per
group (csrc/optim.hip).  Gradients come from the engine's hand-written backward.

Opt-in extensions (training_config.py: weight_decay, global_clipnorm, adam_epsilon), all read at every step:
  * config.weight_decay > 0: decoupled decay of every trained tensor, p -= lr * weight_decay * p (tf.keras AdamW);
  * config.global_clipnorm = c: ONE L2 norm G over every tensor of every trained group, all gradients scaled by
    c / max(G, c) (tf.clip_by_global_norm).  It REPLACES the per-tensor gradient_norm_clipping ("global wins").  No group
    can be updated before the gradient of all of them is complete, so `aggregate_grad_and_apply` only accumulates and
    the update of all trained groups -- three launches: partial sums, finalize, update (JointAdam) -- runs in the call
    of the LAST trained group of GROUPS at an apply step;
  * optimizer_state / load_optimizer_state (+ the .npz file forms) save and restore moments, step counts, pending
    gradient accumulators and the engine's dropout step counter;
  * config.ema_decay = d: an exponential moving average of the weights (tf.train.ExponentialMovingAverage) in a second flat
    fp32 buffer, `store.ema`: ONE launch per apply step, after the update of the last trained group, over the chunk list of
    all trained groups (WeightEMA); `ema_weights(model)` swaps the averaged weights in for evaluation / saving and back.
With the defaults nothing below differs from the three Adam(clipnorm) optimisers: same launches, same bits.
"""
import math
from ctypes import byref, c_float

import numpy as np
import torch

from . import _hip as hip
from .params import GROUPS

CHUNK = 8192


class GroupAdam:
    """tf.keras.optimizers.Adam(learning_rate=<callable>, clipnorm=...) for one variable group
    (optimizers.py:86-88): beta1 .9, beta2 .999, epsilon 1e-7, bias-corrected step size."""

    def __init__(self, store, group_id, lr_getter, clipnorm, nlayers, engine=None, config=None):
        self.store, self.group_id, self.lr_getter, self.clipnorm = store, group_id, lr_getter, clipnorm
        self.config = config          # weight_decay / adam_epsilon are read from it at every step (None: 0 / 1e-7)
        self.engine = engine          # its derived weight copies (BN-folded kernels, bf16 shadow) go stale with every apply
        self.iterations = 0
        self.beta_1, self.beta_2, self.epsilon = 0.9, 0.999, 1e-7
        dev = store.device
        tables = store.build_tables(nlayers, CHUNK)
        grp = tables["group_host"]
        keep = [i for i, t in enumerate(tables["chunk_tensor"].tolist()) if grp[t] == group_id]
        self.names = [n for n, g in zip(tables["names"], grp) if g == group_id]
        self.n_chunks = len(keep)
        idx = torch.tensor(keep, dtype=torch.int64, device=dev)
        self.chunk_tensor = tables["chunk_tensor"][idx].contiguous() if keep else None
        self.chunk_start = tables["chunk_start"][idx].contiguous() if keep else None
        self.seg_end = tables["seg_end"]
        self.tensor_group = torch.tensor(grp, dtype=torch.int32, device=dev)
        self.sumsq = torch.zeros(max(1, self.n_chunks), dtype=torch.float32, device=dev)     # one partial sum of squares per chunk
        if not hasattr(store, "adam_m"):            # the groups own disjoint slices of shared moment buffers
            store.adam_m = torch.zeros_like(store.flat)
            store.adam_v = torch.zeros_like(store.flat)
        self.m, self.v = store.adam_m, store.adam_v
        self.hyper = torch.zeros(16, dtype=torch.float32, device=dev)     # the Adam(clipnorm) kernels read the first 8

    def learning_rate(self):
        return float(self.lr_getter())

    def weight_decay(self):
        return float(getattr(self.config, "weight_decay", 0.0) or 0.0)

    def step_sizes(self):
        """(lr, bias-corrected step size) at the current `iterations`."""
        t, lr = self.iterations, self.learning_rate()
        return lr, lr * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def set_step_hyper(self):
        """Advances the Adam step counter and writes this step's hyper-parameters (bias-corrected step size, clipnorm,
        betas, epsilon) to DEVICE memory.  Separate from the kernels that consume them, so that a captured training
        step (training.GraphedTrainStep) can be replayed with fresh values."""
        self.iterations += 1
        t = self.iterations
        self.epsilon = float(getattr(self.config, "adam_epsilon", self.epsilon))
        lr_t = self.learning_rate() * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)
        clip = self.clipnorm if self.clipnorm is not None else 0.0
        wd = self.weight_decay()
        if wd > 0.0:                  # the decay-aware kernel reads the 16-float block (csrc/optim.hip)
            lr = self.learning_rate()
            write_hyper16(self.hyper, [lr_t, lr_t, lr_t, clip, self.beta_1, self.beta_2, self.epsilon, wd, lr, lr, lr, 1.0, 1.0, 1.0,
                                       0.0, 0.0])
            return
        hip.call("detr_hip_set_floats8_f32", self.hyper.data_ptr(), lr_t, lr_t, lr_t, clip, self.beta_1, self.beta_2,
                 self.epsilon, 0.0)

    def apply_gradients(self, grad_flat, hyper_ready=False):
        """One Keras Adam step (AdamW with config.weight_decay > 0) on this group's tensors using the flat gradient buffer;
        the clip is per tensor here whatever config.global_clipnorm says (the joint norm needs all groups: JointAdam).
        Called directly (outside aggregate_grad_and_apply) it does NOT update the weight average of config.ema_decay."""
        if not hyper_ready:
            self.set_step_hyper()
        if self.engine is not None:
            self.engine.bump_weights_version()
        if self.n_chunks == 0:
            return
        hip.call("detr_hip_sumsq_segments_f32", grad_flat.data_ptr(), self.chunk_tensor.data_ptr(),
                 self.chunk_start.data_ptr(), self.seg_end.data_ptr(), self.n_chunks, CHUNK, self.sumsq.data_ptr())
        if self.weight_decay() > 0.0:
            hip.call("detr_hip_adamw_f32", self.store.flat.data_ptr(), grad_flat.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                     self.chunk_tensor.data_ptr(), self.chunk_start.data_ptr(), self.seg_end.data_ptr(), self.tensor_group.data_ptr(),
                     self.sumsq.data_ptr(), self.hyper.data_ptr(), None, self.n_chunks, CHUNK)
            return
        hip.call("detr_hip_clip_adam_f32", self.store.flat.data_ptr(), grad_flat.data_ptr(), self.m.data_ptr(),
                 self.v.data_ptr(), self.chunk_tensor.data_ptr(), self.chunk_start.data_ptr(), self.seg_end.data_ptr(),
                 self.tensor_group.data_ptr(), self.sumsq.data_ptr(), self.hyper.data_ptr(), self.n_chunks, CHUNK)


def write_hyper16(dst, values):
    """The 16-float hyper-parameter block of the AdamW kernels (include/detr_hip.h), written stream-ordered."""
    hip.call("detr_hip_set_floats16_f32", dst.data_ptr(), byref((c_float * 16)(*[float(x) for x in values])))


def clip_mode(config):
    """"joint": config.global_clipnorm is set and replaces the per-tensor clip ("global wins"); "tensor" otherwise."""
    return "joint" if getattr(config, "global_clipnorm", None) is not None else "tensor"


def decay_active(config):
    return float(getattr(config, "weight_decay", 0.0) or 0.0) > 0.0


def trained_groups(config):
    return [n for n in GROUPS if getattr(config, f"train_{n}")]


def trained_chunk_table(tables, group_host, trained, device, cache):
    """(chunk_tensor, chunk_start, n) of the chunks of the `trained` groups, in tensor order: the table of every launch that
    covers all trained groups at once (JointAdam, WeightEMA).  Built once per set of trained groups (`cache`)."""
    key = tuple(trained)
    if key not in cache:
        gids = {GROUPS.index(n) for n in trained}
        keep = [i for i, t in enumerate(tables["chunk_tensor"].tolist()) if group_host[t] in gids]
        idx = torch.tensor(keep, dtype=torch.int64, device=device)
        cache[key] = (tables["chunk_tensor"][idx].contiguous(), tables["chunk_start"][idx].contiguous(), len(keep))
    return cache[key]


class JointAdam:
    """All trained groups in three launches: per-chunk sums of squares, a fixed-order finalize that leaves the clip factor
    c / max(G, c) in device memory, and one clip + decay + Adam launch.  The per-group step counts stay on the GroupAdam
    objects; learning rates, step sizes, decay and the trained flags travel through one 16-float device block."""

    def __init__(self, store, group_opts, config, nlayers, engine=None):
        self.store, self.opts, self.config, self.engine = store, list(group_opts), config, engine
        dev = store.device
        self.tables = store.build_tables(nlayers, CHUNK)
        self.group_host = list(self.tables["group_host"])
        self.tensor_group = torch.tensor(self.group_host, dtype=torch.int32, device=dev)
        self.seg_end = self.tables["seg_end"]
        self.sumsq = torch.zeros(max(1, self.tables["n_chunks"]), dtype=torch.float32, device=dev)
        self.hyper = torch.zeros(16, dtype=torch.float32, device=dev)
        self.scale = torch.ones(2, dtype=torch.float32, device=dev)      # [clip factor, G] of the last apply
        self._chunks = {}
        # element ranges of each group in the flat buffers (consecutive tensors of a group merged, alignment gaps included)
        names = self.tables["names"]
        self.runs = {g: [] for g in range(len(GROUPS))}
        for i, k in enumerate(names):
            o = store.offsets[k][0]
            end = store.offsets[names[i + 1]][0] if i + 1 < len(names) else store.total
            runs = self.runs[self.group_host[i]]
            if runs and runs[-1][1] == o and i > 0 and self.group_host[i - 1] == self.group_host[i]:
                runs[-1][1] = end
            else:
                runs.append([o, end])

    def _table(self, trained):
        """Chunk list of the trained groups, in tensor order (built once per set of trained groups)."""
        return trained_chunk_table(self.tables, self.group_host, trained, self.store.device, self._chunks)

    def prepare(self):
        """Builds what the next apply needs on the device (nothing is allocated inside a recorded step)."""
        self._table(trained_groups(self.config))

    def set_step_hyper(self):
        """Advances the step count of every trained group and writes this step's block to device memory."""
        cfg = self.config
        trained = trained_groups(cfg)
        lr_t, lr, flag = [0.0] * 3, [0.0] * 3, [0.0] * 3
        eps = 1e-7
        for name in trained:
            g = GROUPS.index(name)
            opt = self.opts[g]
            opt.iterations += 1
            opt.epsilon = eps = float(getattr(cfg, "adam_epsilon", opt.epsilon))
            lr[g], lr_t[g] = opt.step_sizes()
            flag[g] = 1.0
        o = self.opts[0]
        write_hyper16(self.hyper, lr_t + [float(cfg.global_clipnorm), o.beta_1, o.beta_2, eps, float(getattr(cfg, "weight_decay", 0.0) or 0.0)]
                      + lr + flag + [0.0, 0.0])

    def apply(self, grad_flat, hyper_ready=False):
        """One AdamW step of every trained group on the flat gradient buffer, clipped by their joint norm."""
        if not hyper_ready:
            self.set_step_hyper()
        if self.engine is not None:
            self.engine.bump_weights_version()
        ct, cs, n = self._table(trained_groups(self.config))
        if n == 0:
            return
        st = self.store
        hip.call("detr_hip_sumsq_segments_f32", grad_flat.data_ptr(), ct.data_ptr(), cs.data_ptr(), self.seg_end.data_ptr(), n, CHUNK,
                 self.sumsq.data_ptr())
        hip.call("detr_hip_global_clip_scale_f32", self.sumsq.data_ptr(), ct.data_ptr(), self.tensor_group.data_ptr(),
                 self.hyper.data_ptr(), n, self.scale.data_ptr())
        hip.call("detr_hip_adamw_f32", st.flat.data_ptr(), grad_flat.data_ptr(), st.adam_m.data_ptr(), st.adam_v.data_ptr(),
                 ct.data_ptr(), cs.data_ptr(), self.seg_end.data_ptr(), self.tensor_group.data_ptr(), self.sumsq.data_ptr(),
                 self.hyper.data_ptr(), self.scale.data_ptr(), n, CHUNK)

    def accumulator(self, optimizers):
        """The ONE gradient accumulator of the joint mode (each group owns its slices).  Per-group accumulators left by the
        per-tensor mode or by load_optimizer_state move into it."""
        acc = optimizers.get("_joint_gradients")
        if not isinstance(acc, torch.Tensor):
            acc = optimizers["_joint_gradients"] = torch.zeros_like(self.store.grad)
        for g, name in enumerate(GROUPS):
            own = optimizers.get(f"{name}_gradients")
            if isinstance(own, torch.Tensor) and own is not acc and own is not self.store.grad:
                for a, b in self.runs[g]:
                    acc[a:b].copy_(own[a:b])
                optimizers[f"{name}_gradients"] = acc
        return acc


def joint_optimizer(optimizers, config):
    """The JointAdam of this optimiser dict (built at the first joint step)."""
    joint = optimizers.get("_joint")
    if joint is None or joint.config is not config:
        joint = optimizers["_joint"] = JointAdam(optimizers["_store"], [optimizers[f"{n}_optimizer"] for n in GROUPS], config,
                                                 optimizers.get("_nlayers", getattr(config, "nlayers", [])), engine=optimizers.get("_engine"))
    return joint


# ---- exponential moving average of the weights ---------------------------------------------------------------------------
def ema_active(config):
    return getattr(config, "ema_decay", None) is not None


def ema_step_decay(decay, warmup, num_updates):
    """This update's decay, in double: `decay`, or with warmup min(decay, (1 + n) / (10 + n)) for n = the updates done before
    this one (tf.train.ExponentialMovingAverage(decay, num_updates=n))."""
    d = float(decay)
    if not 0.0 <= d < 1.0:
        raise ValueError(f"ema_decay must satisfy 0 <= ema_decay < 1, got {decay!r}")
    if warmup:
        d = min(d, (1.0 + num_updates) / (10.0 + num_updates))
    return d


def _in_ema_scope(store, what):
    if getattr(store, "ema_swapped", False):
        raise RuntimeError(f"{what}: not inside ema_weights(model) -- the parameter buffer holds the averaged weights there")


class WeightEMA:
    """tf.train.ExponentialMovingAverage over every trained tensor, on the device.  The shadow is `store.ema`, a flat fp32
    buffer laid out like `store.flat` and created as a copy of it; per apply step ONE launch (detr_hip_ema_f32) over the chunk
    list of all trained groups applies  t = shadow - w; t = (1 - d) * t; shadow -= t  with each operation rounded on its own.
    1 - d travels through a device block written by set_step_hyper(), which also advances `num_updates`: a captured step is
    replayed with fresh values.  Tensors of untrained groups are not visited (their shadow stays the copy it started as).
    config.ema_decay and config.ema_warmup are read at every update; ema_decay = None pauses the updates and keeps the shadow.
    The update belongs to `aggregate_grad_and_apply` (and training.GraphedTrainStep): a direct GroupAdam.apply_gradients or
    JointAdam.apply does NOT average.
    Data parallelism needs no communication: every rank applies the same update to identical parameters."""

    def __init__(self, store, config, nlayers):
        self.store, self.config, self.nlayers = store, config, list(nlayers)
        self.tables = self.group_host = self.seg_end = self.hyper = None
        self._chunks = {}
        self.last_decay = None                 # the decay of the last update (after the warmup rule)

    @property
    def num_updates(self):
        return self.store.ema_num_updates

    @num_updates.setter
    def num_updates(self, n):
        self.store.ema_num_updates = int(n)

    def prepare(self):
        """Everything the next update needs on the device: the shadow (a copy of the current weights, if there is none yet),
        the hyper block and the chunk table of the trained groups.  Called before a step is recorded; never inside one."""
        st = self.store
        if st.ema is None:
            st.ema = st.flat.clone()
            st.ema_num_updates = 0
        if self.tables is None:
            self.tables = st.build_tables(self.nlayers, CHUNK)
            self.group_host = list(self.tables["group_host"])
            self.seg_end = self.tables["seg_end"]
            self.hyper = torch.zeros(8, dtype=torch.float32, device=st.device)
        return trained_chunk_table(self.tables, self.group_host, trained_groups(self.config), st.device, self._chunks)

    def set_step_hyper(self):
        """Advances num_updates and writes this update's 1 - decay (float32 of the double difference) to device memory."""
        d = ema_step_decay(self.config.ema_decay, bool(getattr(self.config, "ema_warmup", False)), self.num_updates)
        if self.hyper is None:
            self.prepare()
        self.last_decay = d
        self.num_updates += 1
        hip.call("detr_hip_set_floats8_f32", self.hyper.data_ptr(), float(np.float32(1.0 - d)), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)

    def apply(self, hyper_ready=False):
        """One update of the shadow from the current weights (one launch; none when no trained group has a tensor)."""
        if not hyper_ready:
            self.set_step_hyper()
        ct, cs, n = self.prepare()
        if n == 0:
            return
        st = self.store
        hip.call("detr_hip_ema_f32", st.ema.data_ptr(), st.flat.data_ptr(), ct.data_ptr(), cs.data_ptr(), self.seg_end.data_ptr(),
                 self.hyper.data_ptr(), n, CHUNK)


def weight_ema(optimizers, config):
    """The WeightEMA of this optimiser dict (built when config.ema_decay is first found set, or by a state that carries one)."""
    ema = optimizers.get("_ema")
    if ema is None or ema.config is not config:
        ema = optimizers["_ema"] = WeightEMA(optimizers["_store"], config, optimizers.get("_nlayers", getattr(config, "nlayers", [])))
    return ema


class ema_weights:
    """`with ema_weights(model):` -- the model computes with the AVERAGED weights inside the scope (evaluation, save_weights).
    Entry is one detr_hip_exchange_f32 launch over [0, total) of store.flat and store.ema followed by store.on_change() (the
    frozen BN is refolded, the bf16 shadow and the evaluation graph go stale); exit does the same again.  The exchange is
    exact, so training after the scope continues bit-identically.  The evaluation graph is keyed on the weights version:
    every scope re-records it once (and the first evaluation after the scope once more).
    Inside the scope aggregate_grad_and_apply, GraphedTrainStep.__call__, optimizer_state / load_optimizer_state, load_weights
    and a nested scope raise RuntimeError.  Without a shadow: ValueError."""

    def __init__(self, model):
        self.store = model.engine.P if hasattr(model, "engine") else model

    def _swap(self):
        st = self.store
        hip.call("detr_hip_exchange_f32", st.flat.data_ptr(), st.ema.data_ptr(), st.total)
        if st.on_change is not None:
            st.on_change()

    def __enter__(self):
        st = self.store
        if getattr(st, "ema", None) is None:
            raise ValueError("ema_weights: this model has no averaged weights (config.ema_decay was never set)")
        _in_ema_scope(st, "ema_weights (nested)")
        self._swap()
        st.ema_swapped = True
        return self

    def __exit__(self, *exc):
        self.store.ema_swapped = False
        self._swap()
        return False


def setup_optimizers(model, config):
    """optimizers.py:67-107: returns the dict the training loop threads through."""
    store = model.engine.P
    out = {}
    for gid, name in enumerate(GROUPS):
        # resolved at every step: `config.backbone_lr = 1e-4` (rebinding) works like `.assign(1e-4)` on the cell
        getter = (lambda n=name: float(getattr(config, f"{n}_lr")))
        opt = GroupAdam(store, gid, getter, config.gradient_norm_clipping, config.nlayers, engine=model.engine, config=config)
        out[f"{name}_optimizer"] = opt
        out[f"{name}_variables"] = [store.views[n] for n in opt.names]
    out["_store"] = store
    out["_engine"] = model.engine
    out["_nlayers"] = list(config.nlayers)
    if ema_active(config):              # the shadow starts as a copy of the weights the optimisers were set up on
        weight_ema(out, config).prepare()
    return out


class GroupGradients:
    """Handle on one group's slice of the flat gradient buffer (what the reference's
    gradient_steps[name]["gradients"] list is)."""

    def __init__(self, store, opt):
        self.store, self.opt = store, opt

    def tensors(self):
        return [self.store.gviews[n] for n in self.opt.names]


def gather_gradient(model, optimizers, total_loss, m_outputs, config, log, loss_scale=1.0):
    """optimizers.py:110-133.  The reference calls tape.gradient here; this runs the set-loss
    gradient kernel and the engine's backward into the (zeroed) flat gradient buffer."""
    eng = model.engine
    eng.zero_grad()
    d_logits, d_boxes = m_outputs.set_loss.grad(loss_scale)
    need_backbone = bool(getattr(config, "train_backbone", True))
    dp = model.dp
    eng.backward(d_logits, d_boxes, backbone=need_backbone, on_bucket=(dp.on_bucket if dp is not None else None))
    if dp is not None:
        dp.finish()
    steps = {}
    for name in GROUPS:
        steps[name] = {"gradients": GroupGradients(eng.P, optimizers[f"{name}_optimizer"])}
        log[f"{name}_lr"] = optimizers[f"{name}_optimizer"].learning_rate()
    return steps


def aggregate_grad_and_apply(name, optimizers, gradients, step, config):
    """optimizers.py:137-163: zero the accumulator at step % agg == 0, add this step's gradient,
    apply at (step+1) % agg == 0; skipped when config.train_<name> is falsy.
    With config.global_clipnorm set, a call only accumulates; the call of the LAST trained group of GROUPS at an apply
    step updates all trained groups at once (JointAdam), clipped by the norm of their whole (accumulated) gradient.
    With config.ema_decay set, the call of the last trained group at an apply step ends with the ONE launch that averages
    the weights of all trained groups into store.ema (WeightEMA): in both clip modes, never at a step that only accumulates."""
    gradient_aggregate = None
    if config.target_batch is not None:
        gradient_aggregate = int(config.target_batch // config.batch_size)
    if not getattr(config, f"train_{name}"):
        return
    store = optimizers["_store"]
    _in_ema_scope(store, "aggregate_grad_and_apply")
    opt = optimizers[f"{name}_optimizer"]
    gname = f"{name}_gradients"
    if ema_active(config):              # (the shadow starts as a copy of the weights BEFORE the first averaged update)
        weight_ema(optimizers, config).prepare()
    if clip_mode(config) == "joint":
        joint = joint_optimizer(optimizers, config)
        last = name == trained_groups(config)[-1]
        if gradient_aggregate is None or gradient_aggregate <= 1:
            optimizers[gname] = store.grad
            if last:
                joint.apply(store.grad)
                applied(name, optimizers, config)
            return
        acc = optimizers[gname] = joint.accumulator(optimizers)
        for a, b in joint.runs[opt.group_id]:           # only this group's slices of the shared accumulator
            if step % gradient_aggregate == 0:
                hip.call("detr_hip_memset_zero", acc.data_ptr() + 4 * a, 4 * (b - a))
            hip.call("detr_hip_axpy_f32", acc.data_ptr() + 4 * a, store.grad.data_ptr() + 4 * a, c_float(1.0), b - a)
        if last and (step + 1) % gradient_aggregate == 0:
            joint.apply(acc)
            applied(name, optimizers, config)
        return
    if gradient_aggregate is None or gradient_aggregate <= 1:
        optimizers[gname] = store.grad
        opt.apply_gradients(store.grad)
        applied(name, optimizers, config)
        return
    acc = optimizers.get(gname)
    if not isinstance(acc, torch.Tensor) or acc is store.grad or acc is optimizers.get("_joint_gradients"):
        acc = optimizers[gname] = torch.zeros_like(store.grad)
    elif step % gradient_aggregate == 0:
        hip.zero_(acc)
    # only this group's tensors are accumulated (the others are untouched slices of the same buffer)
    for n in opt.names:
        o, cnt = store.offsets[n]
        hip.call("detr_hip_axpy_f32", acc.data_ptr() + 4 * o, store.grad.data_ptr() + 4 * o, c_float(1.0), cnt)
    if (step + 1) % gradient_aggregate == 0:
        opt.apply_gradients(acc)
        applied(name, optimizers, config)


def applied(name, optimizers, config):
    """After the update of group `name` at an apply step: the derived weight copies are stale, and behind the LAST trained
    group the weight average takes its one update."""
    model_dirty(optimizers)
    if ema_active(config) and name == trained_groups(config)[-1]:
        weight_ema(optimizers, config).apply()


def model_dirty(optimizers):
    eng = optimizers.get("_engine")
    if eng is not None:
        eng.bump_weights_version()


# ---- resumable state ---------------------------------------------------------------------------------------------------
def optimizer_state(optimizers):
    """Everything a stopped run needs besides the weights, as NumPy arrays: the Adam moments by parameter name
    (`m/<name>`, `v/<name>`), each group's step count (`iterations/<group>`), the gradient accumulators that exist
    (`accum/<name>`, target_batch > batch_size) and the engine's dropout step counter (`engine/step_no`).  When the weight
    average exists (config.ema_decay was set: store.ema), also `ema/<name>` per parameter and `ema/num_updates`; without it
    the keys are exactly the ones above.  Under data parallelism every rank holds the same average: rank 0's state suffices."""
    store = optimizers["_store"]
    _in_ema_scope(store, "optimizer_state")
    m, v = store.adam_m.cpu().numpy(), store.adam_v.cpu().numpy()
    out = {}
    for k, (o, n) in store.offsets.items():
        out[f"m/{k}"] = m[o:o + n].reshape(store.shapes[k]).copy()
        out[f"v/{k}"] = v[o:o + n].reshape(store.shapes[k]).copy()
    for name in GROUPS:
        opt = optimizers[f"{name}_optimizer"]
        out[f"iterations/{name}"] = np.asarray(opt.iterations, dtype=np.int64)
        acc = optimizers.get(f"{name}_gradients")
        if isinstance(acc, torch.Tensor) and acc is not store.grad:
            host = acc.cpu().numpy()
            for k in opt.names:
                o, n = store.offsets[k]
                out[f"accum/{k}"] = host[o:o + n].reshape(store.shapes[k]).copy()
    eng = optimizers.get("_engine")
    if eng is not None:
        out["engine/step_no"] = np.asarray(eng._step_no, dtype=np.int64)
    if getattr(store, "ema", None) is not None:
        e = store.ema.cpu().numpy()
        for k, (o, n) in store.offsets.items():
            out[f"ema/{k}"] = e[o:o + n].reshape(store.shapes[k]).copy()
        out["ema/num_updates"] = np.asarray(store.ema_num_updates, dtype=np.int64)
    return out


def load_optimizer_state(optimizers, state):
    """Restores what optimizer_state returned.  Every name and shape is checked BEFORE the first copy: a state of another
    model raises ValueError and leaves the optimisers as they were.  The moments are overwritten in place and the step
    counts / the dropout counter reach the device with the next step's hyper-parameter writes, so a recorded training
    graph stays valid.
    The weight average: `ema/*` keys restore store.ema in place (and create it when there is none) with `ema/num_updates`; a
    state WITHOUT them loaded where a shadow exists resets the shadow to the current weights and num_updates to 0."""
    store = optimizers["_store"]
    _in_ema_scope(store, "load_optimizer_state")
    problems = []
    known = set(store.shapes)
    for key in state:
        kind, _, k = key.partition("/")
        if kind in ("m", "v", "accum") and k not in known:
            problems.append(f"{key}: no such parameter")
        if kind == "ema" and k != "num_updates" and k not in known:
            problems.append(f"{key}: no such parameter")
    has_ema = any(key.startswith("ema/") for key in state)
    kinds = ("m", "v", "ema") if has_ema else ("m", "v")
    staged = {kind: np.zeros(store.total, np.float32) for kind in kinds}
    if has_ema and "ema/num_updates" not in state:
        problems.append("ema/num_updates: missing")
    for kind in kinds:
        for k, (o, n) in store.offsets.items():
            if f"{kind}/{k}" not in state:
                problems.append(f"{kind}/{k}: missing")
                continue
            a = np.asarray(state[f"{kind}/{k}"])
            if tuple(a.shape) != tuple(store.shapes[k]):
                problems.append(f"{kind}/{k}: shape {tuple(a.shape)} != {tuple(store.shapes[k])}")
                continue
            staged[kind][o:o + n] = a.astype(np.float32, copy=False).ravel()
    accum = {}
    for name in GROUPS:
        if f"iterations/{name}" not in state:
            problems.append(f"iterations/{name}: missing")
        names = optimizers[f"{name}_optimizer"].names
        have = [k for k in names if f"accum/{k}" in state]
        if not have:
            continue
        host = np.zeros(store.total, np.float32)
        for k in names:
            if f"accum/{k}" not in state:
                problems.append(f"accum/{k}: missing (the accumulator of group {name} is incomplete)")
                continue
            a = np.asarray(state[f"accum/{k}"])
            if tuple(a.shape) != tuple(store.shapes[k]):
                problems.append(f"accum/{k}: shape {tuple(a.shape)} != {tuple(store.shapes[k])}")
                continue
            o, n = store.offsets[k]
            host[o:o + n] = a.astype(np.float32, copy=False).ravel()
        accum[name] = host
    if problems:
        raise ValueError("optimizer state does not fit this model: " + "; ".join(problems[:8])
                         + (f"; ... ({len(problems)} in all)" if len(problems) > 8 else ""))
    store.adam_m.copy_(torch.from_numpy(staged["m"]))
    store.adam_v.copy_(torch.from_numpy(staged["v"]))
    if has_ema:
        if store.ema is None:
            store.ema = torch.empty_like(store.flat)
        store.ema.copy_(torch.from_numpy(staged["ema"]))
        store.ema_num_updates = int(np.asarray(state["ema/num_updates"]))
    elif getattr(store, "ema", None) is not None:
        store.reset_ema()
    optimizers.pop("_joint_gradients", None)
    for name in GROUPS:
        optimizers[f"{name}_optimizer"].iterations = int(np.asarray(state[f"iterations/{name}"]))
        optimizers.pop(f"{name}_gradients", None)
        if name in accum:           # one accumulator per group; the joint mode gathers them into its shared one
            optimizers[f"{name}_gradients"] = torch.from_numpy(accum[name]).to(store.device)
    eng = optimizers.get("_engine")
    if eng is not None and "engine/step_no" in state:
        eng._step_no = int(np.asarray(state["engine/step_no"]))


def save_optimizer_state(optimizers, path):
    np.savez(path, **optimizer_state(optimizers))


def load_optimizer_state_file(optimizers, path):
    with np.load(path) as z:
        load_optimizer_state(optimizers, {k: z[k] for k in z.files})
