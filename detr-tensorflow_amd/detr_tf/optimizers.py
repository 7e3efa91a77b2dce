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
    gradient accumulators and the engine's dropout step counter.
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
        the clip is per tensor here whatever config.global_clipnorm says (the joint norm needs all groups: JointAdam)."""
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
        key = tuple(trained)
        if key not in self._chunks:
            gids = {GROUPS.index(n) for n in trained}
            keep = [i for i, t in enumerate(self.tables["chunk_tensor"].tolist()) if self.group_host[t] in gids]
            idx = torch.tensor(keep, dtype=torch.int64, device=self.store.device)
            self._chunks[key] = (self.tables["chunk_tensor"][idx].contiguous(), self.tables["chunk_start"][idx].contiguous(), len(keep))
        return self._chunks[key]

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
    step updates all trained groups at once (JointAdam), clipped by the norm of their whole (accumulated) gradient."""
    gradient_aggregate = None
    if config.target_batch is not None:
        gradient_aggregate = int(config.target_batch // config.batch_size)
    if not getattr(config, f"train_{name}"):
        return
    store = optimizers["_store"]
    opt = optimizers[f"{name}_optimizer"]
    gname = f"{name}_gradients"
    if clip_mode(config) == "joint":
        joint = joint_optimizer(optimizers, config)
        last = name == trained_groups(config)[-1]
        if gradient_aggregate is None or gradient_aggregate <= 1:
            optimizers[gname] = store.grad
            if last:
                joint.apply(store.grad)
                model_dirty(optimizers)
            return
        acc = optimizers[gname] = joint.accumulator(optimizers)
        for a, b in joint.runs[opt.group_id]:           # only this group's slices of the shared accumulator
            if step % gradient_aggregate == 0:
                hip.call("detr_hip_memset_zero", acc.data_ptr() + 4 * a, 4 * (b - a))
            hip.call("detr_hip_axpy_f32", acc.data_ptr() + 4 * a, store.grad.data_ptr() + 4 * a, c_float(1.0), b - a)
        if last and (step + 1) % gradient_aggregate == 0:
            joint.apply(acc)
            model_dirty(optimizers)
        return
    if gradient_aggregate is None or gradient_aggregate <= 1:
        optimizers[gname] = store.grad
        opt.apply_gradients(store.grad)
        model_dirty(optimizers)
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
        model_dirty(optimizers)


def model_dirty(optimizers):
    eng = optimizers.get("_engine")
    if eng is not None:
        eng.bump_weights_version()


# ---- resumable state ---------------------------------------------------------------------------------------------------
def optimizer_state(optimizers):
    """Everything a stopped run needs besides the weights, as NumPy arrays: the Adam moments by parameter name
    (`m/<name>`, `v/<name>`), each group's step count (`iterations/<group>`), the gradient accumulators that exist
    (`accum/<name>`, target_batch > batch_size) and the engine's dropout step counter (`engine/step_no`)."""
    store = optimizers["_store"]
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
    return out


def load_optimizer_state(optimizers, state):
    """Restores what optimizer_state returned.  Every name and shape is checked BEFORE the first copy: a state of another
    model raises ValueError and leaves the optimisers as they were.  The moments are overwritten in place and the step
    counts / the dropout counter reach the device with the next step's hyper-parameter writes, so a recorded training
    graph stays valid."""
    store = optimizers["_store"]
    problems = []
    known = set(store.shapes)
    for key in state:
        kind, _, k = key.partition("/")
        if kind in ("m", "v", "accum") and k not in known:
            problems.append(f"{key}: no such parameter")
    staged = {"m": np.zeros(store.total, np.float32), "v": np.zeros(store.total, np.float32)}
    for kind in ("m", "v"):
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
