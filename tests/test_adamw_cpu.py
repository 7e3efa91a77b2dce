"""AdamW decay, model-wide norm clipping and the resumable optimiser state, host side: tests/adamw_ref.py pinned against
torch.optim.AdamW + clip_grad_norm_, the new configuration surface, the launch sequences of detr_tf/optimizers.py (the
binding's `call` replaced by a recorder, parameter store on the CPU: no GPU needed) and the state round trip."""
import os
import re
import types

import numpy as np
import pytest
import torch

import adamw_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------
# the reference arithmetic against an independent implementation
# ------------------------------------------------------------------------------------------
def test_adamw_ref_matches_torch_adamw_with_clip_grad_norm():
    """float64 on both sides, eps = 0 (where the Keras placement of epsilon, sqrt(v) + eps under the bias-corrected step size,
    and torch's coincide), gradients non-zero everywhere.  5 tensors in 2 groups with different lr, c = 0.1: three steps with
    G >= 1 (torch scales by c / (G + 1e-6), this by c / max(G, c): <= 1e-6 relative apart) and one with G < c (no clip on
    either side).  Bound: 1e-5 of the largest parameter change of the tensor in that step."""
    rng = np.random.default_rng(11)
    shapes = [(7, 5), (3,), (64,), (2, 3, 4), (33,)]
    groups = {0: "a", 1: "b", 2: "a", 3: "b", 4: "b"}
    lrs = {"a": 1e-2, "b": 3e-3}
    wd, c = 1e-2, 0.1
    p0 = [rng.normal(size=s) for s in shapes]
    tp = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in p0]
    topt = torch.optim.AdamW([{"params": [tp[i] for i in range(5) if groups[i] == g], "lr": lrs[g]} for g in ("a", "b")],
                             betas=(0.9, 0.999), eps=0.0, weight_decay=wd)
    ref = A.AdamW(lrs, groups, weight_decay=wd, global_clipnorm=c, eps=0.0)
    params = {i: p.copy() for i, p in enumerate(p0)}
    for step in range(4):
        grads = {}
        for i, s in enumerate(shapes):
            z = rng.normal(size=s)
            grads[i] = np.sign(z) * (np.abs(z) + 0.1)
        G = A.global_norm(grads.values())
        target = [3.0, 40.0, 1.0, 0.05][step]
        grads = {i: g * (target / G) for i, g in grads.items()}
        assert (step < 3) == (A.global_norm(grads.values()) >= 1.0 - 1e-12)
        before = {i: params[i].copy() for i in params}
        s = ref.step(grads, params)
        assert (s == 1.0) == (step == 3)
        for i in range(5):
            tp[i].grad = torch.tensor(grads[i], dtype=torch.float64)
        torch.nn.utils.clip_grad_norm_(tp, c)
        topt.step()
        for i in range(5):
            d_ref = params[i] - before[i]
            d_torch = tp[i].detach().numpy() - before[i]
            err, scale = float(np.abs(d_ref - d_torch).max()), float(np.abs(d_torch).max())
            assert err <= 1e-5 * scale, (step, i, err, scale)
    assert ref.t == {"a": 4, "b": 4}


def test_adamw_ref_per_tensor_clip_and_untrained_tensors():
    """clipnorm mode is tf.clip_by_norm per tensor; a tensor absent from `grads` neither moves nor counts in G, and its
    group's step count only advances when one of its tensors is trained."""
    p = {0: np.ones(4), 1: np.ones(3)}
    ref = A.AdamW({"a": 0.1, "b": 0.1}, {0: "a", 1: "b"}, weight_decay=0.0, global_clipnorm=1.0)
    s = ref.step({0: np.full(4, 2.0)}, p)
    assert s == pytest.approx(0.25) and ref.last_norm == pytest.approx(4.0) and ref.t == {"a": 1, "b": 0}
    assert np.array_equal(p[1], np.ones(3)) and np.allclose(p[0], 0.9, atol=1e-6)       # first Adam step: -lr * sign(g)
    q = {0: np.ones(4)}
    A.AdamW({"a": 0.1}, {0: "a"}, weight_decay=0.5, clipnorm=0.1).step({0: np.full(4, 1e-3)}, q)
    # no clip (||g|| = 2e-3 < 0.1); decay by lr * wd, then lr * g / (g + eps / sqrt(1 - b2)) at t = 1
    assert np.allclose(q[0], 1.0 - 0.1 * 0.5 - 0.1 * 1e-3 / (1e-3 + 1e-7 / 0.001 ** 0.5), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------
def test_config_defaults_and_flags():
    from detr_tf.optimizers import clip_mode, decay_active
    from detr_tf.training_config import TrainingConfig, training_config_parser
    cfg = TrainingConfig()
    assert cfg.weight_decay == 0.0 and cfg.global_clipnorm is None and cfg.adam_epsilon == 1e-7
    assert cfg.gradient_norm_clipping == 0.1
    assert clip_mode(cfg) == "tensor" and not decay_active(cfg)
    args = training_config_parser().parse_args([])
    assert args.weight_decay == 0.0 and args.global_clipnorm is None and args.adam_epsilon == 1e-7
    cfg.update_from_args(training_config_parser().parse_args(["--weight_decay", "1e-4", "--global_clipnorm", "0.1",
                                                              "--adam_epsilon", "1e-8"]))
    assert cfg.weight_decay == 1e-4 and cfg.global_clipnorm == 0.1 and cfg.adam_epsilon == 1e-8
    # "global wins": gradient_norm_clipping keeps its non-None default and is ignored
    assert cfg.gradient_norm_clipping == 0.1 and clip_mode(cfg) == "joint" and decay_active(cfg)


def test_c_abi_declares_the_adamw_entry_points():
    from detr_tf import _hip
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _hip.load()
    for name in ("detr_hip_set_floats16_f32", "detr_hip_global_clip_scale_f32", "detr_hip_adamw_f32"):
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.detr_hip_abi_version() == _hip.ABI_VERSION == 9          # appended entry points: the version stays
    # null operands are rejected on the host, before any launch
    assert lib.detr_hip_adamw_f32(None, None, None, None, None, None, None, None, None, None, None, 1, 64, None) != 0
    assert lib.detr_hip_global_clip_scale_f32(None, None, None, None, 1, None, None) != 0
    assert lib.detr_hip_set_floats16_f32(None, None, None) != 0


# ------------------------------------------------------------------------------------------
# the Python layer on a CPU parameter store, launches recorded instead of run
# ------------------------------------------------------------------------------------------
@pytest.fixture()
def rig(monkeypatch):
    from detr_tf import optimizers as O
    from detr_tf.params import ParamStore
    from detr_tf.training_config import TrainingConfig
    store = ParamStore("cpu", blocks=(1, 1, 1, 1), num_enc=1, num_dec=1, num_queries=10)
    engine = types.SimpleNamespace(P=store, _step_no=0, bumps=0)
    engine.bump_weights_version = lambda: setattr(engine, "bumps", engine.bumps + 1)
    cfg = TrainingConfig()
    cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
    cfg.target_batch, cfg.batch_size = None, 2
    calls = []
    monkeypatch.setattr(O.hip, "call", lambda name, *a: calls.append((name, a)))
    opt = O.setup_optimizers(types.SimpleNamespace(engine=engine), cfg)
    return types.SimpleNamespace(O=O, store=store, engine=engine, cfg=cfg, opt=opt, calls=calls)


def _names(calls):
    return [c[0] for c in calls]


def _loop(rig, step=0):
    del rig.calls[:]
    for name in rig.O.GROUPS:
        rig.O.aggregate_grad_and_apply(name, rig.opt, None, step, rig.cfg)
    return _names(rig.calls)


def test_default_launch_sequence_is_unchanged(rig):
    """Defaults: per group one hyper-parameter write and the two Adam(clipnorm) launches (no head layers registered: the
    nlayers group is empty and launches nothing)."""
    per_group = ["detr_hip_set_floats8_f32", "detr_hip_sumsq_segments_f32", "detr_hip_clip_adam_f32"]
    assert _loop(rig) == per_group * 2 + ["detr_hip_set_floats8_f32"]
    assert [rig.opt[f"{n}_optimizer"].iterations for n in rig.O.GROUPS] == [1, 1, 1]
    assert "_joint" not in rig.opt


def test_weight_decay_alone_keeps_the_per_tensor_clip(rig):
    rig.cfg.weight_decay = 1e-4
    per_group = ["detr_hip_set_floats16_f32", "detr_hip_sumsq_segments_f32", "detr_hip_adamw_f32"]
    assert _loop(rig) == per_group * 2 + ["detr_hip_set_floats16_f32"]
    name, args = rig.calls[2]
    assert args[10] is None                             # no joint scale: the kernel clips per tensor
    block = list(rig.calls[0][1][1]._obj)               # the backbone group's 16 floats
    lr = float(rig.cfg.backbone_lr)
    assert block[3] == pytest.approx(0.1) and block[7] == pytest.approx(1e-4) and block[8] == pytest.approx(lr)
    assert block[0] == pytest.approx(lr * (1 - 0.999) ** 0.5 / (1 - 0.9)) and block[11:14] == [1.0, 1.0, 1.0]
    rig.cfg.weight_decay = 0.0                          # read at every step: back to the Adam(clipnorm) launches
    assert "detr_hip_clip_adam_f32" in _loop(rig, 1) and "detr_hip_adamw_f32" not in _names(rig.calls)


def test_global_clipnorm_wins_and_defers_the_update_to_the_last_trained_group(rig):
    O, cfg = rig.O, rig.cfg
    cfg.global_clipnorm, cfg.weight_decay = 0.1, 1e-4
    assert cfg.gradient_norm_clipping == 0.1            # still set: ignored ("global wins")
    joint_seq = ["detr_hip_set_floats16_f32", "detr_hip_sumsq_segments_f32", "detr_hip_global_clip_scale_f32", "detr_hip_adamw_f32"]
    del rig.calls[:]
    O.aggregate_grad_and_apply("backbone", rig.opt, None, 0, cfg)
    O.aggregate_grad_and_apply("transformers", rig.opt, None, 0, cfg)
    assert rig.calls == [] and rig.engine.bumps == 0    # nothing may move before every trained group's gradient is there
    O.aggregate_grad_and_apply("nlayers", rig.opt, None, 0, cfg)
    assert _names(rig.calls) == joint_seq
    assert [rig.opt[f"{n}_optimizer"].iterations for n in O.GROUPS] == [1, 1, 1]
    joint = rig.opt["_joint"]
    block = list(rig.calls[0][1][1]._obj)
    assert block[3] == pytest.approx(0.1) and block[7] == pytest.approx(1e-4) and block[11:14] == [1.0, 1.0, 1.0]
    assert block[8:11] == [pytest.approx(float(getattr(cfg, f"{n}_lr"))) for n in O.GROUPS]
    assert rig.calls[3][1][10] == joint.scale.data_ptr()
    n_all = rig.calls[1][1][4]
    assert n_all == rig.store.build_tables([], O.CHUNK)["n_chunks"]
    # a frozen group: not counted, not stepped, and the LAST TRAINED group applies
    cfg.train_nlayers = cfg.train_backbone = False
    assert _loop(rig, 1) == joint_seq
    assert [rig.opt[f"{n}_optimizer"].iterations for n in O.GROUPS] == [1, 2, 1]
    block = list(rig.calls[0][1][1]._obj)
    assert block[11:14] == [0.0, 1.0, 0.0] and block[0] == 0.0 and block[1] > 0.0
    assert 0 < rig.calls[1][1][4] < n_all               # the chunk list holds the trained group only


def test_joint_accumulation_shares_one_accumulator_and_zeroes_only_own_slices(rig):
    O, cfg, st = rig.O, rig.cfg, rig.store
    cfg.global_clipnorm, cfg.target_batch = 0.1, 4
    seq0 = _loop(rig, 0)
    assert "detr_hip_adamw_f32" not in seq0 and "detr_hip_set_floats16_f32" not in seq0
    acc = rig.opt["_joint_gradients"]
    assert all(rig.opt[f"{n}_gradients"] is acc for n in O.GROUPS) and acc.numel() == st.total
    zeroed = sorted((c[1][0] - acc.data_ptr()) // 4 for c in rig.calls if c[0] == "detr_hip_memset_zero")
    runs = rig.opt["_joint"].runs
    assert zeroed == sorted(a for g in runs for a, _ in runs[g])
    # the runs of the three groups tile the flat buffer without overlap
    flat = sorted((a, b) for g in runs for a, b in runs[g])
    assert flat[0][0] == 0 and flat[-1][1] == st.total and all(flat[i][1] == flat[i + 1][0] for i in range(len(flat) - 1))
    for g, name in enumerate(O.GROUPS):
        for k in rig.opt[f"{name}_optimizer"].names:
            o, n = st.offsets[k]
            assert any(a <= o and o + n <= b for a, b in runs[g]), k
    seq1 = _loop(rig, 1)
    assert "detr_hip_memset_zero" not in seq1
    assert seq1[-4:] == ["detr_hip_set_floats16_f32", "detr_hip_sumsq_segments_f32", "detr_hip_global_clip_scale_f32", "detr_hip_adamw_f32"]
    assert rig.calls[-1][1][1] == acc.data_ptr()         # the update reads the accumulated gradient
    assert rig.opt["backbone_optimizer"].iterations == 1


# ------------------------------------------------------------------------------------------
# resumable state
# ------------------------------------------------------------------------------------------
def test_optimizer_state_round_trip_and_mismatch(rig, tmp_path):
    O, st = rig.O, rig.store
    gen = torch.Generator().manual_seed(3)
    st.adam_m.copy_(torch.randn(st.total, generator=gen))
    st.adam_v.copy_(torch.rand(st.total, generator=gen))
    for i, n in enumerate(O.GROUPS):
        rig.opt[f"{n}_optimizer"].iterations = 40 + i
    rig.engine._step_no = 123
    acc = torch.randn(st.total, generator=gen)
    rig.opt["transformers_gradients"] = acc               # a pending accumulator of one group
    rig.opt["backbone_gradients"] = st.grad               # (no accumulation: the live gradient buffer is not state)
    state = O.optimizer_state(rig.opt)
    assert all(isinstance(v, np.ndarray) for v in state.values())
    k0 = "transformer/decoder/layer_0/linear1/kernel"
    assert state[f"m/{k0}"].shape == st.shapes[k0] and int(state["iterations/nlayers"]) == 42 and int(state["engine/step_no"]) == 123
    assert f"accum/{k0}" in state and "accum/backbone/conv1/kernel" not in state
    path = os.path.join(tmp_path, "opt.npz")
    O.save_optimizer_state(rig.opt, path)

    m0, v0 = st.adam_m.clone(), st.adam_v.clone()
    valid = torch.zeros(st.total, dtype=torch.bool)       # the alignment gaps between tensors are not state
    for o, n in st.offsets.values():
        valid[o:o + n] = True

    def wipe():
        st.adam_m.zero_(), st.adam_v.zero_()
        for n in O.GROUPS:
            rig.opt[f"{n}_optimizer"].iterations = 0
            rig.opt.pop(f"{n}_gradients", None)
        rig.engine._step_no = 0

    for load in (lambda: O.load_optimizer_state(rig.opt, state), lambda: O.load_optimizer_state_file(rig.opt, path)):
        wipe()
        load()
        assert torch.equal(st.adam_m[valid], m0[valid]) and torch.equal(st.adam_v[valid], v0[valid])
        assert [rig.opt[f"{n}_optimizer"].iterations for n in O.GROUPS] == [40, 41, 42] and rig.engine._step_no == 123
        got = rig.opt["transformers_gradients"]
        for k in rig.opt["transformers_optimizer"].names:
            o, n = st.offsets[k]
            assert torch.equal(got[o:o + n], acc[o:o + n])
        assert "backbone_gradients" not in rig.opt and "_joint_gradients" not in rig.opt

    # a mismatch raises before anything is written
    wipe()
    bad_shape = dict(state)
    bad_shape[f"v/{k0}"] = np.zeros((3, 3), np.float32)
    renamed = {(k.replace("linear1", "linear9") if k.startswith("m/") else k): v for k, v in state.items()}
    missing_it = {k: v for k, v in state.items() if k != "iterations/backbone"}
    partial_acc = {k: v for k, v in state.items() if k != f"accum/{k0}"}
    for bad, word in ((bad_shape, "shape"), (renamed, "no such parameter"), (missing_it, "iterations/backbone"), (partial_acc, "incomplete")):
        with pytest.raises(ValueError, match=word):
            O.load_optimizer_state(rig.opt, bad)
        assert not st.adam_m.any() and not st.adam_v.any() and rig.engine._step_no == 0
        assert [rig.opt[f"{n}_optimizer"].iterations for n in O.GROUPS] == [0, 0, 0] and "transformers_gradients" not in rig.opt


def test_loaded_group_accumulators_move_into_the_joint_one(rig):
    """A state saved in the middle of an accumulation window is loaded as one accumulator per group; the joint mode gathers
    them into its shared buffer before it adds to it."""
    O, st = rig.O, rig.store
    gen = torch.Generator().manual_seed(5)
    accs = {n: torch.randn(st.total, generator=gen) for n in O.GROUPS}
    for n in O.GROUPS:
        rig.opt[f"{n}_gradients"] = accs[n]
    state = O.optimizer_state(rig.opt)
    O.load_optimizer_state(rig.opt, state)
    rig.cfg.global_clipnorm, rig.cfg.target_batch = 0.1, 4
    _loop(rig, 1)
    shared = rig.opt["_joint_gradients"]
    for n in O.GROUPS:
        assert rig.opt[f"{n}_gradients"] is shared
        for k in rig.opt[f"{n}_optimizer"].names:
            o, cnt = st.offsets[k]
            assert torch.equal(shared[o:o + cnt], accs[n][o:o + cnt]), k
