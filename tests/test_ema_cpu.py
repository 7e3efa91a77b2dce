"""CPU tests of the weight average (config.ema_decay): the reference arithmetic of tests/ema_ref.py against its closed form,
the decay rule, the configuration, the two C entry points' declarations and host-side argument checks, and the Python layer
on a CPU parameter store with the launches recorded instead of run (the rig of test_adamw_cpu)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ema_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ema_ref_equals_the_closed_form():
    """Five updates in float32 against s = d s + (1 - d) p in float64.  With M = max(|s|, |p|), one update rounds the
    difference (|.| <= 2M: 2 * 2^-24 M), the product (<= 2M: 2 * 2^-24 M) and the result (<= M: 2^-24 M), and float32(1 - d)
    is off by at most 2^-24 relative, times |s - p| <= 2M: below 6 * 2^-24 M per update in all; an earlier error is carried
    with the factor d <= 1."""
    rng = np.random.default_rng(0)
    s0 = rng.normal(size=4096).astype(np.float32)
    ps = [rng.normal(size=4096).astype(np.float32) for _ in range(5)]
    decays = [0.0, 0.5, 0.9, 0.9998, 0.99]
    s = s0
    for p, d in zip(ps, decays):
        s = E.update(s, p, E.omd_of(d))
    want = E.closed_form(s0, ps, decays)
    big = max(float(np.abs(a).max()) for a in [s0] + ps)
    err = float(np.abs(s.astype(np.float64) - want).max())
    assert 0.0 < err <= 5 * 6 * 2.0 ** -24 * big, (err, big)
    # omd = 0: unchanged exactly
    assert np.array_equal(E.update(s0, ps[0], np.float32(0.0)), s0)


def test_warmup_sequence():
    from detr_tf.optimizers import ema_step_decay
    want = [0.1, 2 / 11, 3 / 12, 4 / 13]
    for n, w in enumerate(want):
        assert E.step_decay(0.9998, True, n) == ema_step_decay(0.9998, True, n) == (1.0 + n) / (10.0 + n)
        assert abs(E.step_decay(0.9998, True, n) - w) < 1e-15
    assert E.step_decay(0.2, True, 0) == 0.1 and E.step_decay(0.2, True, 2) == 0.2 == ema_step_decay(0.2, True, 2)      # capped
    assert E.step_decay(0.9998, True, 10 ** 6) == 0.9998 and E.step_decay(0.9, False, 0) == 0.9 == ema_step_decay(0.9, False, 0)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ema_step_decay(bad, False, 0)
    assert float(E.omd_of(0.9998)) == float(np.float32(1.0 - 0.9998))


def test_config_defaults_and_flags():
    from detr_tf.optimizers import ema_active
    from detr_tf.training_config import TrainingConfig, training_config_parser
    cfg = TrainingConfig()
    assert cfg.ema_decay is None and cfg.ema_warmup is False and not ema_active(cfg)
    args = training_config_parser().parse_args([])
    assert args.ema_decay is None and args.ema_warmup is False
    cfg.update_from_args(training_config_parser().parse_args(["--ema_decay", "0.9998", "--ema_warmup"]))
    assert cfg.ema_decay == 0.9998 and cfg.ema_warmup is True and ema_active(cfg)


def test_c_abi_declares_the_ema_entry_points():
    from detr_tf import _hip
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    assert "tf.train.ExponentialMovingAverage" in hdr
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _hip.load()
    for name in ("detr_hip_ema_f32", "detr_hip_exchange_f32"):
        assert name in declared and name in _hip._SIGNATURES and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.detr_hip_abi_version() == _hip.ABI_VERSION == 9          # appended entry points: the version stays
    # rejected on the host, before any launch (the pointers below are host memory: a launch would not survive them)
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    assert lib.detr_hip_ema_f32(None, None, None, None, None, None, 1, 64, None) != 0
    assert lib.detr_hip_ema_f32(a, a + 128, a, a, a, None, 1, 64, None) != 0          # null hyper
    assert lib.detr_hip_ema_f32(a, a + 128, a, a, a, a, 0, 64, None) != 0             # bad chunking
    assert lib.detr_hip_ema_f32(a, a + 128, a, a, a, a, 1, 0, None) != 0
    assert lib.detr_hip_ema_f32(a, a, a, a, a, a, 1, 64, None) != 0                   # shadow == param
    assert lib.detr_hip_exchange_f32(None, None, 4, None) != 0
    assert lib.detr_hip_exchange_f32(a, None, 4, None) != 0
    assert lib.detr_hip_exchange_f32(a, a, 4, None) != 0                              # a == b
    assert lib.detr_hip_exchange_f32(a, a + 8, 4, None) != 0                          # overlapping ranges
    assert lib.detr_hip_exchange_f32(a + 8, a, 4, None) != 0
    assert lib.detr_hip_exchange_f32(a, a + 128, 0, None) != 0
    assert b"exchange" in lib.detr_hip_last_error()


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


def _loop(rig, step=0):
    del rig.calls[:]
    for name in rig.O.GROUPS:
        rig.O.aggregate_grad_and_apply(name, rig.opt, None, step, rig.cfg)
    return [c[0] for c in rig.calls]


PER_GROUP = ["detr_hip_set_floats8_f32", "detr_hip_sumsq_segments_f32", "detr_hip_clip_adam_f32"]
EMA = ["detr_hip_set_floats8_f32", "detr_hip_ema_f32"]


def test_off_by_default_nothing_is_allocated_or_launched(rig):
    base = _loop(rig)
    assert base == PER_GROUP * 2 + ["detr_hip_set_floats8_f32"]
    assert rig.store.ema is None and "_ema" not in rig.opt
    assert not any(k.startswith("ema/") for k in rig.O.optimizer_state(rig.opt))
    with pytest.raises(ValueError):
        with rig.O.ema_weights(types.SimpleNamespace(engine=rig.engine)):
            pass
    with pytest.raises(ValueError):
        rig.store.state_dict(weights="ema")


def test_one_ema_launch_after_the_last_trained_group(rig):
    """Per-tensor mode: the launches of the groups as before, then the hyper write and ONE detr_hip_ema_f32 over the chunks of
    all trained groups; the shadow is created (a copy of the weights) at the first step that finds ema_decay set."""
    rig.cfg.ema_decay = 0.9
    before = rig.store.flat.clone()
    assert _loop(rig) == PER_GROUP * 2 + ["detr_hip_set_floats8_f32"] + EMA
    ema = rig.opt["_ema"]
    assert torch.equal(rig.store.ema, before) and rig.store.ema is not rig.store.flat and ema.num_updates == 1
    name, args = rig.calls[-1]
    n_all = sum(rig.opt[f"{g}_optimizer"].n_chunks for g in rig.O.GROUPS)
    assert args[0] == rig.store.ema.data_ptr() and args[1] == rig.store.flat.data_ptr() and args[6] == n_all and args[7] == rig.O.CHUNK
    assert rig.calls[-2][1][1] == float(np.float32(1.0 - 0.9))
    # the last trained group changes with the trained set; the chunk list follows
    rig.cfg.train_transformers = rig.cfg.train_nlayers = False
    assert _loop(rig, 1) == PER_GROUP + EMA
    assert rig.calls[-1][1][6] == rig.opt["backbone_optimizer"].n_chunks and ema.num_updates == 2
    # paused: no launch, the shadow and the count stay
    rig.cfg.ema_decay = None
    assert _loop(rig, 2) == PER_GROUP and ema.num_updates == 2 and rig.store.ema is not None
    rig.cfg.ema_decay = 1.0
    with pytest.raises(ValueError):
        _loop(rig, 3)


def test_joint_mode_and_accumulation(rig):
    rig.cfg.ema_decay, rig.cfg.ema_warmup, rig.cfg.global_clipnorm = 0.9998, True, 0.1
    joint = ["detr_hip_set_floats16_f32", "detr_hip_sumsq_segments_f32", "detr_hip_global_clip_scale_f32", "detr_hip_adamw_f32"]
    assert _loop(rig) == joint + EMA
    assert rig.calls[-2][1][1] == float(np.float32(1.0 - 0.1)) and rig.opt["_ema"].last_decay == 0.1
    assert _loop(rig, 1)[-2:] == EMA and rig.calls[-2][1][1] == float(np.float32(1.0 - 2.0 / 11.0))
    # target_batch = 2 x batch_size: the average moves at apply steps only
    rig.cfg.target_batch = 4
    assert "detr_hip_ema_f32" not in _loop(rig, 0) and rig.opt["_ema"].num_updates == 2
    assert _loop(rig, 1)[-2:] == EMA and rig.opt["_ema"].num_updates == 3
    rig.cfg.global_clipnorm = None
    assert "detr_hip_ema_f32" not in _loop(rig, 2)
    names = _loop(rig, 3)
    assert names[-2:] == EMA and names.count("detr_hip_ema_f32") == 1 and rig.opt["_ema"].num_updates == 4


def test_setup_creates_the_shadow_when_the_decay_is_already_set(rig):
    rig.cfg.ema_decay = 0.5
    opt = rig.O.setup_optimizers(types.SimpleNamespace(engine=rig.engine), rig.cfg)
    assert torch.equal(rig.store.ema, rig.store.flat) and opt["_ema"].num_updates == 0


def test_state_reload_and_scope_rules(rig):
    O, st = rig.O, rig.store
    parent_keys = set(O.optimizer_state(rig.opt))
    rig.cfg.ema_decay = 0.9
    _loop(rig)
    st.ema.add_(1.0)                                   # (no kernel runs here: make the shadow differ from the weights)
    state = O.optimizer_state(rig.opt)
    assert set(state) == parent_keys | {f"ema/{k}" for k in st.shapes} | {"ema/num_updates"} and int(state["ema/num_updates"]) == 1
    k0 = next(iter(st.shapes))
    o, n = st.offsets[k0]
    assert np.array_equal(state[f"ema/{k0}"].ravel(), st.ema[o:o + n].numpy())
    # restored in place; a wrong shape is refused before the first copy
    saved, ptr = st.ema.clone(), st.ema.data_ptr()
    st.ema.zero_()
    st.ema_num_updates = 7
    O.load_optimizer_state(rig.opt, state)
    valid = torch.zeros(st.total, dtype=torch.bool)
    for o, n in st.offsets.values():
        valid[o:o + n] = True
    assert torch.equal(st.ema[valid], saved[valid]) and st.ema.data_ptr() == ptr and st.ema_num_updates == 1
    bad = dict(state)
    bad[f"ema/{k0}"] = np.zeros((3,), np.float32)
    st.adam_m.fill_(5.0)
    with pytest.raises(ValueError):
        O.load_optimizer_state(rig.opt, bad)
    assert float(st.adam_m[0]) == 5.0
    with pytest.raises(ValueError):
        O.load_optimizer_state(rig.opt, {**state, "ema/nope": np.zeros(1, np.float32)})
    # a state without ema/* : the shadow restarts from the weights
    O.load_optimizer_state(rig.opt, {k: v for k, v in state.items() if not k.startswith("ema/")})
    assert torch.equal(st.ema, st.flat) and st.ema_num_updates == 0
    # a state with ema/* creates the shadow where there is none
    st.ema = None
    O.load_optimizer_state(rig.opt, state)
    assert torch.equal(st.ema[valid], saved[valid]) and st.ema_num_updates == 1
    # load_dict restarts the average
    st.load_dict({k0: np.ones(st.shapes[k0], np.float32)})
    assert torch.equal(st.ema, st.flat) and st.ema_num_updates == 0 and float(st.ema[st.offsets[k0][0]]) == 1.0
    # the scope: one exchange + on_change on entry and on exit, and what it forbids
    st.ema.add_(1.0)
    changes = []
    st.on_change = lambda: changes.append(1)
    model = types.SimpleNamespace(engine=rig.engine)
    del rig.calls[:]
    with O.ema_weights(model):
        assert [c[0] for c in rig.calls] == ["detr_hip_exchange_f32"] and len(changes) == 1
        assert rig.calls[0][1] == (st.flat.data_ptr(), st.ema.data_ptr(), st.total)
        for forbidden in (lambda: O.aggregate_grad_and_apply("backbone", rig.opt, None, 0, rig.cfg), lambda: O.optimizer_state(rig.opt),
                          lambda: O.load_optimizer_state(rig.opt, state), lambda: st.load_dict({}), lambda: O.ema_weights(model).__enter__()):
            with pytest.raises(RuntimeError):
                forbidden()
        assert st.ema_swapped
    assert [c[0] for c in rig.calls] == ["detr_hip_exchange_f32"] * 2 and len(changes) == 2 and not st.ema_swapped
