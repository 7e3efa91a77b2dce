"""GPU tests of the weight average (config.ema_decay): the two kernels of csrc/optim.hip through the C ABI, the update through
setup_optimizers / aggregate_grad_and_apply in both clip modes, its hipGraph replay, the ema_weights scope, the resumable state
and the reload rule.  Reference arithmetic: tests/ema_ref.py (NumPy float32; it reads no GPU result).  EVERY comparison is
torch.equal / byte equality: the update is three individually rounded fp32 operations.  Inputs are of normal magnitude.
Model-level tests inject seeded gradients into the flat gradient buffer, as tests/test_gpu_adamw.py does (the set loss uses fp32
atomics, so real steps are not bit-reproducible); the layouts and the small model are the ones of that file."""
import gc
import os

import numpy as np
import pytest
import torch

import ema_ref as E
from test_gpu_adamw import GROUPS, KCHUNK, SIZES, TGROUP, _build, _cfg, _tables, _valid, g

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 12345.0


@pytest.fixture(autouse=True)
def _release_models():
    yield
    gc.collect()


# ------------------------------------------------------------------------------------------
# kernels through the C ABI
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["aligned", "packed", "aligned_base_off_by_one_float"])
@pytest.mark.parametrize("groups", [(0, 1, 2), (0, 2)])
def test_ema_kernel_vs_ref(hip, groups, layout):
    """detr_hip_ema_f32 on the layout of test_gpu_adamw (sizes 1, 5, 64, 65, 4097, 20000; chunk 64): tensor starts at multiples
    of 8 floats (the 16-byte path with its scalar tail), back to back (`packed`: odd starts, scalar code), and the aligned
    layout in buffers that start one float past a 16-byte boundary (scalar code by the pointer rule).  Three updates with
    omd from the decays 0, 0.5 and 0.9998 on fresh parameters, then one with omd = 0 (shadow unchanged).  The shadow equals
    ema_ref bit for bit; the gaps between tensors and the tensors of an unlisted group keep their sentinel bytes; `param`
    is not written."""
    packed = layout == "packed"
    shift = 1 if layout == "aligned_base_off_by_one_float" else 0
    offs, total, ct, cs = _tables(packed)
    listed = [t for t in range(len(SIZES)) if TGROUP[t] in groups]
    keep = [i for i, t in enumerate(ct) if TGROUP[t] in groups]
    ctd = g(torch.tensor([ct[i] for i in keep], dtype=torch.int32))
    csd = g(torch.tensor([cs[i] for i in keep], dtype=torch.int64))
    sed = g(torch.tensor([o + n for o, n in zip(offs, SIZES)], dtype=torch.int64))
    rng = np.random.default_rng(11)
    s_host = np.full(total, SENTINEL, np.float32)
    for t in listed:
        s_host[offs[t]:offs[t] + SIZES[t]] = rng.normal(size=SIZES[t]).astype(np.float32)
    sbuf, pbuf = torch.zeros(total + 4, device=DEV), torch.zeros(total + 4, device=DEV)
    shadow, param = sbuf[shift:shift + total], pbuf[shift:shift + total]
    assert shadow.data_ptr() % 16 == 4 * shift and param.data_ptr() % 16 == 4 * shift
    shadow.copy_(torch.from_numpy(s_host))
    hyper = torch.zeros(8, device=DEV)
    mask = np.zeros(total, bool)
    for t in listed:
        mask[offs[t]:offs[t] + SIZES[t]] = True
    for decay in (0.0, 0.5, 0.9998, None):
        omd = np.float32(0.0) if decay is None else E.omd_of(decay)
        p_host = rng.normal(size=total).astype(np.float32)
        param.copy_(torch.from_numpy(p_host))
        hip.call("detr_hip_set_floats8_f32", hyper.data_ptr(), float(omd), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
        hip.call("detr_hip_ema_f32", shadow.data_ptr(), param.data_ptr(), ctd.data_ptr(), csd.data_ptr(), sed.data_ptr(), hyper.data_ptr(),
                 len(keep), KCHUNK)
        want = s_host.copy()
        want[mask] = E.update(s_host, p_host, omd)[mask]
        got = shadow.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (decay, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert param.cpu().numpy().tobytes() == p_host.tobytes()
        if decay is None:
            assert want.tobytes() == s_host.tobytes()
        else:
            assert not np.array_equal(want[mask], s_host[mask])
        s_host = want
    assert (s_host[~mask] == SENTINEL).all() and (~mask).sum() == total - sum(SIZES[t] for t in listed)
    assert not sbuf[:shift].any() and not sbuf[shift + total:].any() and not pbuf[shift + total:].any()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 7, 8, 1023, 20000])
def test_exchange(hip, n, off):
    """detr_hip_exchange_f32 with both pointers 16-byte aligned (off 0) and both one float past that (off 1): swapped exactly,
    restored by a second call, and the elements just outside [0, n) untouched."""
    gen = torch.Generator(device=DEV).manual_seed(n + off)
    abuf, bbuf = (torch.randn(n + 16, device=DEV, generator=gen) for _ in range(2))
    a0, b0 = abuf.clone(), bbuf.clone()
    lo = 4 + off
    a, b = abuf[lo:lo + n], bbuf[lo:lo + n]
    assert a.data_ptr() % 16 == 4 * off and b.data_ptr() % 16 == 4 * off
    hip.call("detr_hip_exchange_f32", a.data_ptr(), b.data_ptr(), n)
    assert torch.equal(a, b0[lo:lo + n]) and torch.equal(b, a0[lo:lo + n])
    for buf, ref in ((abuf, a0), (bbuf, b0)):
        assert torch.equal(buf[:lo], ref[:lo]) and torch.equal(buf[lo + n:], ref[lo + n:])
    hip.call("detr_hip_exchange_f32", a.data_ptr(), b.data_ptr(), n)
    assert torch.equal(abuf, a0) and torch.equal(bbuf, b0)


def test_exchange_past_two_gib(hip):
    """n = 2^29 + 5 floats: byte offsets past 2^31 (64-bit indexing in the body, the tail and the grid stride)."""
    n = 2 ** 29 + 5
    a = torch.empty(n + 4, device=DEV)
    b = torch.empty(n + 4, device=DEV)
    a.copy_(torch.arange(n + 4, device=DEV, dtype=torch.int32).bitwise_and_(0xFFFF))       # small integers: exact in fp32
    b.copy_(torch.arange(n + 4, device=DEV, dtype=torch.int32).bitwise_and_(0xFFFF).add_(0x10000))
    hip.call("detr_hip_exchange_f32", a.data_ptr(), b.data_ptr(), n)
    torch.cuda.synchronize()
    assert bool((a[:n] >= 0x10000).all()) and bool((b[:n] < 0x10000).all())
    assert bool((a[n:] < 0x10000).all()) and bool((b[n:] >= 0x10000).all())          # just outside: untouched
    for t, base in ((a, 0x10000), (b, 0)):
        for i in (0, 1, 2 ** 29 - 1, 2 ** 29, n - 1):
            assert float(t[i]) == float((i & 0xFFFF) + base), i
    # every element moved to the same index: the low 16 bits of the index survive the swap everywhere
    idx = torch.arange(n, device=DEV, dtype=torch.int32).bitwise_and_(0xFFFF)
    assert bool((b[:n].to(torch.int32) == idx).all())
    del idx
    assert bool((a[:n].to(torch.int32).sub_(0x10000) == torch.arange(n, device=DEV, dtype=torch.int32).bitwise_and_(0xFFFF)).all())


# ------------------------------------------------------------------------------------------
# through setup_optimizers on a small model (1 encoder layer, 2 decoder layers), gradients injected
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    from oracle import detr_ref as R
    return R.make_params(5, num_enc=1, num_dec=2)


@pytest.fixture(scope="module")
def rig(hip, weights):
    cfg = _cfg()
    model, opt = _build(weights, cfg)
    store = model.engine.P
    flat0 = store.flat.clone()
    gen = torch.Generator(device=DEV).manual_seed(23)
    unit = [torch.randn(store.total, device=DEV, generator=gen) for _ in range(4)]

    class Rig:
        pass
    r = Rig()
    r.cfg, r.model, r.opt, r.store, r.flat0, r.unit = cfg, model, opt, store, flat0, unit

    def reset(**settings):
        base = dict(weight_decay=0.0, global_clipnorm=None, adam_epsilon=1e-7, gradient_norm_clipping=0.1, target_batch=None,
                    train_backbone=True, train_transformers=True, train_nlayers=True, ema_decay=None, ema_warmup=False)
        base.update(settings)
        for k, val in base.items():
            setattr(cfg, k, val)
        store.flat.copy_(flat0)
        store.adam_m.zero_(), store.adam_v.zero_()
        store.ema, store.ema_num_updates = None, 0         # as before config.ema_decay was ever set
        opt.pop("_ema", None)
        for n in GROUPS:
            opt[f"{n}_optimizer"].iterations = 0
            opt[f"{n}_optimizer"].clipnorm = cfg.gradient_norm_clipping
            opt.pop(f"{n}_gradients", None)
        opt.pop("_joint_gradients", None)
        model.engine.bump_weights_version()
    r.reset = reset

    def step(grad, i=0):
        from detr_tf.optimizers import aggregate_grad_and_apply
        store.grad.copy_(grad)
        for n in GROUPS:
            aggregate_grad_and_apply(n, opt, None, i, cfg)
    r.step = step
    yield r
    r.__dict__.clear()
    del model, opt, store, flat0, unit, reset, step
    gc.collect()


def _trained_mask(store, opt, cfg):
    mask = np.zeros(store.total, bool)
    for n in GROUPS:
        if getattr(cfg, f"train_{n}"):
            for k in opt[f"{n}_optimizer"].names:
                o, cnt = store.offsets[k]
                mask[o:o + cnt] = True
    return mask


def _want(shadow_before, flat_after, decay, mask):
    """ema_ref over the elements of the trained tensors; everything else of the shadow as it was."""
    s, p = shadow_before.cpu().numpy(), flat_after.cpu().numpy()
    want = s.copy()
    want[mask] = E.update(s, p, E.omd_of(decay))[mask]
    return want


def _same_bytes(t, want):
    return t.cpu().numpy().tobytes() == want.tobytes()


GRAD_SCALE = [1e-3, 1e-1, 1e-2, 1e-3]


@pytest.mark.parametrize("mode", ["tensor", "joint"])
def test_model_steps_vs_ref_and_trained_weights_unchanged(hip, rig, mode):
    """Three steps with ema_decay 0.9 in the per-tensor and in the joint clip mode: after every step store.ema is ema_ref of
    the previous shadow and the read-back parameters, bit for bit; parameters and moments are torch.equal to the same run with
    ema_decay None.  The transformers group is then frozen: its shadow keeps equal to its (unmoved) weights."""
    extra = dict(global_clipnorm=0.1, weight_decay=1e-4) if mode == "joint" else {}
    rig.reset(**extra)
    plain = []
    for i in range(3):
        rig.step(rig.unit[i] * GRAD_SCALE[i], i)
        plain.append((rig.store.flat.clone(), rig.store.adam_m.clone(), rig.store.adam_v.clone()))
    assert rig.store.ema is None and "_ema" not in rig.opt
    rig.reset(ema_decay=0.9, **extra)
    mask = _trained_mask(rig.store, rig.opt, rig.cfg)
    shadow = rig.flat0.clone()                      # created at the first apply step as a copy of the weights before it
    for i in range(3):
        rig.step(rig.unit[i] * GRAD_SCALE[i], i)
        st = rig.store
        assert torch.equal(st.flat, plain[i][0]) and torch.equal(st.adam_m, plain[i][1]) and torch.equal(st.adam_v, plain[i][2]), i
        want = _want(shadow, st.flat, 0.9, mask)
        assert _same_bytes(st.ema, want), i
        assert not np.array_equal(want[mask], shadow.cpu().numpy()[mask])
        shadow = st.ema.clone()
    assert rig.opt["_ema"].num_updates == 3
    # train_transformers=False from the start: that group's shadow equals its weights, the others are averaged
    rig.reset(ema_decay=0.9, train_transformers=False, **extra)
    for i in range(2):
        rig.step(rig.unit[i] * GRAD_SCALE[i], i)
    tr = np.zeros(rig.store.total, bool)
    for k in rig.opt["transformers_optimizer"].names:
        o, cnt = rig.store.offsets[k]
        tr[o:o + cnt] = True
    tr = torch.from_numpy(tr).to(DEV)
    assert torch.equal(rig.store.ema[tr], rig.store.flat[tr]) and torch.equal(rig.store.flat[tr], rig.flat0[tr])
    ok = _valid(rig.store)
    assert not torch.equal(rig.store.ema[ok & ~tr], rig.store.flat[ok & ~tr])


def test_warmup_uses_the_num_updates_rule(hip, rig):
    """ema_warmup with ema_decay 0.9998: the decays used are 0.1, 2/11, 3/12 (checked through the shadow's bits)."""
    rig.reset(ema_decay=0.9998, ema_warmup=True)
    mask = _trained_mask(rig.store, rig.opt, rig.cfg)
    shadow = rig.flat0.clone()
    for i, d in enumerate([0.1, 2.0 / 11.0, 3.0 / 12.0]):
        rig.step(rig.unit[i] * GRAD_SCALE[i], i)
        assert E.step_decay(0.9998, True, i) == d == rig.opt["_ema"].last_decay
        assert _same_bytes(rig.store.ema, _want(shadow, rig.store.flat, d, mask)), i
        assert not _same_bytes(rig.store.ema, _want(shadow, rig.store.flat, 0.9998, mask))
        shadow = rig.store.ema.clone()


@pytest.mark.parametrize("mode", ["tensor", "joint"])
def test_accumulation_averages_at_apply_steps_only(hip, rig, mode):
    """target_batch = 2 x batch_size: of four steps the shadow moves at the second and the fourth only."""
    extra = dict(global_clipnorm=0.1) if mode == "joint" else {}
    rig.reset(ema_decay=0.9, target_batch=2 * rig.cfg.batch_size, **extra)
    mask = _trained_mask(rig.store, rig.opt, rig.cfg)
    shadow = rig.flat0.clone()
    for i in range(4):
        rig.step(rig.unit[i] * GRAD_SCALE[i], i)
        if i % 2 == 0:
            assert torch.equal(rig.store.ema, shadow), i
        else:
            assert _same_bytes(rig.store.ema, _want(shadow, rig.store.flat, 0.9, mask)) and not torch.equal(rig.store.ema, shadow), i
            shadow = rig.store.ema.clone()
    assert rig.opt["_ema"].num_updates == 2


def test_resume_and_state_keys(hip, rig, weights, tmp_path):
    """Save weights + state after step 2, a FRESH model and optimisers load both and run step 3: shadow and num_updates equal
    the uninterrupted run's (with warmup, so that a lost num_updates would change the decay).  Without a shadow the state has
    exactly the keys it had before this feature; a state without ema/* resets the shadow of an EMA-enabled run."""
    from detr_tf.optimizers import (aggregate_grad_and_apply, load_optimizer_state, load_optimizer_state_file, optimizer_state,
                                    save_optimizer_state)
    rig.reset()
    rig.step(rig.unit[0] * 1e-3, 0)
    st = rig.store
    parent_keys = ({f"{kind}/{k}" for kind in ("m", "v") for k in st.shapes} | {f"iterations/{n}" for n in GROUPS} | {"engine/step_no"})
    plain_state = optimizer_state(rig.opt)
    assert set(plain_state) == parent_keys and st.ema is None
    settings = dict(ema_decay=0.9998, ema_warmup=True)
    grads = [rig.unit[i] * GRAD_SCALE[i] for i in range(3)]
    rig.reset(**settings)
    for i in range(3):
        rig.step(grads[i], i)
    full = (st.flat.clone(), st.ema.clone(), rig.opt["_ema"].num_updates)
    rig.reset(**settings)
    for i in range(2):
        rig.step(grads[i], i)
    wpath, spath = os.path.join(tmp_path, "w.npz"), os.path.join(tmp_path, "opt.npz")
    st.save(wpath)
    save_optimizer_state(rig.opt, spath)
    assert set(optimizer_state(rig.opt)) == parent_keys | {f"ema/{k}" for k in st.shapes} | {"ema/num_updates"}

    cfg2 = _cfg()
    for k, val in settings.items():
        setattr(cfg2, k, val)
    model2, opt2 = _build(weights, cfg2)
    st2 = model2.engine.P
    assert st2.ema is not None and torch.equal(st2.ema, st2.flat)          # setup_optimizers found ema_decay set
    assert st2.load(wpath) == []
    ptr = st2.ema.data_ptr()
    load_optimizer_state_file(opt2, spath)
    assert st2.ema.data_ptr() == ptr and st2.ema_num_updates == 2          # restored in place
    st2.grad.copy_(grads[2])
    for n in GROUPS:
        aggregate_grad_and_apply(n, opt2, None, 2, cfg2)
    ok = _valid(st2)
    assert torch.equal(st2.flat[ok], full[0][ok]) and torch.equal(st2.ema[ok], full[1][ok]) and opt2["_ema"].num_updates == full[2] == 3
    # a state without ema/* : the shadow restarts from the current weights
    assert not torch.equal(st2.ema[ok], st2.flat[ok])
    load_optimizer_state(opt2, plain_state)
    assert torch.equal(st2.ema, st2.flat) and st2.ema_num_updates == 0


def test_load_weights_restarts_the_average(hip, rig, weights):
    rig.reset(ema_decay=0.5)
    rig.step(rig.unit[0] * 1e-2, 0)
    ok = _valid(rig.store)
    assert not torch.equal(rig.store.ema[ok], rig.store.flat[ok]) and rig.store.ema_num_updates == 1
    ptr = rig.store.ema.data_ptr()
    rig.model.load_weights(weights)
    assert torch.equal(rig.store.ema, rig.store.flat) and rig.store.ema_num_updates == 0 and rig.store.ema.data_ptr() == ptr
    assert torch.equal(rig.store.flat, rig.flat0)


# ------------------------------------------------------------------------------------------
# the ema_weights scope
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_scope_computes_with_the_saved_averaged_model(hip, weights, tmp_path, precision):
    """Inside ema_weights(model) logits and boxes on a seeded image are torch.equal to those of a fresh model loaded from
    save_weights(path, weights="ema"); after the scope store.flat and store.ema hold the bytes they held before it."""
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.optimizers import aggregate_grad_and_apply, ema_weights, setup_optimizers
    cfg = _cfg()
    cfg.ema_decay = 0.5

    def build():
        m = get_detr_model(cfg, include_top=True, num_encoder_layers=1, num_decoder_layers=2, dropout=0.1, precision=precision)
        m.load_weights(weights)
        return m
    model = build()
    opt = setup_optimizers(model, cfg)
    st = model.engine.P
    gen = torch.Generator(device=DEV).manual_seed(31)
    for i in range(2):
        st.grad.copy_(torch.randn(st.total, device=DEV, generator=gen) * 1e-1)
        for n in GROUPS:
            aggregate_grad_and_apply(n, opt, None, i, cfg)
    ok = _valid(st)
    assert not torch.equal(st.ema[ok], st.flat[ok])
    images = torch.randn(2, 96, 128, 3, device=DEV, generator=gen)
    out_model = model(images, training=False)
    flat_b, ema_b = st.flat.clone(), st.ema.clone()
    path = os.path.join(tmp_path, "averaged")
    model.save_weights(path, weights="ema")
    with ema_weights(model):
        assert torch.equal(st.flat, ema_b) and torch.equal(st.ema, flat_b)
        out_ema = model(images, training=False)
        inside = st.state_dict(weights="ema")                 # the same tensors, read through the exchanged buffers
    assert st.flat.cpu().numpy().tobytes() == flat_b.cpu().numpy().tobytes()
    assert st.ema.cpu().numpy().tobytes() == ema_b.cpu().numpy().tobytes()
    with np.load(path + ".npz") as z:
        assert set(z.files) == set(inside) == set(st.state_dict()) and all(np.array_equal(z[k], inside[k]) for k in z.files)
    fresh = build()
    assert fresh.load_weights(path) == []
    out_fresh = fresh(images, training=False)
    assert torch.equal(out_ema["pred_logits"], out_fresh["pred_logits"]) and torch.equal(out_ema["pred_boxes"], out_fresh["pred_boxes"])
    assert not torch.equal(out_ema["pred_logits"], out_model["pred_logits"])
    # and the trained model answers as before the scope
    again = model(images, training=False)
    assert torch.equal(again["pred_logits"], out_model["pred_logits"]) and torch.equal(again["pred_boxes"], out_model["pred_boxes"])


def test_training_continues_bit_identically_after_a_scope(hip, rig):
    """Two steps, a scope with a forward pass in it, a third step: parameters, shadow and moments equal, bit for bit, those of
    the same three steps without the scope."""
    from detr_tf.optimizers import ema_weights
    images = torch.randn(1, 96, 128, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))

    def run(scope):
        rig.reset(ema_decay=0.9)
        rig.step(rig.unit[0] * 1e-3, 0)
        rig.step(rig.unit[1] * 1e-1, 1)
        if scope:
            trained = rig.store.flat.clone()
            with ema_weights(rig.model):
                assert not torch.equal(rig.store.flat, trained) and torch.equal(rig.store.ema, trained)
                rig.model(images, training=False)
            assert torch.equal(rig.store.flat, trained)
        rig.step(rig.unit[2] * 1e-2, 2)
        return rig.store.flat.clone(), rig.store.ema.clone(), rig.store.adam_m.clone(), rig.store.adam_v.clone()
    plain, scoped = run(False), run(True)
    assert all(torch.equal(a, b) for a, b in zip(plain, scoped)) and rig.opt["_ema"].num_updates == 3


def test_scope_forbids_what_would_corrupt_the_average(hip, rig, weights, tmp_path):
    from detr_tf import training
    from detr_tf.optimizers import aggregate_grad_and_apply, ema_weights, load_optimizer_state, optimizer_state
    from test_gpu_training import _batches
    rig.reset()
    with pytest.raises(ValueError):
        with ema_weights(rig.model):
            pass
    with pytest.raises(ValueError):
        rig.model.save_weights(os.path.join(tmp_path, "never_written"), weights="ema")
    rig.reset(ema_decay=0.9)
    rig.step(rig.unit[0] * 1e-3, 0)
    state = optimizer_state(rig.opt)
    before = (rig.store.flat.clone(), rig.store.ema.clone())
    stepper = training.GraphedTrainStep(rig.model, rig.opt, rig.cfg, launch="eager")
    (im, tb, tc), = _batches(1, seed=2)
    with ema_weights(rig.model):
        for forbidden in (lambda: aggregate_grad_and_apply("backbone", rig.opt, None, 1, rig.cfg), lambda: stepper(im, tb, tc, 1),
                          lambda: optimizer_state(rig.opt), lambda: load_optimizer_state(rig.opt, state),
                          lambda: rig.model.load_weights(weights), lambda: ema_weights(rig.model).__enter__()):
            with pytest.raises(RuntimeError):
                forbidden()
    assert torch.equal(rig.store.flat, before[0]) and torch.equal(rig.store.ema, before[1]) and rig.opt["_ema"].num_updates == 1


# ------------------------------------------------------------------------------------------
# real training steps: eager train_step against the hipGraph replay
# ------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_switching_on_rerecords(hip, weights):
    """training.train_step against GraphedTrainStep(launch="graph") on 96 x 128 images, B = 2, compared as
    test_graph_replay_of_the_joint_step_equals_eager does (state copied from the eager to the graphed model before every step;
    loss to 1e-5, update to 2e-2 in relative L2: the set loss uses float atomics).  Two steps without the average, then
    ema_decay 0.9 is switched on: the step is re-recorded, and in BOTH runs the shadow after every step is ema_ref of that
    run's own previous shadow and parameters, bit for bit; num_updates agree."""
    from detr_tf import training
    from test_gpu_training import _batches
    data = _batches(5, seed=4)
    cfg_e, cfg_g = _cfg(), _cfg()
    (m_e, o_e), (m_g, o_g) = _build(weights, cfg_e), _build(weights, cfg_g)
    st_e, st_g = m_e.engine.P, m_g.engine.P
    stepper = training.GraphedTrainStep(m_g, o_g, cfg_g, eager_steps=1, launch="graph")
    mask = _trained_mask(st_e, o_e, cfg_e)
    first = None
    for i, (im, tb, tc) in enumerate(data):
        if i == 2:
            first = (stepper.step_graph, stepper.apply_graph)
            assert first[0] is not None and st_g.ema is None
            cfg_e.ema_decay = cfg_g.ema_decay = 0.9
        for src, dst in ((st_e.flat, st_g.flat), (st_e.adam_m, st_g.adam_m), (st_e.adam_v, st_g.adam_v)):
            dst.copy_(src)
        if st_e.ema is not None and st_g.ema is not None:
            st_g.ema.copy_(st_e.ema)
        m_g.engine.bump_weights_version()
        before = st_e.flat.clone()
        sh_e = st_e.ema.clone() if st_e.ema is not None else before.clone()
        sh_g = st_g.ema.clone() if st_g.ema is not None else before.clone()
        _, tot_e, _ = training.train_step(m_e, im, tb, tc, o_e, cfg_e, i)
        _, tot_g, _ = stepper(im, tb, tc, i)
        assert abs(float(tot_e) - float(tot_g)) <= 1e-5 * abs(float(tot_e)), (i, float(tot_e), float(tot_g))
        de, dg = st_e.flat - before, st_g.flat - before
        rel = float((de - dg).norm()) / float(de.norm())
        assert rel <= 2e-2, (i, rel)
        if i >= 2:
            assert _same_bytes(st_e.ema, _want(sh_e, st_e.flat, 0.9, mask)), i
            assert _same_bytes(st_g.ema, _want(sh_g, st_g.flat, 0.9, mask)), i
            assert not torch.equal(st_g.ema, sh_g)
            assert o_e["_ema"].num_updates == o_g["_ema"].num_updates == i - 1
        if i == 3:                       # step 2 ran eagerly (new signature), step 3 recorded anew
            assert stepper.step_graph is not None and stepper.apply_graph is not first[1]
            second = (stepper.step_graph, stepper.apply_graph)
    assert (stepper.step_graph, stepper.apply_graph) == second           # step 4: a replay with a fresh 1 - decay, no re-recording
    assert st_e.ema_num_updates == st_g.ema_num_updates == 3


def test_auto_launch_counts_every_update(hip, weights):
    """launch="auto" (warm-up, recording, timed replays, timed eager steps, decision): every one of its steps is an ordinary
    training step with one update of the average; the shadow follows ema_ref through all of them."""
    from detr_tf import training
    from test_gpu_training import _batches
    cfg = _cfg()
    cfg.ema_decay, cfg.ema_warmup = 0.9998, True
    model, opt = _build(weights, cfg)
    st = model.engine.P
    stepper = training.GraphedTrainStep(model, opt, cfg, eager_steps=1, launch="auto")
    data = _batches(2, seed=6)
    mask = _trained_mask(st, opt, cfg)
    steps = stepper.settle_calls + 1
    for i in range(steps):
        im, tb, tc = data[i % 2]
        sh = st.ema.clone()
        stepper(im, tb, tc, i)
        assert _same_bytes(st.ema, _want(sh, st.flat, E.step_decay(0.9998, True, i), mask)), i
    assert opt["_ema"].num_updates == steps and stepper.probe is not None
