"""GPU tests of the AdamW path of csrc/optim.hip and detr_tf/optimizers.py: decoupled weight decay, ONE gradient norm over
every trained tensor (config.global_clipnorm), the deferred joint apply, its hipGraph replay and the resumable optimiser
state.  Reference arithmetic: tests/adamw_ref.py (float64, pinned against torch.optim.AdamW in tests/test_adamw_cpu.py).
Model-level tests inject seeded gradients into the flat gradient buffer: the set loss uses fp32 atomics, so real steps are
not bit-reproducible (see test_gpu_training.test_graph_replay_equals_eager_steps)."""
import gc
import math
import os

import numpy as np
import pytest
import torch

import adamw_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"


def g(t):
    return t.to(DEV).contiguous()


def close(a, b, rtol, what=""):
    """The metric of test_gpu_kernels.close: max abs error against rtol times the largest reference magnitude."""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    scale = float(b.abs().max()) + 1e-30
    err = float((a - b).abs().max())
    assert err <= rtol * scale, f"{what}: max abs err {err:.3e} > {rtol * scale:.3e} (scale {scale:.3e})"


GROUPS = ("backbone", "transformers", "nlayers")


@pytest.fixture(autouse=True)
def _release_models():
    """A model is cyclic garbage once dropped (engine <-> parameter store): release what a test built when it ends, not at
    some later collection in the middle of another test."""
    yield
    gc.collect()


# ------------------------------------------------------------------------------------------
# kernels through the C ABI
# ------------------------------------------------------------------------------------------
SIZES = [1, 5, 64, 65, 4097, 20000]       # one element, a ragged 16-byte tail, one chunk, one chunk + 1, many chunks
TGROUP = [0, 1, 0, 2, 1, 1]
KCHUNK = 64
LRS = [1e-2, 3e-3, 1e-3]
WD = 1e-2


def _tables(packed):
    """Chunk tables of SIZES at chunk = 64 (383 chunks: the finalize strides over more than 256 partials).  Tensor starts
    are multiples of 8 floats as in the parameter store, or back to back (`packed`: odd starts, the scalar path)."""
    offs, o = [], 0
    for n in SIZES:
        offs.append(o)
        o += n if packed else (n + 7) // 8 * 8
    ct, cs = [], []
    for t, (o0, n) in enumerate(zip(offs, SIZES)):
        for st in range(0, n, KCHUNK):
            ct.append(t)
            cs.append(o0 + st)
    assert len(ct) > 256
    return offs, o, ct, cs


def _flatten(arrs, offs, total):
    out = np.zeros(total, np.float32)
    for a, o in zip(arrs, offs):
        out[o:o + a.size] = a
    return out


def _hyper16(hip, dst, step, clip, trained, wd=WD):
    from detr_tf.optimizers import write_hyper16
    lr_t = [lr * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step) for lr in LRS]
    write_hyper16(dst, lr_t + [clip, 0.9, 0.999, 1e-7, wd] + LRS + [1.0 if t else 0.0 for t in trained] + [0.0, 0.0])


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("trained", [(True, True, True), (True, False, True)])
def test_joint_adamw_kernels_vs_ref(hip, trained, packed):
    """Partial sums, finalize and update through the C ABI against adamw_ref, parameters compared after every step with the
    metric of test_clip_adam_vs_oracle (max abs error <= 1e-5 of the largest parameter).  c = 0.2: the gradient scales 1e-3,
    10 and 1 put G (0.156, 1557, 156 over all 24232 elements) below, far above and far above the threshold; a fourth step
    is scaled to G = 1.05 c, just above it.  With group 1 untrained its parameters and moments stay bit-identical and G
    leaves it out (the device's G is compared with the reference's).
    Largest deviation seen on an MI355X: 1.77e-7 of the largest parameter (step 4, all four parametrisations), against
    the 1e-5 allowed; the device's G and clip factor agree with the reference's to all 7 printed digits."""
    offs, total, ct, cs = _tables(packed)
    rng = np.random.default_rng(3)
    c = 0.2
    p0 = [rng.normal(size=n).astype(np.float32) for n in SIZES]
    m0 = [(rng.normal(size=n) * 1e-2).astype(np.float32) for n in SIZES]      # non-zero moments: an untouched tensor must keep them
    v0 = [(rng.random(size=n) * 1e-3).astype(np.float32) for n in SIZES]
    flat, m, v = (g(torch.tensor(_flatten(a, offs, total))) for a in (p0, m0, v0))
    ctd, csd = g(torch.tensor(ct, dtype=torch.int32)), g(torch.tensor(cs, dtype=torch.int64))
    sed = g(torch.tensor([o + n for o, n in zip(offs, SIZES)], dtype=torch.int64))
    tgd = g(torch.tensor(TGROUP, dtype=torch.int32))
    hyper, scale = torch.zeros(16, device=DEV), torch.zeros(2, device=DEV)
    ref = A.AdamW(dict(enumerate(LRS)), dict(enumerate(TGROUP)), weight_decay=WD, global_clipnorm=c)
    ref.m = {i: m0[i].astype(np.float64) for i in range(len(SIZES))}
    ref.v = {i: v0[i].astype(np.float64) for i in range(len(SIZES))}
    params = {i: p.astype(np.float64) for i, p in enumerate(p0)}
    live = [i for i in range(len(SIZES)) if trained[TGROUP[i]]]
    worst = 0.0
    for step in range(1, 5):
        raw = [rng.normal(size=n) for n in SIZES]
        if step < 4:
            sc = [1e-3, 10.0, 1.0][step - 1]
        else:
            sc = 1.05 * c / A.global_norm([raw[i] for i in live])
        grads = [(r * sc).astype(np.float32) for r in raw]
        gflat = g(torch.tensor(_flatten(grads, offs, total)))
        sumsq = torch.zeros(len(ct), device=DEV)
        _hyper16(hip, hyper, step, c, trained)
        hip.call("detr_hip_sumsq_segments_f32", gflat.data_ptr(), ctd.data_ptr(), csd.data_ptr(), sed.data_ptr(), len(ct), KCHUNK,
                 sumsq.data_ptr())
        hip.call("detr_hip_global_clip_scale_f32", sumsq.data_ptr(), ctd.data_ptr(), tgd.data_ptr(), hyper.data_ptr(), len(ct),
                 scale.data_ptr())
        hip.call("detr_hip_adamw_f32", flat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), ctd.data_ptr(), csd.data_ptr(),
                 sed.data_ptr(), tgd.data_ptr(), sumsq.data_ptr(), hyper.data_ptr(), scale.data_ptr(), len(ct), KCHUNK)
        s_ref = ref.step({i: grads[i] for i in live}, params)
        s_dev, G_dev = (float(x) for x in scale.cpu())
        print(f"step {step}: G device {G_dev:.7g} ref {ref.last_norm:.7g}, s device {s_dev:.7g} ref {s_ref:.7g}")
        assert abs(G_dev - ref.last_norm) <= 1e-5 * ref.last_norm           # (the norm of the TRAINED tensors only)
        assert (s_dev == 1.0) == (ref.last_norm <= c) and abs(s_dev - s_ref) <= 1e-5 * s_ref
        want = _flatten([params[i] for i in range(len(SIZES))], offs, total)
        err = float((flat.cpu().double() - torch.tensor(want).double()).abs().max()) / float(np.abs(want).max())
        worst = max(worst, err)
        print(f"step {step}: max abs err / max |p| = {err:.3e}")
        close(flat, torch.tensor(want), rtol=1e-5, what=f"joint adamw step {step}")
        for arr, refd, what in ((m, ref.m, "m"), (v, ref.v, "v")):
            close(arr, torch.tensor(_flatten([refd[i] for i in range(len(SIZES))], offs, total)), rtol=1e-5, what=f"{what} step {step}")
    for i in range(len(SIZES)):
        if i not in live:                      # untrained: bit-identical parameters and moments
            sl = slice(offs[i], offs[i] + SIZES[i])
            assert torch.equal(flat[sl].cpu(), torch.tensor(p0[i])) and torch.equal(m[sl].cpu(), torch.tensor(m0[i]))
            assert torch.equal(v[sl].cpu(), torch.tensor(v0[i]))
    if not packed:                             # the alignment gaps between tensors are never written
        gaps = torch.ones(total, dtype=torch.bool)
        for o, n in zip(offs, SIZES):
            gaps[o:o + n] = False
        assert not flat.cpu()[gaps].any() and not m.cpu()[gaps].any() and not v.cpu()[gaps].any()
    print(f"largest deviation: {worst:.3e}")


@pytest.mark.parametrize("packed", [False, True])
def test_per_tensor_clip_with_decay_vs_ref(hip, packed):
    """The per-tensor clip (clipnorm 0.1, as test_clip_adam_vs_oracle) with weight decay: detr_hip_adamw_f32 without a joint
    scale.  At gradient scale 1e-3 only the 20000-element tensor (norm 0.141) is clipped.  Largest deviation seen on an
    MI355X: 1.17e-7 of the largest parameter (bound 1e-5)."""
    offs, total, ct, cs = _tables(packed)
    rng = np.random.default_rng(4)
    p0 = [rng.normal(size=n).astype(np.float32) for n in SIZES]
    flat = g(torch.tensor(_flatten(p0, offs, total)))
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    ctd, csd = g(torch.tensor(ct, dtype=torch.int32)), g(torch.tensor(cs, dtype=torch.int64))
    sed = g(torch.tensor([o + n for o, n in zip(offs, SIZES)], dtype=torch.int64))
    tgd = g(torch.tensor(TGROUP, dtype=torch.int32))
    hyper = torch.zeros(16, device=DEV)
    ref = A.AdamW(dict(enumerate(LRS)), dict(enumerate(TGROUP)), weight_decay=WD, clipnorm=0.1)
    params = {i: p.astype(np.float64) for i, p in enumerate(p0)}
    for step in range(1, 4):
        sc = [1e-3, 10.0, 1.0][step - 1]
        grads = [(rng.normal(size=n) * sc).astype(np.float32) for n in SIZES]
        gflat = g(torch.tensor(_flatten(grads, offs, total)))
        sumsq = torch.zeros(len(ct), device=DEV)
        _hyper16(hip, hyper, step, 0.1, (True, True, True))
        hip.call("detr_hip_sumsq_segments_f32", gflat.data_ptr(), ctd.data_ptr(), csd.data_ptr(), sed.data_ptr(), len(ct), KCHUNK,
                 sumsq.data_ptr())
        hip.call("detr_hip_adamw_f32", flat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), ctd.data_ptr(), csd.data_ptr(),
                 sed.data_ptr(), tgd.data_ptr(), sumsq.data_ptr(), hyper.data_ptr(), None, len(ct), KCHUNK)
        ref.step(dict(enumerate(grads)), params)
        want = _flatten([params[i] for i in range(len(SIZES))], offs, total)
        err = float((flat.cpu().double() - torch.tensor(want).double()).abs().max()) / float(np.abs(want).max())
        print(f"per-tensor step {step}: max abs err / max |p| = {err:.3e}")
        close(flat, torch.tensor(want), rtol=1e-5, what=f"per-tensor adamw step {step}")


# ------------------------------------------------------------------------------------------
# through setup_optimizers on a small model (1 encoder layer, 2 decoder layers), gradients injected
# ------------------------------------------------------------------------------------------
def _cfg():
    from test_gpu_training import _cfg as base
    return base()


@pytest.fixture(scope="module")
def weights():
    from oracle import detr_ref as R
    return R.make_params(5, num_enc=1, num_dec=2)


def _build(weights, cfg):
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.optimizers import setup_optimizers
    model = get_detr_model(cfg, include_top=True, num_encoder_layers=1, num_decoder_layers=2, dropout=0.1)
    model.load_weights(weights)
    return model, setup_optimizers(model, cfg)


@pytest.fixture(scope="module")
def rig(hip, weights):
    """One model + optimisers shared by the injected-gradient tests; every test starts from `reset`."""
    cfg = _cfg()
    model, opt = _build(weights, cfg)
    store = model.engine.P
    flat0 = store.flat.clone()
    gen = torch.Generator(device=DEV).manual_seed(17)
    unit = [torch.randn(store.total, device=DEV, generator=gen) for _ in range(3)]     # seeded gradients, unit scale

    class Rig:
        pass
    r = Rig()
    r.cfg, r.model, r.opt, r.store, r.flat0, r.unit = cfg, model, opt, store, flat0, unit

    def reset(**settings):
        base = dict(weight_decay=0.0, global_clipnorm=None, adam_epsilon=1e-7, gradient_norm_clipping=0.1, target_batch=None,
                    train_backbone=True, train_transformers=True, train_nlayers=True)
        base.update(settings)
        for k, val in base.items():
            setattr(cfg, k, val)
        store.flat.copy_(flat0)
        store.adam_m.zero_(), store.adam_v.zero_()
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


def _ref_step(rig, ref, params, grad):
    host = grad.cpu().numpy()
    st = rig.store
    ref.step({k: host[o:o + n] for k, (o, n) in st.offsets.items()}, params)
    want = np.zeros(st.total)
    for k, (o, n) in st.offsets.items():
        want[o:o + n] = params[k]
    return want


def _model_ref(rig, **kw):
    st, cfg = rig.store, rig.cfg
    from detr_tf.params import variable_group
    groups = {k: variable_group(k, cfg.nlayers) for k in st.shapes}
    ref = A.AdamW({i: float(getattr(cfg, f"{n}_lr")) for i, n in enumerate(GROUPS)}, groups, **kw)
    host = rig.flat0.cpu().numpy().astype(np.float64)
    return ref, {k: host[o:o + n].copy() for k, (o, n) in st.offsets.items()}


def _check_update(flat, want, rig, ok, steps):
    """The learning rates of the model (1e-5, 1e-4) make an update far smaller than 1e-5 of the largest parameter, so the
    update itself is bounded too: per step the fp32 parameter is rounded twice (after the decay and after the Adam term:
    2 * 2^-24 of the largest parameter) and the update is held to 1e-5 of the largest total change."""
    d_dev = (flat - rig.flat0).cpu().double()[ok]
    d_ref = (torch.tensor(want) - rig.flat0.cpu().double())[ok]
    bound = steps * 2.0 ** -23 * float(np.abs(want).max()) + 1e-5 * float(d_ref.abs().max())
    err = float((d_dev - d_ref).abs().max())
    print(f"update: max abs err {err:.3e}, bound {bound:.3e}, largest change {float(d_ref.abs().max()):.3e}")
    assert err <= bound


def _valid(store):
    mask = torch.zeros(store.total, dtype=torch.bool, device=store.flat.device)
    for o, n in store.offsets.values():
        mask[o:o + n] = True
    return mask


def test_defaults_reproduce_the_two_legacy_entry_points(hip, rig):
    """With the new settings at their defaults aggregate_grad_and_apply gives, bit for bit, what the Adam(clipnorm) entry
    points give when called directly on copies (two steps: the second runs on non-zero moments).  Passes on the parent
    commit by construction; it guards the default path."""
    from detr_tf.optimizers import CHUNK
    rig.reset()
    st = rig.store
    flat, m, v = st.flat.clone(), torch.zeros_like(st.flat), torch.zeros_like(st.flat)
    for step in (1, 2):
        grad = rig.unit[step] * 1e-3
        rig.step(grad, step - 1)
        for n in GROUPS:
            o = rig.opt[f"{n}_optimizer"]
            if o.n_chunks == 0:
                continue
            lr_t = float(getattr(rig.cfg, f"{n}_lr")) * math.sqrt(1.0 - 0.999 ** step) / (1.0 - 0.9 ** step)
            hyper = torch.tensor([lr_t, lr_t, lr_t, 0.1, 0.9, 0.999, 1e-7, 0.0], dtype=torch.float32, device=DEV)
            sumsq = torch.zeros(o.n_chunks, device=DEV)
            hip.call("detr_hip_sumsq_segments_f32", grad.data_ptr(), o.chunk_tensor.data_ptr(), o.chunk_start.data_ptr(),
                     o.seg_end.data_ptr(), o.n_chunks, CHUNK, sumsq.data_ptr())
            hip.call("detr_hip_clip_adam_f32", flat.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), o.chunk_tensor.data_ptr(),
                     o.chunk_start.data_ptr(), o.seg_end.data_ptr(), o.tensor_group.data_ptr(), sumsq.data_ptr(), hyper.data_ptr(),
                     o.n_chunks, CHUNK)
        assert torch.equal(st.flat, flat) and torch.equal(st.adam_m, m) and torch.equal(st.adam_v, v), step
    assert not torch.equal(st.flat, rig.flat0) and "_joint" not in rig.opt


def test_joint_step_is_reproducible_and_matches_ref(hip, rig):
    """Two runs of two joint steps from the same state give torch.equal parameters and moments, and the result is
    adamw_ref's at rtol 1e-5 (metric of test_clip_adam_vs_oracle).  G = 5.4 and 540 against c = 0.1."""
    runs = []
    for _ in range(2):
        rig.reset(global_clipnorm=0.1, weight_decay=1e-4)
        rig.step(rig.unit[0] * 1e-3, 0)
        rig.step(rig.unit[1] * 1e-1, 1)
        runs.append((rig.store.flat.clone(), rig.store.adam_m.clone(), rig.store.adam_v.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert [rig.opt[f"{n}_optimizer"].iterations for n in GROUPS] == [2, 2, 2]
    ref, params = _model_ref(rig, weight_decay=1e-4, global_clipnorm=0.1)
    _ref_step(rig, ref, params, rig.unit[0] * 1e-3)
    want = _ref_step(rig, ref, params, rig.unit[1] * 1e-1)
    G_dev = float(rig.opt["_joint"].scale[1])
    assert abs(G_dev - ref.last_norm) <= 1e-5 * ref.last_norm
    ok = _valid(rig.store).cpu()
    close(runs[0][0].cpu()[ok], torch.tensor(want)[ok], rtol=1e-5, what="joint model step")
    _check_update(runs[0][0], want, rig, ok, steps=2)


@pytest.mark.parametrize("wd", [1e-4, 1e-2])
def test_norm_below_threshold_equals_clipping_off(hip, rig, wd):
    """G <= c: s is exactly 1.0 and the joint step equals, bit for bit, the same AdamW step with clipping disabled
    (global_clipnorm None and gradient_norm_clipping None: the per-tensor variant of the same kernel, which never fuses a
    multiply into an add).  Not comparable that way at weight_decay == 0: with clipping off that setting runs the
    Adam(clipnorm) kernel, whose paired and remainder loop iterations already round differently from each other (one fuses
    b*m + (1-b)*g, the other does not), so no second kernel can match its bits element by element."""
    grad = rig.unit[2] * 1e-6                         # G = 5.4e-3 < 0.1
    rig.reset(global_clipnorm=0.1, weight_decay=wd)
    rig.step(grad, 0)
    rig.step(grad * 2.0, 1)
    assert float(rig.opt["_joint"].scale[0]) == 1.0 and float(rig.opt["_joint"].scale[1]) < 0.1
    joint = (rig.store.flat.clone(), rig.store.adam_m.clone(), rig.store.adam_v.clone())
    rig.reset(global_clipnorm=None, gradient_norm_clipping=None, weight_decay=wd)
    rig.step(grad, 0)
    rig.step(grad * 2.0, 1)
    assert torch.equal(joint[0], rig.store.flat) and torch.equal(joint[1], rig.store.adam_m) and torch.equal(joint[2], rig.store.adam_v)
    assert not torch.equal(joint[0], rig.flat0)


def test_joint_accumulation_applies_the_summed_gradient_once(hip, rig):
    """target_batch = 2 x batch_size in joint mode: nothing moves after the first call sequence, and after the second the
    parameters are adamw_ref's for the SUMMED gradient (one step, G of the sum); the transformers group is frozen for the
    first window's check of 'frozen groups neither count nor move'."""
    rig.reset(global_clipnorm=0.1, weight_decay=1e-4, target_batch=2 * rig.cfg.batch_size)
    g0, g1 = rig.unit[0] * 1e-3, rig.unit[1] * 1e-3
    rig.step(g0, 0)
    assert torch.equal(rig.store.flat, rig.flat0) and not rig.store.adam_m.any()
    assert [rig.opt[f"{n}_optimizer"].iterations for n in GROUPS] == [0, 0, 0]
    rig.step(g1, 1)
    assert [rig.opt[f"{n}_optimizer"].iterations for n in GROUPS] == [1, 1, 1]
    ref, params = _model_ref(rig, weight_decay=1e-4, global_clipnorm=0.1)
    want = _ref_step(rig, ref, params, g0 + g1)
    ok = _valid(rig.store).cpu()
    close(rig.store.flat.cpu()[ok], torch.tensor(want)[ok], rtol=1e-5, what="accumulated joint step")
    _check_update(rig.store.flat, want, rig, ok, steps=1)
    # second window with a frozen group: its slices keep their bits, G is the norm of the others' accumulated gradient
    before = rig.store.flat.clone()
    rig.cfg.train_transformers = False
    rig.step(g0, 2)
    rig.step(g1, 3)
    tr = torch.zeros(rig.store.total, dtype=torch.bool, device=DEV)
    for k in rig.opt["transformers_optimizer"].names:
        o, n = rig.store.offsets[k]
        tr[o:o + n] = True
    assert torch.equal(rig.store.flat[tr], before[tr]) and not torch.equal(rig.store.flat[~tr], before[~tr])
    host = (g0 + g1).cpu().numpy()
    G = A.global_norm([host[o:o + n] for k, (o, n) in rig.store.offsets.items() if k not in set(rig.opt["transformers_optimizer"].names)])
    assert abs(float(rig.opt["_joint"].scale[1]) - G) <= 1e-5 * G
    assert [rig.opt[f"{n}_optimizer"].iterations for n in GROUPS] == [2, 1, 2]


def test_resume_from_saved_state_equals_the_uninterrupted_run(hip, rig, weights, tmp_path):
    """Two joint steps, save weights + optimiser state, a FRESH model and optimiser load both and run the third step:
    parameters, moments, step counts and the engine's dropout step counter equal the uninterrupted three-step run."""
    from detr_tf.optimizers import load_optimizer_state_file, save_optimizer_state
    settings = dict(global_clipnorm=0.1, weight_decay=1e-4)
    grads = [rig.unit[0] * 1e-3, rig.unit[1] * 1e-2, rig.unit[2] * 1e-3]
    eng = rig.model.engine
    step0 = eng._step_no
    rig.reset(**settings)
    for i in range(3):
        eng.advance_dropout_step()
        rig.step(grads[i], i)
    full = (rig.store.flat.clone(), rig.store.adam_m.clone(), rig.store.adam_v.clone(), eng._step_no, eng._step_seed)
    eng._step_no = step0
    rig.reset(**settings)
    for i in range(2):
        eng.advance_dropout_step()
        rig.step(grads[i], i)
    wpath, spath = os.path.join(tmp_path, "w.npz"), os.path.join(tmp_path, "opt.npz")
    rig.store.save(wpath)
    save_optimizer_state(rig.opt, spath)

    cfg2 = _cfg()
    for k, val in settings.items():
        setattr(cfg2, k, val)
    model2, opt2 = _build(weights, cfg2)
    st2 = model2.engine.P
    assert st2.load(wpath) == []
    load_optimizer_state_file(opt2, spath)
    assert model2.engine._step_no == step0 + 2
    model2.engine.advance_dropout_step()
    from detr_tf.optimizers import aggregate_grad_and_apply
    st2.grad.copy_(grads[2])
    for n in GROUPS:
        aggregate_grad_and_apply(n, opt2, None, 2, cfg2)
    ok = _valid(st2)
    assert torch.equal(st2.flat[ok], full[0][ok]) and torch.equal(st2.adam_m[ok], full[1][ok]) and torch.equal(st2.adam_v[ok], full[2][ok])
    assert [opt2[f"{n}_optimizer"].iterations for n in GROUPS] == [3, 3, 3]
    assert model2.engine._step_no == full[3] and model2.engine._step_seed == full[4]


# ------------------------------------------------------------------------------------------
# real training steps: eager train_step against the hipGraph replay
# ------------------------------------------------------------------------------------------
def test_graph_replay_of_the_joint_step_equals_eager(hip, weights):
    """training.train_step against GraphedTrainStep(launch="graph") with weight_decay 1e-4 and global_clipnorm 0.1 on
    96 x 128 images, B = 2, state copied from the eager to the graphed model before every step and the bounds of
    test_graph_replay_equals_eager_steps (logits 1e-5 of their scale, loss 1e-5, update 2e-2 in relative L2).  Then a new
    config.weight_decay (5.0: the decay term is then a large part of the update, so a replay that kept the old value would
    miss the bound) is picked up by the next replay WITHOUT a re-recording."""
    from detr_tf import training
    from test_gpu_training import _batches
    data = _batches(4, seed=3)
    cfg_e, cfg_g = _cfg(), _cfg()
    for c in (cfg_e, cfg_g):
        c.weight_decay, c.global_clipnorm = 1e-4, 0.1
    (m_e, o_e), (m_g, o_g) = _build(weights, cfg_e), _build(weights, cfg_g)
    stepper = training.GraphedTrainStep(m_g, o_g, cfg_g, eager_steps=1, launch="graph")
    recorded = None
    for i, (im, tb, tc) in enumerate(data):
        if i == 3:
            cfg_e.weight_decay = cfg_g.weight_decay = 5.0
            recorded = (stepper.step_graph, stepper.apply_graph)
            assert recorded[0] is not None
        for src, dst in ((m_e.engine.P.flat, m_g.engine.P.flat), (m_e.engine.P.adam_m, m_g.engine.P.adam_m),
                         (m_e.engine.P.adam_v, m_g.engine.P.adam_v)):
            dst.copy_(src)
        m_g.engine.bump_weights_version()
        before = m_e.engine.P.flat.clone()
        out_e, tot_e, log_e = training.train_step(m_e, im, tb, tc, o_e, cfg_e, i)
        lg_e = out_e["pred_logits"].clone()
        out_g, tot_g, log_g = stepper(im, tb, tc, i)
        lg_g = out_g["pred_logits"].clone()
        assert float((lg_e - lg_g).abs().max()) <= 1e-5 * float(lg_e.abs().max()), (i, float((lg_e - lg_g).abs().max()))
        assert abs(float(tot_e) - float(tot_g)) <= 1e-5 * abs(float(tot_e)), (i, float(tot_e), float(tot_g))
        de, dg = m_e.engine.P.flat - before, m_g.engine.P.flat - before
        rel = float((de - dg).norm()) / float(de.norm())
        print(f"step {i}: update rel L2 difference {rel:.3e}, G eager {float(o_e['_joint'].scale[1]):.4g} graph {float(o_g['_joint'].scale[1]):.4g}")
        assert rel <= 2e-2, (i, rel)
        if i == 3:
            # the decay the replay had to pick up: lr * 5.0 * p, a large part of this step's update
            dec = torch.zeros_like(before)
            for gi, n in enumerate(GROUPS):
                for a, b in o_e["_joint"].runs[gi]:
                    dec[a:b] = float(getattr(cfg_e, f"{n}_lr")) * 5.0 * before[a:b]
            assert float(dec.norm()) >= 0.1 * float(de.norm())
    assert (stepper.step_graph, stepper.apply_graph) == recorded and stepper.calls == 4
    assert [o_g[f"{n}_optimizer"].iterations for n in GROUPS] == [o_e[f"{n}_optimizer"].iterations for n in GROUPS] == [4, 4, 4]


def test_recording_keeps_the_garbage_collector_out(hip, weights, monkeypatch):
    """A collection in the middle of a stream capture destroys device objects of dropped models (engine <-> store cycles)
    and has aborted the process: the recording collects first and runs with the collector off, then restores it."""
    from detr_tf import training
    from test_gpu_training import _batches
    cfg = _cfg()
    model, opt = _build(weights, cfg)
    seen = []
    real = training.run_train_step

    def spy(m, *a, **kw):
        seen.append((bool(m.engine._graph_replay), gc.isenabled()))
        return real(m, *a, **kw)
    monkeypatch.setattr(training, "run_train_step", spy)
    stepper = training.GraphedTrainStep(model, opt, cfg, eager_steps=1, launch="graph")
    (im, tb, tc), = _batches(1, seed=9)
    assert gc.isenabled()
    stepper(im, tb, tc, 0)
    stepper(im, tb, tc, 1)
    assert seen == [(False, True), (True, False)] and gc.isenabled() and stepper.step_graph is not None
