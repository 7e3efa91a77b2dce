"""GPU tests of the training / evaluation LOOP of the drop-in API (reference detr_tf/training.py:35-87): console
format, `config.global_step`, the `evaluation_step` break, gradient accumulation through `fit`, and the hipGraph replay
of the step (`training.GraphedTrainStep`) against the eager step."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TRAIN_LINE = re.compile(r"^Epoch: \[(\d+)\], \t Step: \[(\d+)\], \t ce: \[(-?\d+\.\d\d)\] \t giou : \[(-?\d+\.\d\d)\] \t "
                        r"l1 : \[(-?\d+\.\d\d)\] \t time : \[(\d+\.\d\d)\]$")
VAL_LINE = re.compile(r"^Validation step: \[(\d+)\], \t ce: \[(-?\d+\.\d\d)\] \t giou : \[(-?\d+\.\d\d)\] \t "
                      r"l1 : \[(-?\d+\.\d\d)\] \t time : \[(\d+\.\d\d)\]$")


def _cfg():
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
    cfg.target_batch = None
    cfg.batch_size = 2
    return cfg


def _model(cfg, dropout=0.1, precision="fp32", seed=5):
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref as R
    model = get_detr_model(cfg, include_top=True, num_encoder_layers=1, num_decoder_layers=2, dropout=dropout, precision=precision)
    model.load_weights(R.make_params(seed, num_enc=1, num_dec=2))
    return model


def _batches(n, seed=0, B=2, H=96, W=128):
    from oracle import set_loss_ref as L
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        tb, tc = L.make_targets(B, seed=100 + seed + i, force_full=False)
        out.append((rng.normal(size=(B, H, W, 3)).astype(np.float32), tb, tc))
    return out


def test_fit_console_global_step_and_oracle_loss(hip, capsys):
    """training.fit on a 3-batch iterable: one console line (step 0; the next would be step 100) in the reference's
    format (training.py:60), global_step advanced per batch, and the printed numbers are the oracle's first-step losses
    (dropout masks shared with the oracle)."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    from oracle import detr_ref as R, dropout_ref as DR, set_loss_ref as L
    cfg = _cfg()
    cfg.use_graph = False
    model = _model(cfg)
    opt = setup_optimizers(model, cfg)
    data = _batches(3)
    cfg.global_step = 7
    training.fit(model, data, opt, cfg, epoch_nb=4, class_names=[])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    m = TRAIN_LINE.match(lines[0])
    assert m, repr(lines[0])
    assert (int(m.group(1)), int(m.group(2))) == (4, 0)
    assert cfg.global_step == 10
    assert all(o.iterations == 3 for o in (opt["backbone_optimizer"], opt["transformers_optimizer"], opt["nlayers_optimizer"]))
    # the oracle on the first batch with the same weights and the same dropout masks (step 1 of this engine)
    params = R.make_params(5, num_enc=1, num_dec=2)
    seed1 = DR.step_seed(model.engine.dropout_seed, 1, 0)
    ref_out = R.detr_forward(torch.from_numpy(data[0][0]), R.to_torch(params), num_enc=1, num_dec=2, drop=DR.Dropper(0.1, seed1))
    _, ref_log = L.get_losses(ref_out, torch.from_numpy(data[0][1]), torch.from_numpy(data[0][2]), 91)
    for grp, key in ((3, "label_cost"), (4, "giou_loss"), (5, "l1_loss")):
        assert abs(float(m.group(grp)) - float(ref_log[key])) <= 0.011, (key, m.group(grp), float(ref_log[key]))


def test_eval_console_and_evaluation_step_break(hip, capsys):
    """training.eval (training.py:68-87): a line at validation steps 0, 10, 20..., stops after `evaluation_step` batches,
    never touches the parameters or global_step."""
    from detr_tf import training
    cfg = _cfg()
    model = _model(cfg)
    before = model.engine.P.flat.clone()
    one = _batches(1)[0]
    consumed = []

    def stream():
        for i in range(40):
            consumed.append(i)
            yield one

    training.eval(model, stream(), cfg, class_name=[], evaluation_step=12)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert [int(VAL_LINE.match(l).group(1)) for l in lines] == [0, 10], lines
    assert len(consumed) == 12 and cfg.global_step == 0
    assert torch.equal(before, model.engine.P.flat)
    assert lines[0].split("ce:")[1].split("time")[0] == lines[1].split("ce:")[1].split("time")[0]     # same batch, eval mode


def test_fit_gradient_accumulation_applies_every_target_batch(hip):
    """target_batch / batch_size = 2 (optimizers.py:137-163 through training.fit): parameters move after batches 1 and 3 only."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    cfg = _cfg()
    cfg.target_batch = 4
    cfg.use_graph = True               # accumulation falls back to the eager step
    model = _model(cfg, dropout=0.0)
    opt = setup_optimizers(model, cfg)
    snaps = []

    class Data:
        def __iter__(self):
            for b in _batches(4):
                snaps.append(model.engine.P.flat.clone())
                yield b

    training.fit(model, Data(), opt, cfg, epoch_nb=0, class_names=[])
    snaps.append(model.engine.P.flat.clone())
    moved = [not torch.equal(snaps[i], snaps[i + 1]) for i in range(4)]
    assert moved == [False, True, False, True], moved
    assert opt["backbone_optimizer"].iterations == 2


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replay_equals_eager_steps(hip, precision):
    """The hipGraph replay of the training step reproduces the eager step: with dropout 0.1 (new masks every step from the
    device-resident seed), Adam step sizes from device memory and the derived weight copies rebuilt inside the graph.
    Both models start every step from the SAME state (the eager model's parameters and Adam moments are copied over:
    the set-loss sums use fp32 atomics, and Hungarian matching of a near-degenerate random-init cost matrix amplifies that
    rounding noise into different assignments within a few steps), then the logits must agree to rounding, the loss to
    1e-5 and the parameter update in relative L2."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    data = _batches(5, seed=3)
    cfg_e, cfg_g = _cfg(), _cfg()
    m_e, m_g = _model(cfg_e, precision=precision), _model(cfg_g, precision=precision)
    o_e, o_g = setup_optimizers(m_e, cfg_e), setup_optimizers(m_g, cfg_g)
    stepper = training.GraphedTrainStep(m_g, o_g, cfg_g, eager_steps=1)
    losses = []
    for i, (im, tb, tc) in enumerate(data):
        for src, dst in ((m_e.engine.P.flat, m_g.engine.P.flat), (m_e.engine.P.adam_m, m_g.engine.P.adam_m),
                         (m_e.engine.P.adam_v, m_g.engine.P.adam_v)):
            dst.copy_(src)
        m_g.engine.bump_weights_version()
        before = m_e.engine.P.flat.clone()
        out_e, tot_e, log_e = training.train_step(m_e, im, tb, tc, o_e, cfg_e, i)
        lg_e = out_e["pred_logits"].clone()
        out_g, tot_g, log_g = stepper(im, tb, tc, i)
        lg_g = out_g["pred_logits"].clone()
        assert m_e.engine._drop == m_g.engine._drop and m_e.engine._drop[0] == pytest.approx(0.1)
        assert float((lg_e - lg_g).abs().max()) <= 1e-5 * float(lg_e.abs().max()), (i, float((lg_e - lg_g).abs().max()))
        assert abs(float(tot_e) - float(tot_g)) <= 1e-5 * abs(float(tot_e)), (i, float(tot_e), float(tot_g))
        assert abs(float(log_e["giou_loss_0"]) - float(log_g["giou_loss_0"])) <= 1e-5
        de, dg = m_e.engine.P.flat - before, m_g.engine.P.flat - before
        assert float((de - dg).norm()) <= 2e-2 * float(de.norm()), (i, float((de - dg).norm()) / float(de.norm()))
        losses.append(float(tot_g))
    assert stepper.step_graph is not None and len(stepper.step_graph.graphs) == 1 and stepper.calls == 5
    assert len(set(losses)) == 5 and losses[-1] < losses[0]      # five different batches / masks, and it trains


def test_graph_falls_back_on_new_shape_and_eval_sees_new_weights(hip):
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    cfg = _cfg()
    model = _model(cfg, dropout=0.0)
    opt = setup_optimizers(model, cfg)
    stepper = training.GraphedTrainStep(model, opt, cfg)
    a = _batches(3, seed=1)
    for i, (im, tb, tc) in enumerate(a):
        stepper(im, tb, tc, i)
    # eval after graph replays must use the updated parameters (derived copies are version-stamped)
    out_graph = model(a[0][0], training=False)["pred_logits"].clone()
    cfg2 = _cfg()
    m2 = _model(cfg2, dropout=0.0)
    o2 = setup_optimizers(m2, cfg2)
    for i, (im, tb, tc) in enumerate(a):
        training.train_step(m2, im, tb, tc, o2, cfg2, i)
    o_eager = m2(a[0][0], training=False)["pred_logits"]
    assert float((out_graph - o_eager).abs().max()) <= 1e-4 * float(o_eager.abs().max())
    m3 = _model(_cfg(), dropout=0.0)                     # the un-trained model is far away: eval really saw the new weights
    assert float((m3(a[0][0], training=False)["pred_logits"] - o_eager).abs().max()) > 1e-2 * float(o_eager.abs().max())
    # another image size: eager fallback, still a valid step
    b = _batches(1, seed=9, H=64, W=96)[0]
    before = model.engine.P.flat.clone()
    _, total, _ = stepper(b[0], b[1], b[2], 3)
    assert np.isfinite(float(total)) and not torch.equal(before, model.engine.P.flat)


def test_setup_optimizers_alone_keeps_derived_weights_fresh(hip):
    """a loop that calls gather_gradient / GroupAdam.apply_gradients directly (never run_train_step's
    bookkeeping) must still see the BN-folded / bf16 weight copies rebuilt after an apply."""
    from detr_tf.loss.loss import get_losses
    from detr_tf.optimizers import gather_gradient, setup_optimizers
    cfg = _cfg()
    model = _model(cfg, dropout=0.0, precision="bf16")
    opt = setup_optimizers(model, cfg)
    im, tb, tc = _batches(1)[0]
    out = model(im, training=True)
    total, log = get_losses(out, tb, tc, cfg)
    steps = gather_gradient(model, opt, total, out, cfg, log)
    l0 = float(total)
    cfg.backbone_lr = 1e-2          # rebinding the attribute (not .assign): must be picked up
    cfg.transformers_lr = 1e-2
    for name in ("backbone", "transformers", "nlayers"):
        opt[f"{name}_optimizer"].apply_gradients(model.engine.P.grad)
    assert opt["backbone_optimizer"].learning_rate() == pytest.approx(1e-2)
    out2 = model(im, training=True)
    total2, _ = get_losses(out2, tb, tc, cfg)
    # the big step changed every weight: with stale folded backbone kernels / bf16 shadow the loss would not move
    eng = model.engine
    w = eng.P.views["backbone/layer1/0/conv1/kernel"]
    ws16 = eng._bufs["ws16:backbone/layer1/0/conv1/kernel"].float()
    want = (w * eng.bn_scale["backbone/layer1/0/bn1"]).to(torch.bfloat16).float()
    assert torch.equal(ws16, want)
    assert abs(float(total2) - l0) > 1e-3 * abs(l0)


def test_eval_graph_survives_a_forward_of_another_shape(hip):
    """eval shapes A, A (recorded), B (eager: re-allocates every activation buffer), A again.  The recorded
    graph of A addresses freed buffers by then -- it must be dropped (engine.buf_generation), not replayed: the outputs of
    every A call equal a fresh eager model's."""
    cfg = _cfg()
    model = _model(cfg, dropout=0.0)
    ref = _model(_cfg(), dropout=0.0)
    ref.eval_graph = False
    a = torch.from_numpy(_batches(1, seed=2)[0][0]).cuda()
    b = torch.from_numpy(_batches(1, seed=3, H=64, W=160)[0][0]).cuda()
    want_a = ref(a, training=False)["pred_logits"].clone()
    want_b = ref(b, training=False)["pred_logits"].clone()
    seq = [(a, want_a), (a, want_a), (a, want_a), (b, want_b), (a, want_a), (a, want_a), (a, want_a), (b, want_b), (b, want_b), (a, want_a)]
    gens = []
    for i, (x, want) in enumerate(seq):
        got = model(x, training=False)["pred_logits"]
        gens.append(model.engine.buf_generation)
        assert torch.equal(got, want), (i, float((got - want).abs().max()))
    assert model._eval_graph is not None                      # the graph path was exercised ...
    assert gens[3] > gens[2] and gens[4] > gens[3]            # ... and the buffers really were re-allocated in between


def test_train_graph_is_rerecorded_after_an_eval_of_another_shape(hip):
    """ADVICE r2 (high), training side: graph steps at shape A, an eval forward at shape B (the engine re-allocates), graph
    steps at A again -- compared step by step with an eager model that sees the same sequence."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    cfg_g, cfg_e = _cfg(), _cfg()
    m_g, m_e = _model(cfg_g, dropout=0.0), _model(cfg_e, dropout=0.0)
    o_g, o_e = setup_optimizers(m_g, cfg_g), setup_optimizers(m_e, cfg_e)
    stepper = training.GraphedTrainStep(m_g, o_g, cfg_g)
    data = _batches(6, seed=11)
    other = torch.from_numpy(_batches(1, seed=12, H=64, W=160)[0][0]).cuda()
    kept = []
    for i, (im, tb, tc) in enumerate(data):
        if i == 3:
            assert stepper.step_graph is not None
            gen = m_g.engine.buf_generation
            ev_g = m_g(other, training=False)["pred_logits"]
            ev_e = m_e(other, training=False)["pred_logits"]
            assert m_g.engine.buf_generation > gen
            assert float((ev_g - ev_e).abs().max()) <= 1e-4 * float(ev_e.abs().max())
        # both models start every step from the same state (see test_graph_replay_equals_eager_steps)
        for src, dst in ((m_e.engine.P.flat, m_g.engine.P.flat), (m_e.engine.P.adam_m, m_g.engine.P.adam_m),
                         (m_e.engine.P.adam_v, m_g.engine.P.adam_v)):
            dst.copy_(src)
        m_g.engine.bump_weights_version()
        before = m_e.engine.P.flat.clone()
        _, tot_g, log_g = stepper(im, tb, tc, i)
        _, tot_e, log_e = training.train_step(m_e, im, tb, tc, o_e, cfg_e, i)
        kept.append((tot_g, log_g["label_cost"]))
        assert abs(float(tot_g) - float(tot_e)) <= 1e-5 * abs(float(tot_e)), (i, float(tot_g), float(tot_e))
        de, dg = m_e.engine.P.flat - before, m_g.engine.P.flat - before
        assert float((de - dg).norm()) <= 2e-2 * float(de.norm()), (i, float((de - dg).norm()) / float(de.norm()))
    assert stepper.step_graph is not None and stepper.calls == 3          # dropped at step 3, eager, re-recorded, replayed
    # every step hands out FRESH loss tensors -- a kept history is not N aliases of the last step
    vals = [float(t) for t, _ in kept]
    assert len(set(vals)) == len(vals) and len({t.data_ptr() for t, _ in kept}) == len(kept)


def test_auto_launch_probe_settles_and_check_matching_runs_eagerly(hip, capsys):
    """training.fit's default launch path ("auto"): eager step, recording pass, 3 timed replays, 3 timed eager steps, then ONE
    path for the rest of the run; `config.check_matching` (a host synchronisation inside the loss) never records a graph."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    cfg = _cfg()
    assert training._launch_mode(cfg) == "auto"
    model = _model(cfg, dropout=0.1)
    opt = setup_optimizers(model, cfg)
    one = _batches(1, seed=21)[0]
    training.fit(model, [one] * 10, opt, cfg, epoch_nb=0, class_names=[])
    st = opt["_graphed_step"]
    assert st.launch == "auto" and st.calls == 10 and st.settle_calls == 8
    assert st.probe is not None and st.choice in ("graph", "eager")
    assert st.probe["graph_ms"] > 0 and st.probe["eager_ms"] > 0
    assert (st.choice == "graph") == (st.probe["graph_ms"] <= st.probe["eager_ms"])
    assert opt["backbone_optimizer"].iterations == 10 and cfg.global_step == 10
    cfg2 = _cfg()
    cfg2.check_matching = True
    m2 = _model(cfg2, dropout=0.0)
    o2 = setup_optimizers(m2, cfg2)
    training.fit(m2, [one] * 4, o2, cfg2, epoch_nb=0, class_names=[])
    assert o2["_graphed_step"].step_graph is None and o2["backbone_optimizer"].iterations == 4


def test_auto_launch_decision_is_taken_once_per_stepper(hip):
    """the launch probe contains the stepper's only collective, so it must run on a schedule that a rank-local
    re-recording cannot restart: the decision is taken once (call 8) and survives a change of the step signature."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    cfg = _cfg()
    model = _model(cfg, dropout=0.1)
    opt = setup_optimizers(model, cfg)
    st = training.GraphedTrainStep(model, opt, cfg, launch="auto")
    a = _batches(1, seed=31)[0]
    b = _batches(1, seed=32, H=128, W=96)[0]
    for i in range(8):
        st(*a, i)
    first = (st.choice, dict(st.probe))
    assert st.total_calls == 8 and st.probe is not None
    for i in range(4):                 # a new shape: re-recorded (if the choice is "graph"), never re-probed
        st(*b, 8 + i)
    assert (st.choice, st.probe) == first and st.total_calls == 12
    # a stepper whose probe window is disturbed by a shape change still decides at call 8, and falls back to eager
    st2 = training.GraphedTrainStep(model, opt, cfg, launch="auto")
    for i in range(8):
        st2(*(a if i < 3 else b), i)
    assert st2.probe is not None and st2.choice in ("graph", "eager") and st2.total_calls == 8


def test_bf16_training_curve_tracks_the_fp32_curve(hip):
    """convergence evidence for the headline precision on CURRENT code.  The full six-layer model is trained
    for 100 steps on TWO fixed synthetic batches taken in turn (B = 4, 384x512, dropout 0.1) three times: exact fp32, precision="bf16"
    with the SAME dropout masks, and exact fp32 with ANOTHER dropout stream -- the yardstick: training on a fixed batch with
    Hungarian matching is chaotic (a flipped assignment moves the loss by a few %), so "bf16 tracks fp32" is stated relative to how
    far fp32 strays from itself.  Compared on 10-step window means (the two batches have different loss levels): all three curves
    must fall by more than 20 % (two batches in turn learn slower than one: 38.1 -> 28.5 measured); every window of the bf16 curve
    within 10 % of the fp32 window; over the second half the bf16 curve no further from fp32 than 1.5 x the fp32-vs-fp32 distance (or
    3 % of the loss, whichever is larger).  Measured (round 5): second-half mean |bf16 - fp32| = 0.58 against |fp32' - fp32| = 0.50 at a
    loss of 28.8; the largest window gap 3.4 %."""
    from detr_tf import training
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.optimizers import setup_optimizers
    from oracle.set_loss_ref import make_targets
    cfg = _cfg()
    cfg.batch_size = 4
    STEPS = 100
    batches = []
    for b in range(2):
        images = torch.from_numpy(np.random.default_rng(7 + b).normal(size=(4, 384, 512, 3)).astype(np.float32)).cuda()
        tb, tc = make_targets(4, seed=8 + b, force_full=False)
        batches.append((images, torch.from_numpy(tb).cuda(), torch.from_numpy(tc).cuda()))
    curves = {}
    for tag, prec, skip in (("fp32", "fp32", 0), ("bf16", "bf16", 0), ("fp32_other_masks", "fp32", 1000)):
        model = get_detr_model(cfg, include_top=True, device="cuda:0", seed=0, dropout=0.1, precision=prec)
        opt = setup_optimizers(model, cfg)
        model.engine._step_no += skip               # another dropout stream: same weights, same batches, other masks
        losses = []
        for i in range(STEPS):
            images, tb, tc = batches[i % 2]
            out, total, log, steps = training.run_train_step(model, images, tb, tc, opt, cfg)
            for name in steps:
                training.aggregate_grad_and_apply(name, opt, steps[name]["gradients"], i, cfg)
            losses.append(float(total))
        curves[tag] = np.array(losses)
        del model, opt
        torch.cuda.empty_cache()
    win = lambda c: c.reshape(-1, 10).mean(axis=1)            # 10 steps = 5 of each batch
    f, h, f2 = (win(curves[k]) for k in ("fp32", "bf16", "fp32_other_masks"))
    for k, v in curves.items():
        print(f"[train sanity] {k} (window means):", np.round(win(v), 3).tolist())
    for c in (f, h, f2):
        assert c[-1] < 0.8 * c[0], (c[0], c[-1])
    rel = np.abs(h - f) / np.abs(f)
    d_bf16, d_self = float(np.abs(h - f)[5:].mean()), float(np.abs(f2 - f)[5:].mean())
    print(f"[train sanity] max window |bf16 - fp32| / fp32 = {rel.max():.4f}; second-half mean |bf16 - fp32| = {d_bf16:.3f}, "
          f"|fp32' - fp32| = {d_self:.3f} at a loss of {float(f[5:].mean()):.2f}")
    # (the bounds of the one-batch version of this test, where they still hold -- the measured largest window gap is 3.4 %)
    assert rel.max() < 0.08, rel.round(4).tolist()
    assert d_bf16 <= max(1.25 * d_self, 0.02 * float(f[5:].mean())), (d_bf16, d_self)


def test_keep_bits_generated_one_step_ahead_are_the_bits_of_their_own_step(hip, monkeypatch):
    """Round 6: in bf16 mode the attention sites' dropout keep BITS of step t + 1 are generated during step t, next to the matcher
    (engine.DROPMASK_AHEAD = 2, eager launches).  They must be the bits the step would have generated for itself (= 0): same logits and
    same loss, bit for bit, over steps that include a change of the batch shape (the bits generated ahead for the old shape must be dropped)."""
    from detr_tf import engine as engine_mod, training
    from detr_tf.optimizers import setup_optimizers
    data = _batches(2, seed=9) + _batches(2, seed=10, H=64, W=96) + _batches(1, seed=11)
    runs = {}
    for mode in (0, 2):
        monkeypatch.setattr(engine_mod, "DROPMASK_AHEAD", mode)
        cfg = _cfg()
        model = _model(cfg, precision="bf16")
        opt = setup_optimizers(model, cfg)
        got = []
        for i, (im, tb, tc) in enumerate(data):
            out, tot, _ = training.train_step(model, im, tb, tc, opt, cfg, i)
            got.append((out["pred_logits"].clone(), float(tot)))
        assert model.engine.attn16 and model.engine._drop[0] == pytest.approx(0.1)
        runs[mode] = got
    for (lg0, t0), (lg2, t2) in zip(runs[0], runs[2]):
        assert torch.equal(lg0, lg2) and t0 == pytest.approx(t2, rel=1e-6)      # (the loss sums use fp32 atomics: last-ulp freedom)
    assert len({t for _, t in runs[2]}) == len(data)


# work queued on the engine's mask stream in front of every step of the test below: BALLAST_FILLS fills of BALLAST_FLOATS floats
BALLAST_FLOATS, BALLAST_FILLS = 1 << 28, 160


def test_keep_bits_generated_ahead_stay_ordered_behind_a_busy_mask_stream(hip, monkeypatch):
    """The same comparison (generation ahead at the matcher against generation at the head of the step: equal logits, every step)
    with the engine's mask stream kept busy: just before every step of the mode-2 run, fills of a 1 GiB tensor are queued on it that
    outlast the step, so whatever the generator launched there may still be waiting when the next step begins.
    advance_dropout_step() rewrites the device seed block that launch reads and must wait for it (streams.DropMasks.settle).
    Sizing, measured on an MI355X: one undisturbed eager step of this shape (bf16, 2 x 96 x 128, 1 + 2 layers) takes 6.39 ms
    between two events (median of 10, 6.28 ... 6.44), one fill 0.155 ms (50 fills: 7.75 ms); 160 fills = 24.8 ms = 3.9 steps.
    (The engine before DropMasks.settle passes this test as well: NOTEBOOK section 25 says why it cannot expose the missing order.)"""
    from detr_tf import engine as engine_mod, training
    from detr_tf.optimizers import setup_optimizers
    data = _batches(4, seed=9)
    runs = {}
    for mode in (0, 2):
        monkeypatch.setattr(engine_mod, "DROPMASK_AHEAD", mode)
        cfg = _cfg()
        model = _model(cfg, precision="bf16")
        opt = setup_optimizers(model, cfg)
        ballast = torch.empty(BALLAST_FLOATS, device=model.device) if mode == 2 else None
        got = []
        for i, (im, tb, tc) in enumerate(data):
            if mode == 2:
                with torch.cuda.stream(model.engine.masks.stream):
                    for _ in range(BALLAST_FILLS):
                        ballast.fill_(float(i))
            out, _, _ = training.train_step(model, im, tb, tc, opt, cfg, i)
            got.append(out["pred_logits"].clone())
        assert model.engine.attn16 and model.engine._drop[0] == pytest.approx(0.1)
        runs[mode] = got
    for lg0, lg2 in zip(runs[0], runs[2]):
        assert torch.equal(lg0, lg2)
