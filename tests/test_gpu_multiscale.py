"""csrc/augment_padded.hip on the device: every interpolation x flip x window against the model of tests/augment_padded_ref.py,
bit-exact anchors against DeviceInputStage.images_padded and .augmented, padding / guard regions, clamping of out-of-range
records, and the loaders' "multiscale" / "shortest_side" modes driving eager and captured training steps and eval_model."""
import ctypes

import numpy as np
import pytest
import torch

import augment_padded_ref as P
from test_augment_cpu import _Cfg, make_coco

pytestmark = pytest.mark.gpu

DEV = "cuda"
# the reported total loss carries the set-loss sums' float-atomic last-bit noise run to run (test_gpu_padding.py: LOSS_NOISE)
LOSS_NOISE = 1e-6


def _stage(method="torch_resnet"):
    from detr_tf.data.processing import DeviceInputStage
    cfg = _Cfg()
    cfg.normalized_method = method
    return DeviceInputStage(cfg)


def test_augment_padded_kernel_vs_model(hip):
    """Acceptance rule of test_gpu_augment.py:50: share of elements differing by more than 1e-6 below 1e-3, maximum difference
    below 1.6 quantisation levels; masks and padding exact.  (test_multiscale_cpu.py holds the model alone to the same rule
    against a float64 restatement on the same inputs.)"""
    from detr_tf.data import transformation as T
    cases = list(P.kernel_cases(T))
    assert len({im.shape for _, images, _, _ in cases for im in images}) >= 6 and len({len(c[1]) for c in cases}) == 2
    for method in ("torch_resnet", "tf_resnet"):
        st = _stage(method)
        lut = st.lut.cpu().numpy()
        lvl = 1.0 / (255.0 * 0.224) if method == "torch_resnet" else 1.0
        for tag, images, recs, (H, W) in cases:
            got, gmask = st.augmented_padded(images, recs, canvas=(H, W))
            assert got.shape == (len(images), H, W, 3) and gmask.shape == (len(images), H, W) and gmask.dtype == torch.bool
            got, gmask = got.cpu().numpy(), gmask.cpu().numpy()
            ref, rmask = P.augment_padded(images, recs, H, W, lut, st.perm)
            assert np.array_equal(gmask, rmask), (method, tag)
            assert got[rmask].tobytes() == np.zeros((int(rmask.sum()), 3), np.float32).tobytes(), (method, tag)     # +0.0, not -0.0
            diff = np.abs(got - ref)
            share, mx = float((diff > 1e-6).mean()), float(diff.max())
            print(f"{method} {tag}: share {share:.2e} max {mx / lvl:.3f} levels")
            assert share < 1e-3 and mx < 1.6 * lvl, (method, tag, share, mx)


def test_anchor_identity_equals_images_padded(hip):
    """Full window, no flip, (hd, wd) = (h0, w0): the pixels and masks of images_padded on the same images, bit for bit."""
    from detr_tf.data import transformation as T
    rng = np.random.default_rng(3)
    sizes = [(37, 50), (64, 21), (5, 64), (48, 48)]
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    for method in ("torch_resnet", "tf_resnet"):
        st = _stage(method)
        for interp in range(4):
            recs = [T.PaddedRecord(h, w, False, 0, 0, h, w, h, w, interp) for h, w in sizes]
            x, m = st.augmented_padded(imgs, recs, multiple=1)
            x0, m0 = st.images_padded(imgs)
            assert x.shape == x0.shape == (4, 64, 64, 3)
            assert torch.equal(m, m0) and x.cpu().numpy().tobytes() == x0.cpu().numpy().tobytes()
            x, m = st.augmented_padded(imgs, recs, canvas=(70, 99))
            x0, m0 = st.images_padded(imgs, canvas=(70, 99))
            assert torch.equal(m, m0) and x.cpu().numpy().tobytes() == x0.cpu().numpy().tobytes()
    x, m = st.augmented_padded(imgs, recs)                        # canvas=None rounds up to multiples of 32
    assert x.shape == (4, 64, 64, 3)
    x, m = st.augmented_padded(imgs[:1], recs[:1])
    assert x.shape == (1, 64, 64, 3) and not m[0, :37, :50].any() and m[0, 37:].all() and m[0, :, 50:].all()
    with pytest.raises(ValueError, match="canvas"):
        st.augmented_padded(imgs, recs, canvas=(63, 64))
    with pytest.raises(ValueError):
        st.augmented_padded(imgs[:1], [recs[1]])                  # record of another image
    with pytest.raises(ValueError):
        st.augmented_padded(imgs[:1], [recs[0]._replace(wc=51)])


def test_anchor_full_canvas_equals_augmented(hip):
    """Full window, destination equal to the canvas: `augmented` with the plain Transform(h0, w0, iff=interp), mask all False."""
    from detr_tf.data import transformation as T
    from detr_tf.data.processing import DeviceInputStage
    rng = np.random.default_rng(4)
    sizes = [(150, 210), (37, 53), (96, 128), (333, 200)]
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    for size in ((96, 128), (75, 131)):                           # 75 x 131: the canvas the 16-byte stores do not fit
        st = DeviceInputStage(_Cfg(size=size))
        for interp in range(4):
            for flip in (False, True):
                want = st.augmented(imgs, [T.Transform(h, w, flip=flip, iff=interp) for h, w in sizes])
                got, m = st.augmented_padded(imgs, [T.PaddedRecord(h, w, flip, 0, 0, h, w, size[0], size[1], interp) for h, w in sizes],
                                             canvas=size)
                assert not bool(m.any())
                assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (size, interp, flip)


def _direct(st, packed, irec, B, H, W, dst, mask):
    from detr_tf import _hip
    perm = (ctypes.c_int32 * 3)(*st.perm)
    _hip._check(_hip.load().detr_hip_augment_padded(packed.data_ptr(), packed.numel(), irec.data_ptr(), B, H, W, st.lut.data_ptr(),
                                                    ctypes.cast(perm, ctypes.c_void_p), dst.data_ptr(), mask.data_ptr(), _hip._stream()),
                "detr_hip_augment_padded")


def test_padding_is_zero_and_guards_survive(hip):
    """dst and mask sit inside larger buffers filled with sentinels: the launch writes its canvas and nothing else, for aligned
    and unaligned placements (vector and scalar store paths) and for records far out of range, which are clamped, not trusted."""
    from detr_tf.data import transformation as T
    st = _stage()
    rng = np.random.default_rng(9)
    shapes = ((50, 70), (90, 40), (30, 30), (40, 60))
    images = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in shapes]
    packed = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(DEV)
    offs = np.cumsum([0] + [im.size for im in images[:-1]])
    good = [T.PaddedRecord(50, 70, True, 5, 6, 40, 60, 33, 47, 2), T.PaddedRecord(90, 40, False, 0, 0, 90, 40, 64, 28, 3),
            T.PaddedRecord(30, 30, False, 0, 0, 30, 30, 64, 80, 1), T.PaddedRecord(40, 60, True, 10, 10, 1, 1, 17, 80, 0)]
    wild = [T.PaddedRecord(50, 70, True, 10 ** 6, -5, 10 ** 6, 0, 10 ** 6, 10 ** 6, 2),       # window and destination past everything
            T.PaddedRecord(90, 40, False, -7, 39, -3, 500, -4, 12, 9),                        # negative sizes, bad interpolation code
            T.PaddedRecord(30000, 30000, False, 0, 0, 30000, 30000, 64, 80, 3),               # source larger than the buffer
            T.PaddedRecord(40, 60, True, 0, 0, 40, 60, 64, 80, 1)]
    B, G = 4, 4096
    for H, W, shift in ((64, 80, 0), (64, 80, 1), (61, 79, 0)):           # shift: mask placed 1 byte off a 4-byte boundary
        for recs, is_wild in ((good, False), (wild, True)):
            irec_h = T.pack_padded_records(recs, offs)
            if is_wild:
                irec_h[3, 0] = -17                                        # low offset word = 0xFFFFFFEF, high word 0: far beyond src_bytes
            irec = torch.from_numpy(irec_h).to(DEV)
            n = B * H * W
            fbuf = torch.full((G + n * 3 + G,), -7.25, dtype=torch.float32, device=DEV)
            mbuf = torch.full((G + n + G,), 0xAB, dtype=torch.uint8, device=DEV)
            dst = fbuf[G:G + n * 3].view(B, H, W, 3)
            mask = mbuf[G + shift:G + shift + n].view(B, H, W)
            _direct(st, packed, irec, B, H, W, dst, mask)
            torch.cuda.synchronize()
            assert bool((fbuf[:G] == -7.25).all()) and bool((fbuf[G + n * 3:] == -7.25).all())
            assert bool((mbuf[:G + shift] == 0xAB).all()) and bool((mbuf[G + shift + n:] == 0xAB).all())
            assert bool(torch.isfinite(dst).all()) and bool((mask <= 1).all())
            assert bool((dst[mask.bool()] == 0.0).all())
            hm = mask.cpu().numpy().astype(bool)
            if not is_wild and (H, W) == (64, 80):
                ref, rmask = P.augment_padded(images, recs, H, W, st.lut.cpu().numpy(), st.perm)
                assert np.array_equal(hm, rmask) and float(np.abs(dst.cpu().numpy() - ref).max()) < 1.6 / (255.0 * 0.224)
            if is_wild:
                assert not hm[0].any()                                    # destination clamped to the whole canvas
                assert hm[1].all()                                        # hd < 1: the whole canvas is padding
                assert not hm[2].any() and bool((dst[2] == dst[2, 0, 0]).all())      # one pixel at offset 0, everywhere
    with pytest.raises(ValueError):
        st.augmented_padded(images, wild[:2] + good[2:])                  # the host checks the records


# ------------------------------------------------------------------------------------------------------------------------------
# through the loaders
# ------------------------------------------------------------------------------------------------------------------------------
CANVAS = (160, 160)


def _loader(tmp_path, mode, batch=2, seed=0, canvas=CANVAS):
    from detr_tf.data import load_coco_dataset
    from detr_tf.training_config import TrainingConfig
    tmp_path.mkdir(exist_ok=True)
    ann_file, img_dir = make_coco(tmp_path)
    cfg = TrainingConfig()
    cfg.target_batch = None
    cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
    ds, names = load_coco_dataset(cfg, batch, augmentation=mode, ann_file=ann_file, img_dir=img_dir, seed=seed, scales=(96, 112, 128),
                                  max_size=160, canvas=canvas)
    return cfg, ds, names


def _model(cfg, precision="bf16"):
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref as R
    model = get_detr_model(cfg, include_top=True, num_encoder_layers=1, num_decoder_layers=1, dropout=0.0, precision=precision)
    assert not model.load_weights(R.make_params(2, num_enc=1, num_dec=1))
    return model


def _valid_extents(masks):
    """[(h, w)] of the top-left valid rectangle of every image; asserts the mask is exactly that rectangle."""
    out = []
    for m in masks.cpu().numpy():
        h, w = int((~m[:, 0]).sum()), int((~m[0]).sum())
        assert h >= 1 and w >= 1 and not m[:h, :w].any() and m[h:].all() and m[:, w:].all()
        out.append((h, w))
    return out


def test_multiscale_loader_yields_pairs_and_trains_eagerly(hip, tmp_path):
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    cfg, ds, _ = _loader(tmp_path / "a", "multiscale", canvas=None)
    assert cfg.background_class == 8 and len(ds) == 3
    model = _model(cfg)
    opt = setup_optimizers(model, cfg)
    seen = set()
    for (images, masks), t_bbox, t_class in ds:
        B, H, W, _ = images.shape
        assert B == 2 and H % 32 == 0 and W % 32 == 0 and max(H, W) <= 160 and images.is_cuda and images.dtype == torch.float32
        assert masks.dtype == torch.bool and tuple(masks.shape) == (B, H, W) and tuple(t_bbox.shape) == (2, 100, 4)
        ext = _valid_extents(masks)
        assert max(h for h, _ in ext) > H - 32 and max(w for _, w in ext) > W - 32          # the canvas hugs the largest image
        seen.update(ext)
        assert bool((images[masks] == 0).all())
        n = t_bbox[:, 0, 0].cpu().numpy()
        assert (n >= 1).all()
        boxes = t_bbox[:, 1:].cpu().numpy()
        assert (boxes >= 0).all() and (boxes[..., :2] + boxes[..., 2:] / 2 <= 1 + 1e-6).all()       # normalised per image
        _, total, _, _ = training.run_train_step(model, (images, masks), t_bbox, t_class, opt, cfg)      # masks pass the model's validation
        model.engine.check_mask_status()
        assert np.isfinite(float(total))
    assert len(seen) >= 4                                          # images of differing sizes
    # same seed: bit-identical batches
    _, ds2, _ = _loader(tmp_path / "b", "multiscale", seed=5)
    _, ds3, _ = _loader(tmp_path / "c", "multiscale", seed=5)
    b2, b3 = list(ds2), list(ds3)
    assert len(b2) == len(b3) >= 1
    for ((i2, m2), tb2, tc2), ((i3, m3), tb3, tc3) in zip(b2, b3):
        assert tuple(i2.shape) == (2,) + CANVAS + (3,)
        assert torch.equal(i2, i3) and torch.equal(m2, m3) and torch.equal(tb2, tb3) and torch.equal(tc2, tc3)


def test_multiscale_fixed_canvas_keeps_the_training_graph(hip, tmp_path):
    """Consecutive batches of differing image sizes on one fixed canvas replay ONE recording, and every replayed step equals the
    eager step on the same batch (test_graphed_train_step_with_masks_equals_eager's tolerance: parameters bit-identical, losses
    to the set loss's atomic noise)."""
    from detr_tf import training
    from detr_tf.optimizers import setup_optimizers
    cfg, ds, _ = _loader(tmp_path, "multiscale")
    batches = []
    for _ in range(4):                                             # (an epoch can yield fewer than len(ds) batches)
        batches += list(ds)
    batches = batches[:6]
    assert len(batches) >= 5
    extents = [tuple(_valid_extents(b[0][1])) for b in batches]
    assert len(set(extents)) == len(extents)                       # no two batches alike
    results = {}
    for launch in ("eager", "graph"):
        model = _model(cfg)
        opt = setup_optimizers(model, cfg)
        stepper = training.GraphedTrainStep(model, opt, cfg, eager_steps=1, launch=launch)
        losses, recorded = [], None
        for i, ((images, masks), t_bbox, t_class) in enumerate(batches):
            _, total, _ = stepper((images, masks), t_bbox, t_class, i)
            losses.append(float(total))
            if launch == "graph" and i >= 1:
                assert stepper.step_graph is not None
                if recorded is None:
                    recorded = stepper.step_graph
                assert stepper.step_graph is recorded, f"the recording was dropped at batch {i}"
        torch.cuda.synchronize()
        model.engine.check_mask_status()
        results[launch] = (losses, {n: v.detach().clone() for n, v in model.engine.P.views.items()})
    assert all(np.isfinite(results["graph"][0]))
    for n, v in results["eager"][1].items():
        assert torch.equal(v, results["graph"][1][n]), n
    for a, b in zip(*[results[k][0] for k in ("eager", "graph")]):
        assert abs(a - b) <= LOSS_NOISE * abs(a), results


def test_shortest_side_loader_feeds_eval_model(hip, tmp_path):
    from detr_tf.data import transformation as T
    from detr_tf.evaluation import eval_model
    cfg, ds, _ = _loader(tmp_path, "shortest_side")
    batches = list(ds)
    assert len(batches) == 3
    for (images, masks), t_bbox, _ in batches:
        assert tuple(images.shape) == (2,) + CANVAS + (3,)
        for h, w in _valid_extents(masks):
            assert (min(h, w) == 128 or max(h, w) == 160) and max(h, w) <= 160
    sizes = _valid_extents(torch.cat([b[0][1] for b in batches]))
    assert len(set(sizes)) == 6 and set(sizes) <= {T.target_size(40 + 7 * i, 60 + 5 * i, 128, 160) for i in range(7)}
    cfg.background_class = 91                                      # the model has 92 logits: score every class it can predict
    names = [f"c{i}" for i in range(92)]
    for graph in (False, True):
        model = _model(cfg)
        model.eval_graph = graph
        host = eval_model(model, cfg, names, iter(batches), print_result=False)
        device = eval_model(model, cfg, names, iter(batches), print_result=False, accumulate="device")
        assert device == host
        if graph:
            assert model._eval_graph is not None and model._eval_graph["key"][-1] is True       # one masked recording, replayed


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_batch_isolation_through_the_padded_path(hip, precision):
    """Changing another image of the batch (its pixels, its record, its extent) leaves image 0's outputs bit-identical."""
    from detr_tf.data import transformation as T
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    model = _model(cfg, precision)
    model.eval_graph = False
    st = _stage()
    rng = np.random.default_rng(11)
    a, b, c = (rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((90, 120), (77, 50), (60, 140)))
    ra = T.PaddedRecord(90, 120, True, 10, 20, 70, 90, 112, 144, 1)
    rb = T.PaddedRecord(77, 50, False, 0, 0, 77, 50, 154, 100, 2)
    base_in = st.augmented_padded([a, b], [ra, rb], canvas=CANVAS)
    base = model(base_in)
    lg0, bx0 = base["pred_logits"][0].clone(), base["pred_boxes"][0].clone()
    others = [(c, T.PaddedRecord(60, 140, False, 0, 0, 60, 140, 68, 160, 3)),          # another image
              (b, rb._replace(flip=True)),                                             # same image, other pixels
              (b, rb._replace(hd=96, wd=62))]                                          # same image, other extent
    for img, rec in others:
        x, m = st.augmented_padded([a, img], [ra, rec], canvas=CANVAS)
        assert torch.equal(x[0], base_in[0][0]) and torch.equal(m[0], base_in[1][0])
        out = model((x, m))
        assert torch.equal(out["pred_logits"][0], lg0) and torch.equal(out["pred_boxes"][0], bx0)
        assert not torch.equal(out["pred_logits"][1], base["pred_logits"][1])
