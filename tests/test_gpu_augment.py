"""csrc/augment.hip on the device: every stage-B kind x every final interpolation against the model of tests/augment_ref.py,
bit-exact anchors against DeviceInputStage.images, robustness to out-of-range records, and the COCO loader driving the
training step."""
import ctypes

import numpy as np
import pytest
import torch

import augment_ref as A
from test_augment_cpu import _Cfg, make_coco

KINDS = ("none", "resize", "crop", "affine")


def _stage(method, size):
    from detr_tf.data.processing import DeviceInputStage
    cfg = _Cfg(size=size)
    cfg.normalized_method = method
    return DeviceInputStage(cfg)


def _records(images, kind, interp, size):
    from detr_tf.data import transformation as T
    recs = []
    for i, im in enumerate(images):
        h0, w0 = im.shape[:2]
        hc, wc = T.crop_size(h0, w0, size)
        recs.append(T.Transform(h0, w0, flip=bool(i % 2), kind=T.KINDS[kind], ia=interp, iff=interp,
                                y0=(h0 - hc) // 3, x0=(w0 - wc) * 2 // 3, sx=[0.7, 1.3, 0.55][i % 3], sy=[1.25, 0.8, 1.45][i % 3]))
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("shapes,size", [(((37, 53), (480, 640), (120, 90)), (96, 128)), (((480, 640), (333, 517)), (200, 300))])
def test_augment_kernel_vs_model(hip, shapes, size):
    rng = np.random.default_rng(sum(size))
    images = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in shapes]
    for method in ("torch_resnet", "tf_resnet"):
        st = _stage(method, size)
        lut = st.lut.cpu().numpy()
        lvl = 1.0 / (255.0 * 0.224) if method == "torch_resnet" else 1.0
        for kind in KINDS:
            for interp in range(4):
                recs = _records(images, kind, interp, size)
                got = st.augmented(images, recs).cpu().numpy()
                ref = np.stack([A.normalise(A.augment_uint8(im, r, *size), lut.reshape(3, 256), st.perm) for im, r in zip(images, recs)])
                assert got.shape == ref.shape == (len(images),) + size + (3,)
                diff = np.abs(got - ref)
                assert float((diff > 1e-6).mean()) < 1e-3 and float(diff.max()) < 1.6 * lvl, \
                    (method, kind, A.NAMES[interp], float((diff > 1e-6).mean()), float(diff.max()))


@pytest.mark.gpu
def test_augment_bit_exact_anchors(hip):
    from detr_tf.data import transformation as T
    rng = np.random.default_rng(4)
    st = _stage("torch_resnet", (96, 128))
    img = rng.integers(0, 256, (150, 210, 3)).astype(np.uint8)
    plain = st.augmented([img], [T.Transform(150, 210)]).cpu().numpy()           # no flip, no stage B, final cubic
    assert np.array_equal(plain, st.images(img[None]).cpu().numpy())
    img = rng.integers(0, 256, (96, 128, 3)).astype(np.uint8)
    flipped = st.augmented([img], [T.Transform(96, 128, flip=True, iff=3)]).cpu().numpy()
    assert np.array_equal(flipped, st.images(np.ascontiguousarray(img[None, :, ::-1])).cpu().numpy())
    # a plain record (no flip, no stage B) in every interpolation detr_hip_input_stage has: one resample() serves both kernels
    from detr_tf.data.processing import INTERPOLATIONS
    small = rng.integers(0, 256, (37, 53, 3)).astype(np.uint8)
    same = rng.integers(0, 256, (64, 96, 3)).astype(np.uint8)
    for name in ("nearest", "linear", "cubic"):
        st2 = _stage("torch_resnet", (64, 96))
        st2.interpolation = INTERPOLATIONS[name]
        for im in (small, same):                                                    # 37 x 53 -> 64 x 96, and the identity
            got = st2.augmented([im], [T.Transform(*im.shape[:2], iff=INTERPOLATIONS[name])]).cpu().numpy()
            want = st2.images(im[None]).cpu().numpy()
            assert np.array_equal(got, want), (name, im.shape, int((got != want).sum()))
    # a batch mixing both gives the same images as one at a time
    both = st.augmented([np.zeros((150, 210, 3), np.uint8) + 9, img], [T.Transform(150, 210), T.Transform(96, 128, flip=True)])
    assert np.array_equal(both[1].cpu().numpy(), flipped[0])


@pytest.mark.gpu
def test_augment_out_of_range_records_stay_finite(hip):
    from detr_tf import _hip
    from detr_tf.data import transformation as T
    st = _stage("torch_resnet", (64, 80))
    rng = np.random.default_rng(9)
    images = [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((50, 70), (90, 40), (30, 30), (40, 60))]
    packed = np.concatenate([im.reshape(-1) for im in images])
    offs = np.cumsum([0] + [im.size for im in images[:-1]])
    recs = [T.Transform(50, 70, kind=2, y0=10 ** 6, x0=-5, iff=2),                     # crop window past the edge
            T.Transform(90, 40, kind=3, sx=1e30, sy=1e-30, iff=3),                     # huge / tiny zoom
            T.Transform(30000, 30000, kind=1, ia=3),                                   # source larger than the buffer
            T.Transform(40, 60, flip=True, kind=3, sx=1.0, sy=1.0, iff=7)]             # bad interpolation code
    irec, frec = T.pack_records(recs, offs)
    irec[3, 0] = -17                                                                   # negative offset
    src = torch.from_numpy(packed).cuda()
    ir, fr = torch.from_numpy(irec).cuda(), torch.from_numpy(frec).cuda()
    dst = torch.full((4, 64, 80, 3), float("nan"), device="cuda")
    perm = (ctypes.c_int32 * 3)(*st.perm)
    _hip._check(_hip.load().detr_hip_augment(src.data_ptr(), packed.size, ir.data_ptr(), fr.data_ptr(), 4, 64, 80, st.lut.data_ptr(),
                                             ctypes.cast(perm, ctypes.c_void_p), dst.data_ptr(), _hip._stream()), "detr_hip_augment")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dst).all())
    with pytest.raises(ValueError):
        st.augmented(images[:1], recs[:1])                                             # the host checks the records


def _coco_loader(tmp_path, seed):
    from detr_tf.data import load_coco_dataset
    from detr_tf.training_config import TrainingConfig
    tmp_path.mkdir(exist_ok=True)
    ann_file, img_dir = make_coco(tmp_path)
    cfg = TrainingConfig()
    cfg.image_size, cfg.target_batch = (96, 128), None
    cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
    ds, names = load_coco_dataset(cfg, 2, augmentation=True, ann_file=ann_file, img_dir=img_dir, seed=seed)
    return cfg, ds, names


@pytest.mark.gpu
def test_coco_loader_drives_training_steps(hip, tmp_path):
    from detr_tf import training
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.optimizers import setup_optimizers
    from oracle import detr_ref as R
    cfg, ds, names = _coco_loader(tmp_path / "a", 0)
    assert cfg.background_class == 8 and len(ds) == 3
    model = get_detr_model(cfg, include_top=True, num_encoder_layers=1, num_decoder_layers=1, dropout=0.0)
    model.load_weights(R.make_params(2, num_enc=1, num_dec=1))
    opt = setup_optimizers(model, cfg)
    it = iter(ds)
    for _ in range(2):
        images, t_bbox, t_class = next(it)
        assert tuple(images.shape) == (2, 96, 128, 3) and images.is_cuda and tuple(t_bbox.shape) == (2, 100, 4)
        n = t_bbox[:, 0, 0].cpu().numpy()
        assert (n >= 1).all()
        _, total, _, _ = training.run_train_step(model, images, t_bbox, t_class, opt, cfg)
        assert np.isfinite(float(total))
    # two loaders with the same seed: bit-identical batches
    _, ds2, _ = _coco_loader(tmp_path / "b", 0)
    _, ds3, _ = _coco_loader(tmp_path / "c", 0)
    b2, b3 = list(ds2), list(ds3)
    assert len(b2) == len(b3) >= 1
    for x, y in zip(b2, b3):
        for u, v in zip(x, y):
            assert torch.equal(u, v)


@pytest.mark.gpu
def test_loader_without_augmentation_native_and_padded(hip, tmp_path):
    from detr_tf.data import load_coco_dataset
    from detr_tf.data.processing import normalized_images
    from detr_tf.data.loader import decode_image
    ann_file, img_dir = make_coco(tmp_path)
    cfg = _Cfg()
    ds, _ = load_coco_dataset(cfg, 1, augmentation=None, ann_file=ann_file, img_dir=img_dir, seed=3)
    order = np.random.default_rng(3).permutation(len(ds.samples))
    images, t_bbox, _ = next(iter(ds))
    s = ds.samples[int(order[0])]
    host = decode_image(s.path)
    assert tuple(images.shape) == (1,) + host.shape
    assert np.array_equal(images[0].cpu().numpy(), normalized_images(host, cfg))
    np.testing.assert_array_equal(t_bbox[0, 1:1 + len(s.boxes)].cpu().numpy(), s.boxes)
    ds, _ = load_coco_dataset(cfg, 3, augmentation=None, ann_file=ann_file, img_dir=img_dir)
    (images, masks), t_bbox, t_class = next(iter(ds))
    assert images.shape[0] == 3 and masks.dtype == torch.bool and tuple(t_class.shape) == (3, 100, 1)
