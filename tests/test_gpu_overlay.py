"""detr_hip_overlay on the GPU against its NumPy restatement (tests/overlay_ref.py), byte for byte: ragged batches with unaligned
sources and canaries round the outputs, every box / label / blending / heat-map edge of include/detr_hip.h: detr_overlay_desc, the
LDS command list's capacity, in-place and repeated runs, and the public interface end to end on a small model."""
import ctypes

import numpy as np
import pytest
import torch

import overlay_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
FRAMES = ((1, 1), (7, 5), (33, 65), (97, 130))
CANARY = 0xA5


def _font():
    from detr_tf import overlay as O
    return O.font_atlas(), (ord("0") - 32, ord(":") - 32, ord(".") - 32)


def _names(words):
    from detr_tf import overlay as O
    return [O.encode_text(w) for w in words]


WORDS = ("cat", "a", "person", "traffic light", "", "Zebra_9")


def _frames(seed=0, sizes=FRAMES):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in sizes]


def _pack(rows, D=None):
    """per image (boxes [k, 4], labels [k], scores [k]) -> boxes [B, D, 4], labels [B, D], scores [B, D], counts [B]"""
    D = D or max(1, max(len(r[0]) for r in rows))
    B = len(rows)
    boxes, labels, scores = np.zeros((B, D, 4), F), np.zeros((B, D), np.int64), np.zeros((B, D), F)
    for b, (bx, lb, sc) in enumerate(rows):
        k = len(bx)
        boxes[b, :k], labels[b, :k], scores[b, :k] = np.asarray(bx, F).reshape(-1, 4), lb, sc
    return boxes, labels, scores, np.array([len(r[0]) for r in rows], np.int32)


def run(hip, images, boxes, labels, scores, counts, *, names=None, colors=None, atlas=None, glyphs=None, thickness=2, scales=None,
        label_alpha=255, fill_alpha=0, heat=None, map_step=None, map_valid=None, map_scale=None, lut=None, heat_alpha=160, inplace=False,
        compare=True):
    """One call of the C entry point on a source packed at unaligned offsets and a destination with canary bytes round its 16-byte
    aligned images; returns (the drawn images, the status word) after checking the canaries and, with `compare`, the restatement."""
    from detr_tf import overlay as O
    lib, dev = hip.load(), torch.device("cuda:0")
    font, fglyphs = _font()
    atlas = font if atlas is None else atlas
    glyphs = fglyphs if glyphs is None else glyphs
    names = _names(WORDS) if names is None else names
    colors = O.class_palette(7) if colors is None else colors
    B, D = boxes.shape[:2]
    sizes = np.array([im.shape[:2] for im in images], np.int32)
    scales = np.array([1] * B if scales is None else scales, np.int32)
    nbytes = [im.size for im in images]
    # destination: canary, image at a multiple of 16, canary ...
    dst_off, at = [], 16
    for n in nbytes:
        dst_off.append(at)
        at = (at + n + 15) // 16 * 16 + 16
    dst_h = np.full(at, CANARY, np.uint8)
    if inplace:
        for im, o in zip(images, dst_off):
            dst_h[o:o + im.size] = im.reshape(-1)
        dst = src = torch.from_numpy(dst_h).to(dev)
        src_off = list(dst_off)
    else:
        src_off, at = [], 1                                         # odd offsets, odd gaps: every alignment of a source image occurs
        for i, n in enumerate(nbytes):
            src_off.append(at)
            at += n + (1, 2, 3, 5)[i % 4]
        src_h = np.full(at + 8, 0x3C, np.uint8)
        for im, o in zip(images, src_off):
            src_h[o:o + im.size] = im.reshape(-1)
        src, dst = torch.from_numpy(src_h).to(dev), torch.from_numpy(dst_h).to(dev)
    cap = max(1, max((len(n) for n in names), default=1))
    table = np.zeros((max(len(names), 1), cap), np.uint8)
    for i, n in enumerate(names):
        table[i, :len(n)] = n
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = dict(src_off=up(np.array(src_off, np.int64)), dst_off=up(np.array(dst_off, np.int64)), sizes=up(sizes), boxes=up(boxes), labels=up(labels),
             counts=up(np.asarray(counts, np.int32)), colors=up(colors), names=up(table), name_len=up(np.array([len(n) for n in names] or [0], np.int32)),
             atlas=up(atlas), scale=up(scales))
    if scores is not None:
        t["scores"] = up(scores)
    d = hip.OverlayDesc()
    d.B, d.D = B, D
    d.src, d.dst, d.sizes_host = src.data_ptr(), dst.data_ptr(), sizes.ctypes.data
    for k, v in t.items():
        setattr(d, k, v.data_ptr())
    if not names:
        d.names = d.name_len = None
    d.thickness, d.label_alpha, d.fill_alpha, d.heat_alpha = thickness, label_alpha, fill_alpha, heat_alpha
    d.n_colors, d.n_names, d.name_cap = len(colors), len(names), cap
    d.n_glyph, d.gh, d.gw = atlas.shape
    d.glyph_digit0, d.glyph_colon, d.glyph_dot = glyphs
    if heat is not None:
        ht = heat if isinstance(heat, torch.Tensor) else up(heat)
        t.update(heat=ht, map_step=up(np.asarray(map_step, F)), map_valid=up(np.asarray(map_valid, np.int32)), map_scale=up(np.asarray(map_scale, F)), lut=up(lut))
        d.heat, d.sH_b, d.sH_y, d.sH_x, d.Hf, d.Wf = ht.data_ptr(), ht.stride(0), ht.stride(1), ht.stride(2), ht.shape[1], ht.shape[2]
        d.map_step, d.map_valid, d.map_scale, d.lut = (t[k].data_ptr() for k in ("map_step", "map_valid", "map_scale", "lut"))
    need = lib.detr_hip_workspace_bytes_overlay(ctypes.byref(d))
    assert need > 0
    ws = torch.full((need + 64,), 0x77, dtype=torch.uint8, device=dev)           # its tail is a canary too
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    d.workspace, d.workspace_bytes, d.status = ws.data_ptr(), need, status.data_ptr()
    hip._check(lib.detr_hip_overlay(ctypes.byref(d), hip._stream()), "detr_hip_overlay")
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (ws[need:].cpu().numpy() == 0x77).all()
    outside = np.ones(got.shape, bool)
    out = []
    for (h, w), o in zip(sizes.tolist(), dst_off):
        outside[o:o + h * w * 3] = False
        out.append(got[o:o + h * w * 3].reshape(h, w, 3).copy())
    assert (got[outside] == CANARY).all(), "bytes outside the output images were written"
    if compare:
        hm = None if heat is None else (heat.cpu().numpy() if isinstance(heat, torch.Tensor) else heat)
        want = R.draw_batch(images, boxes, labels, scores, counts, scales=scales, names=names, colors=colors, atlas=atlas, glyphs=glyphs,
                            thickness=thickness, label_alpha=label_alpha, fill_alpha=fill_alpha, heat=hm, map_step=map_step, map_valid=map_valid,
                            map_scale=map_scale, lut=lut, heat_alpha=heat_alpha)
        for b, (g, w) in enumerate(zip(out, want)):
            bad = np.argwhere((g != w).any(-1))
            assert bad.size == 0, f"image {b} {g.shape}: {len(bad)} pixels differ, first (y, x) = {bad[0].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"
    return out, int(status.item())


def geometry_rows(H, W, rng):
    nan, inf = float("nan"), float("inf")
    boxes = [
        [0, 0, W, H],                                               # the full image
        [10.2, 5, 10.9, 20],                                        # x1 == x2
        [20, 30, 22.5, 60],                                         # thinner than 2 * thickness
        [-5, 10, 8, 20], [W - 6, 10, W + 9, 25], [30, -7, 50, 6], [30, H - 5, 60, H + 10],      # cut by each border
        [-50, -50, -20, -10], [W + 10, H + 10, W + 50, H + 60], [-1e9, 3, 1e9, 9.5],           # unclipped corners outside the image
        [nan, 1, 5, 5], [1, 1, inf, 5], [-inf, 2, 7, 9], [3, nan, 9, nan],                      # skipped
        [50, 10, 40, 20], [5, 30, 25, 29.5],                        # x1 < x0, y1 < y0: skipped
        [8, 8, 28, 18],                                             # (label -1 below: skipped)
        [40, 40, 60, 50], [45, 42, 65, 52],                         # equal areas: the lower index is painted first
        [10, 10, 90, 80], [30, 30, 50, 45],                         # a small box nested in a large one
    ]
    labels = np.array([i % 9 for i in range(len(boxes))], np.int64)          # 6..8 lie beyond the six names
    labels[16] = -1
    scores = rng.random(len(boxes)).astype(F)
    return boxes, labels, scores


@pytest.mark.parametrize("scored", [True, False])
@pytest.mark.parametrize("thickness", [1, 2, 3])
def test_ragged_batch_box_geometry(hip, scored, thickness):
    rng = np.random.default_rng(1)
    images = _frames(1)
    boxes, labels, scores, counts = _pack([geometry_rows(h, w, rng) for h, w in FRAMES])
    out, status = run(hip, images, boxes, labels, scores if scored else None, counts, thickness=thickness, scales=[1, 1, 2, 1])
    assert status == 0
    assert any((o != im).any() for o, im in zip(out, images))


def test_zero_counts_reproduce_the_input_and_bad_counts_are_flagged(hip):
    rng = np.random.default_rng(2)
    images = _frames(2)
    boxes, labels, scores, counts = _pack([geometry_rows(h, w, rng) for h, w in FRAMES])
    out, status = run(hip, images, boxes, labels, scores, np.zeros(4, np.int32))
    assert status == 0 and all((o == im).all() for o, im in zip(out, images))
    D = boxes.shape[1]
    out, status = run(hip, images, boxes, labels, scores, np.array([-3, D + 5, 2, 0], np.int32))        # clamped to 0, D, 2, 0
    assert status == 1 and list(hip.OVERLAY_BAD) == [1]                                                 # DETR_OVERLAY_BAD_COUNT
    assert (out[0] == images[0]).all() and (out[3] == images[3]).all() and (out[1] != images[1]).any()


def test_labels(hip):
    rng = np.random.default_rng(3)
    images = _frames(3)
    names = _names(("cat", "a rather long class name", "exactly12chr", "", "dog"))
    assert max(len(n) for n in names) == 24
    rows = []
    for h, w in FRAMES:
        boxes = [[5, 5, 40, 30],                                    # label 1: wider than the 65-pixel frame at scale 2
                 [w - 12, h - 9, w - 2, h - 1],                     # at the bottom right: the label shifts inwards
                 [20, 50, 100, 90],                                 # label 2: a name of name_cap ... (see the second call)
                 [60, 10, 110, 40], [2, 60, 50, 95],                # labels 5, 77: beyond class_names
                 [30, 20, 70, 70]]                                  # label 3: the empty name
        rows.append((boxes, np.array([1, 0, 2, 5, 77, 3], np.int64), rng.random(6).astype(F)))
    boxes, labels, scores, counts = _pack(rows)
    for scales in ([1, 2, 3, 2], [3, 1, 2, 1]):
        run(hip, images, boxes, labels, scores, counts, names=names, scales=scales)
        run(hip, images, boxes, labels, None, counts, names=names, scales=scales)          # scores=None: unnamed labels draw no rectangle
    short = _names(("cat", "a", "exactly12chr"))                    # name_cap == 12 == the longest name
    run(hip, images, boxes, labels, scores, counts, names=short, scales=[1, 1, 1, 2])
    run(hip, images, boxes, labels, scores, counts, names=[], scales=[1, 1, 1, 2])         # no names at all: n_names == 0, null tables
    # scores the text rule meets at its edges: ties, 0, 1, beyond the clamp, NaN, negative
    scores[:, :6] = np.array([0.125, 0.995, 1.0, 12.5, np.nan, -0.3], F)
    run(hip, images, boxes, labels, scores, counts, names=names, scales=[1, 2, 1, 1])


def test_random_atlas(hip):
    rng = np.random.default_rng(4)
    atlas = (rng.random((40, 5, 8)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (40, 5, 8)).astype(np.uint8)      # gh = 5, gw = 8; ink = non-zero
    names = [list(rng.integers(0, 60, n)) for n in (3, 7, 1)]       # indices >= 40 draw nothing
    images = _frames(4)
    rows = [([[4, 4, 60, 30], [50, 40, 120, 90], [10, 50, 30, 60]], np.array([0, 1, 2], np.int64), rng.random(3).astype(F)) for _ in FRAMES]
    boxes, labels, scores, counts = _pack(rows)
    run(hip, images, boxes, labels, scores, counts, names=names, atlas=atlas, glyphs=(3, 20, 45), scales=[1, 2, 1, 3])    # the dot's glyph is beyond the atlas


@pytest.mark.parametrize("label_alpha", [0, 128, 255])
def test_label_alpha(hip, label_alpha):
    rng = np.random.default_rng(5)
    images = _frames(5)
    boxes, labels, scores, counts = _pack([geometry_rows(h, w, rng) for h, w in FRAMES])
    run(hip, images, boxes, labels, scores, counts, label_alpha=label_alpha)


def test_fill_alpha_on_overlapping_boxes(hip):
    rng = np.random.default_rng(6)
    images = _frames(6)
    rows = [([[10, 10, 70, 60], [30, 20, 100, 80], [20, 40, 90, 95]], np.array([0, 1, 2], np.int64), rng.random(3).astype(F)) for _ in FRAMES]
    boxes, labels, scores, counts = _pack(rows)
    run(hip, images, boxes, labels, scores, counts, fill_alpha=64)
    run(hip, images, boxes, labels, scores, counts, fill_alpha=64, label_alpha=100, thickness=1)


@pytest.mark.parametrize("fill_alpha", [0, 64])
def test_wide_frames_runs_inside_a_box(hip, fill_alpha):
    """Frames wider than a wave's run of 256 pixels: whole runs lie inside a box's outline, where the raster kernel skips the box
    (without a tint) -- but not the labels and boxes nested there."""
    rng = np.random.default_rng(12)
    sizes = ((3, 700), (40, 300), (5, 1100))
    images = _frames(12, sizes)
    rows = []
    for h, w in sizes:
        boxes = [[2, 0, w - 3, h - 1], [0, 0, w, h], [300.5, 1, 420, h - 2], [30, 0, 290, h], [w - 280, 1, w - 8, h - 1]]
        rows.append((boxes, np.array([0, 1, 2, 7, 3], np.int64), rng.random(5).astype(F)))
    boxes, labels, scores, counts = _pack(rows)
    for thickness in (1, 2):
        run(hip, images, boxes, labels, scores, counts, thickness=thickness, fill_alpha=fill_alpha, label_alpha=200)


def test_more_boxes_on_a_tile_than_the_lds_list_holds(hip):
    """300 boxes that all contain rows 16..31 of a 64 x 64 frame -- one tile of the raster kernel, whose LDS lists hold 64 commands per
    wave: the tile is processed in chunks, and with a tint the order of every one of them shows."""
    rng = np.random.default_rng(7)
    n = 300
    x0, y0 = rng.integers(0, 20, n), rng.integers(0, 14, n)
    x1, y1 = rng.integers(40, 64, n), rng.integers(34, 64, n)
    boxes = np.stack([x0, y0, x1, y1], 1).astype(F) + rng.random((n, 4)).astype(F)
    rows = [(boxes, rng.integers(0, 9, n), rng.random(n).astype(F))]
    images = _frames(7, ((64, 64),))
    b, lb, sc, counts = _pack(rows)
    run(hip, images, b, lb, sc, counts, fill_alpha=32, label_alpha=90, thickness=1)


def test_d_2048_and_beyond(hip):
    rng = np.random.default_rng(8)
    n = hip.TILE_MAX_CAND
    assert n == 2048
    x0, y0 = rng.uniform(-5, 125, n), rng.uniform(-5, 92, n)
    boxes = np.stack([x0, y0, x0 + rng.uniform(0, 40, n), y0 + rng.uniform(0, 30, n)], 1).astype(F)
    rows = [(boxes, rng.integers(0, 12, n), rng.random(n).astype(F)), (boxes[:5], np.arange(5), rng.random(5).astype(F))]
    images = _frames(8, ((97, 130), (33, 65)))
    b, lb, sc, counts = _pack(rows)
    assert b.shape[1] == 2048
    run(hip, images, b, lb, sc, counts, fill_alpha=20)
    from detr_tf.inference import draw_detections
    with pytest.raises(ValueError, match="2049"):
        draw_detections([images[0]], [(np.zeros((2049, 4), F), np.zeros(2049, np.int64), None)])
    d = hip.OverlayDesc()
    d.B, d.D, d.name_cap = 1, 2049, 4
    assert hip.load().detr_hip_workspace_bytes_overlay(ctypes.byref(d)) < 0 and hip.load().detr_hip_overlay(ctypes.byref(d), None) < 0
    assert "bad shape" in hip.load().detr_hip_last_error().decode()


@pytest.mark.parametrize("Hf,Wf", [(1, 1), (2, 3), (25, 38)])
@pytest.mark.parametrize("heat_alpha", [0, 160, 255])
def test_heat_map(hip, Hf, Wf, heat_alpha):
    from detr_tf import overlay as O
    rng = np.random.default_rng(9)
    images = _frames(9)
    heat = rng.random((4, Hf, 2 * Wf)).astype(F)
    heat[1] *= 3.0                                                  # values above 1 after the scale: clamped
    heat[2] = 0.0                                                   # an all-zero map: the bytes of the plain drawing
    heat[3, Hf // 2, 2 * (Wf // 2)] = np.nan                        # a NaN cell: 0 wherever it is a tap
    heat_d = torch.from_numpy(heat).cuda()[:, :, ::2]               # strided in x
    extent = np.array([[Hf, Wf], [Hf * 0.63, Wf * 0.81], [Hf, Wf * 0.5], [max(1.0, Hf - 0.4), max(1.0, Wf - 1.7)]])      # fractional; part of the canvas
    sizes = np.array(FRAMES, np.float64)
    step = (extent / sizes).astype(F)
    valid = np.minimum(np.ceil(extent), [Hf, Wf]).astype(np.int32)
    gstep, gvalid = O.heat_geometry(extent, FRAMES, Hf, Wf)
    assert gstep.tobytes() == step.tobytes() and (gvalid == valid).all()
    mscale = np.array([1.0, 0.7, 1.0, 1.3], F)
    boxes, labels, scores, counts = _pack([geometry_rows(h, w, rng) for h, w in FRAMES])
    kw = dict(heat=heat_d, map_step=step, map_valid=valid, map_scale=mscale, lut=O.heat_colormap(), heat_alpha=heat_alpha)
    out, _ = run(hip, images, boxes, labels, scores, counts, **kw)
    plain, _ = run(hip, images, boxes, labels, scores, counts, compare=False)
    bare, _ = run(hip, images, boxes, labels, scores, np.zeros(4, np.int32), **kw)          # the heat map alone
    assert (out[2] == plain[2]).all() and (bare[2] == images[2]).all()
    if heat_alpha == 0:
        assert all((o == p).all() for o, p in zip(out, plain)) and all((o == p).all() for o, p in zip(bare, images))
    else:
        # image 3 covers 1 x 1 / 2 x 2 cells of the two small maps and the NaN cell is one of them: it is a tap of EVERY pixel (the
        # second tap is clamped onto it), and a tap of weight 0 still makes the sum NaN -> 0: nothing is drawn.  On the 25 x 38 map
        # only the pixels round cell (12, 19) go to 0.
        some = (Hf, Wf) == (25, 38)
        assert (bare[0] != images[0]).any() and (bare[1] != images[1]).any()
        assert (bare[3] != images[3]).any() == some and (out[3] != plain[3]).any() == some


def test_in_place_and_repeatable(hip):
    from detr_tf import overlay as O
    rng = np.random.default_rng(10)
    images = _frames(10)
    boxes, labels, scores, counts = _pack([geometry_rows(h, w, rng) for h, w in FRAMES])
    heat = rng.random((4, 5, 7)).astype(F)
    step = (np.array([[5, 7]] * 4) / np.array(FRAMES, np.float64)).astype(F)
    kw = dict(heat=heat, map_step=step, map_valid=np.array([[5, 7]] * 4, np.int32), map_scale=np.ones(4, F), lut=O.heat_colormap(), fill_alpha=40,
              label_alpha=200, scales=[1, 1, 2, 1])
    a, _ = run(hip, images, boxes, labels, scores, counts, **kw)
    b, _ = run(hip, images, boxes, labels, scores, counts, compare=False, **kw)
    c, _ = run(hip, images, boxes, labels, scores, counts, compare=False, inplace=True, **kw)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


# ---- the public interface, end to end ------------------------------------------------------------------------------------------------
def _config():
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.image_size = (64, 96)
    return cfg


@pytest.fixture(scope="module")
def model(hip):
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref as Rf
    m = get_detr_model(_config(), include_top=True, num_encoder_layers=1, num_decoder_layers=1, dropout=0.0)
    assert not m.load_weights(Rf.make_params(2, num_enc=1, num_dec=1))
    return m


NAMES = [f"class{i}" for i in range(40)]                              # labels above 39 are drawn with their score alone


def _e2e_images():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((96, 128), (120, 80))]


def _ref(images, dets, heat=None, **kw):
    from detr_tf import overlay as O
    font, glyphs = _font()
    out = []
    for b, (im, d) in enumerate(zip(images, dets)):
        h = {} if heat is None else {k: v[b] for k, v in heat.items() if k != "lut"}
        if heat is not None:
            h["lut"] = heat["lut"]
        out.append(R.draw_image(im, d.boxes.cpu().numpy(), d.labels.cpu().numpy(), d.scores.cpu().numpy(), names=_names(NAMES),
                                colors=O.class_palette(100), atlas=font, glyphs=glyphs, thickness=2, scale=max(1, (im.shape[0] + 250) // 500), **h, **kw))
    return out


def _equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == w.shape and g.data_ptr() % 16 == 0
        assert (g.cpu().numpy() == w).all()


def test_detector_draw_end_to_end(hip, model):
    from detr_tf import overlay as O
    from detr_tf.data import transformation as T
    from detr_tf.inference import Detector
    cfg, imgs = _config(), _e2e_images()
    det = Detector(model, cfg, score_threshold=0.0, max_detections=20, shortest_side=64, max_size=96, canvas=(96, 96))
    dets = det(imgs)
    assert all(d.scores.shape[0] >= 1 for d in dets)
    want = _ref(imgs, dets)
    assert any((w != im).any() for w, im in zip(want, imgs))
    _equal(det.draw(imgs, dets, NAMES), want)
    _equal(det.draw(None, dets, NAMES), want)                        # the frames of the last call, still on the device
    _equal(det.draw([torch.from_numpy(im).cuda() for im in imgs], dets, NAMES), want)      # device tensors: used where they are
    assert (det.draw(imgs[1], dets[1], NAMES).cpu().numpy() == want[1]).all()              # one image in, one tensor out
    # with the attention maps of the same call
    dets2, maps = det(imgs, need_weights=True)
    site = model.default_attn_sites()[-1]
    m = maps[site]
    heat = torch.stack([m[b].index_select(0, d.query.to(torch.int64)).sum(0) for b, d in enumerate(dets2)]).float()
    peak = heat.amax(dim=(1, 2))
    scale = torch.where(peak > 0, 1.0 / peak, torch.zeros_like(peak))
    recs = [T.eval_record(96, 128, 64, 96, T.CUBIC), T.eval_record(120, 80, 64, 96, T.CUBIC)]
    extent = np.array([(r.hd / 32, r.wd / 32) for r in recs])         # 64 x 85 and 96 x 64 pixels of the 96 x 96 canvas, stride 32
    assert tuple(m.shape[-2:]) == (3, 3) and extent.tolist() == [[2.0, 85 / 32], [3.0, 2.0]]
    sizes = np.array([(96, 128), (120, 80)], np.float64)
    hk = dict(heat=heat.cpu().numpy(), map_step=(extent / sizes).astype(F), map_valid=np.ceil(extent).astype(np.int32), map_scale=scale.cpu().numpy(),
              lut=O.heat_colormap())
    want2 = _ref(imgs, dets2, heat=hk, heat_alpha=160)
    assert any((a != b).any() for a, b in zip(want2, want))
    _equal(det.draw(imgs, dets2, NAMES, maps=maps), want2)
    _equal(det.draw(None, dets2, NAMES, maps=maps, site=site), want2)
    with pytest.raises(ValueError, match="xyxy"):
        Detector(model, cfg, bbox_format="xywh").draw(imgs, dets, NAMES)


def test_tiled_detector_draw(hip, model):
    from detr_tf.inference import Detector, TiledDetections
    cfg, imgs = _config(), _e2e_images()
    det = Detector(model, cfg, score_threshold=0.0, max_detections=20, shortest_side=64, max_size=96, tiles=(2, 2))
    dets = det(imgs)
    assert all(isinstance(d, TiledDetections) and d.scores.shape[0] >= 1 for d in dets)
    want = _ref(imgs, dets)
    _equal(det.draw(imgs, dets, NAMES), want)
    _equal(det.draw(None, dets, NAMES), want)
    with pytest.raises(NotImplementedError, match="tiles"):
        det.draw(imgs, dets, NAMES, maps={})


def test_numpy_bbox_to_image(hip):
    from detr_tf.inference import draw_detections, numpy_bbox_to_image
    rng = np.random.default_rng(11)
    cfg = _config()
    image = np.clip(rng.normal(0.0, 0.8, (60, 90, 3)), -1.7, 2.2).astype(F)          # de-normalises into [0, 1]
    bbox = np.array([[0.5, 0.5, 0.4, 0.6], [0.2, 0.3, 0.3, 0.2], [0.9, 0.9, 0.4, 0.4]], F)
    labels, scores = np.array([1, 0, 2]), np.array([0.91, 0.505, 0.125], F)
    names = ["person", "cat", "dog"]
    frame = (((image * np.array([0.229, 0.224, 0.225])) + np.array([0.485, 0.456, 0.406])) * 255).astype(np.uint8)       # inference.py:15-19
    xyxy = np.stack([(bbox[:, 0] - bbox[:, 2] / 2) * 90, (bbox[:, 1] - bbox[:, 3] / 2) * 60, (bbox[:, 0] + bbox[:, 2] / 2) * 90,
                     (bbox[:, 1] + bbox[:, 3] / 2) * 60], 1).astype(F)
    got = numpy_bbox_to_image(image, bbox, labels, scores, class_name=names, config=cfg)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == frame.shape
    assert (got == draw_detections([frame], [(xyxy, labels, scores)], names)[0].cpu().numpy()).all()
    from detr_tf import overlay as O
    font, glyphs = _font()
    assert (got == R.draw_image(frame, xyxy, labels, scores, names=_names(names), colors=O.class_palette(100), atlas=font, glyphs=glyphs)).all()
    plain = numpy_bbox_to_image(rng.random((60, 90, 3)).astype(F), bbox, class_name=names)        # no config: float32 in [0, 1], labels all 0
    assert plain.dtype == F and plain.min() >= 0.0 and plain.max() <= 1.0
    cfg.normalized_method = "tf_resnet"
    with pytest.raises(ValueError, match="tf_resnet"):
        numpy_bbox_to_image(image, bbox, labels, scores, class_name=names, config=cfg)
