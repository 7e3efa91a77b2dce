"""csrc/tile_merge.hip on the device: detr_hip_tile_merge (inference.merge_tiles) against the NumPy restatement of
tests/tile_merge_ref.py, EXACTLY -- the kept set, its order, labels, query, tile and counts equal, boxes and scores bit-equal --, and
the tiled Detector end to end against the chain assembled by hand.

The comparison can be exact because nothing is left to rounding: the reference gets the fp32 scores and labels of every query from
detr_hip_detect (the merge kernel runs the same scoring code; `whole-image windows` below checks that they do agree), maps the boxes
with the same fp32 operations in the same order, and evaluates the match measure with the same IEEE fp64 operations."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tile_merge_ref as M

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
FORMATS = M.FORMATS
ARGS = ("score", "label", "boxes", "tile_start", "windows", "sizes", "bg")       # tile_merge_ref.merge's positional arguments


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def scores_labels(logits, bg):
    """fp32 score / label of every query as the device computes them: one detr_hip_detect launch over the N tiles, scattered back to
    [N, Q].  Background and NaN queries (which detect drops) come back as background: the merge drops them too."""
    from detr_tf.inference import _detect
    N, Q, _ = logits.shape
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(DEV)
    _, out_l, out_s, out_q, counts = _detect(lg, torch.zeros(N, Q, 4, device=DEV), np.ones((N, 2), np.int32), bg, -1.0, Q, "xy_center", False)
    out_l, out_s, out_q, counts = out_l.cpu().numpy(), out_s.cpu().numpy(), out_q.cpu().numpy(), counts.cpu().numpy()
    score, label = np.zeros((N, Q), F), np.full((N, Q), bg, np.int64)
    for n in range(N):
        k = counts[n]
        score[n, out_q[n, :k]], label[n, out_q[n, :k]] = out_s[n, :k], out_l[n, :k]
    return score, label


def run(case, **kw):
    from detr_tf.inference import merge_tiles
    out = {"pred_logits": torch.from_numpy(case["logits"].copy()).to(DEV), "pred_boxes": torch.from_numpy(case["boxes"].copy()).to(DEV)}
    return merge_tiles(out, case["tile_start"], case["windows"].copy(), case["sizes"].copy(), case["bg"], **kw)


def same(got, want):
    """got: [TiledDetections]; want: tile_merge_ref.merge's list.  Exact."""
    assert len(got) == len(want)
    for g, (wb, wl, ws, wq, wt, _) in zip(got, want):
        assert g.query.cpu().numpy().tolist() == wq.tolist() and g.tile.cpu().numpy().tolist() == wt.tolist()
        assert g.labels.dtype == torch.int64 and g.labels.cpu().numpy().tolist() == wl.tolist()
        assert g.scores.cpu().numpy().tobytes() == ws.tobytes()
        assert g.boxes.dtype == torch.float32 and tuple(g.boxes.shape) == wb.shape and g.boxes.cpu().numpy().tobytes() == wb.tobytes()


def check(case, **kw):
    """merge_tiles == the reference, exactly; returns the reference's result."""
    want = M.merge(case["score"], case["label"], case["boxes"], case["tile_start"], case["windows"], case["sizes"], case["bg"], **kw)
    same(run(case, **kw), want)
    return want


def grid_windows(size, rows, cols, full=True):
    from detr_tf.data import transformation as T
    recs = T.tile_records(size[0], size[1], rows, cols, 0.2, include_full=full)
    return [(t.y0, t.x0, t.hc, t.wc) for t in recs]


def make_case(seed, tiles_per_image, sizes, Q, C, windows, fg=0.6, n_labels=None, box_lo=0.05, box_hi=0.5):
    """Seeded synthetic outputs: a share `fg` of the queries confidently foreground (labels below n_labels), the rest confidently
    background; box centres anywhere in the tile, sides in [box_lo, box_hi] of it."""
    rng = np.random.default_rng(seed)
    N, bg = sum(tiles_per_image), C - 1
    logits = rng.normal(0.0, 1.0, (N, Q, C)).astype(F)
    hot = rng.random((N, Q)) < fg
    n_labels = max(bg, 1) if n_labels is None else n_labels
    logits[hot, rng.integers(0, n_labels, int(hot.sum()))] += rng.uniform(3.0, 9.0, int(hot.sum())).astype(F)
    logits[hot, bg] = -20.0
    logits[~hot, bg] += 8.0
    boxes = np.concatenate([rng.random((N, Q, 2)), rng.uniform(box_lo, box_hi, (N, Q, 2))], -1).astype(F)
    case = dict(logits=logits, boxes=boxes, tile_start=np.concatenate([[0], np.cumsum(tiles_per_image)]).astype(np.int32),
                windows=np.array(windows, np.int32).reshape(N, 4), sizes=np.array(sizes, np.int32).reshape(-1, 2), bg=bg)
    return finish(case)


def finish(case):
    case["score"], case["label"] = scores_labels(case["logits"], case["bg"])
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def two_images():
    """B = 2 with 1 and 3 tiles, Q = 70 (no multiple of 64), C = 5: a whole-image window; the whole image and its two halves."""
    sizes = [(90, 120), (100, 200)]
    windows = [(0, 0, 90, 120)] + grid_windows(sizes[1], 1, 2)
    assert windows[1:] == [(0, 0, 100, 200), (0, 0, 100, 111), (0, 89, 100, 111)]
    return make_case(1, (1, 3), sizes, 70, 5, windows)


@functools.lru_cache(maxsize=None)
def grid_image():
    """B = 1, 3 x 3 tiles + the whole image of a 300 x 400 image, Q = 50, C = 7: tiles that touch the border and one that does not."""
    windows = grid_windows((300, 400), 3, 3)
    assert any(y > 0 and x > 0 and y + h < 300 and x + w < 400 for y, x, h, w in windows)
    return make_case(2, (10,), [(300, 400)], 50, 7, windows)


# ---- the smallest shape ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("foreground", (True, False))
@pytest.mark.parametrize("confident", (True, False))
def test_one_query(hip, foreground, confident):
    logits = np.array([[[2.0, 0.0] if confident else [0.2, 0.0]]], F)               # scores 0.88 / 0.55, label 0
    case = finish(dict(logits=logits, boxes=np.array([[[0.5, 0.5, 0.25, 0.5]]], F), tile_start=np.array([0, 1], np.int32),
                       windows=np.array([[0, 0, 8, 16]], np.int32), sizes=np.array([[8, 16]], np.int32), bg=1 if foreground else 0))
    want = check(case, score_threshold=0.7)
    assert len(want[0][3]) == int(foreground and confident)
    if foreground and confident:
        assert want[0][0].tolist() == [[6.0, 2.0, 10.0, 6.0]]


# ---- every option against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("clip", (True, False))
def test_formats_and_clip(hip, fmt, clip):
    want = check(two_images(), score_threshold=0.5, bbox_format=fmt, clip=clip, nms_threshold=0.3)
    assert all(0 < len(w[3]) < w[5] for w in want)                                  # something kept, something suppressed
    assert sorted(set(want[1][4].tolist())) == [0, 1, 2]                            # survivors from every tile


@pytest.mark.parametrize("match", ("iou", "ios"))
@pytest.mark.parametrize("agnostic", (False, True))
def test_match_modes_and_class_agnostic(hip, match, agnostic):
    kept = {}
    for case in (two_images(), grid_image()):
        want = check(case, score_threshold=0.5, nms_threshold=0.4, match=match, class_agnostic=agnostic, max_detections=600)
        kept[id(case)] = [len(w[3]) for w in want]
    base = [len(w[3]) for w in M.merge(*(grid_image()[k] for k in ARGS),
                                       score_threshold=0.5, nms_threshold=0.4, max_detections=600)]
    if match == "ios" or agnostic:
        assert kept[id(grid_image())][0] < base[0]                                   # both switches suppress more than class-wise IoU


@pytest.mark.parametrize("margin", (0.0, 4.0))
def test_edge_rule(hip, margin):
    for case in (two_images(), grid_image()):
        want = check(case, score_threshold=0.5, nms_threshold=0.5, edge_margin=margin, clip=False, max_detections=600)
        plain = M.merge(*(case[k] for k in ARGS), score_threshold=0.5, nms_threshold=0.5, clip=False, max_detections=600)
        if margin:
            assert want[-1][5] < plain[-1][5]                                       # the rule dropped candidates of the tiled image ...
            whole = want[-1][4] == 0
            assert whole.sum() == (plain[-1][4] == 0).sum() or len(want[-1][3]) != len(plain[-1][3])
            if case is two_images():                                                # ... and none of an image that is one whole window
                assert want[0][5] == plain[0][5] and want[0][3].tolist() == plain[0][3].tolist()


@pytest.mark.parametrize("K", (1, 7, 600))
def test_max_detections_and_zero_tail(hip, K):
    case = grid_image()
    want = check(case, score_threshold=0.5, nms_threshold=0.5, max_detections=K)
    full = M.merge(*(case[k] for k in ARGS), score_threshold=0.5,
                   nms_threshold=0.5, max_detections=2048)
    n = len(full[0][3])
    assert 7 < n < 600 and len(want[0][3]) == min(K, n) and want[0][3].tolist() == full[0][3][:K].tolist()
    raw = raw_merge(case, K, score_threshold=0.5, nms_threshold=0.5)
    assert raw["status"] == 0 and raw["counts"].tolist() == [min(K, n)]
    for name in ("boxes", "labels", "scores", "query", "tile"):
        assert not raw[name][0, min(K, n):].any(), name                              # rows past the count are zero


# ---- sizes and orders at which the kernel can go wrong ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eleven_tiles():
    """B = 1, N = 11, Q = 100, C = 92, every query foreground: 1100 candidates, past the 256- and 1024-boundaries of the kernel's loops."""
    windows = [(0, 0, 600, 800)] + grid_windows((600, 800), 2, 5, full=False)
    return make_case(3, (11,), [(600, 800)], 100, 92, windows, fg=1.1, box_lo=0.05, box_hi=0.3)


def test_eleven_hundred_candidates(hip):
    case = eleven_tiles()
    want = check(case, score_threshold=0.0, nms_threshold=0.3, max_detections=2048)
    assert want[0][5] == 1100 and 256 < len(want[0][3]) < 1100
    want = check(case, score_threshold=0.0, nms_threshold=0.2, class_agnostic=True, match="ios", max_detections=1100)
    assert want[0][5] == 1100 and len(want[0][3]) < 256
    again = run(case, score_threshold=0.0, nms_threshold=0.3, max_detections=2048)
    same(again, M.merge(*(case[k] for k in ARGS), score_threshold=0.0,
                        nms_threshold=0.3, max_detections=2048))                     # a rerun gives the same bits


def chain_case(boxes_px, scores, size=(64, 64), labels=None, tiles=1):
    """Hand-made candidates in ONE image: boxes (x0, y0, x1, y1) in pixels (powers of two keep the mapping exact), given scores
    through two-class logits, every tile a whole-image window; the entries are dealt to the tiles round-robin."""
    H, W = size
    n = len(boxes_px)
    Q = -(-n // tiles)
    logits = np.zeros((tiles, Q, 3), F)
    logits[:, :, 2] = 20.0                                                          # unused slots: background
    boxes = np.zeros((tiles, Q, 4), F)
    for i, ((x0, y0, x1, y1), s) in enumerate(zip(boxes_px, scores)):
        t, q = i % tiles, i // tiles
        logits[t, q] = 0.0
        logits[t, q, 0 if labels is None else labels[i]] = np.log(s / (1 - s) * 2)      # softmax = s / ... over three classes
        logits[t, q, 2] = 0.0
        boxes[t, q] = ((x0 + x1) / 2 / W, (y0 + y1) / 2 / H, (x1 - x0) / W, (y1 - y0) / H)
    return finish(dict(logits=logits, boxes=boxes, tile_start=np.array([0, tiles], np.int32), windows=np.array([(0, 0, H, W)] * tiles, np.int32),
                       sizes=np.array([size], np.int32), bg=2))


def test_identical_boxes_one_survivor(hip):
    case = chain_case([(8, 8, 40, 24)] * 300, [0.5] * 300, tiles=3)                  # equal scores too: the first of tile 0 wins
    want = check(case, nms_threshold=0.5)
    assert want[0][5] == 300 and want[0][3].tolist() == [0] and want[0][4].tolist() == [0]


def test_greedy_order_a_b_c(hip):
    # IoU(A, B) = IoU(B, C) = 24 / 40 = 0.6, IoU(A, C) = 16 / 48: A suppresses B, B is gone, so C survives
    case = chain_case([(0, 0, 32, 16), (8, 0, 40, 16), (16, 0, 48, 16)], [0.9, 0.8, 0.7])
    want = check(case, nms_threshold=0.5)
    assert want[0][3].tolist() == [0, 2]
    case = chain_case([(0, 0, 32, 16), (8, 0, 40, 16), (16, 0, 48, 16)], [0.7, 0.9, 0.8])   # B first: it takes both
    assert check(case, nms_threshold=0.5)[0][3].tolist() == [1]


def test_all_scores_equal_tie_order(hip):
    rng = np.random.default_rng(5)
    px = [(int(x), int(y), int(x) + 16, int(y) + 8) for x, y in rng.integers(0, 40, (90, 2))]
    case = chain_case(px, [0.6] * 90, tiles=4)
    assert len(set(case["score"][case["label"] != 2].tolist())) == 1
    want = check(case, nms_threshold=1.0)                                           # nothing suppressed: the order is (tile, query)
    assert list(zip(want[0][4].tolist(), want[0][3].tolist())) == sorted(zip(want[0][4].tolist(), want[0][3].tolist())) and len(want[0][3]) == 90
    want = check(case, nms_threshold=0.3)
    assert 1 < len(want[0][3]) < 90


def test_exact_threshold_pair_is_kept(hip):
    case = chain_case([(0, 0, 2, 1), (0, 0, 1, 1)], [0.75, 0.5], size=(4, 4))        # IoU = 0.5 exactly
    assert check(case, nms_threshold=0.5)[0][3].tolist() == [0, 1]                   # strict >
    assert check(case, nms_threshold=0.49)[0][3].tolist() == [0]
    assert check(case, nms_threshold=0.5, match="ios")[0][3].tolist() == [0]         # IoS = 1


def test_zero_area_boxes(hip):
    px = [(8, 8, 8, 8), (8, 8, 8, 8), (8, 8, 8, 24), (8, 8, 8, 24), (0, 0, 32, 32), (16, 16, 16, 16)]
    case = chain_case(px, [0.9, 0.8, 0.7, 0.6, 0.5, 0.4])
    for match in ("iou", "ios"):
        want = check(case, nms_threshold=0.0, match=match)                          # zero denominators and zero intersections give 0
        assert want[0][3].tolist() == [0, 1, 2, 3, 4, 5]


def test_nan_logits(hip):
    base = two_images()
    logits = base["logits"].copy()
    logits[0, 3, :] = np.nan
    logits[2, 10, 1] = np.nan
    logits[3, :5, 0] = np.nan
    case = finish(dict(base, logits=logits))
    want = check(case, score_threshold=0.5, nms_threshold=0.4)
    assert (0, 3) not in set(zip(want[0][4].tolist(), want[0][3].tolist()))
    assert not {(1, 10), (2, 0), (2, 4)} & set(zip(want[1][4].tolist(), want[1][3].tolist()))
    assert all(np.isfinite(w[2]).all() for w in want)


# ---- whole-image windows: detect's bits ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def whole_image_cases():
    """(case, score_threshold, K, candidates): three images of Q = 100, C = 92; and B = 2 of Q = 300, C = 4 with every query foreground and
    the threshold at 0 -- 300 candidates per image, so the compaction of a tile takes a second pass of 256 (under the cap of 2048)."""
    sizes = [(480, 640), (1333, 800), (1, 1)]
    first = make_case(7, (1, 1, 1), sizes, 100, 92, [(0, 0, h, w) for h, w in sizes], box_lo=0.0, box_hi=1.0)
    second = make_case(8, (1, 1), sizes[:2], 300, 4, [(0, 0, h, w) for h, w in sizes[:2]], fg=1.0, box_lo=0.0, box_hi=1.0)
    return (first, 0.5, 100, None), (second, 0.0, 300, 300)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("clip", (True, False))
def test_whole_image_windows_equal_detect(hip, fmt, clip):
    from detr_tf.inference import detect_batched
    for case, thr, K, candidates in whole_image_cases():
        out = {"pred_logits": torch.from_numpy(case["logits"].copy()).to(DEV), "pred_boxes": torch.from_numpy(case["boxes"].copy()).to(DEV)}
        want = detect_batched(out, case["sizes"], case["bg"], score_threshold=thr, max_detections=K, bbox_format=fmt, clip=clip)
        got = run(case, score_threshold=thr, max_detections=K, bbox_format=fmt, clip=clip, nms_threshold=1.0, edge_margin=4.0)
        assert sum(int(w.scores.shape[0]) for w in want) > 100
        assert candidates is None or [int(w.scores.shape[0]) for w in want] == [candidates] * len(want)
        for g, w in zip(got, want):
            assert not g.tile.any()
            for a, b in zip(g[:4], w):
                assert a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- the candidate cap -----------------------------------------------------------------------------------------------------------
GUARD = 64


def raw_merge(case, K, **kw):
    """detr_hip_tile_merge called directly on output buffers with GUARD poisoned elements on both sides; asserts the guards are
    intact and returns the outputs, counts and the status word."""
    from detr_tf import _hip
    from detr_tf.inference import DETECT_FORMATS, MATCH_MODES
    lg, bx = torch.from_numpy(case["logits"].copy()).to(DEV), torch.from_numpy(case["boxes"].copy()).to(DEV)
    B, (N, Q, C) = len(case["sizes"]), lg.shape
    start_h = np.ascontiguousarray(case["tile_start"], np.int32)
    start_d, win_d, size_d = (torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV) for a in (start_h, case["windows"], case["sizes"]))
    spec = dict(boxes=(B * K * 4, torch.float32, 1.5), labels=(B * K, torch.int64, -7), scores=(B * K, torch.float32, 2.5),
                query=(B * K, torch.int32, -7), tile=(B * K, torch.int32, -7), counts=(B, torch.int32, -7), status=(1, torch.int32, -7))
    bufs = {n: torch.full((GUARD + size + GUARD,), poison, dtype=dt, device=DEV) for n, (size, dt, poison) in spec.items()}
    bufs["status"][GUARD] = 0
    d = _hip.TileMergeDesc()
    d.B, d.N, d.Q, d.C = B, N, Q, C
    d.logits, d.sL_b, d.sL_q = lg.data_ptr(), lg.stride(0), lg.stride(1)
    d.boxes, d.sB_b, d.sB_q = bx.data_ptr(), bx.stride(0), bx.stride(1)
    d.tile_start, d.tile_start_host, d.windows, d.sizes = start_d.data_ptr(), start_h.ctypes.data, win_d.data_ptr(), size_d.data_ptr()
    d.background_class, d.score_threshold, d.max_detections = case["bg"], kw.get("score_threshold", 0.0), K
    d.bbox_format, d.clip = DETECT_FORMATS[kw.get("bbox_format", "xyxy")], int(kw.get("clip", True))
    d.match, d.class_agnostic = MATCH_MODES[kw.get("match", "iou")], int(kw.get("class_agnostic", False))
    d.edge_margin, d.nms_threshold = kw.get("edge_margin", 0.0), kw.get("nms_threshold", 0.5)
    for field, name in (("out_boxes", "boxes"), ("out_labels", "labels"), ("out_scores", "scores"), ("out_query", "query"), ("out_tile", "tile"),
                        ("counts", "counts"), ("status", "status")):
        setattr(d, field, bufs[name].data_ptr() + GUARD * bufs[name].element_size())
    _hip._check(_hip.load().detr_hip_tile_merge(ctypes.byref(d), _hip._stream()), "detr_hip_tile_merge")
    torch.cuda.synchronize()
    out = {}
    for n, (size, dt, poison) in spec.items():
        h = bufs[n].cpu().numpy()
        assert (h[:GUARD] == poison).all() and (h[GUARD + size:] == poison).all(), f"a guard word of {n} was overwritten"
        out[n] = h[GUARD:GUARD + size]
    out["status"] = int(out["status"][0])
    for n in ("labels", "scores", "query", "tile"):
        out[n] = out[n].reshape(B, K)
    out["boxes"] = out["boxes"].reshape(B, K, 4)
    return out


def test_over_the_candidate_cap(hip):
    """Three images, the middle one with 21 tiles x 100 foreground queries = 2100 candidates > 2048."""
    from detr_tf import _hip
    assert _hip.TILE_MAX_CAND == 2048
    sizes = [(90, 120), (600, 800), (100, 200)]
    windows = [(0, 0, 90, 120)] + [(0, 0, 600, 800)] + grid_windows((600, 800), 4, 5, full=False) + grid_windows((100, 200), 1, 2)
    case = make_case(11, (1, 21, 3), sizes, 100, 92, windows, fg=1.1)
    K = 150
    with pytest.raises(ValueError, match="2048"):
        run(case, score_threshold=0.0, max_detections=K)
    raw = raw_merge(case, K, score_threshold=0.0)
    assert raw["status"] == 1                                                       # DETR_TILE_OVER_CAP
    want = M.merge(*(case[k] for k in ARGS), score_threshold=0.0, max_detections=K)
    assert want[1][5] == 2100 and raw["counts"][1] == 0
    for name in ("boxes", "labels", "scores", "query", "tile"):
        assert not raw[name][1].any(), name                                         # the image over the cap: no detections, zero rows
    for b in (0, 2):                                                                # its neighbours: as if it were not there
        wb, wl, ws, wq, wt, _ = want[b]
        k = len(wq)
        assert raw["counts"][b] == k and raw["query"][b, :k].tolist() == wq.tolist() and raw["tile"][b, :k].tolist() == wt.tolist()
        assert raw["labels"][b, :k].tolist() == wl.tolist() and raw["scores"][b, :k].tobytes() == ws.tobytes()
        assert raw["boxes"][b, :k].tobytes() == wb.tobytes() and not raw["boxes"][b, k:].any()
    # exactly at the cap is fine: 20 tiles x 100 + 48 of the last tile
    logits = case["logits"].copy()
    logits[21, 48:, :] = 0.0
    logits[21, 48:, 91] = 20.0
    at_cap = finish(dict(case, logits=logits))
    want = check(at_cap, score_threshold=0.0, max_detections=K)
    assert want[1][5] == 2048


# ---- the Detector ----------------------------------------------------------------------------------------------------------------
def _config():
    from detr_tf.training_config import TrainingConfig
    cfg = TrainingConfig()
    cfg.background_class = 91
    cfg.image_size = (64, 96)
    return cfg


@pytest.fixture(scope="module")
def model(hip):
    """The committed tiny model: the configuration and seed of tests/golden/tiny_r50_e1d2_64x96.npz."""
    import os
    from detr_tf.networks.detr import get_detr_model
    from oracle import detr_ref as R
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_r50_e1d2_64x96.npz")) as z:
        seed, num_enc, num_dec = (int(v) for v in z["meta"][:3])
    m = get_detr_model(_config(), include_top=True, num_encoder_layers=num_enc, num_decoder_layers=num_dec, dropout=0.0)
    m.load_weights(R.make_params(seed, num_enc=num_enc, num_dec=num_dec))
    return m


def _images():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in ((96, 128), (80, 150))]


def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert type(x) is type(y)
        for s, t in zip(x, y):
            assert s.dtype == t.dtype and s.shape == t.shape and s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()


def test_tiled_detector_equals_the_hand_assembled_chain(hip, model):
    from detr_tf.data import transformation as T
    from detr_tf.data.processing import DeviceInputStage
    from detr_tf.inference import Detector, TiledDetections
    cfg, imgs = _config(), _images()
    canvas = (96, 128)
    kw = dict(score_threshold=0.0, max_detections=40, nms_threshold=0.4, edge_margin=2.0)
    det = Detector(model, cfg, shortest_side=64, max_size=96, canvas=canvas, tiles=(2, 2), **kw)
    first = det(imgs)                                                               # eager: the first sighting of the shape
    assert len(first) == 2 and all(isinstance(d, TiledDetections) for d in first)
    # the chain by hand: tile_records -> augmented_tiles -> model -> the reference merge on the device's scores
    recs = [T.tile_records(im.shape[0], im.shape[1], 2, 2, 0.2, 64, 96, T.CUBIC) for im in imgs]
    assert recs == det.tile_records(imgs) and [len(r) for r in recs] == [5, 5]
    x, m, tile_start = DeviceInputStage(cfg).augmented_tiles(imgs, recs, canvas=canvas)
    assert tuple(x.shape) == (10, 96, 128, 3) and tile_start.tolist() == [0, 5, 10]
    whole = DeviceInputStage(cfg).augmented_padded(imgs, [r[0] for r in recs], canvas=canvas)
    assert torch.equal(x[[0, 5]], whole[0]) and torch.equal(m[[0, 5]], whole[1])    # tile 0 is the whole image, as the plain path stages it
    out = model((x, m), training=False)
    logits, boxes = out["pred_logits"].float().cpu().numpy(), out["pred_boxes"].float().cpu().numpy()
    score, label = scores_labels(logits, 91)
    windows = np.array([(t.y0, t.x0, t.hc, t.wc) for r in recs for t in r], np.int32)
    sizes = np.array([im.shape[:2] for im in imgs], np.int32)
    want = M.merge(score, label, boxes, tile_start, windows, sizes, 91, **kw)
    assert all(w[5] >= len(w[3]) >= 1 for w in want)                                # candidates exist
    same(first, want)
    for d, (h, w) in zip(first, sizes.tolist()):
        b = d.boxes.cpu().numpy()
        assert (b >= 0).all() and (b[:, [0, 2]] <= w).all() and (b[:, [1, 3]] <= h).all()
    # the second forward of the shape records the evaluation graph, later calls replay it: no re-record, the same bits
    _same_lists(det(imgs), first)
    assert model._eval_graph is not None
    recorded = model._eval_graph["graph"]
    _same_lists(det(imgs), first)
    _same_lists(det(imgs), first)
    assert model._eval_graph["graph"] is recorded
    # chunks of tiles give the same detections (other batch shapes: other buffers, so this comes last)
    chunked = Detector(model, cfg, shortest_side=64, max_size=96, canvas=canvas, tiles=(2, 2), tile_batch=4, **kw)
    got = chunked(imgs)
    assert len(got) == 2 and all(isinstance(g, TiledDetections) and 1 <= g.scores.shape[0] <= 40 for g in got)
    one = det(imgs[1])                                                              # one array in, one TiledDetections out
    assert isinstance(one, TiledDetections)
    with pytest.raises(NotImplementedError):
        det(imgs, need_weights=True)
    coco = Detector(model, cfg, shortest_side=64, max_size=96, canvas=canvas, tiles=(2, 2), bbox_format="xywh", **kw)
    dets = coco(imgs)
    records = coco.to_coco_results(dets, [7, 9])
    assert len(records) == sum(int(d.scores.shape[0]) for d in dets) and {r["image_id"] for r in records} == {7, 9}


def test_detector_defaults_are_the_plain_path(hip, model):
    from detr_tf.inference import Detections, Detector, TiledDetections, detect_batched
    cfg, imgs = _config(), _images()
    kw = dict(score_threshold=0.0, max_detections=20, shortest_side=64, max_size=96, canvas=(96, 128))
    plain = Detector(model, cfg, **kw)(imgs)
    explicit = Detector(model, cfg, tiles=None, nms_threshold=None, **kw)(imgs)
    assert all(type(d) is Detections for d in explicit)
    _same_lists(explicit, plain)
    # nms_threshold alone: class-wise NMS behind the single pass; at 1.0 nothing is suppressed and the four fields are detect's
    nms = Detector(model, cfg, nms_threshold=1.0, **kw)(imgs)
    assert all(type(d) is TiledDetections and not d.tile.any() for d in nms)
    for a, b in zip(nms, plain):
        for s, t in zip(a[:4], b):
            assert s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()
    tight = Detector(model, cfg, nms_threshold=0.1, class_agnostic=True, **kw)(imgs)
    assert all(1 <= t.scores.shape[0] <= p.scores.shape[0] for t, p in zip(tight, plain))
