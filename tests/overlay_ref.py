"""Plain NumPy restatement of detr_hip_overlay (include/detr_hip.h: detr_overlay_desc): integer geometry, the same integer blend, the
same fp32 operation order for the heat map, Python's "%.2f" for the score text.  A test helper, not product code: one image at a
time, one box at a time, by slicing.  Every comparison with the kernel is exact, byte for byte."""
import math

import numpy as np

F = np.float32


def blend(c, p, a):
    """(c * a + p * (255 - a) + 127) / 255 in integers; c, p: int arrays or scalars."""
    return (np.asarray(c, np.int64) * a + np.asarray(p, np.int64) * (255 - a) + 127) // 255


def score_text(score):
    """'d.dd' as the kernel writes it: Python's "%.2f" where that has four characters (0 <= score < 9.995), else the clamp."""
    s = float(F(score))
    if math.isnan(s) or s <= 0.0:
        return "0.00"
    if s >= 9.995:
        return "9.99"
    return "%.2f" % s


def score_digits_rint(score):
    """The device rule itself: q = rint((double)score * 100.0), half to even, clamped to [0, 999], NaN -> 0."""
    q = np.rint(np.float64(F(score)) * 100.0)
    q = 0 if not (q > 0) else (999 if q >= 999 else int(q))
    return "%d.%d%d" % (q // 100, q // 10 % 10, q % 10)


def corners(box, label, H, W):
    """Integer corners (x1, y1, x2, y2) of a box, or None when it is skipped."""
    bx0, by0, bx1, by1 = (float(v) for v in box)
    if not all(math.isfinite(v) for v in (bx0, by0, bx1, by1)) or bx1 < bx0 or by1 < by0 or int(label) < 0:
        return None
    cl = lambda v, hi: int(min(max(math.floor(v), 0), hi))
    return cl(bx0, W - 1), cl(by0, H - 1), cl(bx1, W - 1), cl(by1, H - 1)


def apply_heat(img, heat, step, valid, mscale, lut, heat_alpha):
    """img int64 [H, W, 3]; heat float32 [Hf, Wf]; step (sy, sx) float32; valid (vh, vw)."""
    H, W = img.shape[:2]
    heat = np.asarray(heat, F)
    vh, vw = int(min(max(valid[0], 1), heat.shape[0])), int(min(max(valid[1], 1), heat.shape[1]))
    with np.errstate(all="ignore"):
        def taps(n, st, v):
            f = (np.arange(n, dtype=F) + F(0.5)) * F(st) - F(0.5)
            f = np.minimum(np.maximum(f, F(0)), F(v - 1))
            i0 = np.floor(f).astype(np.int64)
            w = f - i0.astype(F)
            return i0, np.minimum(i0 + 1, v - 1), w
        y0, y1, wy = taps(H, step[0], vh)
        x0, x1, wx = taps(W, step[1], vw)
        wy, wx = wy[:, None], wx[None, :]
        m00, m01, m10, m11 = heat[y0][:, x0], heat[y0][:, x1], heat[y1][:, x0], heat[y1][:, x1]
        top = m00 + wx * (m01 - m00)
        bot = m10 + wx * (m11 - m10)
        m = top + wy * (bot - top)
        v = m * F(mscale)
        v = np.where(v > 0, np.minimum(v, F(1)), F(0)).astype(F)
        idx = (v * F(255.0) + F(0.5)).astype(np.int64)
        al = (v * F(heat_alpha) + F(0.5)).astype(np.int64)
    assert m.dtype == F and v.dtype == F
    c = np.asarray(lut, np.int64)[idx]
    return (c * al[..., None] + img * (255 - al[..., None]) + 127) // 255


def draw_image(image, boxes, labels, scores=None, *, names=(), colors, atlas, glyphs, thickness=2, scale=1, label_alpha=255, fill_alpha=0,
               heat=None, map_step=None, map_valid=None, map_scale=1.0, lut=None, heat_alpha=160):
    """One image.  names: per class a sequence of glyph indices; glyphs = (digit0, colon, dot); colors uint8 [n, 3]; atlas uint8
    [n_glyph, gh, gw]."""
    img = np.asarray(image).astype(np.int64)
    H, W = img.shape[:2]
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    labels = np.asarray(labels, np.int64).reshape(-1)
    atlas = np.asarray(atlas)
    n_glyph, gh, gw = atlas.shape
    digit0, colon, dot = glyphs
    t, s = int(thickness), int(scale)
    if heat is not None:
        img = apply_heat(img, heat, map_step, map_valid, map_scale, lut, heat_alpha)
    todo = []
    for i in range(boxes.shape[0]):
        c = corners(boxes[i], labels[i], H, W)
        if c is not None:
            todo.append(((c[2] - c[0]) * (c[3] - c[1]), i, c))
    todo.sort(key=lambda e: (-e[0], e[1]))
    for _, i, (x1, y1, x2, y2) in todo:
        label = int(labels[i])
        col = np.asarray(colors, np.int64)[label % len(colors)]
        if fill_alpha:
            img[y1:y2 + 1, x1:x2 + 1] = blend(col, img[y1:y2 + 1, x1:x2 + 1], fill_alpha)
        named = label < len(names)
        text = list(names[label]) if named else []
        if scores is not None:
            txt = score_text(scores[i])
            text += ([colon] if named else []) + [digit0 + int(txt[0]), dot, digit0 + int(txt[2]), digit0 + int(txt[3])]
        if named or scores is not None:
            pad = t + s
            width, height = len(text) * gw * s + 2 * pad, gh * s + 2 * pad
            ox, oy = max(0, min(x1, W - width)), max(0, min(y1, H - height))
            img[oy:oy + height, ox:ox + width] = blend(col, img[oy:oy + height, ox:ox + width], label_alpha)      # slicing cuts at the image
            tcol = 0 if 299 * col[0] + 587 * col[1] + 114 * col[2] >= 128000 else 255
            for ci, g in enumerate(text):
                if g >= n_glyph:
                    continue
                ink = np.kron(atlas[g] != 0, np.ones((s, s), bool))
                gy, gx = oy + pad, ox + pad + ci * gw * s
                region = img[gy:gy + gh * s, gx:gx + gw * s]
                region[ink[:region.shape[0], :region.shape[1]]] = tcol
        box = img[y1:y2 + 1, x1:x2 + 1]
        edge = np.ones(box.shape[:2], bool)
        if x2 - t >= x1 + t and y2 - t >= y1 + t:
            edge[t:box.shape[0] - t, t:box.shape[1] - t] = False
        box[edge] = col
    return img.astype(np.uint8)


def draw_batch(images, boxes, labels, scores, counts, *, scales, heat=None, map_step=None, map_valid=None, map_scale=None, **kw):
    """The batch form of the C call: boxes [B, D, 4], labels [B, D], scores [B, D] or None, counts [B] (clamped to [0, D])."""
    out = []
    for b, im in enumerate(images):
        k = int(min(max(counts[b], 0), np.asarray(boxes).shape[1]))
        h = {} if heat is None else dict(heat=heat[b], map_step=map_step[b], map_valid=map_valid[b], map_scale=map_scale[b])
        out.append(draw_image(im, boxes[b][:k], labels[b][:k], None if scores is None else scores[b][:k], scale=scales[b], **h, **kw))
    return out
