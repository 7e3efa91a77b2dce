"""Test model of csrc/augment_padded.hip: flip -> window -> resize to the image's own (hd, wd) -> normalise -> top-left of a
zero canvas with its padding mask, in NumPy, built from tests/augment_ref.py's fp32 resize functions (the kernel's operation
order).  `resize_f64` restates the same four interpolations with float64 coefficients and sums and exact ratios: an independent
computation that tells how far fp32 rounding alone can move a pixel.  `kernel_cases` are the inputs the kernel test uses."""
import numpy as np

import augment_ref as A

IREC = 12


def padded_uint8(img, rec):
    """One image through flip -> window -> resize (uint8)."""
    f = img[:, ::-1] if rec.flip else img
    win = np.ascontiguousarray(f[rec.y0:rec.y0 + rec.hc, rec.x0:rec.x0 + rec.wc])
    return A.resize(win, rec.hd, rec.wd, rec.interp)


def augment_padded(images, records, H, W, lut, perm, resize=padded_uint8):
    """-> (canvas float32 [B, H, W, 3], mask bool [B, H, W])"""
    B = len(images)
    out = np.zeros((B, H, W, 3), np.float32)
    mask = np.ones((B, H, W), bool)
    for b, (im, r) in enumerate(zip(images, records)):
        out[b, :r.hd, :r.wd] = A.normalise(resize(im, r), np.asarray(lut).reshape(3, 256), perm)
        mask[b, :r.hd, :r.wd] = False
    return out, mask


# ---- float64 restatement ---------------------------------------------------------------------------------------------------
def _axis_f64(S, D, mode):
    """Tap indices [D, T] (clamped into the axis) and float64 weights [D, T] of one axis; mode as the kernel's codes.  Area is
    separable in both of its forms; which form applies is decided by the caller."""
    d = np.arange(D, dtype=np.float64)
    r = S / D
    if mode == "nearest":
        return np.clip(np.floor(d * r).astype(np.int64), 0, S - 1)[:, None], np.ones((D, 1))
    if mode == "box":                                         # fractional overlap of [d r, (d + 1) r) with every cell, / r
        f1, f2 = d * r, (d + 1) * r
        lo = np.minimum(np.floor(f1).astype(np.int64), S - 1)
        T = int(np.ceil(r)) + 1
        idx = lo[:, None] + np.arange(T)[None, :]
        w = np.clip(np.minimum(f2[:, None], idx + 1.0) - np.maximum(f1[:, None], idx.astype(np.float64)), 0.0, None) / r
        return np.clip(idx, 0, S - 1), np.where(idx <= S - 1, w, 0.0)
    if mode == "area_linear":
        s = np.floor(d * r).astype(np.int64)
        f = (d + 1) - (s + 1) / r
        f = np.where(f <= 0, 0.0, f - np.floor(f))
        return np.clip(np.stack([s, s + 1], 1), 0, S - 1), np.stack([1 - f, f], 1)
    f = (d + 0.5) * r - 0.5
    i0 = np.floor(f).astype(np.int64)
    t = f - i0
    if mode == "linear":
        return np.clip(np.stack([i0, i0 + 1], 1), 0, S - 1), np.stack([1 - t, t], 1)
    a = -0.75                                                 # cubic, a = -0.75: the four taps' closed forms
    c0 = ((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a
    c1 = ((a + 2) * t - (a + 3)) * t * t + 1
    c2 = ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1
    return np.clip(np.stack([i0 - 1, i0, i0 + 1, i0 + 2], 1), 0, S - 1), np.stack([c0, c1, c2, 1 - c0 - c1 - c2], 1)


def resize_f64(img, Hd, Wd, interp):
    Hs, Ws, _ = img.shape
    if (Hs, Ws) == (Hd, Wd):
        return img.copy()
    name = A.NAMES[interp]
    if name == "area":
        name = "box" if (Hs >= Hd and Ws >= Wd) else "area_linear"
    iy, wy = _axis_f64(Hs, Hd, name)
    ix, wx = _axis_f64(Ws, Wd, name)
    src = img.astype(np.float64)
    acc = np.zeros((Hd, Wd, 3))
    for j in range(iy.shape[1]):
        rows = src[iy[:, j]]
        row = np.zeros((Hd, Wd, 3))
        for k in range(ix.shape[1]):
            row += wx[None, :, k, None] * rows[:, ix[:, k]]
        acc += wy[:, j, None, None] * row
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def padded_uint8_f64(img, rec):
    f = img[:, ::-1] if rec.flip else img
    win = np.ascontiguousarray(f[rec.y0:rec.y0 + rec.hc, rec.x0:rec.x0 + rec.wc])
    return resize_f64(win, rec.hd, rec.wd, rec.interp)


# ---- the kernel test's inputs ----------------------------------------------------------------------------------------------
BATCHES = (((37, 53), (480, 640), (120, 90)), ((333, 517), (64, 200), (200, 64), (96, 128)))


def smooth_images(shapes, seed):
    """uint8 images with image-like content (a few random low-frequency waves per channel plus +-6 levels of noise): resampled
    values then sit at a generic distance from the .5 rounding boundaries, as in a photograph."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in shapes:
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.zeros((h, w, 3))
        for c in range(3):
            for _ in range(4):
                fy, fx, ph = rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08), rng.uniform(0, 2 * np.pi)
                img[..., c] += rng.uniform(10, 40) * np.sin(2 * np.pi * (fy * y + fx * x) + ph)
        img += 128 + rng.uniform(-6, 6, img.shape)
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


def kernel_cases(T):
    """(tag, images, records, (H, W)): every interpolation x {flip, no flip} x {full window, inner window} on two ragged
    batches; destination sizes mix enlargement, reduction and (image 0 of each batch) one axis of each.  The sizes are chosen
    so that no resize ratio is a small rational: at a ratio like 2 / 3 or 5 / 2 the linear weights are exactly 1 / 2 or 1 / 4, sums of
    integer pixels then land exactly on a .5 rounding boundary for a large share of the pixels, and the last bit of an fp32
    coefficient decides each of them -- a property of the ratio, not of the code."""
    for bi, shapes in enumerate(BATCHES):
        images = smooth_images(shapes, 100 + bi)
        for interp in range(4):
            for flip in (False, True):
                for inner in (False, True):
                    recs = []
                    for i, (h0, w0) in enumerate(shapes):
                        if inner:
                            y0, x0 = h0 // 5, w0 // 3
                            hc, wc = max(1, h0 // 2 + i), max(1, w0 // 2 - i)
                        else:
                            y0, x0, hc, wc = 0, 0, h0, w0
                        if i == 0:
                            hd, wd = hc * 3 // 2 + 1, wc * 2 // 3 + 1                  # one axis up, the other down
                        else:
                            hd, wd = T.target_size(hc, wc, (97, 151, 61)[(i + bi) % 3], 223)
                        recs.append(T.PaddedRecord(h0, w0, flip, y0, x0, hc, wc, hd, wd, interp))
                    H = -(-max(r.hd for r in recs) // 32) * 32 + (1 if bi else 0)      # batch 1: H * W is odd, a canvas the
                    W = -(-max(r.wd for r in recs) // 32) * 32 + (3 if bi else 0)      # 16-byte stores do not fit
                    yield (f"batch{bi}-{A.NAMES[interp]}-flip{int(flip)}-inner{int(inner)}", images, recs, (H, W))
