"""Test model of csrc/augment.hip: the stages of one transform record applied one after the other, in NumPy fp32 with the
kernel's operation order.  Nearest / linear / cubic reuse oracle.input_ref.resize_uint8; area and the affine zoom are
restated here (OpenCV's INTER_AREA and cv2.warpAffine with BORDER_CONSTANT, from their documented behaviour: parity with
OpenCV itself is unpinned)."""
import numpy as np

from oracle import input_ref as I

NAMES = ("nearest", "linear", "cubic", "area")
F32 = np.float32


def _box_axis(S, D):
    """Area box weights of one axis (ratio r = S / D >= 1): tap indices and overlaps [D, T], overlap 0 past the footprint."""
    r = F32(S) / F32(D)
    d = np.arange(D, dtype=np.float32)
    f1, f2 = d * r, (d + F32(1.0)) * r
    lo = np.minimum(np.floor(f1).astype(np.int64), S - 1)
    hi = np.minimum(np.ceil(f2).astype(np.int64) - 1, S - 1)
    T = int((hi - lo).max()) + 1
    idx = np.zeros((D, T), np.int64)
    w = np.zeros((D, T), np.float32)
    for t in range(T):
        j = lo + t
        valid = j <= hi
        jj = np.where(valid, j, lo)
        o = np.minimum(f2, (jj + 1).astype(np.float32)) - np.maximum(f1, jj.astype(np.float32))
        idx[:, t] = jj
        w[:, t] = np.where(valid, o, F32(0.0))
    return idx, w, r


def _area_linear_axis(S, D):
    r = F32(S) / F32(D)
    d = np.arange(D, dtype=np.float32)
    s = np.floor(d * r).astype(np.int64)
    f = (d + F32(1.0)) - (s.astype(np.float32) + F32(1.0)) / r
    f = np.where(f <= F32(0.0), F32(0.0), f - np.floor(f)).astype(np.float32)
    idx = np.stack([np.clip(s, 0, S - 1), np.clip(s + 1, 0, S - 1)], 1)
    return idx, np.stack([F32(1.0) - f, f], 1)


def _separable(img, iy, wy, ix, wx):
    src = img.astype(np.float32)
    acc = np.zeros((iy.shape[0], ix.shape[0], 3), np.float32)
    for j in range(iy.shape[1]):
        row = np.zeros_like(acc)
        for k in range(ix.shape[1]):
            row = row + wx[None, :, k, None] * src[iy[:, j]][:, ix[:, k]]
        acc = acc + wy[:, j, None, None] * row
    return acc


def area_resize_uint8(img, Hd, Wd):
    Hs, Ws, _ = img.shape
    if (Hs, Ws) == (Hd, Wd):
        return img.copy()
    ry, rx = F32(Hs) / F32(Hd), F32(Ws) / F32(Wd)
    if ry >= 1 and rx >= 1:
        iy, wy, _ = _box_axis(Hs, Hd)
        ix, wx, _ = _box_axis(Ws, Wd)
        acc = _separable(img, iy, wy, ix, wx) * (F32(1.0) / (rx * ry))
    else:
        iy, wy = _area_linear_axis(Hs, Hd)
        ix, wx = _area_linear_axis(Ws, Wd)
        acc = _separable(img, iy, wy, ix, wx)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def resize(img, Hd, Wd, mode):
    if NAMES[mode] == "area":
        return area_resize_uint8(img, Hd, Wd)
    return I.resize_uint8(img, Hd, Wd, NAMES[mode])


def affine_uint8(img, isx, isy):
    """Zoom about the centre: source = (x - c) * (1/s) + c, c = n/2 - 0.5; bilinear, 0 outside; rounded to uint8."""
    h0, w0, _ = img.shape

    def axis(n, inv):
        c = F32(n) * F32(0.5) - F32(0.5)
        u = (np.arange(n, dtype=np.float32) - c) * F32(inv) + c
        u = np.minimum(np.maximum(u, F32(-2.0)), F32(n) + F32(1.0))
        i0 = np.floor(u).astype(np.int64)
        f = u - i0.astype(np.float32)
        return np.stack([i0, i0 + 1], 1), np.stack([F32(1.0) - f, f], 1)

    iy, wy = axis(h0, isy)
    ix, wx = axis(w0, isx)
    src = img.astype(np.float32)
    acc = np.zeros((h0, w0, 3), np.float32)
    for j in range(2):
        row = np.zeros_like(acc)
        yin = (iy[:, j] >= 0) & (iy[:, j] < h0)
        for k in range(2):
            xin = (ix[:, k] >= 0) & (ix[:, k] < w0)
            p = src[np.clip(iy[:, j], 0, h0 - 1)][:, np.clip(ix[:, k], 0, w0 - 1)]
            p = np.where((yin[:, None] & xin[None, :])[..., None], p, F32(0.0))
            row = row + wx[None, :, k, None] * p
        acc = acc + wy[:, j, None, None] * row
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def augment_uint8(img, rec, Hd, Wd):
    """One image through flip -> stage B -> final resize (uint8 between the stages, as in imgaug)."""
    f = img[:, ::-1] if rec.flip else img
    if rec.kind == 1:
        return resize(f, Hd, Wd, rec.ia)
    if rec.kind == 2:
        hc, wc = min(Hd, rec.h0), min(Wd, rec.w0)
        b = f[rec.y0:rec.y0 + hc, rec.x0:rec.x0 + wc]
    elif rec.kind == 3:
        b = affine_uint8(np.ascontiguousarray(f), np.float32(1.0 / rec.sx), np.float32(1.0 / rec.sy))
    else:
        b = f
    return resize(np.ascontiguousarray(b), Hd, Wd, rec.iff)


def normalise(u8, lut, perm):
    return np.stack([lut[c][u8[..., perm[c]]] for c in range(3)], -1)
