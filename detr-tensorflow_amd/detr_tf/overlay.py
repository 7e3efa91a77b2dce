"""Boxes, name:score labels and attention heat maps drawn onto frames on the device (reference detr_tf/inference.py:10-65,
numpy_bbox_to_image -- there cv2.rectangle / cv2.putText per box on the host).

`draw_detections` is one call of the HIP entry point `detr_hip_overlay` (csrc/overlay.hip; the exact rules are in include/detr_hip.h):
a ragged batch of uint8 RGB frames, the detections exactly as `detect_batched` / `merge_tiles` return them, at most two launches and no
host synchronisation.  `numpy_bbox_to_image` keeps the reference's signature on top of it.  The window (cv2.imshow) stays out of scope.

Deviations from the reference, all deliberate: the font is the built-in 5x7 bitmap font below (not Hershey), colours come from the
deterministic `class_palette` (the reference draws np.random colours), the outline grows inwards from the box's integer corners and
never leaves the image, and config.normalized_method == "tf_resnet" raises ValueError (a NameError in the reference).  Pixel parity
with OpenCV is not claimed.
"""
from ctypes import byref

import numpy as np
import torch

from . import _hip as hip

# ---- the built-in font: 5 x 7 dots in a 6 x 8 cell, ASCII 32..126, glyph index = ord(c) - 32.  Per glyph five column bytes, left to
# right, bit 0 = top row (the classic dot-matrix character generator shapes).
FONT_FIRST, FONT_LAST = 32, 126
FONT_GW, FONT_GH = 6, 8
_FONT_COLUMNS = (
    "0000000000 00005F0000 0007000700 147F147F14 242A7F2A12 2313086462 3649552250 0005030000 "      # space ! " # $ % & '
    "001C224100 0041221C00 14083E0814 08083E0808 0050300000 0808080808 0060600000 2010080402 "      # ( ) * + , - . /
    "3E5149453E 00427F4000 4261514946 2141454B31 1814127F10 2745454539 3C4A494930 0171090503 "      # 0 1 2 3 4 5 6 7
    "3649494936 064949291E 0036360000 0056360000 0814224100 1414141414 0041221408 0201510906 "      # 8 9 : ; < = > ?
    "324979413E 7E1111117E 7F49494936 3E41414122 7F4141221C 7F49494941 7F09090901 3E4149497A "      # @ A B C D E F G
    "7F0808087F 00417F4100 2040413F01 7F08142241 7F40404040 7F020C027F 7F0408107F 3E4141413E "      # H I J K L M N O
    "7F09090906 3E4151215E 7F09192946 4649494931 01017F0101 3F4040403F 1F2040201F 3F4038403F "      # P Q R S T U V W
    "6314081463 0708700807 6151494543 007F414100 0204081020 0041417F00 0402010204 4040404040 "      # X Y Z [ \ ] ^ _
    "0001020400 2054545478 7F48444438 3844444420 384444487F 3854545418 087E090102 0C5252523E "      # ` a b c d e f g
    "7F08040478 00447D4000 2040443D00 7F10284400 00417F4000 7C04180478 7C08040478 3844444438 "      # h i j k l m n o
    "7C14141408 081414187C 7C08040408 4854545420 043F444020 3C4040207C 1C2040201C 3C4030403C "      # p q r s t u v w
    "4428102844 0C5050503C 4464544C44 0008364100 00007F0000 0041360800 1008081008"                 # x y z { | } ~
).split()


def font_atlas():
    """The built-in font as the atlas detr_hip_overlay takes: uint8 [95, 8, 6], 1 = ink."""
    assert len(_FONT_COLUMNS) == FONT_LAST - FONT_FIRST + 1
    atlas = np.zeros((len(_FONT_COLUMNS), FONT_GH, FONT_GW), np.uint8)
    for g, cols in enumerate(_FONT_COLUMNS):
        for x in range(5):
            bits = int(cols[2 * x:2 * x + 2], 16)
            for y in range(7):
                atlas[g, y, x] = (bits >> y) & 1
    return atlas


def encode_text(text):
    """Glyph indices of a string in the built-in font; a character outside ASCII 32..126 becomes '?'."""
    return [(ord(c) if FONT_FIRST <= ord(c) <= FONT_LAST else ord("?")) - FONT_FIRST for c in str(text)]


def class_palette(n):
    """uint8 [n, 3] RGB, deterministic and integer only: hue steps by 137 degrees (consecutive classes far apart), saturation and
    value cycle more slowly, so some hundred classes stay distinguishable.  (The reference draws np.random colours.)"""
    n = int(n)
    if n < 1:
        raise ValueError(f"class_palette: n={n} must be >= 1")
    out = np.zeros((n, 3), np.uint8)
    for i in range(n):
        h = (i * 137 + 20) % 360
        s = (255, 170, 210)[(i // 8) % 3]
        v = (255, 200)[(i // 24) % 2]
        sector, f = divmod(h, 60)
        p = v * (255 - s) // 255
        q = v * (255 * 60 - s * f) // (255 * 60)
        t = v * (255 * 60 - s * (60 - f)) // (255 * 60)
        out[i] = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))[sector]
    return out


def heat_colormap():
    """The built-in colormap, uint8 [256, 3]: blue - cyan - green - yellow - red by the piecewise-linear formula
    channel = clip(384 - |4 i - centre|, 0, 255) with centres 768 (R), 512 (G), 256 (B)."""
    i = np.arange(256, dtype=np.int64)
    return np.stack([np.clip(384 - np.abs(4 * i - c), 0, 255) for c in (768, 512, 256)], 1).astype(np.uint8)


def default_scale(height):
    """Font scale of an image `height` pixels high: max(1, (H + 250) // 500), the reference's H / 500 multiplier rounded."""
    return max(1, (int(height) + 250) // 500)


def heat_geometry(extent, sizes, Hf, Wf):
    """(map_step float32 [B, 2], map_valid int32 [B, 2]) of detr_hip_overlay: image b of sizes[b] = (H, W) pixels covers
    extent[b] = (eh, ew) feature cells (fractional) from the map's top-left: step = cells per pixel, valid = the cells it touches."""
    ext = np.asarray(extent, np.float64).reshape(-1, 2)
    sizes = np.asarray(sizes, np.float64).reshape(-1, 2)
    if ext.shape != sizes.shape or not np.isfinite(ext).all() or (ext <= 0).any():
        raise ValueError(f"heat_extent must be [B, 2] positive finite (cells high, cells wide), got {extent!r}")
    step = (ext / sizes).astype(np.float32)
    valid = np.clip(np.ceil(ext), 1, [Hf, Wf]).astype(np.int32)
    return step, valid


_CONSTANTS = {}


def _constants(device):
    """The built-in atlas and colormap on `device`, uploaded once."""
    key = str(device)
    if key not in _CONSTANTS:
        _CONSTANTS[key] = (torch.from_numpy(font_atlas()).to(device), torch.from_numpy(heat_colormap()).to(device))
    return _CONSTANTS[key]


class RaggedFrames:
    """A ragged batch of uint8 frames already on the device: `buffer` holds image b as [h_b, w_b, 3] bytes at byte offset
    offsets[b]; sizes [B, 2] = (height, width) on the host.  What DeviceInputStage keeps of its last upload."""

    def __init__(self, buffer, offsets, sizes):
        self.buffer, self.offsets, self.sizes = buffer, np.asarray(offsets, np.int64), np.asarray(sizes, np.int32).reshape(-1, 2)

    def views(self):
        return [self.buffer[o:o + h * w * 3].view(h, w, 3) for o, (h, w) in zip(self.offsets.tolist(), self.sizes.tolist())]


def _check_frames(images):
    """Host-side checks: (list of images, sizes int32 [B, 2], on_device)."""
    if isinstance(images, (np.ndarray, torch.Tensor)) and images.ndim == 3:
        images = [images]
    if not isinstance(images, (list, tuple)) or not images:
        raise TypeError("draw_detections expects uint8 images [h, w, 3] (host arrays or device tensors), one or a non-empty list")
    for im in images:
        is_u8 = (isinstance(im, np.ndarray) and im.dtype == np.uint8) or (isinstance(im, torch.Tensor) and im.dtype == torch.uint8)
        if not is_u8 or im.ndim != 3 or im.shape[-1] != 3:
            raise TypeError("draw_detections expects uint8 images [h, w, 3] (host arrays or device tensors)")
        if im.shape[0] < 1 or im.shape[1] < 1 or max(im.shape[:2]) > hip.OVERLAY_MAX_SIDE:
            raise ValueError(f"draw_detections: an image of {im.shape[0]} x {im.shape[1]} pixels (each side 1..{hip.OVERLAY_MAX_SIDE})")
    sizes = np.array([im.shape[:2] for im in images], np.int32)
    return list(images), sizes, all(isinstance(im, torch.Tensor) and im.is_cuda for im in images)


def _upload_frames(images, on_device, device):
    """(keep-alive tensors, base pointer, byte offsets int64 [B]) of the source frames on the device."""
    if on_device:                                                                         # used where they are: no copy
        keep = [im.contiguous() for im in images]
        base = min(t.data_ptr() for t in keep)
        return keep, base, np.array([t.data_ptr() - base for t in keep], np.int64)
    host = [im.cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im) for im in images]
    nbytes = np.array([h.size for h in host], np.int64)
    offsets = np.zeros(len(host), np.int64)
    offsets[1:] = np.cumsum(nbytes)[:-1]
    staging = torch.empty(int(nbytes.sum()), dtype=torch.uint8, pin_memory=True)          # one pinned copy, one transfer
    flat = staging.numpy()
    for h, o in zip(host, offsets):
        flat[o:o + h.size] = h.reshape(-1)
    buf = staging.to(device, non_blocking=True)
    return [buf, staging], buf.data_ptr(), offsets


def _check_detections(detections, B, want_scores):
    """Host-side checks: per image (boxes [k, 4] float32, labels [k] int64, scores [k] float32 or None) tensors, and whether scores
    are drawn."""
    from .inference import Detections, FusedDetections, TiledDetections
    if isinstance(detections, (Detections, TiledDetections, FusedDetections)) or (isinstance(detections, tuple) and len(detections) == 3 and B == 1
                                                                    and hasattr(detections[0], "shape")):
        detections = [detections]
    if not isinstance(detections, (list, tuple)) or len(detections) != B:
        raise ValueError(f"draw_detections: expected one entry of detections per image ({B}), got {type(detections).__name__}"
                         + (f" of {len(detections)}" if isinstance(detections, (list, tuple)) else ""))
    triples = []
    for d in detections:
        if isinstance(d, (Detections, TiledDetections, FusedDetections)):
            triples.append((d.boxes, d.labels, d.scores))
        elif isinstance(d, (tuple, list)) and len(d) == 3:
            triples.append(tuple(d))
        else:
            raise ValueError("draw_detections: detections must be Detections / TiledDetections / FusedDetections in 'xyxy' or (boxes, labels, scores or None)")
    has_scores = [t[2] is not None for t in triples]
    if any(has_scores) != all(has_scores):
        raise ValueError("draw_detections: scores are given for some images and not for others")
    scored = bool(want_scores) and all(has_scores)
    rows = []
    for bx, lb, sc in triples:
        bx = torch.as_tensor(bx)
        if bx.numel() % 4 or (bx.dim() and bx.numel() and bx.shape[-1] != 4):
            raise ValueError(f"draw_detections: boxes must be [k, 4] (x0, y0, x1, y1 in pixels), got {tuple(bx.shape)}")
        bx = bx.to(torch.float32).reshape(-1, 4)
        lb = torch.as_tensor(lb).to(torch.int64).reshape(-1)
        sc = None if not scored else torch.as_tensor(sc).to(torch.float32).reshape(-1)
        if lb.shape[0] != bx.shape[0] or (sc is not None and sc.shape[0] != bx.shape[0]):
            raise ValueError(f"draw_detections: {bx.shape[0]} boxes, {lb.shape[0]} labels" + ("" if sc is None else f", {sc.shape[0]} scores"))
        if bx.shape[0] > hip.TILE_MAX_CAND:
            raise ValueError(f"draw_detections: {bx.shape[0]} detections on one image, at most {hip.TILE_MAX_CAND}")
        rows.append((bx, lb, sc))
    return rows, scored


def _pack_detections(rows, scored, device):
    """boxes [B, D, 4], labels [B, D], scores [B, D] or None on the device, counts on the host: torch glue."""
    B = len(rows)
    counts = [int(r[0].shape[0]) for r in rows]
    D = max(max(counts), 1)
    boxes = torch.zeros(B, D, 4, dtype=torch.float32, device=device)
    labels = torch.zeros(B, D, dtype=torch.int64, device=device)
    scores = torch.zeros(B, D, dtype=torch.float32, device=device) if scored else None
    for b, (bx, lb, sc) in enumerate(rows):
        k = counts[b]
        if k:
            boxes[b, :k] = bx.to(device)
            labels[b, :k] = lb.to(device)
            if scored:
                scores[b, :k] = sc.to(device)
    return boxes, labels, scores, np.array(counts, np.int32)


def _names_table(class_names, device):
    if class_names is None or len(class_names) == 0:
        return None, None, 0, 1
    codes = [encode_text(n) for n in class_names]
    cap = max(1, max(len(c) for c in codes))
    if cap > hip.OVERLAY_MAX_NAME:
        raise ValueError(f"draw_detections: a class name of {cap} characters, at most {hip.OVERLAY_MAX_NAME}")
    table = np.zeros((len(codes), cap), np.uint8)
    for i, c in enumerate(codes):
        table[i, :len(c)] = c
    lens = np.array([len(c) for c in codes], np.int32)
    return torch.from_numpy(table).to(device), torch.from_numpy(lens).to(device), len(codes), cap


def draw_detections(images, detections, class_names=None, *, scores=True, colors=None, thickness=2, scale=None, label_alpha=255,
                    fill_alpha=0, heat=None, heat_extent=None, heat_alpha=160, colormap=None, out=None, heat_scale=None, atlas=None):
    """Draw `detections` onto `images`; returns a list of uint8 [h_i, w_i, 3] DEVICE tensors, views of one packed buffer (every image
    16-byte aligned in it).  One call of detr_hip_overlay: at most two launches, no host synchronisation.

    images: uint8 [h, w, 3] host arrays (uploaded once through one pinned staging buffer) or device tensors (used where they are), one
      or a list of mixed sizes; or a RaggedFrames.  detections: per image a Detections / TiledDetections / FusedDetections with boxes in "xyxy" pixels,
      or a (boxes [k, 4], labels [k], scores [k] or None) triple, e.g. ground truth.  class_names: a sequence indexed by label (a label
      beyond it is drawn with its score alone, or without a label).  scores=False leaves the scores out of the labels.
    colors: uint8 [n, 3] indexed by label % n (None: class_palette(max(len(class_names), 100))).  thickness: outline width in pixels,
      grown inwards.  scale: font scale, an int or one per image (None: default_scale(h_i)).  label_alpha / fill_alpha (0..255): opacity
      of the label background and of a tint over the box interior.
    heat: float32 [B, Hf, Wf] device tensor blended under the boxes through `colormap` (uint8 [256, 3]; None: heat_colormap()) with
      opacity value * heat_alpha; values are multiplied by heat_scale (a [B] device tensor; None: 1) and clamped to [0, 1].
      heat_extent [B, 2]: the (fractional) number of map cells (high, wide) image b covers from the map's top-left (None: the whole
      map); the map is sampled bilinearly.
    out: a list of uint8 [h_i, w_i, 3] device tensors to draw into instead of a new buffer; out[i] may BE images[i] (in place).
    atlas: (uint8 [n_glyph, gh, gw], digit0, colon, dot) to draw with another font: class_names are then sequences of glyph indices."""
    d, keep, result = plan_overlay(images, detections, class_names, scores=scores, colors=colors, thickness=thickness, scale=scale,
                                   label_alpha=label_alpha, fill_alpha=fill_alpha, heat=heat, heat_extent=heat_extent, heat_alpha=heat_alpha,
                                   colormap=colormap, out=out, heat_scale=heat_scale, atlas=atlas)
    launch_overlay(d)
    del keep                    # (freed blocks are reused in stream order: the launches above still own them)
    return result


def launch_overlay(d):
    """One call of detr_hip_overlay on the current stream for a descriptor plan_overlay built."""
    hip._check(hip.load().detr_hip_overlay(byref(d), hip._stream()), "detr_hip_overlay")


def plan_overlay(images, detections, class_names=None, *, scores=True, colors=None, thickness=2, scale=None, label_alpha=255,
                    fill_alpha=0, heat=None, heat_extent=None, heat_alpha=160, colormap=None, out=None, heat_scale=None, atlas=None):
    """draw_detections without the launch: (descriptor, the tensors it points into, the output views).  The caller keeps the second
    value alive while it launches the first (launch_overlay), any number of times: scripts/micro_overlay.py times the call that way."""
    for name, a in (("label_alpha", label_alpha), ("fill_alpha", fill_alpha), ("heat_alpha", heat_alpha)):
        if not 0 <= int(a) <= 255:
            raise ValueError(f"draw_detections: {name}={a} must be in 0..255")
    if not 1 <= int(thickness) <= hip.OVERLAY_MAX_THICKNESS:
        raise ValueError(f"draw_detections: thickness={thickness} must be in 1..{hip.OVERLAY_MAX_THICKNESS}")
    ragged = images if isinstance(images, RaggedFrames) else None
    if ragged is None:
        images, sizes, on_device = _check_frames(images)
    else:
        sizes = ragged.sizes
    B = sizes.shape[0]
    rows, scored = _check_detections(detections, B, scores)
    if scale is not None:
        scales = np.broadcast_to(np.asarray(scale, np.int64), (B,)).astype(np.int32)
        if (scales < 1).any() or (scales > hip.OVERLAY_MAX_SCALE).any():
            raise ValueError(f"draw_detections: scale={scale} must be in 1..{hip.OVERLAY_MAX_SCALE}")
    else:
        scales = np.array([default_scale(h) for h in sizes[:, 0]], np.int32)
    if colors is None:
        colors = class_palette(max(100, 0 if class_names is None else len(class_names)))
    colors_t = torch.as_tensor(colors)
    if colors_t.dtype != torch.uint8 or colors_t.dim() != 2 or colors_t.shape[1] != 3 or colors_t.shape[0] < 1:
        raise ValueError("draw_detections: colors must be uint8 [n, 3] with n >= 1")
    # ---- everything above ran on the host; from here on the device
    if ragged is not None:
        dev, keep, src_base, src_off = ragged.buffer.device, [ragged.buffer], ragged.buffer.data_ptr(), ragged.offsets
    else:
        dev = images[0].device if on_device else torch.device(f"cuda:{torch.cuda.current_device()}")
        keep, src_base, src_off = _upload_frames(images, on_device, dev)
    boxes, labels, score_t, counts = _pack_detections(rows, scored, dev)
    D = boxes.shape[1]
    colors_t = colors_t.to(dev).contiguous()
    font_t, cmap_t = _constants(dev)
    digit0, colon, dot = ord("0") - FONT_FIRST, ord(":") - FONT_FIRST, ord(".") - FONT_FIRST
    if atlas is not None:
        font, digit0, colon, dot = atlas
        font_t = torch.as_tensor(font)
        if font_t.dtype != torch.uint8 or font_t.dim() != 3:
            raise ValueError("draw_detections: atlas must be (uint8 [n_glyph, gh, gw], digit0, colon, dot)")
        font_t = font_t.to(dev).contiguous()
        names_t, lens_t, n_names, cap = _names_table_raw(class_names, dev)
    else:
        names_t, lens_t, n_names, cap = _names_table(class_names, dev)

    # ---- destination: every image 16-byte aligned in one packed buffer, or the caller's tensors
    if out is None:
        nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3
        dst_off = np.zeros(B, np.int64)
        dst_off[1:] = np.cumsum((nbytes + 15) & ~15)[:-1]
        dst_buf = torch.empty(int(dst_off[-1] + ((nbytes[-1] + 15) & ~15)), dtype=torch.uint8, device=dev)
        dst_base = dst_buf.data_ptr()
        result = [dst_buf[o:o + n].view(int(h), int(w), 3) for o, n, (h, w) in zip(dst_off.tolist(), nbytes.tolist(), sizes.tolist())]
    else:
        result = list(out) if isinstance(out, (list, tuple)) else [out]
        if len(result) != B or any(not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
                                        and tuple(t.shape) == (int(h), int(w), 3)) for t, (h, w) in zip(result, sizes.tolist())):
            raise ValueError("draw_detections: out must be one contiguous uint8 [h_i, w_i, 3] device tensor per image")
        dst_base = min(t.data_ptr() for t in result)
        dst_off = np.array([t.data_ptr() - dst_base for t in result], np.int64)
        same = [dst_base + d == src_base + s for d, s in zip(dst_off.tolist(), src_off.tolist())]
        if any(same) and not all(same):
            raise ValueError("draw_detections: out must be the images themselves (in place) or other tensors, not a mixture")

    # ---- heat
    if heat is not None:
        if not (isinstance(heat, torch.Tensor) and heat.is_cuda and heat.dtype == torch.float32 and heat.dim() == 3 and heat.shape[0] == B
                and heat.shape[1] >= 1 and heat.shape[2] >= 1):
            raise ValueError(f"draw_detections: heat must be a float32 device tensor [B={B}, Hf, Wf]")
        Hf, Wf = int(heat.shape[1]), int(heat.shape[2])
        step, valid = heat_geometry(np.tile([[Hf, Wf]], (B, 1)) if heat_extent is None else heat_extent, sizes, Hf, Wf)
        if heat_scale is None:
            heat_scale = torch.ones(B, dtype=torch.float32, device=dev)
        if not (isinstance(heat_scale, torch.Tensor) and heat_scale.is_cuda and heat_scale.dtype == torch.float32 and tuple(heat_scale.shape) == (B,)):
            raise ValueError("draw_detections: heat_scale must be a float32 device tensor [B]")
        heat_scale = heat_scale.contiguous()
        if colormap is not None:
            cmap_t = torch.as_tensor(colormap)
            if cmap_t.dtype != torch.uint8 or tuple(cmap_t.shape) != (256, 3):
                raise ValueError("draw_detections: colormap must be uint8 [256, 3]")
            cmap_t = cmap_t.to(dev).contiguous()
    else:
        step, valid = np.zeros((B, 2), np.float32), np.zeros((B, 2), np.int32)

    # ---- every small per-image array in one transfer: src_off, dst_off (int64) | sizes, counts, scale, map_valid (int32) | map_step
    meta = np.concatenate([src_off.astype(np.int64).view(np.uint8), dst_off.astype(np.int64).view(np.uint8),
                           np.ascontiguousarray(sizes, np.int32).reshape(-1).view(np.uint8), counts.view(np.uint8), scales.view(np.uint8),
                           np.ascontiguousarray(valid).reshape(-1).view(np.uint8), np.ascontiguousarray(step).reshape(-1).view(np.uint8)])
    meta_d = torch.from_numpy(meta).to(dev)
    p = meta_d.data_ptr()
    sizes_h = np.ascontiguousarray(sizes, np.int32)

    d = hip.OverlayDesc()
    d.B, d.D = B, D
    d.src, d.src_off, d.dst, d.dst_off = src_base, p, dst_base, p + 8 * B
    d.sizes, d.sizes_host = p + 16 * B, sizes_h.ctypes.data
    d.counts, d.scale = p + 24 * B, p + 28 * B
    d.boxes, d.labels, d.scores = boxes.data_ptr(), labels.data_ptr(), hip.ptr(score_t)
    d.thickness, d.label_alpha, d.fill_alpha, d.heat_alpha = int(thickness), int(label_alpha), int(fill_alpha), int(heat_alpha)
    d.colors, d.n_colors = colors_t.data_ptr(), int(colors_t.shape[0])
    d.names, d.name_len, d.n_names, d.name_cap = hip.ptr(names_t), hip.ptr(lens_t), n_names, cap
    d.atlas, d.n_glyph, d.gh, d.gw = font_t.data_ptr(), int(font_t.shape[0]), int(font_t.shape[1]), int(font_t.shape[2])
    d.glyph_digit0, d.glyph_colon, d.glyph_dot = int(digit0), int(colon), int(dot)
    if heat is not None:
        d.heat, d.sH_b, d.sH_y, d.sH_x, d.Hf, d.Wf = heat.data_ptr(), heat.stride(0), heat.stride(1), heat.stride(2), Hf, Wf
        d.map_valid, d.map_step, d.map_scale, d.lut = p + 32 * B, p + 40 * B, heat_scale.data_ptr(), cmap_t.data_ptr()
    need = int(hip.load().detr_hip_workspace_bytes_overlay(byref(d)))
    if need < 0:
        raise RuntimeError(f"detr_hip_workspace_bytes_overlay rejected the descriptor: {hip.load().detr_hip_last_error().decode()}")
    ws = torch.empty(need + 4, dtype=torch.uint8, device=dev)              # the command list, then the status word
    status = ws[need:need + 4]
    status.zero_()
    d.workspace, d.workspace_bytes, d.status = ws.data_ptr(), need, ws.data_ptr() + need
    keep += [boxes, labels, score_t, colors_t, font_t, cmap_t, names_t, lens_t, meta_d, sizes_h, ws, heat, heat_scale]
    return d, keep, result


def _names_table_raw(class_names, device):
    """class_names as sequences of glyph indices of a caller's atlas."""
    if class_names is None or len(class_names) == 0:
        return None, None, 0, 1
    cap = max(1, max(len(c) for c in class_names))
    if cap > hip.OVERLAY_MAX_NAME:
        raise ValueError(f"draw_detections: a class name of {cap} glyphs, at most {hip.OVERLAY_MAX_NAME}")
    table = np.zeros((len(class_names), cap), np.uint8)
    for i, c in enumerate(class_names):
        table[i, :len(c)] = np.asarray(c, np.uint8)
    lens = np.array([len(c) for c in class_names], np.int32)
    return torch.from_numpy(table).to(device), torch.from_numpy(lens).to(device), len(class_names), cap


def numpy_bbox_to_image(image, bbox_list, labels=None, scores=None, class_name=[], config=None):
    """inference.py:10-65 with the reference's signature: a float32 image [h, w, 3] -- de-normalised as inference.py:15-19 when
    `config` is given (normalized_method "torch_resnet"), else taken as RGB in [0, 1] --, normalised (xc, yc, w, h) boxes, labels
    (None: all 0) and optional scores.  Returns a NumPy image with the boxes drawn by draw_detections: uint8 with `config`, float32 in
    [0, 1] without (the reference draws into whichever of the two it holds)."""
    image = np.asarray(image)
    assert image.dtype == np.float32 and len(image.shape) == 3                        # inference.py:13
    method = None if config is None else config.normalized_method
    if method == "torch_resnet":
        channel_avg = np.array([0.485, 0.456, 0.406])
        channel_std = np.array([0.229, 0.224, 0.225])
        frame = ((image * channel_std) + channel_avg)
        frame = (frame * 255).astype(np.uint8)                                         # inference.py:18-19
    elif method == "tf_resnet":
        raise ValueError("numpy_bbox_to_image: normalized_method 'tf_resnet' is not supported (the reference's branch adds an undefined `mean`)")
    else:
        frame = np.clip(np.rint(image.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    h, w = frame.shape[:2]
    bbox = np.asarray(bbox_list, np.float32).reshape(-1, 4)
    xyxy = np.stack([(bbox[:, 0] - bbox[:, 2] / 2) * w, (bbox[:, 1] - bbox[:, 3] / 2) * h,
                     (bbox[:, 0] + bbox[:, 2] / 2) * w, (bbox[:, 1] + bbox[:, 3] / 2) * h], 1).astype(np.float32)
    if labels is None:
        labels = np.zeros(bbox.shape[0], np.int64)                                     # inference.py:29
    sc = None if scores is None or len(scores) == 0 else np.asarray(scores, np.float32)
    drawn = draw_detections([frame], [(xyxy, np.asarray(labels, np.int64), sc)], list(class_name))[0].cpu().numpy()
    return drawn if method == "torch_resnet" else drawn.astype(np.float32) / np.float32(255.0)
