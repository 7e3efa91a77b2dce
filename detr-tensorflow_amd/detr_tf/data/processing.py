"""Input stage of the drop-in API (reference detr_tf/data/processing.py:6-55, data/transformation.py:82-91).

The reference prepares every batch on the host: imgaug resize to `config.image_size` (uint8), `normalized_images`
(float64 NumPy arithmetic, cast to float32) and `pad_labels` (TF ops), then ships a float32 batch to the device.
`DeviceInputStage` does the same work on the GPU in two launches of csrc/input_stage.hip: the uint8 batch is what crosses
PCIe (a quarter of the bytes), resize + normalisation write the fp32 NHWC tensor the model reads, and the padded target
tensors with their in-band header row are built from the ragged box lists.  `normalized_images` / `pad_labels` keep the
reference's host-side signatures for callers that still want NumPy.
"""
import ctypes
from ctypes import byref

import numpy as np
import torch

from .. import _hip as hip

INTERPOLATIONS = {"nearest": 0, "linear": 1, "cubic": 2}
MAX_ROWS = 100                       # processing.py:49-50: 99 boxes + the header row


def normalization_table(method):
    """[3][256] float32: the value `normalized_images` (processing.py:6-21) yields for every uint8 pixel value, computed in
    float64 with the reference's own expression and rounded once; plus the source channel each output channel reads."""
    x = np.arange(256, dtype=np.float64)
    if method == "torch_resnet":
        channel_avg = np.array([0.485, 0.456, 0.406])
        channel_std = np.array([0.229, 0.224, 0.225])
        lut = ((x[None, :] / 255.0 - channel_avg[:, None]) / channel_std[:, None]).astype(np.float32)
        perm = (0, 1, 2)
    elif method == "tf_resnet":
        mean = np.array([103.939, 116.779, 123.68])
        lut = (x[None, :] - mean[:, None]).astype(np.float32)
        perm = (2, 1, 0)             # image[..., ::-1]: RGB -> BGR
    else:
        raise Exception("Can't handler thid normalized method")      # processing.py:21
    return np.ascontiguousarray(lut), perm


def normalized_images(image, config):
    """processing.py:6-21 on the host (NumPy), same arithmetic and dtype."""
    if config.normalized_method == "torch_resnet":
        channel_avg = np.array([0.485, 0.456, 0.406])
        channel_std = np.array([0.229, 0.224, 0.225])
        return ((image / 255.0 - channel_avg) / channel_std).astype(np.float32)
    if config.normalized_method == "tf_resnet":
        mean = [103.939, 116.779, 123.68]
        return (image[..., ::-1] - mean).astype(np.float32)
    raise Exception("Can't handler thid normalized method")


def pad_labels(images, t_bbox, t_class):
    """processing.py:35-55 for ONE sample on the host: header row [n, 0, 0, 0] / [0], zero padding to 100 rows."""
    t_bbox = np.asarray(t_bbox, np.float32).reshape(-1, 4)
    t_class = np.asarray(t_class, np.int64).reshape(-1, 1)
    n = t_bbox.shape[0]
    if n > MAX_ROWS - 1:
        raise ValueError(f"at most {MAX_ROWS - 1} boxes per image (the padded layout has {MAX_ROWS} rows incl. the header)")
    out_b = np.zeros((MAX_ROWS, 4), np.float32)
    out_c = np.zeros((MAX_ROWS, 1), np.int64)
    out_b[0, 0] = n
    out_b[1:1 + n] = t_bbox
    out_c[1:1 + n] = t_class
    return images, out_b, out_c


class DeviceInputStage:
    """uint8 images (+ ragged targets) -> what `model(...)` / `get_losses(...)` consume, on the device."""

    def __init__(self, config, device=None, interpolation="cubic"):
        self.device = torch.device(device or f"cuda:{torch.cuda.current_device()}")
        self.image_size = tuple(int(v) for v in config.image_size)                      # (height, width), training_config.py:49
        lut, self.perm = normalization_table(config.normalized_method)
        self.lut = torch.from_numpy(lut).to(self.device)
        self.interpolation = INTERPOLATIONS[interpolation]
        self._aug_img = self._aug_rec = self._aug_event = None         # augmented(): pinned staging buffers, last copy's event
        self.last_upload = None                                        # overlay.RaggedFrames of the last ragged batch: its frames stay on the device
        hip.load()

    def images(self, batch_uint8, out=None):
        """[B, H, W, 3] uint8 (NumPy or torch, host or device) -> float32 [B, image_size[0], image_size[1], 3] on the device."""
        src = torch.as_tensor(batch_uint8)
        if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[-1] != 3:
            raise TypeError("DeviceInputStage.images expects a uint8 tensor [B, H, W, 3]")
        src = src.to(self.device, non_blocking=True).contiguous()
        B, Hs, Ws, _ = src.shape
        Hd, Wd = self.image_size
        dst = out if out is not None else torch.empty(B, Hd, Wd, 3, dtype=torch.float32, device=self.device)
        d = hip.InputDesc()
        d.B, d.Hs, d.Ws, d.Hd, d.Wd = B, Hs, Ws, Hd, Wd
        d.src, d.src_batch_stride, d.dst, d.lut = src.data_ptr(), Hs * Ws * 3, dst.data_ptr(), self.lut.data_ptr()
        d.perm[0], d.perm[1], d.perm[2] = self.perm
        d.interpolation = self.interpolation
        hip._check(hip.load().detr_hip_input_stage(byref(d), hip._stream()), "detr_hip_input_stage")
        return dst

    def images_padded(self, images_uint8, canvas=None):
        """Padded mixed-size batch: a list of uint8 images [h_i, w_i, 3] (NumPy or torch, each already at its final size: no
        resize here) -> (images float32 [B, H, W, 3], masks bool [B, H, W]) on the device, H / W the largest h_i / w_i (or
        `canvas` = (H, W)).  Image i sits at the top-left; its pixels are normalised exactly as images() does, the padding is 0.0
        and masks is True there -- the reference's (images, masks) input (detr.py:65-72).  One launch."""
        srcs = [torch.as_tensor(im) for im in images_uint8]
        if not srcs or any(s.dtype != torch.uint8 or s.dim() != 3 or s.shape[-1] != 3 for s in srcs):
            raise TypeError("DeviceInputStage.images_padded expects a non-empty list of uint8 images [h, w, 3]")
        hw = np.array([[s.shape[0], s.shape[1]] for s in srcs], np.int32)
        H, W = (int(hw[:, 0].max()), int(hw[:, 1].max())) if canvas is None else (int(canvas[0]), int(canvas[1]))
        if (hw[:, 0] > H).any() or (hw[:, 1] > W).any():
            raise ValueError(f"images_padded: an image is larger than the {H} x {W} canvas")
        sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
        offsets = np.zeros(len(srcs), np.int64)
        offsets[1:] = np.cumsum(sizes)[:-1]
        packed = torch.cat([s.reshape(-1) for s in srcs]).to(self.device, non_blocking=True)
        off_d = torch.from_numpy(offsets).to(self.device)
        hw_d = torch.from_numpy(hw.reshape(-1)).to(self.device)
        B = len(srcs)
        dst = torch.empty(B, H, W, 3, dtype=torch.float32, device=self.device)
        mask = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        perm = (ctypes.c_int32 * 3)(*self.perm)
        hip._check(hip.load().detr_hip_input_stage_padded(packed.data_ptr(), off_d.data_ptr(), hw_d.data_ptr(), B, H, W, self.lut.data_ptr(),
                                                          ctypes.cast(perm, ctypes.c_void_p), dst.data_ptr(), mask.data_ptr(), hip._stream()),
                   "detr_hip_input_stage_padded")
        return dst, mask.view(torch.bool)

    def _upload_ragged(self, srcs, rec_arrays):
        """Staging shared by augmented() and augmented_padded(): the uint8 images are packed back to back, `rec_arrays(offsets)`
        builds the record arrays (NumPy) from the images' byte offsets, and both cross PCIe through the pinned staging buffers,
        one copy each; the buffers are reused across batches once their last copy has finished.  Returns (src on the device,
        its size in bytes, the record bytes on the device laid out back to back, the record arrays on the host)."""
        sizes = np.array([s.size for s in srcs], np.int64)
        offsets = np.zeros(len(srcs), np.int64)
        offsets[1:] = np.cumsum(sizes)[:-1]
        total = int(sizes.sum())
        recs = rec_arrays(offsets)
        rec_bytes = sum(r.nbytes for r in recs)
        if self._aug_event is not None:
            self._aug_event.synchronize()           # the previous batch's copies out of the staging buffers have finished
        if self._aug_img is None or self._aug_img.numel() < total:
            self._aug_img = torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True)
        if self._aug_rec is None or self._aug_rec.numel() < rec_bytes:
            self._aug_rec = torch.empty(max(rec_bytes, 4096), dtype=torch.uint8, pin_memory=True)
        img_h, rec_h = self._aug_img.numpy(), self._aug_rec.numpy()
        for s, o in zip(srcs, offsets):
            img_h[o:o + s.size] = s.reshape(-1)
        at = 0
        for r in recs:
            rec_h[at:at + r.nbytes] = r.view(np.uint8).reshape(-1)
            at += r.nbytes
        src = self._aug_img[:total].to(self.device, non_blocking=True)
        rec = self._aug_rec[:rec_bytes].to(self.device, non_blocking=True)
        self._aug_event = torch.cuda.Event()
        self._aug_event.record()
        from ..overlay import RaggedFrames
        self.last_upload = RaggedFrames(src, offsets, [s.shape[:2] for s in srcs])      # Detector.draw(images=None) draws on these
        return src, total, rec, recs

    def augmented(self, images_uint8, records):
        """Training batch with augmentation: a list of uint8 images [h_i, w_i, 3] (host, each at its own size) and one
        transformation.Transform record per image -> float32 [B, image_size[0], image_size[1], 3] on the device: flip,
        stage B, final resize and normalisation in one launch of csrc/augment.hip.  Images and records cross PCIe through
        pinned staging buffers, one copy each; the buffers are reused across batches once their last copy has finished."""
        from . import transformation as T
        srcs = [np.asarray(im) for im in images_uint8]
        if not srcs or len(srcs) != len(records) or any(s.dtype != np.uint8 or s.ndim != 3 or s.shape[-1] != 3 for s in srcs):
            raise TypeError("DeviceInputStage.augmented expects a non-empty list of uint8 images [h, w, 3] and one record per image")
        for s, t in zip(srcs, records):
            if (t.h0, t.w0) != s.shape[:2]:
                raise ValueError(f"transform record for a {t.h0} x {t.w0} image given a {s.shape[0]} x {s.shape[1]} image")
            T.check_record(t, self.image_size)
        src, total, rec, (irec, _) = self._upload_ragged(srcs, lambda offsets: T.pack_records(records, offsets))
        B = len(srcs)
        Hd, Wd = self.image_size
        dst = torch.empty(B, Hd, Wd, 3, dtype=torch.float32, device=self.device)
        perm = (ctypes.c_int32 * 3)(*self.perm)
        hip._check(hip.load().detr_hip_augment(src.data_ptr(), total, rec.data_ptr(), rec.data_ptr() + irec.nbytes, B, Hd, Wd,
                                               self.lut.data_ptr(), ctypes.cast(perm, ctypes.c_void_p), dst.data_ptr(), hip._stream()),
                   "detr_hip_augment")
        return dst

    def augmented_padded(self, images_uint8, records, canvas=None, multiple=32):
        """Aspect-preserving multi-scale batch: a list of uint8 images [h_i, w_i, 3] (host, each at its own size) and one
        transformation.PaddedRecord per image -> (images float32 [B, H, W, 3], masks bool [B, H, W]) on the device.  Image i is
        flipped, windowed, resized to its own (hd_i, wd_i) and normalised at the top-left of the canvas; the padding is 0.0 and
        masks is True there.  One launch of csrc/augment_padded.hip; staging as in augmented().  canvas=None: the batch's
        largest hd / wd, each rounded up to `multiple`; canvas=(H, W): fixed (what a captured graph needs), ValueError if an
        image does not fit."""
        from . import transformation as T
        srcs = [np.asarray(im) for im in images_uint8]
        if not srcs or len(srcs) != len(records) or any(s.dtype != np.uint8 or s.ndim != 3 or s.shape[-1] != 3 for s in srcs):
            raise TypeError("DeviceInputStage.augmented_padded expects a non-empty list of uint8 images [h, w, 3] and one record per image")
        if canvas is None:
            m = max(1, int(multiple))
            H, W = (-(-max(int(t.hd) for t in records) // m) * m, -(-max(int(t.wd) for t in records) // m) * m)
        else:
            H, W = int(canvas[0]), int(canvas[1])
        for s, t in zip(srcs, records):
            if (t.h0, t.w0) != s.shape[:2]:
                raise ValueError(f"padded record for a {t.h0} x {t.w0} image given a {s.shape[0]} x {s.shape[1]} image")
            T.check_padded_record(t, (H, W))
        src, total, rec, _ = self._upload_ragged(srcs, lambda offsets: (T.pack_padded_records(records, offsets),))
        B = len(srcs)
        dst = torch.empty(B, H, W, 3, dtype=torch.float32, device=self.device)
        mask = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        perm = (ctypes.c_int32 * 3)(*self.perm)
        hip._check(hip.load().detr_hip_augment_padded(src.data_ptr(), total, rec.data_ptr(), B, H, W, self.lut.data_ptr(),
                                                      ctypes.cast(perm, ctypes.c_void_p), dst.data_ptr(), mask.data_ptr(), hip._stream()),
                   "detr_hip_augment_padded")
        return dst, mask.view(torch.bool)

    def augmented_tiles(self, images_uint8, records_per_image, canvas=None, multiple=32):
        """Sliced inference: a list of B uint8 images [h_i, w_i, 3] (host) and, per image, a LIST of transformation.PaddedRecord
        (transformation.tile_records: windows of that image) -> (images float32 [N, H, W, 3], masks bool [N, H, W], tile_start int32
        [B + 1]) with N the number of records, the tiles of image i at rows [tile_start[i], tile_start[i + 1]).  Every source image
        is packed and crosses PCIe ONCE: all records of an image point at the same byte offset.  One launch of
        csrc/augment_padded.hip; staging and canvas as in augmented_padded()."""
        from . import transformation as T
        srcs = [np.asarray(im) for im in images_uint8]
        if not srcs or len(srcs) != len(records_per_image) or any(s.dtype != np.uint8 or s.ndim != 3 or s.shape[-1] != 3 for s in srcs):
            raise TypeError("DeviceInputStage.augmented_tiles expects a non-empty list of uint8 images [h, w, 3] and one list of records per image")
        counts = [len(recs) for recs in records_per_image]
        records = [t for recs in records_per_image for t in recs]
        if not records:
            raise ValueError("augmented_tiles: no records")
        tile_start = np.zeros(len(srcs) + 1, np.int32)
        tile_start[1:] = np.cumsum(counts)
        owner = np.repeat(np.arange(len(srcs)), counts)
        if canvas is None:
            m = max(1, int(multiple))
            H, W = (-(-max(int(t.hd) for t in records) // m) * m, -(-max(int(t.wd) for t in records) // m) * m)
        else:
            H, W = int(canvas[0]), int(canvas[1])
        for i, t in zip(owner, records):
            if (t.h0, t.w0) != srcs[i].shape[:2]:
                raise ValueError(f"padded record for a {t.h0} x {t.w0} image given a {srcs[i].shape[0]} x {srcs[i].shape[1]} image")
            T.check_padded_record(t, (H, W))
        src, total, rec, _ = self._upload_ragged(srcs, lambda offsets: (T.pack_padded_records(records, offsets[owner]),))
        N = len(records)
        dst = torch.empty(N, H, W, 3, dtype=torch.float32, device=self.device)
        mask = torch.empty(N, H, W, dtype=torch.uint8, device=self.device)
        perm = (ctypes.c_int32 * 3)(*self.perm)
        hip._check(hip.load().detr_hip_augment_padded(src.data_ptr(), total, rec.data_ptr(), N, H, W, self.lut.data_ptr(),
                                                      ctypes.cast(perm, ctypes.c_void_p), dst.data_ptr(), mask.data_ptr(), hip._stream()),
                   "detr_hip_augment_padded")
        return dst, mask.view(torch.bool), tile_start

    def targets(self, boxes_per_image, classes_per_image):
        """lists (one entry per image) of [n_i, 4] cx,cy,w,h boxes and [n_i] class ids -> (t_bbox [B,100,4] float32,
        t_class [B,100,1] int64) on the device, in the reference's padded layout."""
        B = len(boxes_per_image)
        counts = [int(np.asarray(b).reshape(-1, 4).shape[0]) for b in boxes_per_image]
        if max(counts, default=0) > MAX_ROWS - 1:
            raise ValueError(f"at most {MAX_ROWS - 1} boxes per image")
        offsets = np.zeros(B + 1, np.int32)
        offsets[1:] = np.cumsum(counts)
        n = int(offsets[-1])
        boxes = np.zeros((max(n, 1), 4), np.float32)
        classes = np.zeros(max(n, 1), np.int64)
        if n:
            boxes[:n] = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in boxes_per_image], 0)
            classes[:n] = np.concatenate([np.asarray(c, np.int64).reshape(-1) for c in classes_per_image], 0)
        boxes_d, classes_d = torch.from_numpy(boxes).to(self.device), torch.from_numpy(classes).to(self.device)
        off_d = torch.from_numpy(offsets).to(self.device)
        t_bbox = torch.empty(B, MAX_ROWS, 4, dtype=torch.float32, device=self.device)
        t_class = torch.empty(B, MAX_ROWS, 1, dtype=torch.int64, device=self.device)
        hip.call("detr_hip_pad_labels", boxes_d.data_ptr(), classes_d.data_ptr(), off_d.data_ptr(), B, MAX_ROWS, t_bbox.data_ptr(),
                 t_class.data_ptr())
        return t_bbox, t_class

    def __call__(self, batch_uint8, boxes_per_image, classes_per_image):
        return (self.images(batch_uint8),) + self.targets(boxes_per_image, classes_per_image)
