"""Micro-benchmark: the training augmentation kernel (csrc/augment.hip) at the reference's training shape -- B = 8 sources of
480 x 640 -> 800 x 1333, final cubic resize, half of the images through the affine zoom, the rest plain -- timed with HIP
events on the kernel launch alone (records and images already on the device), next to the all-plain and all-affine batches;
plus the host side of the loader (PIL decode + records + boxes) at num_workers = 4 on generated JPEGs.
usage: python scripts/micro_augment.py [--out FILE.json]"""
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "detr-tensorflow_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

from detr_tf import _hip as hip
from detr_tf.data import transformation as T
from detr_tf.data.processing import normalization_table

B, HS, WS, HD, WD = 8, 480, 640, 800, 1333


def timeit(fn, inner=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(7):
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / inner * 1e3)
    return best


def kernel_us(records, src, lut, perm, dst):
    offs = np.arange(B, dtype=np.int64) * HS * WS * 3
    irec, frec = T.pack_records(records, offs)
    ir, fr = torch.from_numpy(irec).cuda(), torch.from_numpy(frec).cuda()
    cperm = (ctypes.c_int32 * 3)(*perm)
    lib = hip.load()

    def run():
        hip._check(lib.detr_hip_augment(src.data_ptr(), src.numel(), ir.data_ptr(), fr.data_ptr(), B, HD, WD, lut.data_ptr(),
                                        ctypes.cast(cperm, ctypes.c_void_p), dst.data_ptr(), hip._stream()), "detr_hip_augment")
    return timeit(run)


def decode_rate(n=64, workers=4):
    from PIL import Image
    from detr_tf.data.loader import DetectionDataset, Sample

    class Cfg:
        image_size, normalized_method = (HD, WD), "torch_resnet"
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        samples = []
        base = rng.integers(0, 256, (HS // 8, WS // 8, 3)).astype(np.uint8)
        for i in range(n):
            im = np.kron(base, np.ones((8, 8, 1), np.uint8)) + rng.integers(0, 24, (HS, WS, 3)).astype(np.uint8)
            path = os.path.join(d, f"{i}.jpg")
            Image.fromarray(im).save(path, quality=90)
            samples.append(Sample(path, np.array([[0.5, 0.5, 0.3, 0.3]], np.float32), np.array([[1]], np.int64)))
        ds = DetectionDataset(samples, Cfg(), B, augmentation=True, seed=0, num_workers=workers)
        for _ in ds.host_batches():
            pass                                             # warm the page cache
        t0 = time.perf_counter()
        count = sum(len(b) for b in ds.host_batches())
        return count / (time.perf_counter() - t0)


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    hip.load()
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.integers(0, 256, B * HS * WS * 3).astype(np.uint8)).cuda()
    lut_np, perm = normalization_table("torch_resnet")
    lut = torch.from_numpy(lut_np).cuda()
    dst = torch.empty(B, HD, WD, 3, dtype=torch.float32, device="cuda")
    plain = T.Transform(HS, WS, iff=T.CUBIC)
    affine = T.Transform(HS, WS, flip=True, kind=T.KINDS["affine"], iff=T.CUBIC, sx=1.2, sy=0.8)
    res = {"shape": f"B{B} {HS}x{WS} -> {HD}x{WD}, final cubic"}
    res["half_affine_us"] = kernel_us([affine if b % 2 else plain for b in range(B)], src, lut, perm, dst)
    res["plain_us"] = kernel_us([plain] * B, src, lut, perm, dst)
    res["all_affine_us"] = kernel_us([affine] * B, src, lut, perm, dst)
    res["write_bytes"] = B * HD * WD * 3 * 4
    res["write_floor_us_at_6.3TBps"] = res["write_bytes"] / 6.3e12 * 1e6
    res["host_images_per_s_4_workers"] = decode_rate()
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
