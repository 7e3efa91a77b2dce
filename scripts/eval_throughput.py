"""Images/s of evaluation.eval_model with the mAP accumulation on the host (accumulate="host", the default) and on the device
(accumulate="device", csrc/map_match.hip), in one process on one GPU.

    python scripts/eval_throughput.py [--batches 60] [--warmup 6] [--rounds 3] [--precision bf16] [--out FILE.json]

Two configurations: C1 (one 480x640 image per batch) and B=8 at 800x1333.  DETR-R50 with seeded random weights; the images are
a fixed device tensor and the targets synthetic DEVICE tensors in the loaders' layout ([B, 100, 4] / [B, 100, 1] with the
header row), made from the model's own predictions so that the matching has true positives to find.  A randomly initialised
head gives all 100 queries one class, which is either no detection or 100 per image; a trained DETR keeps roughly one query in
seven.  `Spread` therefore adds one fixed seeded noise tensor to the logits after the real forward (one elementwise launch,
the same in both paths): about 18 % of the queries stay foreground, over many classes.  Per configuration both
paths are warmed up (eager pass, graph capture, first replays), then timed alternately `rounds` times over `batches` batches
each: host clock around eval_model, which ends in the read-back of the records (device path) or of the last image's
detections (host path) -- and a device synchronise after it.  The two paths must return the same maps; the script fails if not.
With --coco the same batches (plus the metadata a with_meta=True loader adds: one crowd per image, box areas, the image size) are
also timed through protocol="coco" on the device (csrc/coco_match.hip) and on the host, alternating with the two reference-protocol
loops in every round; the two COCO paths must return the same statistics.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "detr-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


class Spread:
    """The model with a fixed seeded noise on its class logits (see the module docstring)."""

    def __init__(self, model, seed=3):
        self.model, self.engine, self.seed, self.noise = model, model.engine, seed, {}

    def __call__(self, images, training=False):
        out = self.model(images, training=training)
        lg = out["pred_logits"]
        if lg.shape not in self.noise:
            g = torch.Generator().manual_seed(self.seed)
            n = 4.0 * torch.randn(tuple(lg.shape), generator=g)
            n[..., -1] += 14.0                                       # the background column wins for ~82 % of the queries
            self.noise[lg.shape] = n.to(lg.device)
        return {"pred_logits": lg + self.noise[lg.shape], "pred_boxes": out["pred_boxes"]}


def make_targets(model, images, background_class, n_max=12):
    """Device targets in the loaders' layout from the model's own detections (at most n_max per image)."""
    out = model(images, training=False)
    lab = out["pred_logits"].softmax(-1).argmax(-1)
    B = lab.shape[0]
    tb = torch.zeros(B, 100, 4, device=images.device)
    tc = torch.zeros(B, 100, 1, dtype=torch.int64, device=images.device)
    for b in range(B):
        keep = torch.nonzero(lab[b] != background_class).flatten()[:n_max]
        tb[b, 0, 0] = len(keep)
        tb[b, 1:1 + len(keep)] = out["pred_boxes"][b, keep]
        tc[b, 1:1 + len(keep), 0] = lab[b, keep]
    return tb, tc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", choices=["fp32", "bf16", "fp32x3"], default="bf16")
    ap.add_argument("--configs", default="c1,b8", help="comma list of c1 (B=1, 480x640), b8 (B=8, 800x1333)")
    ap.add_argument("--coco", action="store_true", help="also time protocol='coco' on the device and on the host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.batches < 50:
        ap.error("--batches: time at least 50 batches")
    if not torch.cuda.is_available():
        raise SystemExit("eval_throughput: needs a GPU (a timing taken elsewhere says nothing)")
    from detr_tf.evaluation import eval_model
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.training_config import TrainingConfig
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = TrainingConfig()
    cfg.background_class = 91
    names = [f"c{i}" for i in range(92)]
    shapes = {"c1": (1, 480, 640), "b8": (8, 800, 1333)}
    model = Spread(get_detr_model(cfg, include_top=True, device=str(dev), seed=0, dropout=0.0, precision=args.precision))
    result = {"precision": args.precision, "batches": args.batches, "warmup": args.warmup, "rounds": args.rounds, "configs": {}}
    for key in args.configs.split(","):
        B, H, W = shapes[key]
        images = torch.from_numpy(np.random.default_rng(7).normal(size=(B, H, W, 3)).astype(np.float32)).to(dev)
        tb, tc = make_targets(model, images, cfg.background_class)

        meta = None
        if args.coco:                                                      # what a with_meta=True loader adds to a batch
            crowd = torch.zeros(B, tb.shape[1], dtype=torch.uint8, device=dev)
            crowd[:, 1] = (tb[:, 0, 0] > 0).to(torch.uint8)                # the first target of every image is a crowd
            area = (tb[:, :, 2] * W * tb[:, :, 3] * H * 0.7).contiguous()
            area[:, 0] = 0.0
            meta = {"crowd": crowd, "area": area, "image_id": torch.arange(B, device=dev),
                    "size": torch.tensor([[H, W]] * B, dtype=torch.int32, device=dev)}

        def run(how, n):
            coco = how.startswith("coco_")
            loader = ((images, tb, tc, meta) if coco else (images, tb, tc) for _ in range(n))
            torch.cuda.synchronize()
            t = time.perf_counter()
            maps = eval_model(model, cfg, names, loader, print_result=False, accumulate=how.replace("coco_", ""),
                              protocol="coco" if coco else "reference")
            torch.cuda.synchronize()
            return time.perf_counter() - t, maps

        hows = ("host", "device") + (("coco_host", "coco_device") if args.coco else ())
        maps = {how: run(how, args.warmup)[1] for how in hows}
        times = {how: [] for how in hows}
        for _ in range(args.rounds):
            for how in hows:
                d, m = run(how, args.batches)
                times[how].append(d)
                maps[how] = m
        if maps["host"] != maps["device"]:
            raise SystemExit(f"eval_throughput: the two paths disagree at {key}: {maps}")
        ips = {how: [B * args.batches / d for d in ds] for how, ds in times.items()}
        med = {how: statistics.median(v) for how, v in ips.items()}
        result["configs"][key] = {
            "workload": f"eval_model, DETR-R50 {args.precision}, batch {B}, {H}x{W}, {args.batches} batches per timing",
            "targets_per_image": [int(x) for x in tb[:, 0, 0].tolist()],
            "detections_per_image": [int(x) for x in (model(images)["pred_logits"].argmax(-1) != cfg.background_class).sum(1).tolist()], "box_map_all": maps["host"]["box"]["all"],
            "host_images_per_s": [round(v, 2) for v in ips["host"]], "device_images_per_s": [round(v, 2) for v in ips["device"]],
            "host_median": round(med["host"], 2), "device_median": round(med["device"], 2),
            "host_ms_per_batch": round(1e3 * B / med["host"], 3), "device_ms_per_batch": round(1e3 * B / med["device"], 3),
            "device_over_host": round(med["device"] / med["host"], 4)}
        if args.coco:
            if maps["coco_host"] != maps["coco_device"]:
                raise SystemExit(f"eval_throughput: the two COCO paths disagree at {key}")
            result["configs"][key].update({
                "coco_AP": maps["coco_host"]["AP"], "coco_AR100": maps["coco_host"]["AR100"],
                "coco_host_images_per_s": [round(v, 2) for v in ips["coco_host"]], "coco_device_images_per_s": [round(v, 2) for v in ips["coco_device"]],
                "coco_host_median": round(med["coco_host"], 2), "coco_device_median": round(med["coco_device"], 2),
                "coco_device_ms_per_batch": round(1e3 * B / med["coco_device"], 3),
                "coco_device_over_reference_device": round(med["coco_device"] / med["device"], 4)})
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
