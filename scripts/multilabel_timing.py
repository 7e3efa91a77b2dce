"""Device time of the multi-label detection launch (csrc/detect_multilabel.hip) beside the two things it can be compared with,
on one GPU, on the same inputs:

    python scripts/multilabel_timing.py [--Q 300] [--C 92] [--K 100] [--batches 1 16] [--reps 200] [--rounds 7] [--arms abc] [--out FILE.json]

  (a) detr_hip_detect_multilabel: the K best (query, class) pairs of every image;
  (b) detr_hip_detect_scored with scoring 1: one detection per query, the K best queries (what there was before);
  (c) the same rule as (a) written in torch on the device: sigmoid -> flatten -> topk -> gather, plus the box scaling and the clip.

Logits: seeded normal noise around -4 (a focal head starts at the prior 0.01 and moves a few classes up), the background class last;
score_threshold 0, the setting of an evaluation: every pair is a candidate.  Outputs are allocated once; every timed window is
`reps` back-to-back calls on one stream between two HIP events, after a warm-up of the same shape; the arms (--arms, default abc)
are timed alternately `rounds` times and the median window is reported as microseconds per call.  A window of back-to-back calls
cannot go below the rate at which the host enqueues them, so `host_us_per_enqueue` (host clock around the same loop, before the
synchronise) is printed beside every figure: where the two are equal the host bounds the figure, where the events show more the
device does.  (a) and (c) must select the same pairs; the script reports the share of rows on which they agree -- torch's
sigmoid is not bit-identical to sigmoid_score, so a last-bit swap between two near-equal scores is possible and is not an error.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from ctypes import byref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "detr-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=300)
    ap.add_argument("--C", type=int, default=92)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--arms", default="abc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the GPU; there is no CPU fallback"
    from detr_tf import _hip as hip
    from detr_tf.inference import _fill_model_outputs, _ranked_rows
    lib = hip.load()
    dev = "cuda"
    Q, C, K, bg = args.Q, args.C, args.K, args.C - 1
    result = {"device": torch.cuda.get_device_name(0), "Q": Q, "C": C, "K": K, "reps": args.reps, "rounds": args.rounds,
              "selection": "3 histogram passes of 10 bits + 1 collecting pass (+ 1 counting pass when ties exceed the budget at the cut); "
                           "keys re-read from the logits every pass, not kept in LDS", "B": {}}
    for B in args.batches:
        gen = torch.Generator().manual_seed(B)
        logits = (torch.randn(B, Q, C, generator=gen) * 2.0 - 4.0).to(dev)
        boxes = torch.cat([torch.rand(B, Q, 2, generator=gen), torch.rand(B, Q, 2, generator=gen) * 0.5], -1).to(dev)
        sizes = torch.tensor([(800, 1333)] * B, dtype=torch.int32, device=dev)
        scale = torch.tensor([1333.0, 800.0, 1333.0, 800.0], device=dev)
        out_b, out_l, out_s, out_q = _ranked_rows(B, K, dev, 1)
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        d = hip.DetectDesc()
        _fill_model_outputs(d, logits, boxes, bg)
        d.B, d.sizes, d.score_threshold, d.max_detections, d.bbox_format, d.clip = B, sizes.data_ptr(), 0.0, K, 1, 1
        d.out_boxes, d.out_labels, d.out_scores, d.out_query, d.counts = (out_b.data_ptr(), out_l.data_ptr(), out_s.data_ptr(),
                                                                          out_q.data_ptr(), counts.data_ptr())

        def launch_a():
            hip._check(lib.detr_hip_detect_multilabel(byref(d), hip._stream()), "detr_hip_detect_multilabel")

        def launch_b():
            hip._check(lib.detr_hip_detect_scored(byref(d), 1, hip._stream()), "detr_hip_detect_scored")

        def launch_c():
            s = logits[..., :bg].sigmoid()                            # the background class is the last column
            top, idx = s.flatten(1).topk(K, dim=1)
            q, c = idx // bg, idx % bg
            cx, cy, w, h = (boxes.gather(1, q[..., None].expand(-1, -1, 4)) * scale).unbind(-1)
            xyxy = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1)
            return torch.minimum(xyxy.clamp_min(0.0), scale), c, top, q

        # the two must select the same pairs
        launch_a()
        torch.cuda.synchronize()
        a_rows = (out_l.clone(), out_q.clone(), out_s.clone(), out_b.clone())
        c_boxes, c_labels, c_scores, c_query = launch_c()
        agree = float(((a_rows[0] == c_labels) & (a_rows[1] == c_query)).float().mean())
        assert counts.tolist() == [K] * B and agree > 0.98, (counts.tolist(), agree)
        assert float((a_rows[2] - c_scores).abs().max()) < 1e-6 and float((a_rows[3] - c_boxes).abs().max()) < 1e-2

        def window(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            host = (time.perf_counter() - t0) / args.reps * 1e6
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.reps * 1e3, host

        names = {"a_detect_multilabel": launch_a, "b_detect_scored_sigmoid": launch_b, "c_torch_topk": launch_c}
        names = {k: fn for k, fn in names.items() if k[0] in args.arms}
        for fn in names.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        took = {k: [] for k in names}
        for _ in range(args.rounds):
            for k, fn in names.items():
                took[k].append(window(fn))
        row = {"rows_agreeing_with_torch": round(agree, 4)}
        for k, v in took.items():
            us = sorted(t for t, _ in v)
            row[k] = {"us_per_call": round(statistics.median(us), 2), "min": round(us[0], 2), "max": round(us[-1], 2),
                      "host_us_per_enqueue": round(statistics.median(h for _, h in v), 2)}
        result["B"][str(B)] = row
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
