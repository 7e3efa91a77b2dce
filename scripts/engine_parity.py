"""Engine parity record: launches, buffer plan and result bytes of a fixed set of configurations, for comparing two trees.

    PYTHONPATH=<tree>/detr-tensorflow_amd python scripts/engine_parity.py record OUT_DIR [config ...]
    python scripts/engine_parity.py compare DIR_A DIR_B

`record` runs against whichever detr_tf is first on PYTHONPATH (it needs _hip._SIGNATURES, _hip.load() and the public model
API only) and writes <config>.json + <config>.npz.  Per configuration: every call of a _SIGNATURES function on the loaded
library as (name, index of the current stream in first-seen order, CRC of its non-pointer arguments -- descriptor
arguments: every field that is not a c_void_p / POINTER; DETR_PARITY_VERBOSE=1 keeps the arguments themselves), the sorted
(name, shape, dtype) of engine._bufs, and logits / boxes / loss of every step plus SHA-256 digests of every entry of P.grad,
of P.flat, adam_m and adam_v after the last step.  Train configurations run three eager steps and three through GraphedTrainStep
on 2 x 64 x 96 images, then the same on 2 x 70 x 90 (odd feature maps; every buffer is replaced).
`compare` demands equal traces, plans, bytes and digests; the scalar loss (fp32 atomics) at rel 1e-6."""
import ctypes
import hashlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.append(os.path.join(ROOT, "detr-tensorflow_amd"))      # (behind PYTHONPATH: another tree named there wins)

SIZES = ((64, 96), (70, 90))
# name -> (model keywords, engine-module switches, extras)
CONFIGS = {
    "fp32": (dict(precision="fp32"), {}, {}),
    "fp32x3": (dict(precision="fp32x3"), {}, {}),
    "bf16_drop": (dict(precision="bf16", dropout=0.1), {}, {}),
    "bf16_mask": (dict(precision="bf16", dropout=0.0), {}, dict(masks=True)),
    "bf16_dc5": (dict(precision="bf16", dropout=0.0, backbone="resnet50-dc5"), {}, {}),
    "tf_fp32": (dict(precision="fp32", tf_backbone=True), {}, {}),
    "tf_bf16": (dict(precision="bf16", tf_backbone=True), {}, {}),
    "bf16_one_stream": (dict(precision="bf16"), dict(WGRAD_STREAM=False), {}),
    "bf16_no_defer": (dict(precision="bf16"), dict(DEFER_REDUCE=False), {}),
    "bf16_unfused": (dict(precision="bf16"), dict(BWD_FUSED=False), {}),
    "bf16_ahead0": (dict(precision="bf16"), dict(DROPMASK_AHEAD=0), {}),
    "bf16_ahead1": (dict(precision="bf16"), dict(DROPMASK_AHEAD=1), {}),
    "eval_maps": (dict(precision="bf16"), {}, dict(eval_sites=("transformer/encoder/layer_1/self_attn",
                                                               "transformer/decoder/layer_0/multihead_attn"))),
    "nb_class": (dict(precision="bf16", nb_class=7), {}, {}),
}
# host-side plan queries: they launch nothing, a tree may cache or not have them, and what they answer is in the descriptors that follow
QUERIES = ("detr_hip_gemm_split_plan",)
VERBOSE = os.environ.get("DETR_PARITY_VERBOSE", "0") != "0"


def _plain(v):
    return v.value if hasattr(v, "value") else (v.decode() if isinstance(v, bytes) else v)


def _fields(s):
    """Non-pointer fields of a descriptor struct."""
    out = []
    for f in s._fields_:
        t = f[1]
        if t is ctypes.c_void_p or issubclass(t, (ctypes._Pointer, ctypes._CFuncPtr)):
            continue
        v = getattr(s, f[0])
        out.append([f[0], list(v) if isinstance(v, ctypes.Array) else v])
    return out


def _arg(a, argtype, next_int):
    if isinstance(a, ctypes.Array) and issubclass(a._type_, ctypes.Structure):
        return [_fields(a[i]) for i in range(next_int if isinstance(next_int, int) else len(a))]
    obj = getattr(a, "_obj", None)                              # byref(struct)
    if isinstance(obj, ctypes.Structure):
        return _fields(obj)
    if argtype is ctypes.c_void_p or issubclass(argtype, ctypes._Pointer):
        return None                                             # device / host address
    return _plain(a)


class Trace:
    def __init__(self, hip, torch):
        self.calls, self.streams, self.torch = [], {}, torch
        lib = hip.load()
        for name, argtypes in hip._SIGNATURES.items():
            if name not in QUERIES:
                setattr(lib, name, self._wrap(name, getattr(lib, name), argtypes))

    def _wrap(self, name, fn, argtypes):
        def call(*args):
            s = self.torch.cuda.current_stream().cuda_stream
            idx = self.streams.setdefault(s, len(self.streams))
            rec = [_arg(a, t, args[i + 1] if i + 1 < len(args) else None) for i, (a, t) in enumerate(zip(args, argtypes))]
            text = json.dumps(rec, default=str)
            self.calls.append([name, idx, text if VERBOSE else zlib.crc32(text.encode())])
            return fn(*args)
        return call

    def take(self):
        calls, self.calls, self.streams = self.calls, [], {}
        return calls


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_config(name, trace, out_dir):
    import torch
    from detr_tf import engine as engine_mod, training
    from detr_tf.networks.detr import get_detr_model
    from detr_tf.optimizers import setup_optimizers
    from detr_tf.training_config import TrainingConfig
    from oracle import set_loss_ref as L
    model_kw, switches, extra = CONFIGS[name]
    saved = {k: getattr(engine_mod, k) for k in switches}
    for k, v in switches.items():
        setattr(engine_mod, k, v)
    try:
        cfg = TrainingConfig()
        cfg.background_class = 91 if "nb_class" not in model_kw else model_kw["nb_class"] - 1
        cfg.train_backbone = cfg.train_transformers = cfg.train_nlayers = True
        cfg.target_batch = None
        cfg.batch_size = 2
        model = get_detr_model(cfg, include_top="nb_class" not in model_kw, num_encoder_layers=2, num_decoder_layers=2, seed=3, **model_kw)
        eng = model.engine
        arrays, meta = {}, dict(config=name, loss=[], finite=True)
        trace.take()
        rng = np.random.default_rng(11)
        if "eval_sites" in extra:
            for H, W in SIZES:
                out = model(rng.normal(size=(2, H, W, 3)).astype(np.float32), need_weights=extra["eval_sites"])
                for k in ("pred_logits", "pred_boxes"):
                    arrays[f"{H}x{W}:{k}"] = out[k].cpu().numpy()
                for site, w in eng.attn_maps.items():
                    arrays[f"{H}x{W}:{site.replace('/', '.')}"] = w.cpu().numpy()
        else:
            opt = setup_optimizers(model, cfg)
            stepper = training.GraphedTrainStep(model, opt, cfg)
            step = 0
            for H, W in SIZES:
                for kind in ("eager",) * 3 + ("graph",) * 3:
                    images = rng.normal(size=(2, H, W, 3)).astype(np.float32)
                    if extra.get("masks"):
                        masks = np.zeros((2, H, W), bool)
                        masks[1, H - 20:, :], masks[1, :, W - 30:] = True, True
                        images = (images, masks)
                    tb, tc = L.make_targets(2, seed=200 + step, force_full=False)
                    if "nb_class" in model_kw:
                        tc = np.where(tc == 91, cfg.background_class, tc % cfg.background_class).astype(tc.dtype)
                    if kind == "eager":
                        out, tot, _ = training.train_step(model, images, tb, tc, opt, cfg, step)
                    else:
                        out, tot, _ = stepper(images, tb, tc, step)
                    arrays[f"{step}:pred_logits"] = out["pred_logits"].cpu().numpy()
                    arrays[f"{step}:pred_boxes"] = out["pred_boxes"].cpu().numpy()
                    meta["loss"].append(float(tot))
                    step += 1
            store = opt["_store"]
            meta["sha"] = {"flat": _sha(eng.P.flat), "adam_m": _sha(store.adam_m), "adam_v": _sha(store.adam_v)}
            meta["sha"].update({f"grad:{k}": _sha(g) for k, g in eng.P.gviews.items()})
        torch.cuda.synchronize()
        meta["finite"] = all(bool(np.isfinite(a).all()) for a in arrays.values()) and all(np.isfinite(meta["loss"]))
        meta["bufs"] = sorted([k, list(t.shape), str(t.dtype)] for k, t in eng._bufs.items())
        meta["trace"] = trace.take()
        np.savez(os.path.join(out_dir, f"{name}.npz"), **arrays)
        with open(os.path.join(out_dir, f"{name}.json"), "w") as f:
            json.dump(meta, f)
        print(f"{name}: {len(meta['trace'])} launches, {len(meta['bufs'])} buffers, finite {meta['finite']}", flush=True)
    finally:
        for k, v in saved.items():
            setattr(engine_mod, k, v)


def record(out_dir, names):
    import torch
    from detr_tf import _hip as hip
    os.makedirs(out_dir, exist_ok=True)
    print(f"tree: {os.path.dirname(hip.__file__)}  library: {hip.LIB_PATH}", flush=True)
    trace = Trace(hip, torch)
    for name in names or list(CONFIGS):
        run_config(name, trace, out_dir)


def compare(dir_a, dir_b):
    bad = 0
    names = sorted(f[:-5] for f in os.listdir(dir_a) if f.endswith(".json"))
    for name in names:
        a, b = (json.load(open(os.path.join(d, f"{name}.json"))) for d in (dir_a, dir_b))
        za, zb = (np.load(os.path.join(d, f"{name}.npz")) for d in (dir_a, dir_b))
        problems = []
        if a["trace"] != b["trace"]:
            first = next((i for i, (x, y) in enumerate(zip(a["trace"], b["trace"])) if x != y), min(len(a["trace"]), len(b["trace"])))
            problems.append(f"trace differs at call {first} of {len(a['trace'])} / {len(b['trace'])}: "
                            f"{a['trace'][first:first + 1]} vs {b['trace'][first:first + 1]}")
        if a["bufs"] != b["bufs"]:
            problems.append(f"buffer plan differs: {[x for x in a['bufs'] if x not in b['bufs']][:4]} vs {[x for x in b['bufs'] if x not in a['bufs']][:4]}")
        if sorted(za.files) != sorted(zb.files):
            problems.append("different arrays")
        else:
            problems += [f"bytes differ: {k}" for k in za.files if za[k].tobytes() != zb[k].tobytes()]
        if a.get("sha") != b.get("sha"):
            diff = [k for k in a.get("sha", {}) if a["sha"][k] != b.get("sha", {}).get(k)]
            bias = [k for k in diff if k.startswith("grad:") and k.endswith("_conv/bias")]      # tf_backbone: summed with fp32 atomics
            problems.append(f"{len(diff)} of {len(a.get('sha', {}))} digests differ: {len(bias)} conv bias gradients of the tf backbone and "
                            f"{[k for k in diff if k not in bias]}")
        if not np.allclose(a["loss"], b["loss"], rtol=1e-6, atol=0.0):
            problems.append(f"loss differs: {a['loss']} vs {b['loss']}")
        if not (a["finite"] and b["finite"]):
            problems.append("non-finite results")
        print(f"{name:18s} {len(a['trace']):6d} launches  {len(a['bufs']):4d} buffers  {'OK' if not problems else 'DIFFERENT'}")
        for p in problems:
            print("    " + p)
        bad += bool(problems)
    print(f"{len(names) - bad} of {len(names)} configurations identical")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "record":
        record(sys.argv[2], sys.argv[3:])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
