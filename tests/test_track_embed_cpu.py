"""Tracking by appearance without a GPU: the NumPy restatement (tests/track_embed_ref.py, the reference the GPU tests compare
detr_hip_track_embed with) pinned on hand-worked scenarios, the C entry point's declaration / export / descriptor layout / argument
checks, and the argument validation of Tracker(embed_dim=...) and Detector.track."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import abi_header
import track_cases as C
import track_embed_cases as EC
import track_embed_ref as ER
import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SCENARIOS = EC.scenarios()


_lib = abi_header.hip_lib


def _ids(results):
    return [r[4].tolist() for r in results]


def _plain(params, frames):
    """The same boxes through the tracker without appearance."""
    plain = {k: v for k, v in params.items() if k in R.DEFAULTS}
    return C.run_ref(plain, [[f[:3] for f in fr] for fr in frames])


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def test_dot64_is_the_lane_order_of_the_header():
    rng = np.random.default_rng(0)
    for E in (4, 68, 256, 512):
        a, b = rng.normal(0, 1, E).astype(F), rng.normal(0, 1, E).astype(F)
        p = [sum((float(a[k]) * float(b[k]) for k in range(lane, E, 64)), 0.0) for lane in range(64)]
        for o in (32, 16, 8, 4, 2, 1):
            p = [p[lane] + p[lane ^ o] for lane in range(64)]
        assert len(set(p)) == 1 and ER.dot64(a, b) == p[0]
        assert abs(ER.dot64(a, b) - float(a.astype(np.float64) @ b.astype(np.float64))) < 1e-12 * E
    unit, bad = ER.unit(np.array([3, 0, 4, 0], F))
    assert unit.tolist() == [F(0.6), 0, F(0.8), 0] and not bad
    assert ER.unit(np.zeros(4, F))[0].tolist() == [0] * 4 and not ER.unit(np.zeros(4, F))[1]
    for poison in (np.nan, np.inf):
        unit, bad = ER.unit(np.array([1, poison, 0, 0], F))
        assert bad and not unit.any()


@pytest.mark.parametrize("name", sorted(C.scenarios()))
def test_ref_without_appearance_is_track_ref(name):
    params, frames = C.scenarios()[name]
    rng = np.random.default_rng(1)
    want_t, want, want_states = C.run_ref(params, frames)
    ref = ER.RefEmbedTracker(embed_dim=12, appearance_weight=0.0, reid_threshold=None, **params)
    for frame, w, ws in zip(frames, want, want_states):
        rows = C.arrays(frame)
        got = ref.step(*rows, None, rng.normal(0, 1, (len(frame), 12)))
        assert all(np.asarray(g).tobytes() == np.asarray(x).tobytes() for g, x in zip(got, w))
        state = ref.state_dict()
        assert all(np.asarray(state[k]).tobytes() == np.asarray(ws[k]).tobytes() for k in R.KEYS)
    assert not ref.gaps and ref.n_reid == 0


def test_ref_swap_keeps_the_ids_by_appearance():
    assert R.iou(EC.A_BOX, EC.B_BOX) == 960 / 2240                              # 0.43 > match_threshold: both pairs pass the gate
    params, frames = SCENARIOS["swap_w0.5"]
    t, results, states = _plain(params, frames)
    assert _ids(results) == [[1, 2], [1, 2]]                                    # plain: the id stays where the BOX is ...
    t, results, states = EC.run_ref(*SCENARIOS["swap_w0"])
    assert _ids(results) == [[1, 2], [1, 2]]
    t, results, states = EC.run_ref(params, frames)
    assert _ids(results) == [[1, 2], [2, 1]]                                    # ... with w = 0.5 it follows the OBJECT: 0.5 * 0.43 + 0.5 > 0.5 * 1 + 0
    assert states[0]["embed"][0].tolist() == EC.axis(8, 0).tolist() and states[0]["embed"][1].tolist() == EC.axis(8, 1).tolist()
    assert len(t.gaps) == 4 and abs(min(t.gaps) - 0.5 * (960 / 2240)) < 1e-12   # the two pairs of a slot, of a detection, did compete
    assert _ids(EC.run_ref(*SCENARIOS["swap_w1"])[1]) == [[1, 2], [2, 1]]


def test_ref_occlusion_brings_the_old_id_back():
    params, frames = SCENARIOS["occlusion_reid"]
    t, results, states = _plain(params, frames)
    assert _ids(results) == [[], []] + [[1]] * 4 + [[]] * 10 + [[], [], [2], [2]]     # plain: a new id, shown at its third hit
    t, results, states = EC.run_ref(*SCENARIOS["occlusion_reid_off"])
    assert _ids(results) == [[], []] + [[1]] * 4 + [[]] * 10 + [[], [], [2], [2]] and t.n_reid == 0
    t, results, states = EC.run_ref(params, frames)
    assert _ids(results) == [[], []] + [[1]] * 4 + [[]] * 10 + [[1]] * 4 and t.n_reid == 1
    assert [r[5].tolist() for r in results[16:]] == [[7], [8], [9], [10]]
    back = states[16]
    assert int(back["miss"][0]) == 0 and not back["v"][0].any()                 # the track restarts AT the detection, without a velocity
    assert back["x"][0].tolist() == R.to_z(np.array(frames[16][0][0], F)).tolist() and int(back["next_id"]) == 2
    assert int(states[15]["miss"][0]) == 10 and abs(float(states[15]["x"][0][0]) - float(back["x"][0][0])) > 150
    # something else appearing there is a new object: sim = 0.4 < 0.8
    t, results, states = EC.run_ref(*SCENARIOS["occlusion_other_object"])
    assert _ids(results) == [[], []] + [[1]] * 4 + [[]] * 10 + [[], [], [2], [2]] and t.n_reid == 0
    assert min(abs(g - 0.4) for g in t.gaps) < 1e-6                             # |sim - 0.8| was looked at (unit vectors are fp32: 2^-24 each)
    assert sorted(int(i) for i in states[-1]["id"] if i) == [1, 2]


def test_ref_a_low_score_match_leaves_the_bank_alone():
    t, results, states = EC.run_ref(*SCENARIOS["low_score"])
    assert _ids(results) == [[], []] + [[1]] * 6
    assert [r[2].tolist() for r in results[3:7]] == [[F(0.9)], [F(0.5)], [F(0.5)], [F(0.9)]]      # frames 4 and 5 are stage 2's
    want = EC.axis(8, 0).tobytes()
    assert all(s["embed"][0].tobytes() == want for s in states)                # never blended with the other look
    assert not any(s["embed"][1:].any() for s in states)


def test_ref_momentum_update_keeps_unit_norm_and_frees_zero():
    walk = EC.random_walk(EC.WALK_SEEDS[68], 68)
    refs = [ER.RefEmbedTracker(embed_dim=68) for _ in range(3)]
    blended = 0
    for frame in walk:
        for s, ref in enumerate(refs):
            before = ref.bank.copy()
            ref.step(*frame[s])
            live = ref.s["id"] >= 1
            norms = np.sqrt((ref.bank.astype(np.float64) ** 2).sum(1))
            assert (np.abs(norms[live] - 1.0) < 1e-6).all() and not ref.bank[~live].any()
            blended += int(((ref.bank != before).any(1) & before.any(1) & live).sum())
    assert blended > 20 and sum(r.n_reid for r in refs) >= 1                    # rows were blended, and the walk does re-identify


def test_ref_bad_rows_take_the_zero_embedding():
    ref = ER.RefEmbedTracker(embed_dim=4, min_hits=1)
    boxes, labels, scores = C.arrays([(C.square(50.0), 1, 0.9), (C.square(200.0), 1, 0.9), (C.square(350.0), 1, 0.9)])
    emb = np.array([[1, 0, 0, 0], [np.nan, 0, 0, 0]], F)
    out = ref.step(boxes, labels, scores, np.array([0, 1, 2], np.int32), emb)
    assert out[6] == ER.BAD_EMBED and out[4].tolist() == [1, 2, 3]
    assert ref.bank[0].tolist() == [1, 0, 0, 0] and not ref.bank[1:].any()


@pytest.mark.parametrize("E", sorted(EC.WALK_SEEDS))
def test_the_committed_seeds_leave_the_margin(E):
    walk = EC.random_walk(EC.WALK_SEEDS[E], E)                                  # asserts MARGIN itself, for every WALK_PARAMS
    assert len(walk) == 12 and max(len(fr[s][0]) for fr in walk for s in range(3)) >= 6
    refs = [ER.RefEmbedTracker(embed_dim=E) for _ in range(3)]
    for fr in walk:
        for s in range(3):
            refs[s].step(*fr[s])
    gaps = [g for r in refs for g in r.gaps]
    assert len(gaps) >= 5 and min(gaps) >= EC.MARGIN and sum(r.n_reid for r in refs) >= 2      # decisions did hang on similarities


# ---- the C entry point ---------------------------------------------------------------------------------------------------------
def test_track_embed_symbols_declared_exported_appended():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    for name in ("detr_hip_track_embed", "detr_hip_track_embed_state_bytes", "detr_hip_workspace_bytes_track_embed"):
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9 and "#define DETR_HIP_ABI_VERSION 9" in hdr
    assert hdr.index("detr_track_embed_desc;") > hdr.index("detr_hip_track_state_bytes(int32_t")       # appended, behind the newest entry
    assert int(re.search(r"#define DETR_TRACK_BAD_EMBED (\d+)", hdr).group(1)) == ER.BAD_EMBED == 4
    assert sorted(_hip.TRACK_EMBED_BAD) == [1, 2, 4] and all(_hip.TRACK_EMBED_BAD[b] == _hip.TRACK_BAD[b] for b in (1, 2))
    mk = open(os.path.join(ROOT, "detr-tensorflow_amd", "Makefile")).read()
    assert "csrc/track_embed.hip" in mk and "build/track_embed.o: EXTRA = -ffp-contract=off" in mk
    assert "build_asan/track_embed.o: EXTRA = -ffp-contract=off" in mk
    # one body: neither file defines a kernel of its own, both launch the template of track_core.h
    csrc = os.path.join(ROOT, "detr-tensorflow_amd", "csrc")
    for name, launch in (("track.hip", "track_kernel<false>"), ("track_embed.hip", "track_kernel<true>")):
        src = open(os.path.join(csrc, name)).read()
        assert "__global__" not in src and launch in src and '#include "track_core.h"' in src
    core = open(os.path.join(csrc, "track_core.h")).read()
    assert core.count("__global__") == 1 and "static_assert(sizeof(TrackLds) + sizeof(TrackEmbedLds) <= 64 * 1024" in core
    assert "atomicAdd" not in core and core.count("atomicOr(a.status") == 2


def check_track_embed_desc_layout():
    _hip, lib = _lib()
    fields_of = abi_header.header_structs()
    fields = fields_of["detr_track_embed_desc"]
    assert fields == list(_hip.TrackEmbedDesc._fields_)                        # names, order and types of the C declaration
    assert fields[:len(_hip.TrackDesc._fields_)] == fields_of["detr_track_desc"] == list(_hip.TrackDesc._fields_)     # every field of detr_track_desc first
    assert [f for f, _ in fields[len(_hip.TrackDesc._fields_):]] == ["embed", "sE_s", "sE_r", "R", "E", "embed_state", "embed_state_bytes", "workspace",
                                                                   "workspace_bytes", "appearance_weight", "reid", "reid_threshold", "momentum"]
    assert _hip.LAYOUT_STRUCTS[500] is _hip.TrackEmbedDesc
    assert abi_header.library_layout(lib, 500) == _hip.struct_layout_mirror(_hip.TrackEmbedDesc) and abi_header.library_layout(lib, 501) is None
    _hip.check_struct_layouts(lib)                     # the load-time check covers it; every id, drift: test_abi_layout_cpu.py


def test_track_embed_desc_layout_and_sizes_match_the_header():
    check_track_embed_desc_layout()
    _hip, lib = _lib()
    T = _hip.TRACK_MAX
    for streams, E in ((1, 4), (3, 256), (65535, 512)):
        assert lib.detr_hip_track_embed_state_bytes(streams, E) == streams * T * E * 4
    for streams, E in ((0, 256), (65536, 256), (1, 0), (1, 6), (1, 516), (1, -4)):
        assert lib.detr_hip_track_embed_state_bytes(streams, E) < 0 and "embed_dim" in lib.detr_hip_last_error().decode()
    d = _hip.TrackEmbedDesc()
    for S, D in ((1, 1), (8, 100), (65535, 1024)):
        d.S, d.D = S, D
        assert lib.detr_hip_workspace_bytes_track_embed(ctypes.byref(d)) == S * T * D * 8
    for S, D in ((0, 100), (1, 0), (1, 1025)):
        d.S, d.D = S, D
        assert lib.detr_hip_workspace_bytes_track_embed(ctypes.byref(d)) < 0
    assert lib.detr_hip_workspace_bytes_track_embed(None) < 0


def check_track_embed_rejects_bad_arguments():
    """Every call fails its checks before anything is launched or dereferenced: it runs with or without a GPU."""
    _hip, lib = _lib()
    fake = 4096
    ptrs = ("state", "boxes", "labels", "scores", "counts", "active", "out_boxes", "out_labels", "out_scores", "out_query", "out_ids",
            "out_hits", "out_counts", "status", "embed", "embed_state", "workspace")
    S, D, E = 2, 100, 256
    need, bank = lib.detr_hip_track_state_bytes(S), lib.detr_hip_track_embed_state_bytes(S, E)

    def desc(**kw):
        d = _hip.TrackEmbedDesc()
        d.S, d.D, d.state_bytes, d.R, d.E, d.sE_s, d.sE_r, d.embed_state_bytes = S, D, need, 100, E, 100 * E, E, bank
        for n in ptrs + ("query",):
            setattr(d, n, fake)
        d.track_threshold, d.new_threshold, d.match_threshold, d.low_match_threshold = 0.7, 0.7, 0.3, 0.5
        d.max_age, d.min_hits, d.alpha, d.beta, d.class_agnostic = 30, 3, 0.75, 0.25, 0
        d.appearance_weight, d.reid, d.reid_threshold, d.momentum = 0.5, 1, 0.8, 0.9
        d.workspace_bytes = lib.detr_hip_workspace_bytes_track_embed(ctypes.byref(d))
        for n, v in kw.items():
            setattr(d, n, v)
        return d

    def rejected(d, text):
        rc = lib.detr_hip_track_embed(ctypes.byref(d) if d is not None else None, None)
        msg = lib.detr_hip_last_error().decode()
        assert rc < 0 and msg.startswith("track_embed: ") and text in msg, (rc, msg, text)

    rejected(None, "null descriptor")
    for n in ptrs:
        rejected(desc(**{n: None}), "null operand")
    for kw in (dict(S=0), dict(S=65536), dict(D=0), dict(D=1025)):              # detr_hip_track's checks, under this entry point's name
        rejected(desc(**kw), "bad shape")
    rejected(desc(state_bytes=need - 1), "state of")
    rejected(desc(match_threshold=float("nan")), "match_threshold is not finite")
    rejected(desc(min_hits=0), "min_hits")
    for E_bad in (6, 0, 2, 516, -4):
        rejected(desc(E=E_bad, sE_r=1024), "bad shape R=")
    rejected(desc(R=0), "bad shape R=")
    for kw in (dict(sE_r=E - 4), dict(sE_s=-1)):
        rejected(desc(**kw), "strides")
    for w in (1.5, -0.1, float("nan")):
        rejected(desc(appearance_weight=w), "appearance_weight")
    for m in (1.5, -0.1, float("nan")):
        rejected(desc(momentum=m), "momentum")
    for v in (-1, 2):
        rejected(desc(reid=v), "reid=")
    for t in (float("nan"), float("inf")):
        rejected(desc(reid_threshold=t), "reid_threshold is not finite")
    for nbytes in (bank - 1, 0, -1):
        rejected(desc(embed_state_bytes=nbytes), "embed_state of")
    rejected(desc(workspace_bytes=S * 256 * D * 8 - 1), "workspace of")
    for name in ("state", "boxes", "out_boxes", "embed", "embed_state", "workspace"):
        rejected(desc(**{name: fake + 4}), "16-byte aligned")


def test_track_embed_rejects_bad_arguments_without_a_gpu():
    check_track_embed_rejects_bad_arguments()


# ---- Tracker and Detector.track arguments ----------------------------------------------------------------------------------------
class _Cfg:
    background_class = 91
    image_size = (64, 96)
    normalized_method = "torch_resnet"


def test_tracker_appearance_arguments():
    from detr_tf.inference import Detector, Tracker
    sig = inspect.signature(Tracker.__init__).parameters
    assert {k: sig[k].default for k in ER.EMBED_DEFAULTS} == ER.EMBED_DEFAULTS and sig["embed_dim"].default is None
    ref = inspect.signature(ER.RefEmbedTracker.__init__).parameters
    assert {k: ref[k].default for k in ER.EMBED_DEFAULTS} == ER.EMBED_DEFAULTS
    assert "UNTUNED" in Tracker.__doc__ and "BoT-SORT" in Tracker.__doc__
    for kw in (dict(embed_dim=6), dict(embed_dim=0), dict(embed_dim=516), dict(embed_dim=8, appearance_weight=1.5),
               dict(embed_dim=8, appearance_weight=float("nan")), dict(embed_dim=8, momentum=-0.1), dict(embed_dim=8, reid_threshold=float("inf"))):
        with pytest.raises(ValueError):
            Tracker(**kw)
    for name in ("update_rows", "update"):
        assert inspect.signature(getattr(Tracker, name)).parameters["embeddings"].default is None
    image = np.zeros((96, 128, 3), np.uint8)
    stub = Tracker.__new__(Tracker)                                            # Detector.track looks at these two before anything runs
    stub.streams, stub.embed_dim = 1, 128
    with pytest.raises(ValueError, match="256"):
        Detector(None, _Cfg()).track(image, stub)
    stub.embed_dim = 256
    for kw in (dict(nms_threshold=0.5), dict(tiles=(1, 2))):
        with pytest.raises(NotImplementedError, match="per-tile"):
            Detector(None, _Cfg(), **kw).track(image, stub)
