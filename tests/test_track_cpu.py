"""Tracking without a GPU: the NumPy restatement of the tracker on hand-worked scenarios (tests/track_ref.py is the reference the GPU
tests compare detr_hip_track with, so it is pinned here first), the C entry point's declaration / export / descriptor layout /
argument checks, and the argument validation of Tracker and Detector.track."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_header
import track_cases as C
import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SCENARIOS = C.scenarios()


_lib = abi_header.hip_lib


def _run(name):
    params, frames = SCENARIOS[name]
    return (frames,) + C.run_ref(params, frames)


def _live(state):
    return sorted(int(i) for i in state["id"] if i >= 1)


def _emitted_ids(results):
    return [r[4].tolist() for r in results]


def _predicted_corners(state, slot):
    q = state["x"][slot] + state["v"][slot]
    half = F(0.5)
    return (q[0] - q[2] * half, q[1] - q[3] * half, q[0] + q[2] * half, q[1] + q[3] * half)


# ---- the reference on hand-worked scenarios ------------------------------------------------------------------------------------
def test_ref_a_moving_box_keeps_one_id():
    frames, tracker, results, states = _run("steady")
    assert _emitted_ids(results) == [[], []] + [[1]] * 28                      # min_hits = 3: nothing before the third hit
    assert [r[5].tolist() for r in results[2:]] == [[h] for h in range(3, 31)]
    assert all(_live(s) == [1] for s in states) and int(states[-1]["next_id"]) == 2 and int(states[-1]["frame"]) == 30
    for f in range(1, 30):                                                     # the overlap the association sees, frame by frame
        assert R.iou(_predicted_corners(states[f - 1], 0), frames[f][0][0]) >= 0.81
    for r, frame in zip(results[2:], frames[2:]):                              # the detector's bits come back unchanged
        assert r[0].tobytes() == np.array([frame[0][0]], F).tobytes() and r[2].tobytes() == np.array([0.9], F).tobytes()


def test_ref_a_gap_is_coasted_through_by_the_velocity():
    frames, tracker, results, states = _run("gap")
    assert _emitted_ids(results) == [[], []] + [[1]] * 18 + [[]] * 5 + [[1]] * 5
    assert R.iou(_predicted_corners(states[24], 0), frames[25][0][0]) > 0.99   # coasted for five frames, still on the object
    assert [int(s["miss"][0]) for s in states[19:26]] == [0, 1, 2, 3, 4, 5, 0]
    # the contrast: without a velocity the track stands still, 24 px (and its lag) behind: IoU <= 0.25 < 0.3, a new id
    frames, tracker, results, states = _run("gap_no_velocity")
    assert (states[24]["v"] == 0).all()
    assert R.iou(_predicted_corners(states[24], 0), frames[25][0][0]) < 0.25
    assert R.iou((0, 0, 40, 40), (24, 0, 64, 40)) == 0.25
    assert _emitted_ids(results) == [[], []] + [[1]] * 18 + [[]] * 5 + [[], [], [2], [2], [2]]
    assert _live(states[25]) == [1, 2] and _live(states[-1]) == [1, 2]         # the old one coasts on: max_age = 30


def test_ref_max_age_ends_a_track():
    frames, tracker, results, states = _run("gap_max_age_4")
    assert [_live(s) for s in states[19:26]] == [[1], [1], [1], [1], [1], [], [2]]      # miss 5 > 4: freed in the fifth missing frame
    assert _emitted_ids(results)[25:] == [[], [], [2], [2], [2]]
    freed = states[24]
    assert all(not np.asarray(freed[k]).any() for k in ("x", "v", "label", "id", "hits", "miss", "confirmed", "score"))   # a free slot is zeros


def test_ref_a_score_dip_keeps_the_id_and_a_low_score_starts_nothing():
    frames, tracker, results, states = _run("score_dip")
    assert _emitted_ids(results) == [[], []] + [[1]] * 14                      # stage 2 carries frames 8..11
    assert [r[2].tolist() for r in results[7:13]] == [[F(0.9)], [F(0.5)], [F(0.5)], [F(0.5)], [F(0.5)], [F(0.9)]]
    assert all(_live(s) == [1] for s in states) and int(states[-1]["next_id"]) == 2     # the far object never scored above new_threshold
    # a track that is not confirmed yet gets no second chance: the same dip in frames 1..2 loses the object
    t, results, states = C.run_ref({}, C.moving(6, score=lambda f: 0.5 if f in (1, 2) else 0.9))
    assert [_live(s) for s in states] == [[1], [], [], [2], [2], [2]]


def test_ref_unconfirmed_tracks_die_at_once_and_min_hits_gates_the_output():
    frames, tracker, results, states = _run("unconfirmed_miss")
    assert [_live(s) for s in states] == [[1], [], [2], [2], [2], [2], [2], [2]]
    assert _emitted_ids(results) == [[], [], [], [], [2], [2], [2], [2]]
    assert results[4][5].tolist() == [3]                                       # first emitted at its third hit
    t, results, states = C.run_ref(dict(min_hits=1), SCENARIOS["unconfirmed_miss"][1])
    assert _emitted_ids(results) == [[1], []] + [[1]] * 6                      # min_hits = 1: confirmed at birth ...
    assert all(_live(s) == [1] for s in states)                                # ... and so kept through the miss (the box is 8 px on: IoU 2/3)


def test_ref_labels_separate_tracks_unless_class_agnostic():
    frames, tracker, results, states = _run("two_labels")
    for f, r in enumerate(results[2:], 2):
        assert dict(zip(r[1].tolist(), r[4].tolist())) == {1: 1, 2: 2}, f      # whatever the order of the detections
    frames, tracker, results, states = _run("two_labels_agnostic")
    for f, r in enumerate(results[2:], 2):
        assert r[4].tolist() == [1, 2]                                         # exact ties: the lower id takes the lower index ...
        assert r[1].tolist() == ([1, 2] if f % 2 == 0 else [2, 1])             # ... and the detection's label is copied
    assert states[-1]["label"][:2].tolist() == [1, 2]                          # the track's label never changes


def test_ref_ties_go_to_the_lower_id_then_the_lower_index():
    params, frames = SCENARIOS["tie_lower_id"]
    assert R.iou((0, 0, 40, 40), (8, 0, 48, 40)) == R.iou((16, 0, 56, 40), (8, 0, 48, 40))
    t, results, states = C.run_ref(params, frames)
    assert results[1][4].tolist() == [1] and states[1]["hits"][:2].tolist() == [2, 1]
    t = R.RefTracker(**params)                                                 # ids swapped between the slots: the id decides, not the slot
    t.step(*C.arrays(frames[0]))
    state = t.state_dict()
    state["id"][:2] = [2, 1]
    t.load_state_dict(state)
    assert t.step(*C.arrays(frames[1]))[4].tolist() == [1] and t.state_dict()["hits"][:2].tolist() == [1, 2]
    t, results, states = C.run_ref(*SCENARIOS["tie_lower_index"])
    assert results[1][4].tolist() == [1, 2] and results[1][5].tolist() == [2, 1]        # detection 0 matched, detection 1 started track 2


def test_ref_257_detections_fill_the_slots_and_raise_the_flag():
    t, results, states = C.run_ref(*SCENARIOS["overflow"])
    for r, s in zip(results, states):
        assert r[6] == R.FULL and len(r[4]) == 256 and r[4].tolist() == list(range(1, 257))
        assert _live(s) == list(range(1, 257)) and int(s["next_id"]) == 257    # the detection without a slot consumed no id
    assert results[1][5].tolist() == [2] * 256


def test_ref_resumes_from_a_state_dict():
    walk = C.random_walk(11, streams=1, frames=12)
    frames = [f[0] for f in walk]
    straight = R.RefTracker()
    want = [straight.step(*f) for f in frames]
    first = R.RefTracker()
    got = [first.step(*f) for f in frames[:5]]
    second = R.RefTracker()
    second.load_state_dict(first.state_dict())
    got += [second.step(*f) for f in frames[5:]]
    for a, b in zip(want, got):
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))
    a, b = straight.state_dict(), second.state_dict()
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in R.KEYS)
    assert max(len(r[4]) for r in want) >= 2 and int(a["next_id"]) > 4         # the walk does track something


# ---- the C entry point ---------------------------------------------------------------------------------------------------------
def test_track_symbols_declared_exported_appended():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    for name in ("detr_hip_track", "detr_hip_track_state_bytes"):
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9 and "#define DETR_HIP_ABI_VERSION 9" in hdr
    assert hdr.index("detr_track_desc;") > hdr.index("detr_hip_workspace_bytes_overlay(")     # appended, behind the newest entry
    assert f"#define DETR_TRACK_MAX {_hip.TRACK_MAX}" in hdr and _hip.TRACK_MAX == R.TRACK_MAX == 256
    assert sorted(_hip.TRACK_BAD) == [int(re.search(rf"#define {n} (\d+)", hdr).group(1)) for n in ("DETR_TRACK_FULL", "DETR_TRACK_BAD_COUNT")]
    assert (R.FULL, R.BAD_COUNT) == (1, 2)
    mk = open(os.path.join(ROOT, "detr-tensorflow_amd", "Makefile")).read()
    assert "csrc/track.hip" in mk and "build/track.o: EXTRA = -ffp-contract=off" in mk and "build_asan/track.o: EXTRA = -ffp-contract=off" in mk
    src = open(os.path.join(ROOT, "detr-tensorflow_amd", "csrc", "tile_merge.hip")).read()
    assert "match_measure(" in src and "tm_measure" not in src                 # one definition of the measure, in detections.h


def test_track_desc_layout_and_state_size_match_the_header():
    _hip, lib = _lib()
    from detr_tf import inference
    assert abi_header.header_structs()["detr_track_desc"] == list(_hip.TrackDesc._fields_)       # names, order and types of the C declaration
    assert _hip.LAYOUT_STRUCTS[400] is _hip.TrackDesc
    _hip.check_struct_layouts(lib)                     # the load-time check covers it; library, unknown ids, drift: test_abi_layout_cpu.py
    # the state: the header's layout, field by field, is the binding's record, and the library sizes it
    T = _hip.TRACK_MAX
    per_stream = 2 * T * 4 * 4 + T * 8 + T * 4 + 4 * T * 4 + 4 * 4
    assert inference.TRACK_STATE.itemsize == per_stream and per_stream % 16 == 0
    assert [inference.TRACK_STATE.fields[k][1] for k in ("x", "v", "label", "score", "id", "hits", "miss", "confirmed", "frame", "next_id")] == \
        [0, 16 * T, 32 * T, 40 * T, 44 * T, 48 * T, 52 * T, 56 * T, 60 * T, 60 * T + 4]
    for streams in (1, 3, 65535):
        assert lib.detr_hip_track_state_bytes(streams) == streams * per_stream
    for streams in (0, -1, 65536):
        assert lib.detr_hip_track_state_bytes(streams) < 0 and "streams" in lib.detr_hip_last_error().decode()


def test_track_rejects_bad_arguments_without_a_gpu():
    _hip, lib = _lib()
    fake = 4096                                   # never dereferenced: every call below fails its checks first
    ptrs = ("state", "boxes", "labels", "scores", "counts", "active", "out_boxes", "out_labels", "out_scores", "out_query", "out_ids",
            "out_hits", "out_counts", "status")
    need = lib.detr_hip_track_state_bytes(2)

    def desc(**kw):
        d = _hip.TrackDesc()
        d.S, d.D, d.state_bytes = 2, 100, need
        for n in ptrs + ("query",):
            setattr(d, n, fake)
        d.track_threshold, d.new_threshold, d.match_threshold, d.low_match_threshold = 0.7, 0.7, 0.3, 0.5
        d.max_age, d.min_hits, d.alpha, d.beta, d.class_agnostic = 30, 3, 0.75, 0.25, 0
        for n, v in kw.items():
            setattr(d, n, v)
        return d

    def rejected(d, text):
        rc = lib.detr_hip_track(ctypes.byref(d) if d is not None else None, None)
        msg = lib.detr_hip_last_error().decode()
        assert rc < 0 and text in msg, (rc, msg, text)

    rejected(None, "null descriptor")
    for n in ptrs:
        rejected(desc(**{n: None}), "null operand")
    for kw in (dict(S=0), dict(S=-1), dict(S=65536), dict(D=0), dict(D=-3), dict(D=1025)):
        rejected(desc(**kw), "bad shape")
    for nbytes in (need - 1, 0, -1):
        rejected(desc(state_bytes=nbytes), "state of")
    for name in ("track_threshold", "new_threshold", "match_threshold", "low_match_threshold"):
        for t in (float("nan"), float("inf"), float("-inf")):
            rejected(desc(**{name: t}), f"{name} is not finite")
    for name in ("alpha", "beta"):
        for t in (float("nan"), float("inf")):
            rejected(desc(**{name: t}), "alpha and beta must be finite")
    rejected(desc(max_age=-1), "max_age")
    for v in (0, -2):
        rejected(desc(min_hits=v), "min_hits")
    for v in (-1, 2):
        rejected(desc(class_agnostic=v), "class_agnostic")
    for name in ("state", "boxes", "out_boxes"):
        rejected(desc(**{name: fake + 4}), "16-byte aligned")


# ---- Tracker and Detector.track arguments ----------------------------------------------------------------------------------------
class _Cfg:
    background_class = 91
    image_size = (64, 96)
    normalized_method = "torch_resnet"


def test_tracker_and_detector_track_arguments():
    import inspect
    from detr_tf.inference import Detections, Detector, TrackedDetections, Tracker
    assert TrackedDetections._fields == Detections._fields + ("ids", "hits")
    sig = inspect.signature(Tracker.__init__).parameters
    assert {k: sig[k].default for k in R.DEFAULTS} == R.DEFAULTS                # the documented defaults, and the reference's
    assert sig["streams"].default == 1 and sig["device"].default is None
    for kw in (dict(streams=0), dict(streams=65536), dict(track_threshold=float("nan")), dict(new_threshold=float("inf")),
               dict(match_threshold=float("nan")), dict(low_match_threshold=float("-inf")), dict(alpha=float("nan")), dict(beta=float("inf")),
               dict(max_age=-1), dict(min_hits=0)):
        with pytest.raises(ValueError):
            Tracker(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Tracker(device="cpu")
    image = np.zeros((96, 128, 3), np.uint8)
    with pytest.raises(ValueError, match="xyxy"):                               # checked before anything runs
        Detector(None, _Cfg(), bbox_format="xywh").track(image, None)
    with pytest.raises(TypeError, match="Tracker"):
        Detector(None, _Cfg()).track(image, object())
