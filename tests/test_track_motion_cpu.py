"""Camera-motion compensation without a GPU: the NumPy restatement (tests/track_motion_ref.py is the reference the GPU tests compare
detr_hip_track_motion with, so it is pinned here first) on the synthetic videos of tests/track_motion_cases.py, the three C symbols'
declaration / export / descriptor layout / argument checks, and the argument validation of Tracker(motion=) and frames=."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import abi_header
import track_cases as C
import track_motion_cases as MC
import track_motion_ref as M
import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@functools.lru_cache(maxsize=None)
def scenarios():
    return MC.scenarios()


@functools.lru_cache(maxsize=None)
def run_ref(name, motion=True):
    """The reference on one scenario, computed once and shared (tests/test_gpu_track_motion.py reads it too; nobody changes it):
    per frame (out_motion, votes, emitted tuple, motion state_dict, track state_dict)."""
    sc = scenarios()[name]
    mo, tr = M.RefMotion(sc["radius"]), R.RefTracker(**sc["params"])
    steps = []
    for frame, dets in zip(sc["frames"], sc["dets"]):
        out = mo.step(frame, tr.s) if motion else None
        votes = mo.votes
        steps.append((out, votes, tr.step(*C.arrays(dets)), mo.state_dict(), tr.state_dict()))
    return steps


_lib = abi_header.hip_lib


# ---- the reference on synthetic videos -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MC.SHIFTS))
def test_ref_recovers_a_known_shift_exactly(name):
    h, w, radius, (dx, dy), _ = MC.SHIFTS[name]
    f, tw, th, gx, gy = M.geometry(h, w, radius)
    assert (f, gx, gy) == {"a_36x36_r2": (1, 2, 2), "b_80x100_r8": (1, 5, 4), "c_401x778_r8": (3, 15, 7), "d_80x80_r16": (1, 3, 3)}[name]
    assert (tw, th) == (w // f, h // f) and (tw * f < w or th * f < h) == (name == "c_401x778_r8")      # c drops partial edges
    steps = run_ref(name)
    assert steps[0][0].tolist() == [0, 0, 0, 0, 0, f]                          # the first frame has no predecessor
    assert steps[1][0].tolist() == [1, dx * f, dy * f, gx * gy, gx * gy, f]    # every block is textured and votes for the true shift
    assert steps[2][0].tolist() == [1, -dx * f, -dy * f, gx * gy, gx * gy, f]  # and back
    valid, vx, vy, sad = steps[1][1]
    assert valid.all() and (vx == dx).all() and (vy == dy).all() and (sad == 0).all()
    head = dict(zip(M.HEAD, steps[1][3]["motion_head"].tolist()))
    assert head == dict(h=h, w=w, f=f, tw=tw, th=th, valid=1, slot=0, estimated=1, sx=dx * f, sy=dy * f, n=gx * gy, agree=gx * gy)
    assert not steps[1][3]["motion_head"][12:].any()
    # the tracks moved with the camera: both objects keep their ids and are matched with IoU 1 every frame
    assert [s[2][4].tolist() for s in steps] == [[1, 2]] * 3 and [s[2][5].tolist() for s in steps] == [[1, 1], [2, 2], [3, 3]]
    assert all(not s[4]["v"].any() for s in steps)                             # no residual ever reached the velocity


def test_ref_thumbnail_is_the_box_filter_of_the_luma():
    frame = scenarios()["c_401x778_r8"]["frames"][0]
    f, tw, th, _, _ = M.geometry(401, 778, 8)
    thumb = run_ref("c_401x778_r8")[0][3]["motion_thumb"]
    assert (f, tw, th) == (3, 259, 133) and not thumb[0].any() and not thumb[1, th * tw:].any()        # slot 1 first; the tail untouched
    for (i, j) in ((0, 0), (132, 258), (57, 101)):
        cell = frame[3 * i:3 * i + 3, 3 * j:3 * j + 3].astype(int)
        want = sum(int((77 * r + 150 * g + 29 * b + 128) >> 8) for r, g, b in cell.reshape(-1, 3)) // 9
        assert thumb[1, i * tw + j] == want
    assert M.luma(np.array([[[255, 255, 255]]], np.uint8)).tolist() == [[255]] and M.luma(np.array([[[0, 0, 0]]], np.uint8)).tolist() == [[0]]


def test_ref_a_scene_cut_fails_the_agreement_test():
    steps = run_ref("cut")
    est, sx, sy, n, agree, f = steps[1][0].tolist()
    assert (est, sx, sy, n) == (0, 0, 0, 20) and 2 * agree < n                 # textured blocks, votes all over the place
    assert steps[2][0].tolist() == [1, 3, 4, 20, 20, 1]                        # the new scene's thumbnail was stored: the next frame has an estimate
    assert steps[1][4]["x"][:2, :2].tolist() == steps[0][4]["x"][:2, :2].tolist()       # nothing moved on the cut


def test_ref_a_flat_frame_has_no_valid_block():
    steps = run_ref("flat")
    assert [s[0].tolist() for s in steps] == [[0, 0, 0, 0, 0, 1]] * 3
    assert steps[1][1] is not None and not steps[1][1][0].any()                # the blocks were looked at: max - min < MIN_CONTRAST
    assert (steps[2][3]["motion_thumb"][:, :80 * 100] == 117).all()


def test_ref_a_size_change_gives_no_estimate_and_stores_the_thumbnail():
    steps = run_ref("resize")
    assert steps[1][0].tolist() == [0, 0, 0, 0, 0, 1] and steps[1][1] is None   # not even looked at
    head = dict(zip(M.HEAD, steps[1][3]["motion_head"].tolist()))
    assert (head["h"], head["w"], head["valid"], head["slot"]) == (96, 100, 1, 0)
    assert steps[1][3]["motion_thumb"][0, :96 * 100].tobytes() == M.thumbnail(scenarios()["resize"]["frames"][1], 1, 100, 96).tobytes()
    assert steps[2][0].tolist() == [1, -4, 6, 25, 25, 1]


@pytest.mark.parametrize("name", sorted(MC.TOO_SMALL))
def test_ref_frames_too_small_for_the_search_give_no_estimate(name):
    h, w, radius = MC.TOO_SMALL[name]
    f, tw, th, gx, gy = M.geometry(h, w, radius)
    steps = run_ref(name)
    if "r16" in name:                            # the window fits, but on two blocks only: fewer than MIN_BLOCKS
        assert gx * gy == 2 and steps[1][0].tolist() == [0, 0, 0, 2, 0, 1]
    else:                                        # the window does not fit: gx < 1 or gy < 1 (tw == 0 / th == 0 among them)
        assert min(gx, gy) == 0 and steps[1][1] is None and steps[1][0].tolist() == [0, 0, 0, 0, 0, f]
        assert (tw == 0 or th == 0) == ("x3" in name or "3x" in name)
    head = dict(zip(M.HEAD, steps[1][3]["motion_head"].tolist()))
    assert (head["h"], head["w"], head["f"], head["tw"], head["th"], head["valid"], head["slot"]) == (h, w, f, tw, th, 1, 0)
    assert steps[1][4]["x"][:2].tolist() != steps[0][4]["x"][:2].tolist()       # (the tracker itself still followed the boxes)


def test_ref_sad_ties_are_broken_by_the_key():
    steps = run_ref("stripes")
    valid, vx, vy, sad = steps[1][1]
    # the stripes moved by +2; period 4 makes dx = -6, -2, 2, 6 and every dy exact matches: the smallest dx^2 + dy^2 is 4 at dy = 0,
    # and of dx = -2 and dx = 2 the key takes the lower dx
    assert valid.all() and (sad == 0).all() and (vx == -2).all() and (vy == 0).all()
    assert steps[1][0].tolist() == [1, -2, 0, 20, 20, 1]
    cur, prev = (M.thumbnail(fr, 1, 100, 80) for fr in scenarios()["stripes"]["frames"][::-1])
    assert (cur[:, 8:24] == prev[:, 6:22]).all() and (cur[:, 8:24] == prev[:, 10:26]).all()        # both candidates are exact


def test_ref_background_wins_over_a_smaller_moving_foreground():
    steps = run_ref("foreground")
    est, sx, sy, n, agree, f = steps[1][0].tolist()
    assert (est, sx, sy, n, f) == (1, 3, -2, 54, 1) and 27 <= agree < 54
    valid, vx, vy, _ = steps[1][1]
    votes = set(zip(vx[valid].tolist(), vy[valid].tolist()))
    assert (-5, 6) in votes and (3, -2) in votes                               # the rectangle's own motion was seen, and outvoted


def test_ref_jitter_loses_every_track_without_motion_and_none_with_it():
    sc = scenarios()["jitter"]
    assert M.geometry(400, 400, 16)[0] == 2 and MC.JITTER == (32, -32)
    assert R.iou(MC.square(180.0, 170.0), MC.square(212.0, 138.0)) == 64 / 3136    # 8 x 8 pixels still overlap: far below the gate (0.3)
    plain = run_ref("jitter", motion=False)
    assert [s[2][4].tolist() for s in plain] == [[]] * 8                       # the failure being fixed: no id is ever emitted
    assert [int(s[4]["next_id"]) for s in plain] == list(range(2, 10))         # a new track every frame, dropped in the next
    steps = run_ref("jitter")
    assert [s[0].tolist() for s in steps[1:]] == [[1, 32 * (-1) ** f, 32 * (-1) ** (f + 1), 100, 100, 2] for f in range(7)]
    assert [s[2][4].tolist() for s in steps] == [[], []] + [[1]] * 6           # min_hits = 3: from the third frame on
    assert [s[2][5].tolist() for s in steps[2:]] == [[h] for h in range(3, 9)]  # unbroken hits
    assert len(sc["frames"]) == 8 and int(steps[-1][4]["next_id"]) == 2


def test_ref_resumes_from_its_state_dict():
    sc = scenarios()["b_80x100_r8"]
    straight = run_ref("b_80x100_r8")
    mo = M.RefMotion(8)
    mo.load_state_dict(straight[0][3])
    assert mo.step(sc["frames"][1]).tobytes() == straight[1][0].tobytes()
    assert all(mo.state_dict()[k].tobytes() == straight[1][3][k].tobytes() for k in ("motion_head", "motion_thumb"))


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("detr_hip_track_motion", "detr_hip_track_motion_state_bytes", "detr_hip_workspace_bytes_track_motion")


def test_track_motion_symbols_declared_exported_appended():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9 and "#define DETR_HIP_ABI_VERSION 9" in hdr
    assert hdr.index("detr_track_motion_desc;") > hdr.index("detr_hip_workspace_bytes_track_embed(")    # appended, behind the newest entry
    for name, value in (("SIDE", 384), ("BLOCK", 16), ("MIN_BLOCKS", 4), ("MIN_CONTRAST", 16), ("MAX_RADIUS", 16)):
        assert f"#define DETR_MOTION_{name} {value}" in hdr and getattr(_hip, "MOTION_" + name) == value and getattr(M, name) == value
    assert "#define DETR_TRACK_BAD_FRAME 8" in hdr and list(_hip.TRACK_MOTION_BAD) == [8] == [M.BAD_FRAME]
    assert not set(_hip.TRACK_MOTION_BAD) & set(_hip.TRACK_EMBED_BAD)           # the status word is shared with the tracker's launch
    assert M.MAX_SIDE == _hip.OVERLAY_MAX_SIDE
    mk = open(os.path.join(ROOT, "detr-tensorflow_amd", "Makefile")).read()
    assert "csrc/track_motion.hip" in mk and "build/track_motion.o: EXTRA = -ffp-contract=off" in mk
    assert "build_asan/track_motion.o: EXTRA = -ffp-contract=off" in mk


def test_track_motion_desc_layout_and_state_size_match_the_header():
    _hip, lib = _lib()
    from detr_tf import inference
    assert abi_header.header_structs()["detr_track_motion_desc"] == list(_hip.TrackMotionDesc._fields_)   # names, order and types of the C declaration
    assert _hip.LAYOUT_STRUCTS[600] is _hip.TrackMotionDesc

    class Drifted(ctypes.Structure):                   # a field INSERTED behind S (test_abi_layout_cpu.py widens one): every later offset moves
        _fields_ = list(_hip.TrackMotionDesc._fields_[:1]) + [("D", ctypes.c_int64)] + list(_hip.TrackMotionDesc._fields_[1:])
    try:
        _hip.LAYOUT_STRUCTS[600] = Drifted
        with pytest.raises(RuntimeError, match="Drifted"):
            _hip.check_struct_layouts(lib)
    finally:
        _hip.LAYOUT_STRUCTS[600] = _hip.TrackMotionDesc
    _hip.check_struct_layouts(lib)                                             # the load-time check covers it
    per_stream = 16 * 4 + 2 * 384 * 384
    assert inference.MOTION_STATE.itemsize == per_stream and per_stream % 16 == 0
    assert [inference.MOTION_STATE.fields[k][1] for k in ("head", "thumb")] == [0, 64] and inference.MOTION_HEAD == M.HEAD
    for streams in (1, 3, 65535):
        assert lib.detr_hip_track_motion_state_bytes(streams) == streams * per_stream
        d = _hip.TrackMotionDesc()
        d.S = streams
        assert lib.detr_hip_workspace_bytes_track_motion(ctypes.byref(d)) == streams * 23 * 23 * 8
    for streams in (0, -1, 65536):
        assert lib.detr_hip_track_motion_state_bytes(streams) < 0 and "streams" in lib.detr_hip_last_error().decode()
        d = _hip.TrackMotionDesc()
        d.S = streams
        assert lib.detr_hip_workspace_bytes_track_motion(ctypes.byref(d)) < 0
    assert lib.detr_hip_workspace_bytes_track_motion(None) < 0


def test_track_motion_rejects_bad_arguments_without_a_gpu():
    _hip, lib = _lib()
    fake = 4096                                   # never dereferenced: every call below fails its checks first
    ptrs = ("frames", "offsets", "sizes", "active", "motion_state", "state", "workspace", "out_motion", "status")
    S = 2
    need_m, need_t = lib.detr_hip_track_motion_state_bytes(S), lib.detr_hip_track_state_bytes(S)

    def desc(**kw):
        d = _hip.TrackMotionDesc()
        d.S, d.radius, d.frames_bytes = S, 8, 1 << 20
        for n in ptrs:
            setattr(d, n, fake)
        d.motion_state_bytes, d.state_bytes = need_m, need_t
        d.workspace_bytes = lib.detr_hip_workspace_bytes_track_motion(ctypes.byref(d))
        for n, v in kw.items():
            setattr(d, n, v)
        return d

    def rejected(d, text):
        rc = lib.detr_hip_track_motion(ctypes.byref(d) if d is not None else None, None)
        msg = lib.detr_hip_last_error().decode()
        assert rc < 0 and text in msg, (rc, msg, text)

    need_w = desc().workspace_bytes
    rejected(None, "null descriptor")
    for n in ptrs:
        rejected(desc(**{n: None}), "null operand")
    for v in (0, -1, 65536):
        rejected(desc(S=v), "bad shape")
    for v in (0, -1, 17, 1 << 20):
        rejected(desc(radius=v), "radius")
    for v in (0, -5):
        rejected(desc(frames_bytes=v), "frames_bytes")
    for nbytes in (need_m - 1, 0, -1):
        rejected(desc(motion_state_bytes=nbytes), "motion_state of")
    for nbytes in (need_t - 1, 0, -1):
        rejected(desc(state_bytes=nbytes), "state of")
    for nbytes in (need_w - 1, 0, -1):
        rejected(desc(workspace_bytes=nbytes), "workspace of")
    for name in ("motion_state", "state", "workspace"):
        rejected(desc(**{name: fake + 8}), "16-byte aligned")
    rejected(desc(offsets=fake + 4), "8-byte aligned")
    for name in ("sizes", "active", "out_motion", "status"):
        rejected(desc(**{name: fake + 2}), "4-byte aligned")


# ---- Tracker(motion=) and frames= ---------------------------------------------------------------------------------------------------
def test_tracker_motion_arguments():
    import inspect
    from detr_tf.inference import Detector, Tracker
    sig = inspect.signature(Tracker.__init__).parameters
    assert sig["motion"].default is False and sig["motion_radius"].default == 8
    for name in ("update_rows", "update"):
        assert inspect.signature(getattr(Tracker, name)).parameters["frames"].default is None
    for radius in (0, -1, 17):
        with pytest.raises(ValueError, match="motion_radius"):
            Tracker(motion=True, motion_radius=radius)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Tracker(device="cpu", motion=True)
    doc = Tracker.__doc__
    assert "no camera-motion compensation" not in doc and "motion=True" in doc and "UNMEASURED" in doc
    assert "zoom and roll are not modelled" in doc and "quantised" in doc
    assert "last_upload" in Detector.track.__doc__
