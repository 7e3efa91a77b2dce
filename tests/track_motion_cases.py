"""Synthetic videos shared by tests/test_track_motion_cpu.py (which pins tests/track_motion_ref.py on them) and
tests/test_gpu_track_motion.py (which replays them on the device).  A scenario is a dict: radius, params (the tracker's), frames
(uint8 [h, w, 3] arrays) and dets (per frame a list of (box xyxy, label, score), as tests/track_cases.py writes them).
Textures are random 4 x 4-pixel blocks (track_motion_ref.scene); a frame is a crop of one large scene, displaced by a multiple of
the thumbnail factor f, so that the thumbnails of two frames are exact shifts of each other.  The seeds are recorded here: the
statements test_track_motion_cpu.py makes hold for these seeds, nothing is drawn at test time."""
import numpy as np

import track_motion_ref as M
from track_cases import square

# name: (h, w, radius, true shift of the content in THUMBNAIL pixels (dx, dy), seed)
SHIFTS = {"a_36x36_r2": (36, 36, 2, (1, -2), 1), "b_80x100_r8": (80, 100, 8, (5, -7), 2), "c_401x778_r8": (401, 778, 8, (6, 4), 3),
          "d_80x80_r16": (80, 80, 16, (16, -16), 4)}
# frames on which the window of the search does not fit, or fits fewer than MIN_BLOCKS blocks: (h, w, radius)
TOO_SMALL = {"small_64x48_r16": (64, 48, 16), "small_48x64_r16": (48, 64, 16), "small_2000x40": (2000, 40, 8), "small_40x2000": (40, 2000, 8),
             "small_4000x3": (4000, 3, 8), "small_3x4000": (3, 4000, 8)}


def follow(shifts_px, extra=()):
    """The detections of a video whose content is displaced by shifts_px[f] = (x, y) pixels relative to frame 0: two objects that
    stand still in the scene."""
    return [[(square(60.0 + x, 50.0 + y), 1, 0.9), (square(150.0 + x, 90.0 + y, 30.0), 2, 0.8)] + list(extra) for x, y in shifts_px]


def view(big, margin, h, w, shift_px):
    """The frame in which the content of `big` appears displaced by shift_px = (x, y) pixels."""
    return M.crop(big, margin - shift_px[1], margin - shift_px[0], h, w)


def video(seed, h, w, shifts_px):
    margin = max(max(abs(x), abs(y)) for x, y in shifts_px)
    big = M.scene(seed, h + 2 * margin, w + 2 * margin)
    return [view(big, margin, h, w, s) for s in shifts_px]


def stripes(h, w, phase, period=4):
    """Vertical stripes: `period` columns wide in all, half dark, half bright."""
    x = (np.arange(w) + phase) % period
    row = np.where(x < period // 2, 40, 200).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(row[None, :, None], (h, w, 3)))


def scenarios():
    out = {}
    for name, (h, w, R, (dx, dy), seed) in SHIFTS.items():
        f = M.geometry(h, w, R)[0]
        shifts = [(0, 0), (dx * f, dy * f), (0, 0)]                              # there and back again
        out[name] = dict(radius=R, params=dict(min_hits=1), frames=video(seed, h, w, shifts), dets=follow(shifts))
    # a scene cut: the second frame shows another scene, the third that scene moved
    a, b = video(5, 80, 100, [(0, 0)]), video(6, 80, 100, [(0, 0), (3, 4)])
    out["cut"] = dict(radius=8, params=dict(min_hits=1), frames=a + b, dets=follow([(0, 0), (0, 0), (3, 4)]))
    flat = np.full((80, 100, 3), 117, np.uint8)
    out["flat"] = dict(radius=8, params=dict(min_hits=1), frames=video(7, 80, 100, [(0, 0)]) + [flat, flat.copy()], dets=follow([(0, 0)] * 3))
    # the frame size changes: no estimate on that frame, the new thumbnail is stored and serves the next one
    out["resize"] = dict(radius=8, params=dict(min_hits=1), frames=video(8, 80, 100, [(0, 0)]) + video(8, 96, 100, [(0, 0), (-4, 6)]),
                         dets=follow([(0, 0), (0, 0), (-4, 6)]))
    for name, (h, w, R) in TOO_SMALL.items():
        out[name] = dict(radius=R, params=dict(min_hits=1), frames=video(9, h, w, [(0, 0), (1, 0)]), dets=follow([(0, 0), (1, 0)]))
    # SAD ties: stripes of period 4 moved by 2 look the same at dx = ..., -6, -2, 2, 6 and every dy
    out["stripes"] = dict(radius=8, params=dict(min_hits=1), frames=[stripes(80, 100, 0), stripes(80, 100, -2)], dets=follow([(0, 0), (2, 0)]))
    # moving foreground on fewer than half of the blocks: the background's shift wins
    bg = video(10, 120, 160, [(0, 0), (3, -2)])
    fg = M.scene(11, 48, 64)
    for frame, (y, x) in zip(bg, [(40, 50), (46, 45)]):                         # the rectangle moves by (-5, 6)
        frame[y:y + 48, x:x + 64] = fg
    out["foreground"] = dict(radius=8, params=dict(min_hits=1), frames=bg, dets=follow([(0, 0), (3, -2)]))
    out["jitter"] = jitter()
    return out


JITTER = (32, -32)                                                              # pixels, there on odd frames, back on even ones


def jitter(frames=8):
    """The failure camera-motion compensation fixes: ONE 40 x 40 object that stands still in the scene while the camera jitters by
    +-32 pixels per frame.  The box moves by more than the IoU gate forgives (an IoU of 0.02 with where it was), every frame.  400 x 400
    frames: f = 2, so that 32 pixels are 16 thumbnail pixels, the largest radius (at f = 1 the rule's radius ends at 16 pixels)."""
    shifts = [JITTER if f % 2 else (0, 0) for f in range(frames)]
    return dict(radius=16, params={}, frames=video(12, 400, 400, shifts), dets=[[(square(180.0 + x, 170.0 + y), 1, 0.9)] for x, y in shifts])
