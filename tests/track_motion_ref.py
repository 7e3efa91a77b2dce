"""Camera-motion compensation (csrc/track_motion.hip) restated in plain NumPy from its specification (include/detr_hip.h:
detr_track_motion_desc, steps 1..6).  A test helper, not product code.

Everything up to the shift is integer arithmetic, so there is nothing to round: thumbnails, votes, medians and the header are
compared with the device byte for byte.  The shift is added to the track state as np.float32 scalars, one rounding each.
RefMotion is one stream; step(frame, state) shifts the state dict of a track_ref.RefTracker / track_embed_ref tracker in place
BEFORE that tracker's own step, which is how the two compose."""
import numpy as np

F = np.float32
SIDE, BLOCK, MIN_BLOCKS, MIN_CONTRAST, MAX_RADIUS, MAX_SIDE = 384, 16, 4, 16, 16, 32768
HEAD = ("h", "w", "f", "tw", "th", "valid", "slot", "estimated", "sx", "sy", "n", "agree")
BAD_FRAME = 8


def luma(frame):
    p = np.asarray(frame).astype(np.int64)
    return (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8


def geometry(h, w, radius):
    """(f, tw, th, gx, gy) of step 1 and 2; gx, gy are 0 when the window does not fit."""
    f = max(1, -(-w // SIDE), -(-h // SIDE))
    tw, th = w // f, h // f
    gx = (tw - 2 * radius) // BLOCK if tw >= 2 * radius + BLOCK else 0
    gy = (th - 2 * radius) // BLOCK if th >= 2 * radius + BLOCK else 0
    return f, tw, th, gx, gy


def thumbnail(frame, f, tw, th):
    """uint8 [th, tw]: the f x f box filter of the luma, integer division, partial edges dropped."""
    y = luma(frame)[:th * f, :tw * f]
    return (y.reshape(th, f, tw, f).sum(axis=(1, 3)) // (f * f)).astype(np.uint8)


def block_votes(cur, prev, radius, gx, gy):
    """(valid bool [gy, gx], dx int [gy, gx], dy int [gy, gx], sad int [gy, gx]) of step 3; every candidate is tried in the order
    of its key's tail (dx^2 + dy^2, dy, dx), so that a strict `<` on the SAD leaves the smallest key."""
    R = radius
    cur, prev = cur.astype(np.int64), prev.astype(np.int64)
    win = cur[R:R + BLOCK * gy, R:R + BLOCK * gx]
    blocks = win.reshape(gy, BLOCK, gx, BLOCK)
    valid = (blocks.max(axis=(1, 3)) - blocks.min(axis=(1, 3))) >= MIN_CONTRAST
    best = np.full((gy, gx), np.iinfo(np.int64).max)
    bdx, bdy = np.zeros((gy, gx), np.int64), np.zeros((gy, gx), np.int64)
    for dx, dy in sorted(((dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda c: (c[0] ** 2 + c[1] ** 2, c[1], c[0])):
        ref = prev[R - dy:R - dy + BLOCK * gy, R - dx:R - dx + BLOCK * gx]
        sad = np.abs(win - ref).reshape(gy, BLOCK, gx, BLOCK).sum(axis=(1, 3))
        take = sad < best
        best, bdx, bdy = np.where(take, sad, best), np.where(take, dx, bdx), np.where(take, dy, bdy)
    return valid, bdx, bdy, best


def global_shift(valid, dx, dy):
    """(estimated, dx*, dy*, n, agree) of step 4, in thumbnail pixels."""
    vx, vy = dx[valid].reshape(-1), dy[valid].reshape(-1)
    n = int(vx.size)
    if n < MIN_BLOCKS:
        return 0, 0, 0, n, 0
    mx, my = int(np.sort(vx)[(n - 1) // 2]), int(np.sort(vy)[(n - 1) // 2])
    agree = int(((np.abs(vx - mx) <= 1) & (np.abs(vy - my) <= 1)).sum())
    if 2 * agree < n:
        return 0, 0, 0, n, agree
    return 1, mx, my, n, agree


def fresh_motion():
    return {"head": np.zeros(16, np.int32), "thumb": np.zeros((2, SIDE * SIDE), np.uint8)}


class RefMotion:
    """One stream.  step(frame uint8 [h, w, 3], track_state or None) -> out_motion int32 [6] = (estimated, sx, sy, n, agree, f);
    `track_state` (the dict RefTracker.s) is shifted in place.  `votes` keeps the block votes of the last step for the tests.
    bad=True stands for a frame the device refuses (DETR_TRACK_BAD_FRAME): it is run as 0 x 0."""

    def __init__(self, radius=8):
        assert 1 <= radius <= MAX_RADIUS
        self.R = int(radius)
        self.m = fresh_motion()
        self.votes = None

    def state_dict(self):
        return {"motion_head": self.m["head"].copy(), "motion_thumb": self.m["thumb"].copy()}

    def load_state_dict(self, state):
        self.m = {"head": np.array(state["motion_head"], np.int32).reshape(16), "thumb": np.array(state["motion_thumb"], np.uint8).reshape(2, SIDE * SIDE)}

    def step(self, frame, track_state=None, bad=False):
        head, thumb = self.m["head"], self.m["thumb"]
        frame = np.asarray(frame)
        h, w = (0, 0) if bad else (int(frame.shape[0]), int(frame.shape[1]))
        assert bad or (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and frame.dtype == np.uint8 and frame.shape[2] == 3)
        f, tw, th, gx, gy = geometry(h, w, self.R)
        old = {k: int(v) for k, v in zip(HEAD, head)}
        slot = old["slot"] ^ 1
        # 1. the thumbnail, dense in the other slot
        cur = thumbnail(frame, f, tw, th) if tw and th else np.zeros((th, tw), np.uint8)
        thumb[slot, :th * tw] = cur.reshape(-1)
        # 2..4
        est, mx, my, n, agree = 0, 0, 0, 0, 0
        self.votes = None
        if old["valid"] == 1 and (old["h"], old["w"]) == (h, w) and gx >= 1 and gy >= 1:
            prev = thumb[old["slot"], :th * tw].reshape(th, tw)
            self.votes = block_votes(cur, prev, self.R, gx, gy)
            est, mx, my, n, agree = global_shift(*self.votes[:3])
        sx, sy = mx * f, my * f
        # 5. apply
        if est and track_state is not None:
            for t in range(len(track_state["id"])):
                if track_state["id"][t] >= 1:
                    track_state["x"][t, 0] = track_state["x"][t, 0] + F(sx)
                    track_state["x"][t, 1] = track_state["x"][t, 1] + F(sy)
        # 6. book-keeping
        head[:] = 0
        head[:12] = (h, w, f, tw, th, 1, slot, est, sx, sy, n, agree)
        return np.array([est, sx, sy, n, agree, f], np.int32)


def stack_motion(motions):
    """The motion_head / motion_thumb entries of a Tracker with one stream per RefMotion."""
    return {"motion_head": np.stack([m.m["head"] for m in motions]), "motion_thumb": np.stack([m.m["thumb"] for m in motions])}


# ---- synthetic scenes: random 4 x 4-pixel blocks of texture, a frame is a crop of one large scene --------------------------------
def scene(seed, h, w, cell=4):
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, size=(-(-h // cell), -(-w // cell), 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(small, cell, axis=0), cell, axis=1)[:h, :w])


def crop(big, y0, x0, h, w):
    assert 0 <= y0 and y0 + h <= big.shape[0] and 0 <= x0 and x0 + w <= big.shape[1]
    return np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w])


def shifted_pair(seed, h, w, dx, dy, f, margin):
    """Two frames of one scene: the content of the second is the first's moved by (dx, dy) THUMBNAIL pixels (the camera moved the
    other way), margin >= the largest |shift| in image pixels."""
    big = scene(seed, h + 2 * margin, w + 2 * margin)
    return crop(big, margin, margin, h, w), crop(big, margin - dy * f, margin - dx * f, h, w)
