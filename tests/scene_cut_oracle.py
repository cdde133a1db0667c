"""The scene-cut definition in plain numpy, and the clips its tests run on.  Nothing here imports the
code under test (video/scene_cuts.py, vfml_scene_distances): both are held to this file.

For a uint8 RGB frame [H, W, 3]:
  luma        Y = (77 R + 150 G + 29 B + 128) >> 8
  cell        c = (y * 4 // H) * 4 + (x * 4 // W)          16 cells
  signature   S[16][64] = pixels per cell and bin Y >> 2   uint32
  distance    d[t] = sum |S_t - S_{t-1}|, d[0] = 0         at most 2 H W
  score       hs[t] = 1000 * d[t] // (2 * H * W)           per mille, Python integers
  a scene starts at t >= 1 iff hs[t] >= TH and hs[t] >= R * max(hs[t-1], hs[t+1]); a neighbour outside 1..n-1 counts as
  0; frame 0 always starts a scene.  Defaults TH = 200, R = 3."""
import numpy as np

TH, R = 200, 3


def signature(frame):
    H, W = frame.shape[:2]
    r, g, b = (frame[..., k].astype(np.int64) for k in range(3))
    y = (77 * r + 150 * g + 29 * b + 128) >> 8
    cy = np.arange(H) * 4 // H
    cx = np.arange(W) * 4 // W
    cell = cy[:, None] * 4 + cx[None, :]
    counts = np.bincount((cell * 64 + (y >> 2)).reshape(-1), minlength=16 * 64)
    return counts.reshape(16, 64).astype(np.uint32)


def signature_loop(frame):
    """The same, one pixel at a time in Python integers (small frames only)."""
    H, W = frame.shape[:2]
    sig = [[0] * 64 for _ in range(16)]
    for y in range(H):
        for x in range(W):
            r, g, b = (int(v) for v in frame[y, x])
            luma = (77 * r + 150 * g + 29 * b + 128) >> 8
            sig[(y * 4 // H) * 4 + (x * 4 // W)][luma >> 2] += 1
    return np.array(sig, dtype=np.uint32)


def distances(frames, prev_sig=None):
    """-> (signatures uint32 [n, 16, 64], distances uint32 [n]); frame 0 against prev_sig, or 0 without one."""
    sigs = [signature(f) for f in frames]
    out = []
    for t, s in enumerate(sigs):
        p = sigs[t - 1] if t else prev_sig
        out.append(0 if p is None else int(np.abs(s.astype(np.int64) - p.astype(np.int64)).sum()))
    return np.stack(sigs), np.array(out, dtype=np.uint32)


def scores(frames):
    H, W = frames[0].shape[:2]
    return [1000 * int(d) // (2 * H * W) for d in distances(frames)[1]]


def starts(hs, th=TH, r=R):
    n = len(hs)

    def at(t):
        return hs[t] if 1 <= t <= n - 1 else 0
    return [0] + [t for t in range(1, n) if hs[t] >= th and hs[t] >= r * max(at(t - 1), at(t + 1))]


# ------------------------------------------------------------------------------------------------------- the test clips
def grade(frames, gain, offset=0.0):
    """gain * f + offset in float64, clipped to 0..255 and truncated to uint8: a scene's grading."""
    return [np.clip(gain * f.astype(np.float64) + offset, 0, 255).astype(np.uint8) for f in frames]


def graded_clip(height, width):
    """13 frames, scene starts [0, 5, 9]: A = seed 0, 5 frames; B = seed 7 from start=40, 4 frames, graded 0.5 f + 100;
    C = seed 3 from start=9, 4 frames, graded 0.6 f.  (Two seeds of synthetic_clip have the same luma statistics: an
    ungraded splice is not detected, so the scenes are graded, as real cuts are.)"""
    from vfml.synth import synthetic_clip
    a = synthetic_clip(5, height, width, seed=0)
    b = grade(synthetic_clip(4, height, width, seed=7, start=40), 0.5, 100.0)
    c = grade(synthetic_clip(4, height, width, seed=3, start=9), 0.6)
    return a + b + c


GRADED_STARTS = [0, 5, 9]
GRADED_SCENES = [(0, 5), (5, 9), (9, 13)]


def flash_clip(height, width, n=9, at=4):
    """Seed 0 with +60 on one frame: two high scores side by side, no cut."""
    from vfml.synth import synthetic_clip
    frames = synthetic_clip(n, height, width, seed=0)
    frames[at] = np.clip(frames[at].astype(np.int64) + 60, 0, 255).astype(np.uint8)
    return frames


def fade_clip(height, width, n=10):
    """Seed 0 fading to black by 10 % per frame: a run of moderate scores, no cut."""
    from vfml.synth import synthetic_clip
    frames = synthetic_clip(n, height, width, seed=0)
    return [grade([f], max(0.0, 1.0 - 0.1 * t))[0] for t, f in enumerate(frames)]


def insert_clip(height, width, n=9, at=4):
    """Seed 0 with one frame of the graded scene B in place of frame `at`: a one-frame insert is two cuts one frame apart,
    which the isolated-peak rule does not fire on."""
    from vfml.synth import synthetic_clip
    frames = synthetic_clip(n, height, width, seed=0)
    frames[at] = grade(synthetic_clip(1, height, width, seed=7, start=40), 0.5, 100.0)[0]
    return frames
