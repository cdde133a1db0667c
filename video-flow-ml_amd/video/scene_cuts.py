"""Scene cuts: the project's own integer definition, host side.

A frame's signature S[16][64] counts its pixels per cell of a 4x4 grid and per bin Y >> 2 of the integer luma
Y = (77 R + 150 G + 29 B + 128) >> 8; d[t] = sum |S_t - S_{t-1}| (d[0] = 0); the score hs[t] = 1000 d[t] // (2 H W), per
mille.  A scene starts at frame t >= 1 iff hs[t] >= TH and hs[t] >= R * max(hs[t-1], hs[t+1]) - an isolated peak; a
neighbour outside 1..n-1 counts as 0 - and at frame 0.  The device path (vfml_scene_distances) computes the same S and d;
everything from the score on is Python integers here, whichever path made d."""
import json
import os

import numpy as np

DEFAULT_TH, DEFAULT_R = 200, 3          # settings of the definition; not tuned on real footage
CELLS, BINS = 16, 64
SCENES_FILE = "scenes.json"


def frame_signature(frame):
    """uint8 [H,W,3] RGB -> uint32 [16, 64]."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.shape[0] < 1 or frame.shape[1] < 1:
        raise ValueError(f"frame_signature: a uint8 [H,W,3] frame expected, got {frame.dtype} {frame.shape}")
    H, W = frame.shape[:2]
    if H * W >= 1 << 31:
        raise ValueError(f"frame_signature: frame {W}x{H} has 2^31 pixels or more")
    f = frame.astype(np.uint32)
    y = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8
    cell = ((np.arange(H, dtype=np.int64) * 4 // H) * 4)[:, None] + (np.arange(W, dtype=np.int64) * 4 // W)[None, :]
    idx = cell * BINS + (y >> 2).astype(np.int64)
    return np.bincount(idx.reshape(-1), minlength=CELLS * BINS).astype(np.uint32).reshape(CELLS, BINS)


def signature_distance(sig, prev):
    """sum |sig - prev| as a Python integer."""
    return int(np.abs(sig.astype(np.int64) - prev.astype(np.int64)).sum())


def clip_distances(frames, prev_sig=None):
    """frames (a sequence of uint8 [H,W,3]) -> (signatures uint32 [n,16,64], distances: list of Python integers);
    frames[0] is measured against prev_sig, or gets 0 without one."""
    sigs, dist = [], []
    for f in frames:
        s = frame_signature(f)
        dist.append(0 if prev_sig is None else signature_distance(s, prev_sig))
        sigs.append(s)
        prev_sig = s
    return np.stack(sigs), dist


def score(d, height, width):
    """The per-mille score of a distance: Python integers."""
    return 1000 * int(d) // (2 * int(height) * int(width))


def _is_start(hs, t, n, th, r):
    before = hs[t - 1] if t - 1 >= 1 else 0
    after = hs[t + 1] if t + 1 <= n - 1 else 0
    return hs[t] >= th and hs[t] >= r * max(before, after)


def scene_starts(hs, th=DEFAULT_TH, r=DEFAULT_R):
    """Scores of a whole clip (hs[0] is ignored: frame 0 always starts a scene) -> ascending list of scene starts."""
    n = len(hs)
    return [0] * (n > 0) + [t for t in range(1, n) if _is_start(hs, t, n, th, r)]


class SceneIndex:
    """The scenes of a clip of n frames, known as far as scores have arrived (`push`, in frame order from `first` on).
    Whether frame t starts a scene is decided once hs[t+1] is known, or t is the clip's last frame.  `first`: the first frame
    whose score arrives (a job that skips the frames before it); it counts as a scene start, like frame 0.
    `source`: None, or a callable f -> the score of frame f, or None while it has not been measured; a question then takes
    in the scores it needs (a ClipFeeder's index: the frames are measured as they are uploaded)."""

    def __init__(self, n, th=DEFAULT_TH, r=DEFAULT_R, first=0, source=None):
        self.n, self.th, self.r, self.first = int(n), int(th), int(r), int(first)
        self.source = source
        self.hs = [0] * self.n
        self.known = self.first          # scores of frames [first, known) have arrived
        self.starts = [self.first] if self.n else []
        self._decided = self.first       # frames [first, _decided] are classified

    def push(self, hs):
        """The score of frame `known`."""
        if self.known >= self.n:
            raise IndexError(f"SceneIndex: all {self.n} scores are in")
        # (the first frame of the index has no predecessor here: it starts a scene whatever its score)
        self.hs[self.known] = 0 if self.known == self.first else int(hs)
        self.known += 1
        self._advance()

    def _advance(self):
        while self._decided + 1 < self.n and (self._decided + 2 < self.known or self.known == self.n):
            t = self._decided + 1
            if _is_start(self.hs, t, self.n, self.th, self.r):      # (hs[first] is 0, like a neighbour outside 1..n-1)
                self.starts.append(t)
            self._decided = t

    @property
    def decided(self):
        """The last frame known to start a scene or not (-1 before the first score)."""
        return self._decided if self.known > self.first else -1

    def _pull(self, upto):
        while self.source is not None and self.known <= min(upto, self.n - 1):
            v = self.source(self.known)
            if v is None:
                break
            self.push(v)

    def scene_of(self, f, reach=None):
        """-> (a, b): frame f lies in the scene [a, b).  reach=None: b is the scene's end, and every score must be in.
        reach=k: only frames up to f + k matter to the caller (a window that reaches k frames ahead): b is the first scene
        start in (f, f + k], or min(n, f + k + 1) when there is none - the scene goes on at least that far, which gives
        such a window the frames the true end would.  Raises LookupError when the scores needed have not arrived."""
        if not self.first <= f < self.n:
            raise LookupError(f"SceneIndex: frame {f} outside {self.first}..{self.n - 1}")
        last = self.n - 1 if reach is None else min(self.n - 1, f + reach)
        self._pull(last + 1)
        if self.decided < last:
            raise LookupError(f"SceneIndex: the scene of frame {f} needs the score of frame {min(self.n - 1, last + 1)}, "
                              f"scores have arrived up to frame {self.known - 1}")
        a, b = self.first, (self.n if reach is None else last + 1)
        for s in self.starts:
            if s <= f:
                a = s
            elif s <= last:
                b = s
                break
            else:
                break
        return a, b

    def scene_window(self, window_indices, f, half):
        """The window of frame f inside its scene taken as a clip of its own: [a + i for i in window_indices(b - a, f - a)]."""
        a, b = self.scene_of(f, half)
        return [a + i for i in window_indices(b - a, f - a)]


def index_of(hs, th=DEFAULT_TH, r=DEFAULT_R):
    """A complete SceneIndex of a clip's scores."""
    idx = SceneIndex(len(hs), th, r)
    for v in hs:
        idx.push(v)
    return idx


def host_scene_index(frames, th=DEFAULT_TH, r=DEFAULT_R):
    """The numpy path (--device cpu, and the definition the device path is held to): frames -> complete SceneIndex."""
    frames = list(frames)
    h, w = frames[0].shape[:2]
    _, dist = clip_distances(frames)
    return index_of([score(d, h, w) for d in dist], th, r)


def check_scene_cuts(value, source="scene_cuts"):
    """The scene-cut setting -> None (off) or (TH, R): None / False / 0 / "0" are off, True / 1 / "1" the defaults, "TH,R"
    two integers with TH >= 1 and R >= 2; anything else is refused."""
    if value is None or value is False:
        return None
    if value is True:
        return DEFAULT_TH, DEFAULT_R
    if isinstance(value, tuple) and len(value) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in value):
        text = f"{value[0]},{value[1]}"
    else:
        text = str(value).strip() if isinstance(value, (int, str)) else ""
    if text == "0":
        return None
    if text == "1":
        return DEFAULT_TH, DEFAULT_R
    parts = text.split(",")
    if len(parts) == 2 and all(p.strip().isdigit() for p in parts):
        th, r = int(parts[0]), int(parts[1])
        if th >= 1 and r >= 2:
            return th, r
    raise ValueError(f"{source} = {value!r}: scene-cut detection is switched with 0 or 1, or set with TH,R (integers, "
                     f"threshold TH >= 1 per mille, ratio R >= 2)")


def cache_suffix(cuts):
    """What a cache directory's name carries for a job with cuts on: "cuts", or "cuts{TH}x{R}" off the defaults."""
    th, r = cuts
    return "cuts" if (th, r) == (DEFAULT_TH, DEFAULT_R) else f"cuts{th}x{r}"


def write_scenes(cache_dir, index):
    """scenes.json of a finished job: threshold, ratio, starts, score."""
    index.scene_of(index.n - 1)         # (complete, or this raises)
    doc = {"threshold": index.th, "ratio": index.r, "starts": [int(s) for s in index.starts],
           "score": [int(v) for v in index.hs]}
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, SCENES_FILE)
    with open(path + ".tmp", "w") as f:
        json.dump(doc, f)
    os.replace(path + ".tmp", path)
    return path


def read_scenes(cache_dir):
    """-> the dictionary write_scenes wrote, or None when the directory has no scenes.json."""
    path = os.path.join(cache_dir, SCENES_FILE)
    if not os.path.exists(path):
        return None
    with open(path) as f:
        doc = json.load(f)
    if not (isinstance(doc, dict) and isinstance(doc.get("starts"), list) and all(isinstance(s, int) for s in doc["starts"])):
        raise ValueError(f"{path}: not a scenes.json of this project")
    return doc
