"""The uint8 picture resize, stated once in plain numpy: OpenCV's 8-bit INTER_LINEAR scheme as this
project defines it.  `video.resize_frame` (host) and `vfml_resize_u8` (device) must match `resize` byte for byte.  Written
for clarity, not speed; nothing here is shared with the code under test, and nothing is pinned against cv2."""
import numpy as np


def fast_mode_dimensions(width, height):
    """The --fast resolution rule -> (w, h, scale): fit 256 x 256 without enlarging, at most a quarter of a source whose
    longer side exceeds 512 and half of one that exceeds 256, even sides rounded down, at least 64 each."""
    scale = min(256 / width, 256 / height, 1.0)
    if max(width, height) > 512:
        scale = min(scale, 0.25)
    elif max(width, height) > 256:
        scale = min(scale, 0.5)
    w, h = int(width * scale), int(height * scale)
    return max(64, w - w % 2), max(64, h - h % 2), scale


def taps(S, D):
    """One axis, source length S -> destination length D: (s, s1, a0, a1), each an array of D integers."""
    scale = np.float64(S) / np.float64(D)
    s, s1, a0, a1 = [], [], [], []
    for d in range(D):
        f = np.float32((d + 0.5) * scale - 0.5)
        i = int(np.floor(f))
        f = np.float32(f - np.float32(i))
        if i < 0:
            i, f = 0, np.float32(0)
        if i >= S - 1:
            i, f = S - 1, np.float32(0)
        s.append(i)
        s1.append(min(i + 1, S - 1))
        a1.append(int(np.rint(np.float32(f * np.float32(2048)))))
        a0.append(int(np.rint(np.float32((np.float32(1) - f) * np.float32(2048)))))
    return np.array(s), np.array(s1), np.array(a0, dtype=np.int64), np.array(a1, dtype=np.int64)


def resize_values(img, size):
    """img [H,W,3] uint8, size = (h, w) -> the results BEFORE the cast to uint8, int64 [h,w,3]."""
    H, W = img.shape[:2]
    h, w = size
    x = img.astype(np.int64)
    if (h, w) == (H, W):
        return x
    if H == 2 * h and W == 2 * w:
        return (x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2] + 2) >> 2
    xs, xs1, a0, a1 = taps(W, w)
    ys, ys1, b0, b1 = taps(H, h)
    rows = x[:, xs] * a0[None, :, None] + x[:, xs1] * a1[None, :, None]          # horizontal pass, every source row
    r0, r1 = rows[ys], rows[ys1]
    return (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2


def resize(img, size):
    """img [H,W,3] uint8, size = (h, w) -> [h,w,3] uint8."""
    return resize_values(img, size).astype(np.uint8)
