"""Frame extraction with the fast mode's resolution reduction: API mirror of reference video/frame_extractor.py.

`resize_frame` is the uint8 picture resize the reference takes from `cv2.resize(frame, (w, h))`: OpenCV's 8-bit
INTER_LINEAR scheme as this project defines it - unchanged at its own size, the 2x2 mean when
both sides halve exactly, else two taps per axis in 11-bit fixed point with the taps and weights of
`vfml.hip.resize_tables`.  numpy pictures are resized here; device tensors by `vfml_resize_u8`, byte for byte the same.
"""
from typing import List, Optional, Tuple

import numpy as np

from .video_info import VideoInfo, read_frames

try:
    import torch
except ImportError:          # pragma: no cover
    torch = None


def fast_mode_dimensions(orig_width, orig_height):
    """The fast mode's size rule -> (width, height, scale_factor): fit 256 x 256 without enlarging, at most a quarter
    of a source whose longer side exceeds 512 and half of one that exceeds 256; even sides (rounded down), at least
    64 each.  The sides are the rule's even when the factor is 1.0 and nothing is resized."""
    scale = min(256 / orig_width, 256 / orig_height, 1.0)
    longer = max(orig_width, orig_height)
    if longer > 512:
        scale = min(scale, 0.25)
    elif longer > 256:
        scale = min(scale, 0.5)
    width, height = int(orig_width * scale), int(orig_height * scale)
    return max(64, width & ~1), max(64, height & ~1), scale


def resize_frame(frame, size):
    """frame [H,W,3] uint8, size = (w, h) as cv2.resize takes it -> [h,w,3] uint8.  A device tensor goes to
    vfml_resize_u8 and comes back as a device tensor."""
    w, h = int(size[0]), int(size[1])
    if torch is not None and torch.is_tensor(frame) and frame.is_cuda:
        from vfml import hip
        return hip.resize_u8(frame, (h, w))
    from vfml.hip import resize_tables
    img = np.asarray(frame)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError(f"resize_frame: uint8 [H,W,3] picture expected, got {img.dtype} {img.shape}")
    if w < 1 or h < 1:
        raise ValueError(f"resize_frame: size {(w, h)}")
    H, W = img.shape[:2]
    if (h, w) == (H, W):
        return img
    if H == 2 * h and W == 2 * w:
        x = img.astype(np.int32)
        return ((x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    tx, ty = resize_tables(W, w), resize_tables(H, h)
    # horizontal pass over the source rows the vertical taps name, then the vertical pass; int32 throughout
    rows, inv = np.unique(np.concatenate([ty[:, 0], ty[:, 1]]), return_inverse=True)
    x = img[rows].astype(np.int32)
    r = x[:, tx[:, 0]] * tx[:, 2][None, :, None] + x[:, tx[:, 1]] * tx[:, 3][None, :, None]
    r >>= 4
    r0, r1 = r[inv[:h]], r[inv[h:]]
    v = (((ty[:, 2][:, None, None] * r0) >> 16) + ((ty[:, 3][:, None, None] * r1) >> 16) + 2) >> 2
    return v.astype(np.uint8)


DEVICE_BATCH = 16        # frames per upload / vfml_resize_u8 launch of the device path


def _resize_on_device(frames, size, device):
    """The frames resized by vfml_resize_u8, a batch at a time, and copied back."""
    from vfml import hip
    w, h = size
    out = []
    for k in range(0, len(frames), DEVICE_BATCH):
        batch = torch.from_numpy(np.stack(frames[k:k + DEVICE_BATCH])).to(device)
        out.extend(hip.resize_u8(batch, (h, w)).cpu().numpy())
    return out


class FrameExtractor:
    """Video frame extractor with fast mode and time-based extraction."""

    def __init__(self, video_path: str, fast_mode: bool = False, device=None):
        """device: None - frames are resized on the host; a CUDA device - by vfml_resize_u8, in batches, and the small
        frames are copied back.  Either way the frames returned are host arrays."""
        self.video_info = VideoInfo(video_path)
        self.fast_mode = fast_mode
        self.device = device

    def calculate_fast_mode_dimensions(self, orig_width: int, orig_height: int) -> Tuple[int, int, float]:
        if not self.fast_mode:
            return orig_width, orig_height, 1.0
        return fast_mode_dimensions(orig_width, orig_height)

    def _reduce(self, frames, size):
        if self.device is not None and str(self.device).startswith('cuda'):
            return _resize_on_device(frames, size, self.device)
        return [resize_frame(f, size) for f in frames]

    def extract_frames(self, max_frames: int = 1000, start_frame: int = 0, start_time: Optional[float] = None,
                       duration: Optional[float] = None) -> Tuple[List[np.ndarray], float, int, int, int]:
        """-> (frames_list, fps, width, height, actual_start_frame); times, when given, replace the frame arguments."""
        info = self.video_info.get_info()
        fps, orig_width, orig_height = info['fps'], info['width'], info['height']
        if start_time is not None:
            start_frame = self.video_info.time_to_frame(start_time)
            print(f"Start time: {start_time}s -> frame {start_frame}")
        if duration is not None:
            max_frames = self.video_info.time_to_frame(duration)
            print(f"Duration: {duration}s -> {max_frames} frames")
        start_frame, frames_to_extract = self.video_info.validate_frame_range(start_frame, max_frames)
        width, height, scale_factor = self.calculate_fast_mode_dimensions(orig_width, orig_height)
        if self.fast_mode:
            print(f"Fast mode: aggressive resolution reduction from {orig_width}x{orig_height} to {width}x{height} "
                  f"(scale: {scale_factor:.2f})")
        frames, _ = read_frames(self.video_info.video_path, start_frame, frames_to_extract)
        if len(frames) < frames_to_extract:
            print(f"Warning: Could only extract {len(frames)} frames out of {frames_to_extract}")
        if self.fast_mode and scale_factor != 1.0:
            frames = self._reduce(frames, (width, height))
        print(f"Frame range: {start_frame} to {start_frame + len(frames) - 1}")
        return frames, fps, width, height, start_frame

    def extract_time_range(self, start_time: float, duration: float):
        return self.extract_frames(start_time=start_time, duration=duration)

    def get_frame_at_time(self, time_seconds: float) -> np.ndarray:
        """The frame at a time, reduced in fast mode (here, as in the reference, whatever the factor is)."""
        frame_number = self.video_info.time_to_frame(time_seconds)
        frames = []
        if 0 <= frame_number < self.video_info.get_frame_count():
            frames, _ = read_frames(self.video_info.video_path, frame_number, 1)
        if not frames:
            raise ValueError(f"Cannot read frame at time {time_seconds}s (frame {frame_number})")
        frame = frames[0]
        if self.fast_mode:
            info = self.video_info.get_info()
            width, height, _ = self.calculate_fast_mode_dimensions(info['width'], info['height'])
            frame = self._reduce([frame], (width, height))[0]
        return frame

    def print_extraction_info(self, frames_count: int, start_frame: int, fps: float):
        info = self.video_info.get_info()
        print(f"Video properties: {info['width']}x{info['height']} @ {fps:.2f} FPS")
        print(f"Extracting {frames_count} frames starting from frame {start_frame}")
        if self.fast_mode:
            width, height, scale = self.calculate_fast_mode_dimensions(info['width'], info['height'])
            if scale != 1.0:
                print(f"Fast mode: {info['width']}x{info['height']} -> {width}x{height} (scale: {scale:.2f})")
