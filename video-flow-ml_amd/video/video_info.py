"""Video properties: API mirror of reference video/video_info.py (VideoInfo) and the input probing / decoding that
flow_processor.py shares with it.  An input is `synthetic:WxHxF` (vfml.synth), a `.npy` file holding uint8 frames
[F,H,W,3], an `.avi` file of the kinds storage/avi_writer.py writes (storage/avi_reader.py, when OpenCV is not
importable), or any video file when OpenCV is."""
import os
from typing import Any, Dict, Tuple

import numpy as np

SYNTHETIC_FPS = 30.0     # frame rate of `synthetic:` clips and .npy frame stacks (they carry none)


def time_to_frame(time_seconds, fps):
    """Seconds -> frame number, the reference's rule (flow_processor.py:137-139, video/video_info.py:80-93)."""
    if fps <= 0:
        raise ValueError("Cannot convert time to frame: invalid FPS")
    return int(time_seconds * fps)


def validate_frame_range(start_frame, frame_count, total_frames):
    """The reference's clamp (video/video_info.py:110-132): negative starts become 0, a start past the end is an
    error, the count is cut to what the clip holds."""
    if start_frame < 0:
        start_frame = 0
    elif start_frame >= total_frames:
        raise ValueError(f"Start frame {start_frame} exceeds total frames {total_frames}")
    return start_frame, min(frame_count, total_frames - start_frame)


def own_avi_reader(spec):
    """True when `spec` is an .avi file and OpenCV is not importable: storage/avi_reader.py reads it then."""
    if not spec.lower().endswith('.avi'):
        return False
    try:
        import cv2  # noqa: F401
    except ImportError:
        return True
    return False


def _synthetic(spec):
    w, h, n = (int(v) for v in spec.split(':', 1)[1].lower().split('x'))
    return w, h, n


def _npy(spec):
    arr = np.load(spec, mmap_mode='r')
    if arr.ndim != 4 or arr.shape[3] != 3 or arr.dtype != np.uint8:
        raise ValueError(f"{spec}: expected uint8 [F,H,W,3], got {arr.dtype} {arr.shape}")
    return arr


def _cv2_or_exit(spec):
    try:
        import cv2
    except ImportError:
        raise SystemExit(f"Cannot decode {spec}: OpenCV is not installed. Use a .npy frame stack or synthetic:WxHxF.")
    return cv2


def probe_video(spec):
    """-> dict(fps, width, height, total_frames) of an input without decoding it."""
    if spec.startswith('synthetic:'):
        w, h, n = _synthetic(spec)
        return {"fps": SYNTHETIC_FPS, "width": w, "height": h, "total_frames": n}
    if spec.endswith('.npy'):
        shape = np.load(spec, mmap_mode='r').shape
        return {"fps": SYNTHETIC_FPS, "width": int(shape[2]) if len(shape) > 2 else 0,
                "height": int(shape[1]) if len(shape) > 1 else 0, "total_frames": int(shape[0])}
    if own_avi_reader(spec):
        from storage import avi_reader
        info = avi_reader.probe(spec)
        return {"fps": info["fps"], "width": int(info["width"]), "height": int(info["height"]),
                "total_frames": info["frames"]}
    cv2 = _cv2_or_exit(spec)
    cap = cv2.VideoCapture(spec)
    try:
        return {"fps": cap.get(cv2.CAP_PROP_FPS), "width": int(cap.get(cv2.CAP_PROP_FRAME_WIDTH)),
                "height": int(cap.get(cv2.CAP_PROP_FRAME_HEIGHT)), "total_frames": int(cap.get(cv2.CAP_PROP_FRAME_COUNT))}
    finally:
        cap.release()


def read_frames(spec, start_frame, max_frames, fps_default=SYNTHETIC_FPS):
    """-> (frames list of uint8 RGB [H,W,3], fps): frames [start_frame, start_frame + max_frames) of an input, as far
    as it holds them."""
    if spec.startswith('synthetic:'):
        from vfml.synth import synthetic_clip
        w, h, n = _synthetic(spec)
        return synthetic_clip(n, h, w)[start_frame:start_frame + max_frames], fps_default
    if spec.endswith('.npy'):
        return [np.ascontiguousarray(f) for f in _npy(spec)[start_frame:start_frame + max_frames]], fps_default
    if own_avi_reader(spec):
        from storage import avi_reader
        return avi_reader.read_frames(spec, start_frame, max_frames), avi_reader.probe(spec)["fps"] or fps_default
    cv2 = _cv2_or_exit(spec)
    cap = cv2.VideoCapture(spec)
    fps = cap.get(cv2.CAP_PROP_FPS) or fps_default
    cap.set(cv2.CAP_PROP_POS_FRAMES, start_frame)
    frames = []
    while len(frames) < max_frames:
        ok, bgr = cap.read()
        if not ok:
            break
        frames.append(cv2.cvtColor(bgr, cv2.COLOR_BGR2RGB))
    cap.release()
    return frames, fps


class VideoInfo:
    """Video information extractor and utilities (the reference's class; its methods, errors and strings)."""

    def __init__(self, video_path: str):
        self.video_path = str(video_path)
        self._info_cache = None
        if not (self.video_path.startswith('synthetic:') or os.path.exists(self.video_path)):
            raise FileNotFoundError(f"Video file not found: {video_path}")

    def get_info(self) -> Dict[str, Any]:
        """-> dict(fps, width, height, total_frames, duration_seconds, path), probed once."""
        if self._info_cache is not None:
            return self._info_cache
        try:
            p = probe_video(self.video_path)
        except (OSError, ValueError) as e:
            raise ValueError(f"Cannot open video: {self.video_path}") from e
        info = {'fps': p["fps"], 'width': p["width"], 'height': p["height"], 'total_frames': p["total_frames"],
                'duration_seconds': None, 'path': self.video_path}
        if info['fps'] > 0:
            info['duration_seconds'] = info['total_frames'] / info['fps']
        self._info_cache = info
        return info

    def get_fps(self) -> float:
        return self.get_info()['fps']

    def get_dimensions(self) -> Tuple[int, int]:
        """(width, height)"""
        info = self.get_info()
        return info['width'], info['height']

    def get_frame_count(self) -> int:
        return self.get_info()['total_frames']

    def get_duration(self) -> float:
        duration = self.get_info()['duration_seconds']
        if duration is None:
            raise ValueError("Cannot calculate duration: invalid FPS")
        return duration

    def time_to_frame(self, time_seconds: float) -> int:
        return time_to_frame(time_seconds, self.get_fps())

    def frame_to_time(self, frame_number: int) -> float:
        fps = self.get_fps()
        if fps <= 0:
            raise ValueError("Cannot convert frame to time: invalid FPS")
        return frame_number / fps

    def validate_frame_range(self, start_frame: int, frame_count: int) -> Tuple[int, int]:
        return validate_frame_range(start_frame, frame_count, self.get_frame_count())

    def print_info(self):
        info = self.get_info()
        print(f"Video: {info['path']}")
        print(f"Dimensions: {info['width']}x{info['height']}")
        print(f"FPS: {info['fps']:.2f}")
        print(f"Total frames: {info['total_frames']}")
        if info['duration_seconds']:
            print(f"Duration: {info['duration_seconds']:.2f}s")

    def reset_cache(self):
        self._info_cache = None
