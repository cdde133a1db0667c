"""video — video properties and frame extraction (mirror of the reference's video/ package), over the inputs this
project reads: `synthetic:WxHxF`, `.npy` frame stacks, its own AVI reader, and OpenCV where it is installed."""
from .video_info import VideoInfo
from .frame_extractor import FrameExtractor, fast_mode_dimensions, resize_frame

__all__ = ['VideoInfo', 'FrameExtractor', 'fast_mode_dimensions', 'resize_frame']
