"""Output video frames from their tiles: API mirror of reference visualization/video_composer.py (:67-122).

`create_side_by_side` returns a BGR frame as the reference does: original | flow side by side, the two stacked
(`flow_only`), or a 2x2 grid original | flow over TAA | TAA simple, where a TAA history becomes uint8 by
`np.clip(x, 0, 255).astype(np.uint8)` (NaN -> 0).  numpy tiles are composed on the host; device tensors by
`vfml_compose_frame` in one pass, which can also write the frame straight in an AVI chunk's layout (RGB / BGR,
bottom-up rows, padded stride; `compose_device`).

Text labels are NOT drawn: the reference renders them with OpenCV's Hershey font (cv2.putText), which is not a
dependency here.  `add_text_overlay` returns the frame unchanged, so the tiles carry the picture only.
`create_video_grid` and the 6-tile `--flow-input` grid are not built.
"""
from typing import Optional, Tuple, Union

import numpy as np

try:
    import torch
except ImportError:          # pragma: no cover
    torch = None


def _on_gpu(x):
    return torch is not None and torch.is_tensor(x) and x.is_cuda


def history_to_u8(img):
    """np.clip(x, 0, 255).astype(np.uint8) of a TAA history, NaN -> 0 (uint8 tiles pass through)."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img
    with np.errstate(invalid="ignore"):
        c = np.clip(np.nan_to_num(img, nan=0.0), 0, 255)
    return c.astype(np.uint8)


def layout_of(flow_only, taa):
    from vfml import hip
    return hip.COMPOSE_STACKED if flow_only else (hip.COMPOSE_GRID_2X2 if taa else hip.COMPOSE_SIDE_BY_SIDE)


def compose_device(original, flow_viz, taa_frame=None, taa_simple_frame=None, flow_only=False, bgr=True,
                   bottom_up=False, row_stride=None, out=None):
    """Device tiles -> one uint8 device frame [rows, row_stride] (vfml_compose_frame)."""
    from vfml import hip
    if flow_only or taa_frame is None:
        tiles = [original, flow_viz]
    else:
        if taa_simple_frame is None:
            raise ValueError("compose_device: the 2x2 grid needs both TAA frames (the 3-wide layout is host only)")
        tiles = [original, flow_viz, taa_frame, taa_simple_frame]
    return hip.compose_frame(tiles, layout_of(flow_only, taa_frame is not None), bgr=bgr, bottom_up=bottom_up,
                             row_stride=row_stride, out=out)


class VideoComposer:
    """Main class for video composition operations."""

    def add_text_overlay(self, frame, text: str, position: Union[str, Tuple[int, int]] = 'top-left',
                         font_scale: float = 0.4, color: Tuple[int, int, int] = (255, 255, 255), thickness: int = 1):
        """The reference draws `text` with OpenCV's Hershey font; this build has no font renderer and returns the
        frame unchanged."""
        return frame

    def create_side_by_side(self, original, flow_viz, flow_only: bool = False, taa_frame=None, taa_simple_frame=None,
                            model_name: str = "VideoFlow", fast_mode: bool = False, flow_format: str = "gamedev"):
        """Side-by-side, flow-only (stacked) or TAA (2x2 grid; 3 wide with one TAA frame) composition, BGR, without
        the reference's text labels."""
        if _on_gpu(original):
            if taa_frame is not None and taa_simple_frame is None and not flow_only:
                raise ValueError("create_side_by_side: the 3-wide single-TAA layout is host only")
            out = compose_device(original, flow_viz, taa_frame, taa_simple_frame, flow_only)
            return out.view(out.shape[0], -1, 3)
        h, w = original.shape[:2]
        if flow_viz.shape[:2] != (h, w):
            raise ValueError(f"create_side_by_side: flow picture {flow_viz.shape[:2]} is not at the frame's size "
                             f"{(h, w)} (the reference resizes it with OpenCV; not built)")
        orig_bgr = np.ascontiguousarray(original[:, :, ::-1])
        flow_bgr = np.ascontiguousarray(flow_viz[:, :, ::-1])
        if flow_only:
            return np.concatenate([orig_bgr, flow_bgr], axis=0)
        if taa_frame is not None and taa_simple_frame is not None:
            taa_bgr = history_to_u8(taa_frame)[:, :, ::-1]
            simple_bgr = history_to_u8(taa_simple_frame)[:, :, ::-1]
            return np.concatenate([np.concatenate([orig_bgr, flow_bgr], axis=1),
                                   np.concatenate([taa_bgr, simple_bgr], axis=1)], axis=0)
        if taa_frame is not None:
            return np.concatenate([orig_bgr, flow_bgr, history_to_u8(taa_frame)[:, :, ::-1]], axis=1)
        return np.concatenate([orig_bgr, flow_bgr], axis=1)


def add_text_overlay(frame, text: str, position: Union[str, Tuple[int, int]] = 'top-left', font_scale: float = 0.4,
                     color: Tuple[int, int, int] = (255, 255, 255), thickness: int = 1):
    """Returns the frame unchanged (no font renderer in this build)."""
    return VideoComposer().add_text_overlay(frame, text, position, font_scale, color, thickness)


def create_side_by_side(original, flow_viz, flow_only: bool = False, taa_frame: Optional[np.ndarray] = None,
                        taa_simple_frame: Optional[np.ndarray] = None, model_name: str = "VideoFlow",
                        fast_mode: bool = False, flow_format: str = "gamedev"):
    return VideoComposer().create_side_by_side(original, flow_viz, flow_only, taa_frame, taa_simple_frame, model_name,
                                               fast_mode, flow_format)
