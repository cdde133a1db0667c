"""Output video frames from their tiles: API mirror of reference visualization/video_composer.py (:67-122) and of the
two `--flow-input` helpers of the reference's flow_processor.py (create_difference_overlay :490-578,
create_6_video_grid :1218-1269).

`create_side_by_side` returns a BGR frame as the reference does: original | flow side by side, the two stacked
(`flow_only`), or a 2x2 grid original | flow over TAA | TAA simple, where a TAA history becomes uint8 by
`np.clip(x, 0, 255).astype(np.uint8)` (NaN -> 0).  numpy tiles are composed on the host; device tensors by
`vfml_compose_frame` in one pass, which can also write the frame straight in an AVI chunk's layout (RGB / BGR,
bottom-up rows, padded stride; `compose_device`).

`create_difference_overlay` is the radar picture of two flow fields' difference (RGB, a tile) with the legend's
colour squares; `create_6_video_grid` the 2 x 3 grid of `--taa --flow-input` (BGR): original | external flow picture
over TAA | TAA simple over TAA external flow | difference.  Device tensors go to `vfml_flow_diff_overlay` and to
`vfml_compose_frame`'s GRID_2X3 layout.  A filled rectangle is defined here as cv2.rectangle(thickness=-1) is used by
the reference: both corners inclusive, clipped to the picture.

Text labels are NOT drawn: the reference renders them with OpenCV's Hershey font (cv2.putText), which is not a
dependency here.  `add_text_overlay` returns the frame unchanged, so the tiles carry the picture only, and the
difference legend shows its squares without their numbers.  `create_video_grid` is not built.
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
                   bottom_up=False, row_stride=None, out=None, taa_external_frame=None, difference_overlay=None):
    """Device tiles -> one uint8 device frame [rows, row_stride] (vfml_compose_frame).  With `taa_external_frame` and
    `difference_overlay` the frame is the 2 x 3 grid of --flow-input."""
    from vfml import hip
    if taa_external_frame is not None:
        tiles = [original, flow_viz, taa_frame, taa_simple_frame, taa_external_frame, difference_overlay]
        if any(t is None for t in tiles):
            raise ValueError("compose_device: the 2x3 grid needs all six tiles")
        return hip.compose_frame(tiles, hip.COMPOSE_GRID_2X3, bgr=bgr, bottom_up=bottom_up, row_stride=row_stride,
                                 out=out)
    if flow_only or taa_frame is None:
        tiles = [original, flow_viz]
    else:
        if taa_simple_frame is None:
            raise ValueError("compose_device: the 2x2 grid needs both TAA frames (the 3-wide layout is host only)")
        tiles = [original, flow_viz, taa_frame, taa_simple_frame]
    return hip.compose_frame(tiles, layout_of(flow_only, taa_frame is not None), bgr=bgr, bottom_up=bottom_up,
                             row_stride=row_stride, out=out)


# difference classes: upper bounds (the last class is everything above 2.0) and their radar colours, RGB
DIFFERENCE_LEVELS = (0.1, 0.5, 1.0, 2.0)
RADAR_COLORS = ((0, 255, 0), (255, 255, 0), (255, 165, 0), (255, 0, 0), (255, 0, 255))


def fill_rectangle(img, corner0, corner1, color):
    """cv2.rectangle(img, corner0, corner1, color, thickness=-1) as this project defines it: (x, y) corners, both
    inclusive, clipped to the picture; in place."""
    h, w = img.shape[:2]
    xa, xb = sorted((corner0[0], corner1[0]))
    ya, yb = sorted((corner0[1], corner1[1]))
    xa, ya, xb, yb = max(xa, 0), max(ya, 0), min(xb, w - 1), min(yb, h - 1)
    if xa <= xb and ya <= yb:
        img[ya:yb + 1, xa:xb + 1] = color
    return img


def create_difference_overlay(original_flow, decoded_flow, magnitude_threshold=0.9):
    """Two flows [H,W,2] -> RGB [H,W,3] uint8: |original - decoded| per pixel in five classes (<= 0.1 green, <= 0.5
    yellow, <= 1 orange, <= 2 red, above magenta; NaN stays black), compared as numpy compares a float32 array with
    a Python float (in float32), and the legend's five squares at the bottom left, without their numbers.
    `magnitude_threshold` is unused, as in the reference.  Device tensors -> vfml_flow_diff_overlay."""
    if _on_gpu(original_flow):
        from vfml import hip
        if not _on_gpu(decoded_flow):
            decoded_flow = torch.as_tensor(np.asarray(decoded_flow, dtype=np.float32)).to(original_flow.device)
        return hip.flow_diff_overlay(original_flow, decoded_flow)
    with np.errstate(all="ignore"):
        d = original_flow - decoded_flow
        mag = np.sqrt(d[:, :, 0] ** 2 + d[:, :, 1] ** 2)
        h, w = d.shape[:2]
        overlay = np.zeros((h, w, 3), dtype=np.uint8)
        overlay[mag <= DIFFERENCE_LEVELS[0]] = RADAR_COLORS[0]
        for k in range(1, len(DIFFERENCE_LEVELS)):
            overlay[(mag > DIFFERENCE_LEVELS[k - 1]) & (mag <= DIFFERENCE_LEVELS[k])] = RADAR_COLORS[k]
        overlay[mag > DIFFERENCE_LEVELS[-1]] = RADAR_COLORS[-1]
    y0 = h - 20
    for i, color in enumerate(RADAR_COLORS):
        x = 10 + 45 * i
        fill_rectangle(overlay, (x - 1, y0 - 13), (x + 13, y0 + 1), (255, 255, 255))
        fill_rectangle(overlay, (x, y0 - 12), (x + 12, y0), color)
    return overlay


def create_6_video_grid(original_frame, flow_viz, taa_frame, taa_simple_frame, taa_external_frame,
                        difference_overlay):
    """The 2 x 3 grid of --taa --flow-input, BGR [3H, 2W, 3] uint8, without the reference's text labels: original |
    flow picture over TAA | TAA simple over TAA with the external flow | difference overlay.  The TAA histories become
    uint8 as in the 2x2 grid.  Device tensors are composed by vfml_compose_frame (GRID_2X3)."""
    tiles = [original_frame, flow_viz, taa_frame, taa_simple_frame, taa_external_frame, difference_overlay]
    if _on_gpu(original_frame):
        out = compose_device(*tiles[:4], taa_external_frame=taa_external_frame, difference_overlay=difference_overlay)
        return out.view(out.shape[0], -1, 3)
    h, w = original_frame.shape[:2]
    for t in tiles:
        if t.shape[:2] != (h, w):
            raise ValueError(f"create_6_video_grid: tile {t.shape[:2]} is not at the frame's size {(h, w)}")
    bgr = [history_to_u8(t)[:, :, ::-1] for t in tiles]
    return np.concatenate([np.concatenate(bgr[k:k + 2], axis=1) for k in (0, 2, 4)], axis=0)


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
        the reference's text labels.  A flow picture of another size than the frame is resized to it first."""
        h, w = original.shape[:2]
        if tuple(flow_viz.shape[:2]) != (h, w):
            # the reference's cv2.resize(flow_viz, (w, h)): the project's uint8 resize, host or device
            from video.frame_extractor import resize_frame
            flow_viz = resize_frame(flow_viz, (w, h))
        if _on_gpu(original):
            if taa_frame is not None and taa_simple_frame is None and not flow_only:
                raise ValueError("create_side_by_side: the 3-wide single-TAA layout is host only")
            out = compose_device(original, flow_viz, taa_frame, taa_simple_frame, flow_only)
            return out.view(out.shape[0], -1, 3)
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
