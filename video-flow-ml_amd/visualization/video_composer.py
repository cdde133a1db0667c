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

Text labels are drawn with the project's own text (visualization/text.py, DESIGN.md section 9 "Text"): a stroke font
in the Hershey grid, integer coverage and blending, byte-equal between the numpy oracle of the tests, the host path here
and vfml_text_draw on the device; it is not pinned against cv2.putText.  Labels are OFF by default - the fixtures and
the render tests pin the frames without text - and are switched on by VFML_LABELS=1 (or `labels=True`): then
`add_text_overlay` draws, `create_side_by_side` and `create_6_video_grid` carry the reference's labels (none under
`flow_only`) and the difference legend its numbers.  `draw_text` always draws.  `create_video_grid` (host only) always
labels its cells, since that is its purpose.
"""
import os
from typing import Dict, Optional, Tuple, Union

import numpy as np

from . import text as vtext

try:
    import torch
except ImportError:          # pragma: no cover
    torch = None


def _on_gpu(x):
    return torch is not None and torch.is_tensor(x) and x.is_cuda


def labels_switch(default=False):
    """Whether labels are drawn: VFML_LABELS=1|0 when it is set (any other value is refused), else `default`."""
    value = os.environ.get("VFML_LABELS")
    if value is None or value == "":
        return bool(default)
    if value not in ("0", "1"):
        raise ValueError(f"VFML_LABELS = {value!r}: 1 draws the output video's text labels, 0 leaves them out")
    return value == "1"


def _labels(labels):
    return labels_switch() if labels is None else bool(labels)


_PLANS = {}


def device_plan(key, ops, frame_h, frame_w, device):
    """The TextPlan of a layout on `device`, compiled once per (key, frame size, device); `ops` is a callable -> list."""
    from vfml import hip
    key = (key, int(frame_h), int(frame_w), str(device))
    plan = _PLANS.get(key)
    if plan is None:
        plan = _PLANS[key] = hip.TextPlan(vtext.build_plan(ops(), frame_h, frame_w), device)
    return plan


def draw_text(frame, text: str, position: Union[str, Tuple[int, int]] = 'top-left', font_scale: float = 0.4,
              color: Tuple[int, int, int] = (255, 255, 255), thickness: int = 1):
    """The reference's add_text_overlay, always drawing: `text` at `position` ('top-left', 'top-right', 'bottom-left',
    'bottom-right' at margin 5, or the (x, y) of the baseline's left end), black at thickness + 1 under `color` at
    thickness, anti-aliased; `color` in the frame's channel order.  numpy [H,W,3] uint8 -> a new frame; a contiguous
    device tensor [H,W,3] uint8 -> a new tensor (vfml_text_draw)."""
    if frame is None:
        return frame
    if _on_gpu(frame):
        from vfml import hip
        h, w = frame.shape[:2]
        plan = hip.TextPlan(vtext.build_plan(vtext.overlay_ops(text, position, h, w, font_scale=font_scale, color=color,
                                                               thickness=thickness), h, w), frame.device)
        return hip.text_draw(plan, frame.contiguous().clone(), h, w)
    return vtext.draw_text(frame, text, position, font_scale, color, thickness)


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


def create_difference_overlay(original_flow, decoded_flow, magnitude_threshold=0.9, labels=None):
    """Two flows [H,W,2] -> RGB [H,W,3] uint8: |original - decoded| per pixel in five classes (<= 0.1 green, <= 0.5
    yellow, <= 1 orange, <= 2 red, above magenta; NaN stays black), compared as numpy compares a float32 array with
    a Python float (in float32), and the legend's five squares at the bottom left - with their numbers ("0.100" ...
    ">2.000") when labels are on (`labels`, default the VFML_LABELS switch).
    `magnitude_threshold` is unused, as in the reference.  Device tensors -> vfml_flow_diff_overlay (and vfml_text_draw)."""
    labels = _labels(labels)
    if _on_gpu(original_flow):
        from vfml import hip
        if not _on_gpu(decoded_flow):
            decoded_flow = torch.as_tensor(np.asarray(decoded_flow, dtype=np.float32)).to(original_flow.device)
        out = hip.flow_diff_overlay(original_flow, decoded_flow)
        if labels:
            h, w = out.shape[:2]
            hip.text_draw(device_plan("legend", lambda: vtext.legend_ops(h, w, levels=DIFFERENCE_LEVELS), h, w,
                                      out.device), out, h, w)
        return out
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
    if labels:
        overlay = vtext.draw_ops(overlay, vtext.legend_ops(h, w, levels=DIFFERENCE_LEVELS))
    return overlay


def create_6_video_grid(original_frame, flow_viz, taa_frame, taa_simple_frame, taa_external_frame,
                        difference_overlay, labels=None):
    """The 2 x 3 grid of --taa --flow-input, BGR [3H, 2W, 3] uint8: original | flow picture over TAA | TAA simple over
    TAA with the external flow | difference overlay, with the reference's six labels when labels are on (`labels`,
    default the VFML_LABELS switch).  The TAA histories become uint8 as in the 2x2 grid.  Device tensors are composed
    by vfml_compose_frame (GRID_2X3) and labelled by vfml_text_draw."""
    tiles = [original_frame, flow_viz, taa_frame, taa_simple_frame, taa_external_frame, difference_overlay]
    labels = _labels(labels)
    if _on_gpu(original_frame):
        from vfml import hip
        out = compose_device(*tiles[:4], taa_external_frame=taa_external_frame, difference_overlay=difference_overlay)
        if labels:
            th, tw = original_frame.shape[:2]
            hip.text_draw(device_plan("grid6", lambda: vtext.grid6_ops(th, tw), 3 * th, 2 * tw, out.device), out,
                          3 * th, 2 * tw)
        return out.view(out.shape[0], -1, 3)
    h, w = original_frame.shape[:2]
    for t in tiles:
        if t.shape[:2] != (h, w):
            raise ValueError(f"create_6_video_grid: tile {t.shape[:2]} is not at the frame's size {(h, w)}")
    bgr = [history_to_u8(t)[:, :, ::-1] for t in tiles]
    combined = np.concatenate([np.concatenate(bgr[k:k + 2], axis=1) for k in (0, 2, 4)], axis=0)
    return vtext.draw_ops(combined, vtext.grid6_ops(h, w)) if labels else combined


class VideoComposer:
    """Main class for video composition operations."""

    def add_text_overlay(self, frame, text: str, position: Union[str, Tuple[int, int]] = 'top-left',
                         font_scale: float = 0.4, color: Tuple[int, int, int] = (255, 255, 255), thickness: int = 1,
                         labels=None):
        """`draw_text` when labels are on (`labels`, default the VFML_LABELS switch); otherwise the frame comes back
        unchanged, as it always did before the project had text."""
        if frame is None or not _labels(labels):
            return frame
        return draw_text(frame, text, position, font_scale, color, thickness)

    def create_side_by_side(self, original, flow_viz, flow_only: bool = False, taa_frame=None, taa_simple_frame=None,
                            model_name: str = "VideoFlow", fast_mode: bool = False, flow_format: str = "gamedev",
                            labels=None):
        """Side-by-side, flow-only (stacked) or TAA (2x2 grid; 3 wide with one TAA frame) composition, BGR.  With
        labels on (`labels`, default the VFML_LABELS switch) every tile carries the reference's labels, clipped to the
        tile (none under `flow_only`): "Original", "Optical Flow" and "<model_name> (<FLOW_FORMAT>)", with " (Fast)"
        under `fast_mode`, "TAA + Inv.Flow" / "TAA Simple" and "Alpha: 0.1".  A flow picture of another size than the
        frame is resized to it first."""
        labels = _labels(labels) and not flow_only
        taa = 0 if taa_frame is None else (2 if taa_simple_frame is not None else 1)
        h, w = original.shape[:2]
        if tuple(flow_viz.shape[:2]) != (h, w):
            # the reference's cv2.resize(flow_viz, (w, h)): the project's uint8 resize, host or device
            from video.frame_extractor import resize_frame
            flow_viz = resize_frame(flow_viz, (w, h))
        if _on_gpu(original):
            if taa_frame is not None and taa_simple_frame is None and not flow_only:
                raise ValueError("create_side_by_side: the 3-wide single-TAA layout is host only")
            out = compose_device(original, flow_viz, taa_frame, taa_simple_frame, flow_only)
            if labels:
                from vfml import hip
                fh, fw = (2 * h, 2 * w) if taa else (h, 2 * w)
                plan = device_plan(("sbs", taa, model_name, fast_mode, flow_format),
                                   lambda: vtext.side_by_side_ops(h, w, taa, model_name, fast_mode, flow_format), fh, fw,
                                   out.device)
                hip.text_draw(plan, out, fh, fw)
            return out.view(out.shape[0], -1, 3)
        orig_bgr = np.ascontiguousarray(original[:, :, ::-1])
        flow_bgr = np.ascontiguousarray(flow_viz[:, :, ::-1])
        if flow_only:
            return np.concatenate([orig_bgr, flow_bgr], axis=0)
        if taa == 2:
            taa_bgr = history_to_u8(taa_frame)[:, :, ::-1]
            simple_bgr = history_to_u8(taa_simple_frame)[:, :, ::-1]
            frame = np.concatenate([np.concatenate([orig_bgr, flow_bgr], axis=1),
                                    np.concatenate([taa_bgr, simple_bgr], axis=1)], axis=0)
        elif taa == 1:
            frame = np.concatenate([orig_bgr, flow_bgr, history_to_u8(taa_frame)[:, :, ::-1]], axis=1)
        else:
            frame = np.concatenate([orig_bgr, flow_bgr], axis=1)
        if labels:
            # every label carries its tile's clip, so drawing on the joined frame equals drawing on the tiles first
            frame = vtext.draw_ops(frame, vtext.side_by_side_ops(h, w, taa, model_name, fast_mode, flow_format))
        return frame

    def create_video_grid(self, frames_dict: Dict[str, np.ndarray], grid_shape: Tuple[int, int],
                          target_aspect: float = 16 / 9):
        """Labelled frames in a rows x cols grid on a black canvas of the target aspect ratio (reference
        video_composer.py:124-224), BGR uint8, on the host.  The canvas is cols * w wide and int(width / target_aspect)
        high, the grid centred on it; a cell that does not fit is left out, as in the reference.  Every frame ([H,W,3],
        RGB; a float TAA history is clipped to uint8) is reversed to BGR, its label - the dict key, lines split at
        newlines - drawn at scale 0.7, thickness 2 over an outline of thickness 4 at (8, 25 + 30 line), on the backdrop
        (0, 0)..(max line width + 15, 30 lines + 10) dimmed to (3 * dst + 5) // 10.  Labels are always drawn."""
        if not frames_dict:
            return None
        rows, cols = grid_shape
        h, w = next(iter(frames_dict.values())).shape[:2]
        canvas_w = cols * w
        canvas_h = int(canvas_w / target_aspect)
        canvas = np.zeros((canvas_h, canvas_w, 3), dtype=np.uint8)
        y_offset = (canvas_h - rows * h) // 2
        x_offset = (canvas_w - cols * w) // 2
        for i, (label, frame) in enumerate(list(frames_dict.items())[:rows * cols]):
            frame = history_to_u8(np.asarray(frame.cpu() if _on_gpu(frame) else frame))
            if frame.shape != (h, w, 3):
                raise ValueError(f"create_video_grid: frame {label!r} is {frame.shape}, [H,W,3] of {(h, w)} expected")
            cell = vtext.draw_ops(frame[:, :, ::-1], vtext.video_grid_label_ops(label, h, w))
            y, x = y_offset + (i // cols) * h, x_offset + (i % cols) * w
            if y >= 0 and x >= 0 and y + h <= canvas_h and x + w <= canvas_w:
                canvas[y:y + h, x:x + w] = cell
        return canvas


def add_text_overlay(frame, text: str, position: Union[str, Tuple[int, int]] = 'top-left', font_scale: float = 0.4,
                     color: Tuple[int, int, int] = (255, 255, 255), thickness: int = 1, labels=None):
    """Draws when labels are on (VFML_LABELS=1 or labels=True); otherwise returns the frame unchanged."""
    return VideoComposer().add_text_overlay(frame, text, position, font_scale, color, thickness, labels)


def create_side_by_side(original, flow_viz, flow_only: bool = False, taa_frame: Optional[np.ndarray] = None,
                        taa_simple_frame: Optional[np.ndarray] = None, model_name: str = "VideoFlow",
                        fast_mode: bool = False, flow_format: str = "gamedev", labels=None):
    return VideoComposer().create_side_by_side(original, flow_viz, flow_only, taa_frame, taa_simple_frame, model_name,
                                               fast_mode, flow_format, labels)


def create_video_grid(frames_dict: Dict[str, np.ndarray], grid_shape: Tuple[int, int], target_aspect: float = 16 / 9):
    """Create video grid layout (host)."""
    return VideoComposer().create_video_grid(frames_dict, grid_shape, target_aspect)
