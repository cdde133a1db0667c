"""visualization — output-frame composition (mirror of the reference's visualization/ package)."""
from .video_composer import VideoComposer, add_text_overlay, create_side_by_side, create_video_grid, draw_text

__all__ = ["VideoComposer", "add_text_overlay", "create_side_by_side", "create_video_grid", "draw_text"]
