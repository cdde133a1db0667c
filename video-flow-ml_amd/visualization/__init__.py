"""visualization — output-frame composition (mirror of the reference's visualization/ package)."""
from .video_composer import VideoComposer, add_text_overlay, create_side_by_side

__all__ = ["VideoComposer", "add_text_overlay", "create_side_by_side"]
