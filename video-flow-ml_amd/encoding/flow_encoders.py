"""Flow fields -> 8-bit images: the gamedev and motion-vector codes of the reference.

API mirror of reference encoding/flow_encoders.py for the three formats that are pure arithmetic on the
field: `gamedev` (:70-117), `motion-vectors-rg8` (:120-190) and `motion-vectors-rgb8` in its 'rgb+' variant
(the reference's module-level `method`, :10, :242-293, decode :336-343).  Outputs are bytes, so they are
reproduced bit for bit (tests/golden/flow_encoders.npz, cut from the reference).  A field that is still a
device tensor is encoded there by `vfml_flow_encode` (16.6 MB read, 6.2 MB written per 1080p field) and
returned as a device uint8 tensor; numpy input takes the same float32 steps on the host.
`hsv` (:30-67) and `torchvision` (:367-427) are colour wheels normalised by the frame's maximum magnitude; OpenCV's
HSV2RGB and torchvision's wheel are defined by this project, so neither library is needed.  They
are used by flow_processor's render stage and are not registered in FlowEncoderFactory.
"""
from abc import ABC, abstractmethod
from typing import Optional

import numpy as np

try:
    import torch
except ImportError:          # pragma: no cover
    torch = None


def _on_gpu(flow):
    return torch is not None and torch.is_tensor(flow) and flow.is_cuda


def _to_u8(img):
    """rgb in [0,1] (NaN / inf allowed) -> uint8, as the reference finishes every encoder."""
    x = img * 255
    return np.nan_to_num(x, nan=0.0, posinf=255.0, neginf=0.0).astype(np.uint8)


def _clamp_to_unit(v, clamp_range):
    """clip to +-clamp_range, map to [0,1], clip again (the shared tail of gamedev and rg8)."""
    e = (np.clip(v, -clamp_range, clamp_range) + clamp_range) / (2 * clamp_range)
    return np.clip(e, 0, 1)


def _rg_image(e):
    rgb = np.zeros(e.shape[:2] + (3,), dtype=np.float32)
    rgb[:, :, :2] = e
    return _to_u8(rgb)


class FlowEncoder(ABC):
    @abstractmethod
    def encode(self, flow, width: int, height: int):
        """flow [H,W,2] float32 (numpy, or a device tensor) -> RGB [H,W,3] uint8 (same kind)."""


class GamedevFlowEncoder(FlowEncoder):
    """R, G = flow / (width, height) * scale_factor, clamped to +-clamp_range and mapped to [0, 255]; B = 0."""

    def __init__(self, scale_factor: float = 200.0, clamp_range: float = 20.0):
        self.scale_factor = scale_factor
        self.clamp_range = clamp_range

    def encode(self, flow, width: int, height: int):
        if _on_gpu(flow):
            from vfml import hip
            return hip.flow_encode(flow, hip.ENCODE_GAMEDEV, self.clamp_range, width, height, self.scale_factor)
        n = np.array(flow, dtype=np.float32, copy=True)
        n[:, :, 0] /= width
        n[:, :, 1] /= height
        n *= self.scale_factor
        return _rg_image(_clamp_to_unit(n, self.clamp_range))


class MotionVectorsRG8FlowEncoder(FlowEncoder):
    """R, G = flow clamped to +-clamp_range pixels, UNORM 8; B = 0."""

    def __init__(self, clamp_range: float = 64.0):
        self.clamp_range = clamp_range

    def encode(self, flow, width: int, height: int):
        if _on_gpu(flow):
            from vfml import hip
            return hip.flow_encode(flow, hip.ENCODE_RG8, self.clamp_range)
        return _rg_image(_clamp_to_unit(np.asarray(flow, dtype=np.float32), self.clamp_range))

    def decode(self, encoded_flow: np.ndarray) -> np.ndarray:
        rg = encoded_flow.astype(np.float32)[:, :, :2] / 255.0
        return (rg * 2 * self.clamp_range) - self.clamp_range


class MotionVectorsRGB8FlowEncoder(FlowEncoder):
    """'rgb+' code: d = flow / clamp_range shortened to the unit disc; R, G = (d + 1) / 2; B = sqrt(1 - |d|^2)."""

    def __init__(self, clamp_range: float = 32.0):
        self.clamp_range = clamp_range

    def encode(self, flow, width: int, height: int):
        if _on_gpu(flow):
            from vfml import hip
            return hip.flow_encode(flow, hip.ENCODE_RGB8, self.clamp_range)
        f = np.asarray(flow, dtype=np.float32)
        with np.errstate(all="ignore"):
            d = f / self.clamp_range                       # (a fresh array: the steps below write into it)
            dx, dy = d[:, :, 0], d[:, :, 1]
            length = np.sqrt(dx ** 2 + dy ** 2)
            far = length > 1
            dx[far] = dx[far] / length[far]
            dy[far] = dy[far] / length[far]
            rgb = np.zeros(f.shape[:2] + (3,), dtype=np.float32)
            rgb[:, :, 2] = np.sqrt(1 - dx ** 2 - dy ** 2)
            rgb[:, :, 0] = (np.clip(dx, -1, 1) + 1) / 2
            rgb[:, :, 1] = (np.clip(dy, -1, 1) + 1) / 2
            return _to_u8(rgb)

    def decode(self, encoded_flow: np.ndarray) -> np.ndarray:
        n = encoded_flow.astype(np.float32) / 255.0
        with np.errstate(all="ignore"):
            dx, dy = n[:, :, 0] * 2 - 1, n[:, :, 1] * 2 - 1
            magnitude = 1 / np.sqrt(dx ** 2 + dy ** 2 + n[:, :, 2] ** 2) * self.clamp_range
            out = np.zeros(encoded_flow.shape[:2] + (2,), dtype=np.float32)
            out[:, :, 0] = dx * magnitude
            out[:, :, 1] = dy * magnitude
        return out


def _atan2_32(y, x):
    """float32 atan2 as the float64 one rounded to float32 (the device kernel does the same: host and device agree
    on every machine, where numpy's float32 arctan2 may be a vector routine that is not correctly rounded)."""
    return np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32)


def _u8(x):
    """float -> uint8 as numpy's astype does on x86-64 (int32 truncation, low byte; NaN / inf / out of int32 -> 0),
    spelled out so that it holds on every host."""
    x = np.asarray(x)
    ok = (x > -2147483648.0) & (x < 2147483648.0)
    return np.where(ok, np.where(ok, x, 0).astype(np.int64), 0).astype(np.uint8)


# OpenCV's HSV2RGB sector table: (b, g, r) = tab[sector_data[sector]]
_HSV_SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]], dtype=np.int64)


def hsv2rgb_u8(hsv):
    """8-bit HSV (H in 0..180) -> RGB uint8: the cv2.cvtColor(COLOR_HSV2RGB) of this project.
    h = H * float32(6/180) wrapped into [0, 6), s = S / 255, v = V / 255 (float32 quotients), OpenCV's sector table,
    saturate_cast<uchar>(x * 255) rounding half to even."""
    f32 = np.float32
    hsv = np.asarray(hsv, dtype=np.uint8)
    h = hsv[..., 0].astype(f32) * f32(6.0 / 180.0)
    s = hsv[..., 1].astype(f32) / f32(255.0)
    v = hsv[..., 2].astype(f32) / f32(255.0)
    while np.any(h >= 6):
        h = np.where(h >= 6, h - f32(6), h)
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, f32(0), h)
    one = f32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    bgr = np.take_along_axis(tab, _HSV_SECTORS[sector], axis=-1)
    bgr = np.where((hsv[..., 1] == 0)[..., None], v[..., None], bgr)
    rgb = np.rint(bgr[..., ::-1] * f32(255.0))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def hsv_bytes(flow):
    """flow [H,W,2] -> the H, S, V bytes the reference's HSVFlowEncoder hands to cvtColor (:30-63), step by step in
    float32 as numpy >= 2 promotes it."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        f = np.nan_to_num(np.asarray(flow, dtype=f32), nan=0.0, posinf=1.0, neginf=-1.0)
        fx, fy = f[:, :, 0], f[:, :, 1]
        mag = np.sqrt(fx * fx + fy * fy)
        hue = (_atan2_32(fy, fx) + f32(np.pi)) / f32(2 * np.pi) * f32(180)
        hue = _u8(np.clip(hue, 0, 180))
        mx = np.max(mag)
        sat = _u8(mag / mx * f32(255)) if mx > 0 else np.zeros(mag.shape, np.uint8)
    return np.stack([hue, sat, np.full(mag.shape, 255, np.uint8)], axis=2)


def _wheel():
    """The 55-entry Middlebury colour wheel of torchvision.utils.flow_to_image (RY 15, YG 6, GC 4, CB 11, BM 13, MR 6)."""
    rows = []
    for k in range(55):
        if k < 15:
            rows.append((255, 255 * k // 15, 0))
        elif k < 21:
            rows.append((255 - 255 * (k - 15) // 6, 255, 0))
        elif k < 25:
            rows.append((0, 255, 255 * (k - 21) // 4))
        elif k < 36:
            rows.append((0, 255 - 255 * (k - 25) // 11, 255))
        elif k < 49:
            rows.append((255 * (k - 36) // 13, 0, 255))
        else:
            rows.append((255, 0, 255 - 255 * (k - 49) // 6))
    return np.array(rows, dtype=np.float32)


WHEEL = _wheel()


def flow_to_wheel_u8(flow):
    """torchvision.utils.flow_to_image as this project defines it in float32: flow [H,W,2] ->
    uint8 [H,W,3], floor(255 * col), before the reference wrapper's `* 255`."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        f = np.asarray(flow, dtype=f32)
        u, v = f[:, :, 0], f[:, :, 1]
        max_norm = np.max(np.sqrt(u * u + v * v))
        denom = f32(max_norm + np.finfo(f32).eps)
        nu, nv = u / denom, v / denom
        rad = np.sqrt(nu * nu + nv * nv)
        a = _atan2_32(-nv, -nu) / f32(np.pi)
        fk = (a + f32(1)) / f32(2) * f32(54)
        k0 = np.clip(np.where(np.isnan(fk), 0, np.floor(np.nan_to_num(fk))), 0, 54).astype(np.int64)
        k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
        fr = fk - k0.astype(f32)
        out = np.empty(f.shape[:2] + (3,), np.uint8)
        for c in range(3):
            col0 = WHEEL[k0, c] / f32(255)
            col1 = WHEEL[k1, c] / f32(255)
            col = (f32(1) - fr) * col0 + fr * col1
            col = f32(1) - rad * (f32(1) - col)
            out[:, :, c] = _u8(np.floor(f32(255) * col))
    return out


class HSVFlowEncoder(FlowEncoder):
    """Hue = direction (0..180, OpenCV's 8-bit hue), saturation = magnitude / frame maximum, value = 255; then this
    project's HSV2RGB (`hsv2rgb_u8`).  A device tensor is encoded there by `vfml_flow_colorize` (the maximum is reduced
    on the device)."""

    def encode(self, flow, width: int, height: int):
        if _on_gpu(flow):
            from vfml import hip
            return hip.flow_colorize(flow, hip.COLORIZE_HSV)
        return hsv2rgb_u8(hsv_bytes(flow))


class TorchvisionFlowEncoder(FlowEncoder):
    """torchvision's colour wheel (`flow_to_wheel_u8`), then the reference wrapper's uint8 `* 255` (:421-425), which
    wraps: the reference writes (256 - x) mod 256, not the wheel colour x, and so does this encoder.  torchvision is not
    needed; the wheel is defined here.  Device tensors go to `vfml_flow_colorize`."""

    def __init__(self, fallback_encoder: Optional[FlowEncoder] = None):
        self.fallback_encoder = fallback_encoder     # API mirror; the wheel is always available here

    def encode(self, flow, width: int, height: int):
        if _on_gpu(flow):
            from vfml import hip
            return hip.flow_colorize(flow, hip.COLORIZE_WHEEL)
        return flow_to_wheel_u8(flow) * np.uint8(255)


class FlowEncoderFactory:
    _encoders = {'gamedev': GamedevFlowEncoder, 'motion-vectors-rg8': MotionVectorsRG8FlowEncoder,
                 'motion-vectors-rgb8': MotionVectorsRGB8FlowEncoder}
    _not_built = ('hsv', 'torchvision')

    @classmethod
    def create_encoder(cls, format_name: str, **kwargs) -> FlowEncoder:
        format_name = format_name.lower()
        if format_name in cls._not_built:
            raise ValueError(f"Format '{format_name}' needs OpenCV / torchvision and is not part of this build. "
                             f"Available formats: {', '.join(cls._encoders)}")
        if format_name not in cls._encoders:
            raise ValueError(f"Unsupported format '{format_name}'. Available formats: {', '.join(cls._encoders)}")
        return cls._encoders[format_name](**kwargs)

    @classmethod
    def get_available_formats(cls):
        return list(cls._encoders)

    @classmethod
    def register_encoder(cls, format_name: str, encoder_class: type):
        if not issubclass(encoder_class, FlowEncoder):
            raise ValueError("Encoder class must inherit from FlowEncoder")
        cls._encoders[format_name.lower()] = encoder_class


def encode_flow(flow, width: int, height: int, format_name: str = 'gamedev'):
    return FlowEncoderFactory.create_encoder(format_name).encode(flow, width, height)


def encode_motion_vectors(flow, clamp_range: float = 64.0, format_variant: str = 'rgb8'):
    enc = (MotionVectorsRG8FlowEncoder if format_variant.lower() == 'rg8' else MotionVectorsRGB8FlowEncoder)(clamp_range=clamp_range)
    h, w = flow.shape[:2]
    return enc.encode(flow, w, h)


def decode_motion_vectors(encoded_flow: np.ndarray, clamp_range: float = 64.0, format_variant: str = 'rgb8') -> np.ndarray:
    enc = (MotionVectorsRG8FlowEncoder if format_variant.lower() == 'rg8' else MotionVectorsRGB8FlowEncoder)(clamp_range=clamp_range)
    return enc.decode(encoded_flow)
