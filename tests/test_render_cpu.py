"""Render stage on the host: the colour-wheel encoders, the composer and the AVI writer against the reference's own
process_video (tests/golden/render.npz, make_render_fixtures.py), and flow_processor's --taa workflow end to end."""
import os
import struct

import numpy as np
import pytest

from encoding import HSVFlowEncoder, TorchvisionFlowEncoder
from encoding.flow_encoders import hsv2rgb_u8, hsv_bytes
from storage.avi_writer import AviWriter
from visualization.video_composer import create_side_by_side

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "render.npz"))
SPECIALS = ("flow", "small", "zero", "huge")


def hue_near_boundary(flow):
    """Pixels whose float32 hue lies within a few ulp of an integer (where truncation may go either way)."""
    f = np.nan_to_num(np.asarray(flow, np.float32), nan=0.0, posinf=1.0, neginf=-1.0)
    ang = np.arctan2(f[:, :, 1], f[:, :, 0])
    hue = (ang + np.float32(np.pi)) / np.float32(2 * np.pi) * np.float32(180)
    return np.abs(hue - np.round(hue)) <= 8 * np.spacing(np.maximum(np.abs(hue), np.float32(1)))


def check_hue(ours, ref, flow):
    """Hue bytes equal, except on at most 1e-3 of the pixels, which differ by exactly 1 next to a truncation boundary."""
    diff = ours.astype(int) - ref.astype(int)
    bad = diff != 0
    assert bad.mean() <= 1e-3, bad.mean()
    assert np.all(np.abs(diff[bad]) == 1)
    assert np.all(hue_near_boundary(flow)[bad])
    return bad


@pytest.mark.parametrize("key", SPECIALS)
def test_hsv_encoder_matches_reference(key):
    f = GOLD[f"enc_in_{key}"]
    ref_hsv, ref_rgb = GOLD[f"enc_hsvbytes_{key}"], GOLD[f"enc_hsv_{key}"]
    got = hsv_bytes(f)
    np.testing.assert_array_equal(got[:, :, 1:], ref_hsv[:, :, 1:])
    bad = check_hue(got[:, :, 0], ref_hsv[:, :, 0], f)
    rgb = HSVFlowEncoder().encode(f, f.shape[1], f.shape[0])
    np.testing.assert_array_equal(rgb[~bad], ref_rgb[~bad])
    np.testing.assert_array_equal(hsv2rgb_u8(ref_hsv), ref_rgb)     # our HSV2RGB on the reference's own bytes


@pytest.mark.parametrize("key", SPECIALS)
def test_torchvision_encoder_matches_reference(key):
    f = GOLD[f"enc_in_{key}"]
    got = TorchvisionFlowEncoder().encode(f, f.shape[1], f.shape[0])
    np.testing.assert_array_equal(got, GOLD[f"enc_tv_{key}"])


def test_torchvision_wrapper_wraps_the_wheel_bytes():
    from encoding.flow_encoders import flow_to_wheel_u8
    f = GOLD["enc_in_flow"]
    x = flow_to_wheel_u8(f)
    np.testing.assert_array_equal(TorchvisionFlowEncoder().encode(f, 1, 1), ((256 - x.astype(int)) % 256).astype(np.uint8))


def test_hsv2rgb_sector_table():
    hsv = np.array([[[0, 255, 255], [30, 255, 255], [60, 255, 255], [90, 255, 255], [120, 255, 255], [150, 255, 255],
                     [180, 255, 255], [45, 0, 255], [15, 128, 255]]], np.uint8)
    rgb = hsv2rgb_u8(hsv)[0]
    assert rgb[:7].tolist() == [[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255],
                                [255, 0, 0]]
    assert rgb[7].tolist() == [255, 255, 255]
    assert rgb[8].tolist() == [255, 191, 127]      # p = 127.0 -> 127, t = 190.75 -> 191 (saturate_cast rounding)


def _ref_loop(fmt, flow_only=False, taa=False):
    """The reference's loop (process_video :958-1130) on the host paths, for the composer check."""
    from effects.taa_processor import TAAProcessor
    import flow_processor as fp
    frames, fields = GOLD["frames"], GOLD["fields"]
    h, w = frames.shape[1:3]
    enc = fp.render_encoder(fmt, 32.0)
    t1, t2 = TAAProcessor(alpha=0.1), TAAProcessor(alpha=0.1)
    prev, out = None, []
    for i in range(len(frames)):
        viz = enc.encode(fields[i], w, h)
        a = b = None
        if taa:
            a = t1.apply_taa(frames[i], flow_pixels=prev, alpha=0.1, use_flow=True, sequence_id='flow_taa')
            b = t2.apply_taa(frames[i], flow_pixels=None, alpha=0.1, use_flow=False, sequence_id='simple_taa')
        prev = fields[i]
        out.append(create_side_by_side(frames[i], viz, flow_only=flow_only, taa_frame=a, taa_simple_frame=b))
    return np.stack(out)


def _hsv_tile_ok(ours, ref, fields, th, tw):
    """Frames equal, except the flow tile's pixels whose hue byte may differ by one (check_hue)."""
    for i in range(len(fields)):
        d = np.any(ours[i] != ref[i], axis=2)
        flow_tile = np.zeros_like(d)
        flow_tile[:th, tw:2 * tw] = True
        assert not np.any(d & ~flow_tile), i
        bad = d[:th, tw:2 * tw]
        assert bad.mean() <= 1e-3 and np.all(hue_near_boundary(fields[i])[bad])


@pytest.mark.parametrize("name,fmt,flow_only,taa", [("sbs_gamedev", "gamedev", False, False),
                                                     ("flowonly_torchvision", "torchvision", True, False),
                                                     ("taa_hsv", "hsv", False, True)])
def test_host_composer_matches_reference(name, fmt, flow_only, taa):
    ours, ref = _ref_loop(fmt, flow_only, taa), GOLD[f"out_{name}"]
    assert ours.shape == ref.shape
    if fmt == "hsv":
        _hsv_tile_ok(ours, ref, GOLD["fields"], *GOLD["frames"].shape[1:3])
    else:
        np.testing.assert_array_equal(ours, ref)


# ---- a small RIFF / AVI reader (the test's own) -------------------------------------------------------------------------
def _chunks(buf, start, end):
    p = start
    while p + 8 <= end:
        fcc, size = buf[p:p + 4], struct.unpack_from('<I', buf, p + 4)[0]
        yield fcc, p, size
        p += 8 + size + (size & 1)


def parse_avi(path):
    buf = open(path, 'rb').read()
    info = {"frames": [], "riff": [], "ix00": 0}
    for fcc, p, size in _chunks(buf, 0, len(buf)):
        assert fcc == b'RIFF'
        form = buf[p + 8:p + 12]
        info["riff"].append(form)
        _walk(buf, p + 12, p + 8 + size, info)
    return info


def _walk(buf, start, end, info):
    for fcc, p, size in _chunks(buf, start, end):
        body = p + 8
        if fcc == b'LIST':
            _walk(buf, body + 4, body + size, info)
        elif fcc == b'avih':
            usec, _, _, _, total, _, streams, _, w, h = struct.unpack_from('<10I', buf, body)
            info.update(avih_usec=usec, avih_frames=total, width=w, height=h)
        elif fcc == b'strh':
            scale, rate, _, length = struct.unpack_from('<4I', buf, body + 20)
            info.update(fps=rate / scale, strh_frames=length, handler=buf[body + 4:body + 8])
        elif fcc == b'strf':
            info.update(bi=struct.unpack_from('<IiiHH4sI', buf, body))
        elif fcc == b'dmlh':
            info["dmlh_frames"] = struct.unpack_from('<I', buf, body)[0]
        elif fcc == b'indx':
            n = struct.unpack_from('<I', buf, body + 4)[0]
            info["indx"] = [struct.unpack_from('<QII', buf, body + 24 + 16 * k) for k in range(n)]
        elif fcc == b'ix00':
            info["ix00"] += struct.unpack_from('<I', buf, body + 4)[0]
        elif fcc == b'idx1':
            info["idx1"] = size // 16
        elif fcc in (b'00db', b'00dc'):
            info["frames"].append(buf[body:body + size])


def dib_frame(data, w, h):
    stride = (3 * w + 3) // 4 * 4
    rows = np.frombuffer(data, np.uint8).reshape(h, stride)
    assert not rows[:, 3 * w:].any()
    return rows[::-1, :3 * w].reshape(h, w, 3)


def test_avi_writer_round_trip_over_opendml_segments(tmp_path):
    rng = np.random.default_rng(3)
    w, h, n = 37, 21, 13                                     # odd width: every DIB row is padded
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    path = str(tmp_path / "raw.avi")
    wr = AviWriter(path, 0, 24.0, (w, h), segment_bytes=12000)
    for f in frames:
        wr.write(f)
    wr.release()
    info = parse_avi(path)
    assert info["riff"][0] == b'AVI ' and len(info["riff"]) >= 3 and all(r == b'AVIX' for r in info["riff"][1:])
    assert len(info["frames"]) == n and info["dmlh_frames"] == n and info["strh_frames"] == n
    assert info["fps"] == 24.0 and (info["width"], info["height"]) == (w, h)
    assert info["idx1"] == info["avih_frames"] < n
    assert len(info["indx"]) == len(info["riff"]) and sum(e[2] for e in info["indx"]) == n and info["ix00"] == n
    assert info["bi"][:6] == (40, w, h, 1, 24, b'\0\0\0\0')
    buf = open(path, 'rb').read()
    for off, size, dur in info["indx"]:                      # the super index points at the ix00 chunks
        assert buf[off:off + 4] == b'ix00'
    for k, data in enumerate(info["frames"]):
        np.testing.assert_array_equal(dib_frame(data, w, h), frames[k])


def test_avi_writer_mjpg(tmp_path):
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    yy, xx = np.mgrid[0:48, 0:64]
    frames = [np.stack([xx * 3 + 9 * i, yy * 4, (xx + yy) * 2], 2).astype(np.uint8)
              for i in range(5)]
    path = str(tmp_path / "mjpg.avi")
    wr = AviWriter(path, 'MJPG', 30.0, (64, 48), workers=3)
    for f in frames:
        wr.write(f)
    wr.release()
    info = parse_avi(path)
    assert info["handler"] == b'MJPG' and info["fps"] == 30.0 and len(info["frames"]) == 5
    for f, data in zip(frames, info["frames"]):
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).astype(float)
        mse = np.mean((rgb - f[:, :, ::-1].astype(float)) ** 2)
        assert 10 * np.log10(255 ** 2 / max(mse, 1e-9)) > 35


def run_taa_cli(tmp_path, device):
    """flow_processor.main in the visualiser's TAA workflow on a complete fixture cache -> (avi path, stdout)."""
    import contextlib
    import io
    import flow_processor as fp
    from storage import FlowCacheManager
    frames, fields = GOLD["frames"], GOLD["fields"]
    clip = str(tmp_path / "clip.npy")
    np.save(clip, frames)
    cache = tmp_path / "clip_corrected"
    cache.mkdir()
    for i, f in enumerate(fields):
        FlowCacheManager().save_flow_to_cache(f, str(cache), i, 'npz')
    out = tmp_path / f"out_{device}"
    out.mkdir()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = fp.main(["--input", clip, "--output", str(out), "--device", device, "--taa", "--skip-lods", "--tile",
                      "--flow-format", "hsv", "--uncompressed", "--use-flow-cache", str(cache)])
    assert rc == 0, buf.getvalue()
    avis = sorted(os.listdir(out))
    assert avis == ["clip_tile_taa_30fps_uncompressed_I420.avi"], avis
    return str(out / avis[0]), buf.getvalue()


def read_frames(path):
    info = parse_avi(path)
    w, h = info["width"], info["height"]
    return np.stack([dib_frame(d, w, h) for d in info["frames"]]), info


def test_cli_taa_workflow_writes_the_reference_video(tmp_path):
    path, log = run_taa_cli(tmp_path, "cpu")
    assert "Auto-generated output filename: clip_tile_taa_30fps_uncompressed_I420.avi" in log
    assert "[Encoder] Using HSV color space encoder" in log
    got, info = read_frames(path)
    ref = GOLD["out_taa_hsv"]
    assert got.shape == ref.shape and info["dmlh_frames"] == len(ref) and info["fps"] == 30.0
    _hsv_tile_ok(got, ref, GOLD["fields"], *GOLD["frames"].shape[1:3])


def test_cli_interactive_still_stops_at_the_cache(tmp_path):
    import contextlib
    import io
    import flow_processor as fp
    np.save(tmp_path / "clip.npy", GOLD["frames"])
    from storage import FlowCacheManager
    cache = tmp_path / "c"
    cache.mkdir()
    for i, f in enumerate(GOLD["fields"]):
        FlowCacheManager().save_flow_to_cache(f, str(cache), i, 'npz')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = fp.main(["--input", str(tmp_path / "clip.npy"), "--output", str(tmp_path), "--device", "cpu",
                      "--interactive", "--use-flow-cache", str(cache)])
    assert rc == 0 and buf.getvalue().startswith(f"Flow cache complete (npz), nothing to compute: {cache}")
    assert not any(n.endswith(".avi") for n in os.listdir(tmp_path))
