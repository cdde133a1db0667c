"""Text labels on the MI355X: vfml_text_draw byte for byte against tests/text_oracle.py on the draw lists of
tests/test_text_cpu.py, in every frame layout the render stage uses; the composer and flow_processor's output video with
labels on against the host path; and the MJPG path, where a label may only change the MCUs it touches."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import text_oracle as oracle
from test_render_cpu import parse_avi, read_frames
from test_text_cpu import CASES, expected, noise
from visualization import text as vtext
from visualization import video_composer as vc

pytestmark = pytest.mark.gpu


def _draw(gpu, src, ops, bottom_up=False, pad=0):
    """The kernel on a picture laid out as the render stage lays frames out -> (picture top-down, padding bytes)."""
    from vfml import hip
    h, w = src.shape[:2]
    stride = 3 * w + pad
    buf = np.full((h, stride), 0xA5, np.uint8)
    buf[:, :3 * w] = (src[::-1] if bottom_up else src).reshape(h, 3 * w)
    dev = torch.from_numpy(buf).to(gpu)
    plan = hip.TextPlan(vtext.build_plan(ops, h, w), gpu)
    if plan.boxes:
        assert plan.host[2:4].view(np.uint64)[0] == plan.dev.data_ptr()
    hip.text_draw(plan, dev, h, w, row_stride=stride, bottom_up=bottom_up)
    out = dev.cpu().numpy()
    pic = out[:, :3 * w].reshape(h, w, 3)
    return (pic[::-1] if bottom_up else pic), out[:, 3 * w:]


@pytest.mark.parametrize("name", list(CASES))
def test_text_draw_equals_oracle(gpu, name):
    _, h, w, ops = CASES[name]
    src = noise(h, w)
    got, _ = _draw(gpu, src, ops)                                          # top-down, stride 3 w
    np.testing.assert_array_equal(got, expected(name))
    got, padding = _draw(gpu, src, ops, bottom_up=True, pad=(-3 * w) % 4 + 4)     # a padded DIB, bottom-up
    np.testing.assert_array_equal(got, expected(name))
    assert (padding == 0xA5).all()


def test_odd_sizes_leave_padding_untouched(gpu):
    h, w = 47, 131
    src = noise(h, w)
    ops = oracle.side_by_side_ops(23, 65, 2) + oracle.overlay_ops("Edge gjpqy", (100, 46), h, w, font_scale=0.7,
                                                                  thickness=2) + oracle.legend_ops(h, w)
    want = oracle.draw_ops(src, ops)
    for bottom_up, pad in ((False, 0), (False, 3), (True, 3), (True, 7)):
        got, padding = _draw(gpu, src, ops, bottom_up, pad)
        np.testing.assert_array_equal(got, want, err_msg=f"{bottom_up} {pad}")
        assert (padding == 0xA5).all()


def test_torch_op_and_draw_text_on_device_tensors(gpu):
    import vfml.torch_ops  # noqa: F401
    h, w = 48, 128
    src = noise(h, w)
    ops = oracle.overlay_ops("TAA + Inv.Flow", 'bottom-right', h, w, font_scale=0.7, colour=(10, 200, 30), thickness=2)
    want = oracle.draw_ops(src, ops)
    dev = torch.from_numpy(src).to(gpu)
    out = torch.ops.vfml.text_draw(dev, torch.from_numpy(vtext.build_plan(ops, h, w)))
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    np.testing.assert_array_equal(dev.cpu().numpy(), src)                  # the op returns a new frame
    got = vc.draw_text(dev, "TAA + Inv.Flow", 'bottom-right', 0.7, (10, 200, 30), 2)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert vc.add_text_overlay(dev, "x", labels=False) is dev              # switch off: the frame itself, as before


def _tiles(h, w):
    rng = np.random.default_rng(h + w)
    u8 = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    hist = [rng.uniform(-40, 300, (h, w, 3)).astype(np.float32) for _ in range(3)]
    flows = [rng.normal(0, 1, (h, w, 2)).astype(np.float32) for _ in range(2)]
    return u8, hist, flows


def test_composer_with_labels_equals_host(gpu):
    """compose_device followed by text_draw (what the device composer functions do with labels on) against the host
    functions, for SIDE_BY_SIDE, GRID_2X2 and GRID_2X3 at tile 48 x 128."""
    h, w = 48, 128
    (a, b), (t0, t1, t2), (f0, f1) = _tiles(h, w)
    d = lambda x: torch.from_numpy(x).to(gpu)                              # noqa: E731
    for kw in ({}, {"taa_frame": t0, "taa_simple_frame": t1}):
        host = vc.create_side_by_side(a, b, fast_mode=True, flow_format="motion-vectors-rg8", labels=True, **kw)
        dev = vc.create_side_by_side(d(a), d(b), fast_mode=True, flow_format="motion-vectors-rg8", labels=True,
                                     **{k: d(v) for k, v in kw.items()})
        np.testing.assert_array_equal(dev.cpu().numpy(), host)
        assert (host != vc.create_side_by_side(a, b, labels=False, **kw)).any()
    legend_host = vc.create_difference_overlay(f0, f1, labels=True)
    legend_dev = vc.create_difference_overlay(d(f0), d(f1), labels=True)
    np.testing.assert_array_equal(legend_dev.cpu().numpy(), legend_host)
    assert (legend_host != vc.create_difference_overlay(f0, f1, labels=False)).any()
    host = vc.create_6_video_grid(a, b, t0, t1, t2, legend_host, labels=True)
    dev = vc.create_6_video_grid(d(a), d(b), d(t0), d(t1), d(t2), legend_dev, labels=True)
    np.testing.assert_array_equal(dev.cpu().numpy(), host)
    # the render loop's form: one plan for the whole 2x3 frame - legend numbers on the difference tile, then the grid's
    # labels - drawn on an RGB top-down frame and on a BGR bottom-up padded one
    import flow_processor as fp
    from storage.avi_writer import dib_stride
    from vfml import hip
    ops = fp._label_ops(w, h, True, False, True, "VideoFlow", False, "motion-vectors-rg8")
    plan = hip.TextPlan(vtext.build_plan(ops, 3 * h, 2 * w), gpu)
    plain = vc.create_difference_overlay(d(f0), d(f1), labels=False)
    for bgr, bottom_up in ((False, False), (True, True)):
        stride = dib_stride(2 * w) + 4 if bottom_up else 6 * w
        out = vc.compose_device(d(a), d(b), d(t0), d(t1), bgr=bgr, bottom_up=bottom_up, row_stride=stride,
                                taa_external_frame=d(t2), difference_overlay=plain)
        hip.text_draw(plan, out, 3 * h, 2 * w, row_stride=stride, bottom_up=bottom_up)
        img = host if bgr else host[:, :, ::-1]
        got = out.cpu().numpy()[:, :6 * w].reshape(3 * h, 2 * w, 3)
        np.testing.assert_array_equal(got[::-1] if bottom_up else got, img, err_msg=f"{bgr} {bottom_up}")


# ---- flow_processor's output video ---------------------------------------------------------------------------------------
W, H, N = 128, 48, 3


def _run(tmp_path, name, device, labels, extra):
    """flow_processor.main on synthetic:128x48x3 with a complete cache of smooth fields -> the AVI's path."""
    import flow_processor as fp
    from storage import FlowCacheManager
    cache = tmp_path / "cache_corrected"
    if not cache.exists():
        cache.mkdir()
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        for i in range(N):
            f = np.stack([3 * np.sin(xx / 17 + i / 3), 2 * np.cos(yy / 11 - i / 2)], axis=2).astype(np.float32)
            FlowCacheManager().save_flow_to_cache(f, str(cache), i, 'npz')
    out = tmp_path / name
    out.mkdir()
    old = os.environ.pop("VFML_LABELS", None)
    if labels is not None:
        os.environ["VFML_LABELS"] = labels
    try:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            rc = fp.main(["--input", f"synthetic:{W}x{H}x{N}", "--output", str(out), "--device", device, "--frames", str(N),
                          "--skip-lods", "--use-flow-cache", str(cache)] + extra)
        assert rc == 0, buf.getvalue()
    finally:
        os.environ.pop("VFML_LABELS", None)
        if old is not None:
            os.environ["VFML_LABELS"] = old
    avis = [n for n in os.listdir(out) if n.endswith(".avi")]
    assert len(avis) == 1, avis
    return str(out / avis[0])


def test_render_video_with_labels_equals_the_host_path(gpu, tmp_path):
    extra = ["--uncompressed", "--taa"]
    cpu_on_path = _run(tmp_path, "cpu_on", "cpu", "1", extra)
    cpu_on = open(cpu_on_path, 'rb').read()
    dev_on = open(_run(tmp_path, "dev_on", "cuda", "1", extra), 'rb').read()
    cpu_off_path = _run(tmp_path, "cpu_off", "cpu", None, extra)
    dev_off = open(_run(tmp_path, "dev_off", "cuda", None, extra), 'rb').read()
    on, _ = read_frames(cpu_on_path)
    off, _ = read_frames(cpu_off_path)
    diff = np.abs(np.frombuffer(dev_on, np.uint8).astype(int) - np.frombuffer(cpu_on, np.uint8).astype(int)) \
        if len(dev_on) == len(cpu_on) else None
    print("labels on: AVI bytes", len(dev_on), "differing", None if diff is None else int((diff > 0).sum()),
          "max", None if diff is None else int(diff.max()))
    assert dev_on == cpu_on                                               # the labelled video, byte for byte
    assert dev_off == open(cpu_off_path, 'rb').read()                     # switch unset: the video as before
    assert on.shape == off.shape == (N, 2 * H, 2 * W, 3) and (on != off).any()
    ops = oracle.side_by_side_ops(H, W, 2, "VideoFlow", False, "gamedev")
    for k in range(N):
        np.testing.assert_array_equal(on[k], oracle.draw_ops(off[k], ops))


def test_mjpg_device_path_with_labels(gpu, tmp_path, monkeypatch):
    """4:4:4 frames: an MCU is one 8 x 8 block and decodes on its own, so the labelled frame may differ from the plain
    one only in blocks that intersect a label's box."""
    pytest.importorskip("PIL")
    from PIL import Image
    monkeypatch.setenv("VFML_MJPG_SAMPLING", "4:4:4")
    on = parse_avi(_run(tmp_path, "on", "cuda", "1", ["--taa"]))
    off = parse_avi(_run(tmp_path, "off", "cuda", "0", ["--taa"]))
    assert on["handler"] == b'MJPG' and len(on["frames"]) == len(off["frames"]) == N
    boxes = vtext.plan_boxes(vtext.build_plan(oracle.side_by_side_ops(H, W, 2), 2 * H, 2 * W))
    touched = np.zeros((2 * H // 8, 2 * W // 8), bool)
    for x0, y0, x1, y1, _, _ in boxes:
        touched[y0 // 8:y1 // 8 + 1, x0 // 8:x1 // 8 + 1] = True
    for a, b in zip(on["frames"], off["frames"]):
        pa = np.asarray(Image.open(io.BytesIO(a)).convert("RGB")).astype(int)
        pb = np.asarray(Image.open(io.BytesIO(b)).convert("RGB")).astype(int)
        assert pa.shape == pb.shape == (2 * H, 2 * W, 3)
        changed = (pa != pb).any(2).reshape(2 * H // 8, 8, 2 * W // 8, 8).any((1, 3))
        assert changed.any() and not (changed & ~touched).any()
        assert np.abs(pa - pb)[5:20, 5:60].max() > 100                    # "Original" is there: white strokes, black outline
