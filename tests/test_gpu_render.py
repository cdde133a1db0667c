"""Render stage on the MI355X: vfml_flow_colorize and vfml_compose_frame against the host paths byte for byte, and
flow_processor's --taa workflow with --device cuda against the --device cpu run."""
import os

import numpy as np
import pytest
import torch

from encoding import HSVFlowEncoder, TorchvisionFlowEncoder
from test_render_cpu import GOLD, SPECIALS, read_frames, run_taa_cli
from visualization.video_composer import create_side_by_side

pytestmark = pytest.mark.gpu


def _fields(h, w, seed):
    rng = np.random.default_rng(seed)
    f = rng.normal(0, 6, (h, w, 2)).astype(np.float32)
    f[rng.random((h, w)) < 1e-3] = np.nan
    f[rng.random((h, w)) < 1e-3, 0] = np.inf
    f[rng.random((h, w)) < 1e-3, 1] = -np.inf
    return f


def _cases():
    for key in SPECIALS:
        yield key, GOLD[f"enc_in_{key}"]
    for i, f in enumerate(GOLD["fields"]):
        yield f"field{i}", f
    yield "1080p", _fields(1080, 1920, 1)
    yield "3840", _fields(64, 3840, 2)
    yield "zero1080", np.zeros((1080, 1920, 2), np.float32)
    big = _fields(1080, 1920, 3)
    big[500, 700] = (3e38, 3e38)                 # |f| is inf: the frame maximum is inf
    yield "infmag", big


@pytest.mark.parametrize("enc", [HSVFlowEncoder, TorchvisionFlowEncoder])
def test_colorize_equals_host_encoders(gpu, enc):
    for name, f in _cases():
        host = enc().encode(f, f.shape[1], f.shape[0])
        dev = enc().encode(torch.from_numpy(f).to(gpu), f.shape[1], f.shape[0])
        np.testing.assert_array_equal(dev.cpu().numpy(), host, err_msg=name)


def _tiles(h, w, seed, hist_dtype):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    t = [rng.uniform(-40, 300, (h, w, 3)).astype(hist_dtype) for _ in range(2)]
    for x in t:
        x[rng.random((h, w, 3)) < 0.01] = np.nan
        x[0, 0, 0], x[0, 0, 1] = np.inf, -np.inf
    return a, b, t[0], t[1]


@pytest.mark.parametrize("h,w", [(40, 56), (37, 53), (1080, 1920)])
@pytest.mark.parametrize("hist", [np.float32, np.float64])
def test_compose_equals_host_composer(gpu, h, w, hist):
    from storage.avi_writer import bgr_to_dib, dib_stride
    from vfml import hip
    a, b, c, d = _tiles(h, w, h + w, hist)
    dev = [torch.from_numpy(x).to(gpu) for x in (a, b, c, d)]
    for flow_only, taa in ((False, False), (True, False), (False, True)):
        ref = create_side_by_side(a, b, flow_only=flow_only, taa_frame=c if taa else None,
                                  taa_simple_frame=d if taa else None)
        oh, ow = ref.shape[:2]
        tiles = dev if taa else dev[:2]
        layout = hip.COMPOSE_STACKED if flow_only else (hip.COMPOSE_GRID_2X2 if taa else hip.COMPOSE_SIDE_BY_SIDE)
        for bgr in (True, False):
            for bottom_up in (False, True):
                stride = dib_stride(ow) if bottom_up else 3 * ow
                out = hip.compose_frame(tiles, layout, bgr=bgr, bottom_up=bottom_up, row_stride=stride).cpu().numpy()
                img = ref if bgr else ref[:, :, ::-1]
                want = np.frombuffer(bgr_to_dib(img), np.uint8).reshape(oh, stride) if bottom_up else \
                    np.ascontiguousarray(img).reshape(oh, 3 * ow)
                np.testing.assert_array_equal(out, want, err_msg=f"{flow_only} {taa} {bgr} {bottom_up}")


def test_cli_taa_workflow_on_the_device(gpu, tmp_path):
    for sub in ("cpu", "dev", "dev2"):
        (tmp_path / sub).mkdir()
    cpu_path, _ = run_taa_cli(tmp_path / "cpu", "cpu")
    dev_path, log = run_taa_cli(tmp_path / "dev", "cuda")
    dev2_path, _ = run_taa_cli(tmp_path / "dev2", "cuda")
    cpu, _ = read_frames(cpu_path)
    dev, info = read_frames(dev_path)
    assert dev.shape == cpu.shape and info["dmlh_frames"] == len(cpu)
    h, w = GOLD["frames"].shape[1:3]
    np.testing.assert_array_equal(dev[:, :h], cpu[:, :h])           # original | flow: byte for byte
    d = np.abs(dev[:, h:].astype(int) - cpu[:, h:].astype(int))      # TAA tiles: vfml_taa_blend's exp() last ulps
    assert d.max() <= 1 and (d > 0).mean() < 1e-3, ((d > 0).sum(), d.max())
    assert open(dev_path, 'rb').read() == open(dev2_path, 'rb').read()    # deterministic
    assert os.path.getsize(dev_path) == os.path.getsize(cpu_path)
