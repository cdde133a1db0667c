"""--flow-input on the MI355X: vfml_flow_decode bit for bit against the host decoders over every input there is,
vfml_flow_diff_overlay and the GRID_2X3 layout of vfml_compose_frame byte for byte against the host functions, and
flow_processor's comparison mode with --device cuda against the --device cpu run."""
import ctypes

import numpy as np
import pytest
import torch

from test_flow_input_cpu import FX, JOBS, OVERLAYS, run_flow_input_job
from test_render_cpu import GOLD, read_frames

pytestmark = pytest.mark.gpu

CLAMPS = (32.0, 64.0, 20.0, 7.3)


def _decode_both(pic, variant, clamp, gpu):
    from encoding.flow_encoders import decode_motion_vectors
    from vfml import hip
    host = decode_motion_vectors(pic, clamp_range=clamp, format_variant=variant)
    dev = hip.flow_decode(torch.from_numpy(pic).to(gpu), hip.ENCODE_RG8 if variant == "rg8" else hip.ENCODE_RGB8, clamp)
    return host, dev.cpu().numpy()


def _same_bits(dev, host, msg):
    assert dev.dtype == host.dtype == np.float32 and dev.shape == host.shape
    bad = dev.view(np.uint32) != host.view(np.uint32)
    assert not bad.any(), f"{msg}: {bad.sum()} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("clamp", CLAMPS)
def test_decode_rgb8_every_triple(gpu, clamp):
    """The 4096 x 4096 picture that holds every (R, G, B) once."""
    v = np.arange(1 << 24, dtype=np.uint32)
    pic = np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=1).astype(np.uint8).reshape(4096, 4096, 3)
    host, dev = _decode_both(pic, "rgb8", clamp, gpu)
    _same_bits(dev, host, f"rgb8 clamp {clamp}")


@pytest.mark.parametrize("clamp", CLAMPS)
def test_decode_rg8_every_pair(gpu, clamp):
    r, g = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for blue in (0, 255):                                     # B is not read
        pic = np.ascontiguousarray(np.stack([r, g, np.full_like(r, blue)], axis=2))
        host, dev = _decode_both(pic, "rg8", clamp, gpu)
        _same_bits(dev, host, f"rg8 clamp {clamp}")


@pytest.mark.parametrize("variant", ["rg8", "rgb8"])
def test_decode_bottom_half_of_a_frame(gpu, variant):
    """A 1080-row encoded picture addressed inside a 2160-row frame on the device (pointer offset, no copy)."""
    from encoding.flow_encoders import decode_motion_vectors
    from vfml import hip
    frame = np.random.default_rng(5).integers(0, 256, (2160, 1920, 3), dtype=np.uint8)
    dev_frame = torch.from_numpy(frame).to(gpu)
    half = dev_frame[1080:]
    assert half.data_ptr() == dev_frame.data_ptr() + 1080 * 1920 * 3
    dev = hip.flow_decode(half, hip.ENCODE_RG8 if variant == "rg8" else hip.ENCODE_RGB8, 32.0).cpu().numpy()
    _same_bits(dev, decode_motion_vectors(frame[1080:], clamp_range=32.0, format_variant=variant), variant)


def _flow_pair(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 6, (h, w, 2)).astype(np.float32)
    b = (a + rng.normal(0, 1, (h, w, 2)) * rng.choice([0.02, 0.2, 0.5, 1.0, 3.0], (h, w, 1))).astype(np.float32)
    for f in (a, b):
        f[rng.random((h, w)) < 1e-3] = np.nan
        f[rng.random((h, w)) < 1e-3, 0] = np.inf
        f[rng.random((h, w)) < 1e-3, 1] = -np.inf
    return a, b


def _overlay_cases():
    from encoding.flow_encoders import decode_motion_vectors
    for name in OVERLAYS:
        yield name, FX[f"overlay_a_{name}"], FX[f"overlay_b_{name}"]
    h = GOLD["frames"].shape[1]
    for job, fmt in JOBS.items():
        video = FX[f"video_{job}"]
        for i, field in enumerate(GOLD["fields"]):
            ext = decode_motion_vectors(video[min(i, len(video) - 1)][h:], clamp_range=32.0,
                                        format_variant=fmt.rsplit("-", 1)[1])
            yield f"{job}[{i}]", field, ext
    yield "1080p", *_flow_pair(1080, 1920, 1)
    yield "3840", *_flow_pair(64, 3840, 2)


def test_diff_overlay_equals_host(gpu):
    from visualization.video_composer import create_difference_overlay
    seen = set()
    for name, a, b in _overlay_cases():
        host = create_difference_overlay(a, b)
        dev = create_difference_overlay(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu))
        assert dev.is_cuda and dev.dtype == torch.uint8
        np.testing.assert_array_equal(dev.cpu().numpy(), host, err_msg=name)
        seen |= {tuple(c) for c in np.unique(host.reshape(-1, 3), axis=0).tolist()}
    assert seen == {(0, 0, 0), (255, 255, 255), (0, 255, 0), (255, 255, 0), (255, 165, 0), (255, 0, 0), (255, 0, 255)}


def _tiles(h, w, seed, hist_dtype):
    rng = np.random.default_rng(seed)
    u8 = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
    t = [rng.uniform(-40, 300, (h, w, 3)).astype(hist_dtype) for _ in range(3)]
    for x in t:
        x[rng.random((h, w, 3)) < 0.01] = np.nan
        x[0, 0, 0], x[0, 0, 1] = np.inf, -np.inf
    return [u8[0], u8[1], t[0], t[1], t[2], u8[2]]


@pytest.mark.parametrize("h,w", [(40, 56), (37, 53), (1080, 1920)])
@pytest.mark.parametrize("hist", [np.float32, np.float64])
def test_grid_2x3_equals_host_grid(gpu, h, w, hist):
    from storage.avi_writer import bgr_to_dib, dib_stride
    from vfml import hip
    from visualization.video_composer import create_6_video_grid
    tiles = _tiles(h, w, h + w, hist)
    dev = [torch.from_numpy(x).to(gpu) for x in tiles]
    with np.errstate(invalid="ignore"):
        ref = create_6_video_grid(*tiles)
    assert ref.shape == (3 * h, 2 * w, 3)
    np.testing.assert_array_equal(create_6_video_grid(*dev).cpu().numpy(), ref)
    for bgr in (True, False):
        for bottom_up in (False, True):
            stride = dib_stride(2 * w) if bottom_up else 6 * w
            out = hip.compose_frame(dev, hip.COMPOSE_GRID_2X3, bgr=bgr, bottom_up=bottom_up,
                                    row_stride=stride).cpu().numpy()
            img = ref if bgr else ref[:, :, ::-1]
            want = np.frombuffer(bgr_to_dib(img), np.uint8).reshape(3 * h, stride) if bottom_up else \
                np.ascontiguousarray(img).reshape(3 * h, 6 * w)
            np.testing.assert_array_equal(out, want, err_msg=f"{bgr} {bottom_up}")
    # the mixed case the render loop produces: an f32 first history beside f64 ones
    mixed = list(tiles)
    mixed[3] = np.nan_to_num(tiles[3], nan=7.0, posinf=1e9, neginf=-1e9).astype(np.float32)
    got = create_6_video_grid(*[torch.from_numpy(x).to(gpu) for x in mixed]).cpu().numpy()
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(got, create_6_video_grid(*mixed))


@pytest.mark.parametrize("job", list(JOBS))
def test_cli_flow_input_on_the_device(gpu, tmp_path, job):
    cpu_path, cpu_log = run_flow_input_job(tmp_path, "cpu", job, "npy", "cpu")
    dev_path, dev_log = run_flow_input_job(tmp_path, "cuda", job, "avi", "dev")
    dev2_path, _ = run_flow_input_job(tmp_path, "cuda", job, "npy", "dev2")
    cpu, _ = read_frames(cpu_path)
    dev, info = read_frames(dev_path)
    h, w = GOLD["frames"].shape[1:3]
    assert dev.shape == cpu.shape == (6, 3 * h, 2 * w, 3) and info["dmlh_frames"] == 6
    np.testing.assert_array_equal(dev[:, :h], cpu[:, :h])                      # original | external flow picture
    np.testing.assert_array_equal(dev[:, 2 * h:, w:], cpu[:, 2 * h:, w:])      # difference
    np.testing.assert_array_equal(cpu, FX[f"out_{job}"])
    taa_dev = np.concatenate([dev[:, h:2 * h].reshape(6, -1), dev[:, 2 * h:, :w].reshape(6, -1)], axis=1).astype(int)
    taa_cpu = np.concatenate([cpu[:, h:2 * h].reshape(6, -1), cpu[:, 2 * h:, :w].reshape(6, -1)], axis=1).astype(int)
    d = np.abs(taa_dev - taa_cpu)                  # the three TAA tiles: vfml_taa_blend's exp() last ulps
    print(f"{job}: TAA tiles max |diff| {d.max()}, differing share {(d > 0).mean():.2e}")
    assert d.max() <= 1 and (d > 0).mean() < 1e-3, ((d > 0).sum(), d.max())
    assert open(dev_path, 'rb').read() == open(dev2_path, 'rb').read()        # deterministic, .avi or .npy flow video
    block = [ln for ln in dev_log.splitlines() if ln.startswith(("[Flow Input]", "  Flow input", "  Main video"))]
    assert block[:3] == [str(s) for s in FX[f"log_{job}"][:3]]


def test_rejected_arguments_launch_nothing(gpu):
    from vfml import hip
    L = hip.lib()
    pic = torch.zeros((8, 8, 3), dtype=torch.uint8, device=gpu)
    flow = torch.zeros((8, 8, 2), dtype=torch.float32, device=gpu)
    out = torch.zeros((8, 8, 3), dtype=torch.uint8, device=gpu)
    p, f, o = (ctypes.c_void_p(t.data_ptr()) for t in (pic, flow, out))
    odd = ctypes.c_void_p(flow.data_ptr() + 4)
    assert L.vfml_flow_decode(p, 8, 8, hip.ENCODE_RG8, 32.0, f, None) == 0
    assert L.vfml_flow_decode(p, 8, 8, hip.ENCODE_GAMEDEV, 32.0, f, None) != 0 and b"unknown mode" in L.vfml_last_error()
    assert L.vfml_flow_decode(p, 8, 8, 7, 32.0, f, None) != 0
    assert L.vfml_flow_decode(None, 8, 8, hip.ENCODE_RG8, 32.0, f, None) != 0
    assert L.vfml_flow_decode(p, 8, 8, hip.ENCODE_RG8, 32.0, None, None) != 0
    assert L.vfml_flow_decode(p, 8, 7, hip.ENCODE_RGB8, 32.0, odd, None) != 0 and b"aligned" in L.vfml_last_error()
    assert L.vfml_flow_decode(p, 0, 8, hip.ENCODE_RG8, 32.0, f, None) != 0
    assert L.vfml_flow_diff_overlay(f, f, 8, 8, o, None) == 0
    assert L.vfml_flow_diff_overlay(None, f, 8, 8, o, None) != 0
    assert L.vfml_flow_diff_overlay(f, None, 8, 8, o, None) != 0
    assert L.vfml_flow_diff_overlay(f, f, 8, 8, None, None) != 0
    assert L.vfml_flow_diff_overlay(f, odd, 8, 7, o, None) != 0 and b"aligned" in L.vfml_last_error()
    tiles = (ctypes.c_void_p * 6)(*[pic.data_ptr()] * 5, None)
    types = (ctypes.c_int32 * 6)(*[0] * 6)
    big = torch.zeros(24 * 48, dtype=torch.uint8, device=gpu)
    assert L.vfml_compose_frame(tiles, types, 8, 8, hip.COMPOSE_GRID_2X3, 0, 48, ctypes.c_void_p(big.data_ptr()), None) != 0
    assert b"tile 5 missing" in L.vfml_last_error()
    assert L.vfml_compose_frame(tiles, types, 8, 8, 4, 0, 48, ctypes.c_void_p(big.data_ptr()), None) != 0
    torch.cuda.synchronize()
    assert not big.any().item()                                   # nothing was written by the rejected calls
    with pytest.raises(ValueError):
        hip.compose_frame([pic] * 4, hip.COMPOSE_GRID_2X3)
