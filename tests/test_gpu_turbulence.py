"""vfml_flow_turbulence_map on the MI355X against the numpy restatement (tests/turbulence_oracle.py).

Flows quantised to multiples of 2^-8 with |v| <= 64 make every f64 window sum exact, so the result cannot depend on the
summation order and the device must reproduce the restatement bit for bit: tv, lo / hi, the index and the picture.  An
unquantised 1080p field gets the quality map's allowance (index within one step on < 1e-5 of the pixels)."""
import os

import numpy as np
import pytest
import torch

import turbulence_oracle as to

pytestmark = pytest.mark.gpu


def _device_map(flow, h, w, k, gpu):
    from vfml import hip
    fl = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).to(gpu)
    bgr, index, tv, lohi = hip.flow_turbulence_map(fl, h, w, k, want=("index", "tv", "lohi"))
    return {"bgr": bgr.cpu().numpy(), "index": index.cpu().numpy(), "tv": tv.cpu().numpy(), "lohi": lohi.cpu().numpy()}


def _assert_identical(dev, ref, what):
    for name in ("tv", "lohi"):
        a, b = dev[name].view(np.uint32), np.ascontiguousarray(ref[name]).view(np.uint32)
        bad = a != b
        print(f"{what}: {name}: {int(bad.sum())} of {bad.size} bit patterns differ")
        assert a.shape == b.shape and not bad.any(), f"{what}: {name}: {int(bad.sum())} of {bad.size} differ, first at " \
                                                     f"{np.argwhere(bad)[0].tolist()}"
    for name in ("index", "bgr"):
        bad = dev[name] != ref[name]
        print(f"{what}: {name}: {int(bad.sum())} of {bad.size} bytes differ")
        assert dev[name].shape == ref[name].shape and dev[name].dtype == np.uint8 and not bad.any(), \
            f"{what}: {name}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}"


# (field h, field w, frame h, frame w, kernel size)
EXACT_CASES = {
    "45x61": (45, 61, 45, 61, 25),
    "9x200_shorter_than_radius": (9, 200, 9, 200, 25),
    "70x130_partial_tiles": (70, 130, 70, 130, 25),
    "1080x1920": (1080, 1920, 1080, 1920, 25),
    "45x61_k1": (45, 61, 45, 61, 1),
    "45x61_k3": (45, 61, 45, 61, 3),
    "45x61_k63": (45, 61, 45, 61, 63),
    "lod_2x": (54, 80, 108, 160, 25),
    "lod_4x": (27, 40, 108, 160, 25),
    "lod_2x_k63": (54, 80, 108, 160, 63),
}


@pytest.mark.parametrize("case", list(EXACT_CASES))
def test_quantised_fields_bit_identical(gpu, case):
    fh, fw, h, w, k = EXACT_CASES[case]
    flow = to.quantised_flow(fh, fw, seed=len(case) * 1000 + fh + fw + k)
    assert np.abs(flow).max() <= 64 and (flow * 256 == np.round(flow * 256)).all()
    ref = to.turbulence_map(flow, h, w, k)
    if k > 1:       # (k = 1: mean2 = f32(v * v) = mean * mean, tv is 0 everywhere and the flat branch is taken)
        assert ref["lohi"][1] - ref["lohi"][0] > 1e-6        # these cases take the normalising branch
    _assert_identical(_device_map(flow, h, w, k, gpu), ref, case)


def test_quantised_extreme_magnitudes(gpu):
    """|v| up to the 64 the exactness argument allows, signs mixed."""
    rng = np.random.default_rng(11)
    flow = (rng.integers(-64 * 256, 64 * 256 + 1, (90, 150, 2)) / 256.0).astype(np.float32)
    _assert_identical(_device_map(flow, 90, 150, 25, gpu), to.turbulence_map(flow, 90, 150, 25), "extremes")


@pytest.mark.parametrize("case", ["1x1", "all_equal", "all_equal_lod"])
def test_flat_fields_paint_jet0(gpu, case):
    """hi - lo <= 1e-6: every pixel is JET[0]."""
    flow, h, w = {"1x1": (np.array([[[3.25, -1.5]]], np.float32), 1, 1),
                  "all_equal": (np.full((40, 50, 2), 2.75, np.float32), 40, 50),
                  "all_equal_lod": (np.full((10, 13, 2), -1.25, np.float32), 40, 52)}[case]
    ref = to.turbulence_map(flow, h, w, 25)
    assert (ref["index"] == 0).all() and not ref["lohi"][1] - ref["lohi"][0] > 1e-6
    dev = _device_map(flow, h, w, 25, gpu)
    _assert_identical(dev, ref, case)
    assert (dev["bgr"] == to.JET_BGR[0]).all()


def test_unquantised_1080p_within_one_step(gpu):
    """Arbitrary float32 vectors: the f64 sums now round, so the summation order shows in a few tv values; the index may
    move by one step on fewer than 1e-5 of the pixels (the allowance of the quality map, tests/test_quality_map.py)."""
    rng = np.random.default_rng(2024)
    h, w = 1080, 1920
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    flow = np.stack([5 * np.sin(xx / 41 + yy / 67), 4 * np.cos(yy / 31 - xx / 83)], axis=2).astype(np.float32)
    flow += (rng.normal(0, 1, (h, w, 2)) * rng.choice([0.01, 0.1, 1.0, 4.0], (h // 40, w // 40, 1)).repeat(40, 0).repeat(40, 1)
             ).astype(np.float32)
    ref = to.turbulence_map(flow, h, w, 25)
    dev = _device_map(flow, h, w, 25, gpu)
    tv_diff = int((dev["tv"].view(np.uint32) != ref["tv"].view(np.uint32)).sum())
    step = np.abs(dev["index"].astype(np.int32) - ref["index"].astype(np.int32))
    print(f"unquantised 1080p: {tv_diff} of {h * w} tv values differ; index differs on {int((step > 0).sum())} pixels, "
          f"max step {int(step.max())}; lo/hi device {dev['lohi'].tolist()} oracle {ref['lohi'].tolist()}")
    assert step.max() <= 1
    assert (step > 0).mean() < 1e-5
    assert (dev["bgr"] == to.JET_BGR[dev["index"]]).all()


def test_two_calls_and_a_side_stream_give_identical_bytes(gpu):
    flow = to.quantised_flow(270, 480, seed=77) + np.float32(1 / 3)       # unquantised on purpose
    first = _device_map(flow, 270, 480, 25, gpu)
    second = _device_map(flow, 270, 480, 25, gpu)
    side = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        third = _device_map(flow, 270, 480, 25, gpu)
    torch.cuda.synchronize()
    for other in (second, third):
        for name in first:
            assert first[name].tobytes() == other[name].tobytes(), name


def test_numpy_api_and_optional_outputs(gpu):
    import flow_maps
    from vfml import hip
    flow = to.quantised_flow(45, 61, seed=5)
    ref = to.turbulence_map(flow, 45, 61, 25)
    out = flow_maps.generate_turbulence_map(flow, (45, 61, 3), device=gpu)
    assert out.dtype == np.uint8 and (out == ref["bgr"]).all()
    half = to.quantised_flow(23, 31, seed=6)                  # not an exact ratio: the resize path through the numpy API
    out = flow_maps.generate_turbulence_map(half, (45, 61), device="cuda", kernel_size=9)
    assert out.shape == (45, 61, 3) and out.dtype == np.uint8
    assert (out.reshape(-1, 1, 3) == to.JET_BGR[None]).all(2).any(1).all()       # every pixel is a table entry
    fl = torch.from_numpy(flow).to(gpu)
    only = hip.flow_turbulence_map(fl, 45, 61)               # no optional output
    assert torch.is_tensor(only) and (only.cpu().numpy() == ref["bgr"]).all()
    with pytest.raises(ValueError):
        hip.flow_turbulence_map(fl, 45, 61, 24)
    with pytest.raises(ValueError):
        hip.flow_turbulence_map(fl, 45, 61, want=("nope",))


def test_non_finite_vectors_stay_in_bounds(gpu):
    """The picture is unspecified; the call completes and every index is a table entry."""
    flow = to.quantised_flow(64, 96, seed=9)
    flow[5, 7] = np.nan
    flow[40, 60, 0] = np.inf
    flow[50, 3, 1] = -np.inf
    dev = _device_map(flow, 64, 96, 25, gpu)
    assert (dev["bgr"] == to.JET_BGR[dev["index"]]).all()


def test_qa_video_quadrants_equal_the_library_calls(gpu, tmp_path):
    import flow_maps
    from storage.avi_reader import read_frames
    from storage.cache_manager import FlowCacheManager
    from vfml import hip
    from vfml.synth import synthetic_clip
    h, w, n = 48, 66, 4                                       # 2w = 132 pixels: DIB rows need no padding; 66 is no tile multiple
    frames = synthetic_clip(n, h, w)
    clip = tmp_path / "clip.npy"
    np.save(clip, np.stack(frames))
    cache = tmp_path / "cache"
    mgr = FlowCacheManager()
    flows = [to.quantised_flow(h, w, seed=300 + i) for i in range(n)]
    for i in range(n):                                        # the last one has no successor frame: skipped
        mgr.save_flow_to_cache(flows[i], str(cache), i, "npz")
    out = tmp_path / "qa.avi"
    assert flow_maps.main(["--input", str(clip), "--flow-cache", str(cache), "--output", str(out), "--kernel-size", "9",
                           "--threshold", "0.7", "--uncompressed"]) == 0
    video = read_frames(str(out))
    assert len(video) == n - 1
    for i, pic in enumerate(video):
        assert pic.shape == (2 * h, 2 * w, 3)
        f1, f2 = (torch.from_numpy(frames[j]).to(gpu) for j in (i, i + 1))
        fl = torch.from_numpy(flows[i]).to(gpu)
        assert (pic[:h, :w] == frames[i]).all()
        assert (pic[:h, w:] == hip.flow_colorize(fl, hip.COLORIZE_HSV).cpu().numpy()).all()
        assert (pic[h:, :w] == hip.flow_quality_map(f1, f2, fl, 0.7).cpu().numpy()).all()
        bgr = hip.flow_turbulence_map(fl, h, w, 9).cpu().numpy()
        assert (pic[h:, w:] == bgr[:, :, ::-1]).all()
        assert (bgr == to.turbulence_map(flows[i], h, w, 9)["bgr"]).all()
    # a window of the cache
    assert flow_maps.main(["--input", str(clip), "--flow-cache", str(cache), "--output", str(out), "--start-frame", "1",
                           "--frames", "1", "--uncompressed"]) == 0
    one = read_frames(str(out))
    assert len(one) == 1 and (one[0][:h, :w] == frames[1]).all()
    assert os.path.getsize(out) > 0
