"""Turbulence map, the part that needs no GPU: the numpy restatement (tests/turbulence_oracle.py) against a brute-force
double loop, the committed JET table against its generator, the two new C-ABI symbols, flow_maps' error contract and
its command line."""
import ctypes
import os
import re

import numpy as np
import pytest

import turbulence_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "video-flow-ml_amd", "vfml", "csrc")
SYMBOLS = ("vfml_flow_turbulence_workspace_bytes", "vfml_flow_turbulence_map")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("h,w,k", [(9, 11, 5), (6, 7, 3), (4, 5, 25), (3, 2, 63), (1, 1, 25), (7, 6, 1)])
def test_oracle_equals_brute_force(h, w, k):
    """Tiny fields, some smaller than the radius (the border reflects several times).  Quantised values: every sum is
    exact, so all summation orders must agree to the bit."""
    flow = to.quantised_flow(h, w, seed=h * 100 + w)
    want = to.brute_force_tv(flow, k)
    for box in (to.box_mean, lambda a, kk: to.box_mean(a, kk, "cols_first"), to.box_mean_direct):
        got = to.total_variation(flow, h, w, k, box)
        assert (_bits(got) == _bits(want)).all()


def test_reflect_index_is_border_reflect():
    assert to.reflect_index(8, 6).tolist() == [5, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5, 6, 7, 7, 6, 5, 4, 3, 2]
    assert to.reflect_index(2, 5).tolist() == [0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1]     # periodic
    assert to.reflect_index(1, 3).tolist() == [0] * 7


def test_oracle_picture_properties():
    flow = to.quantised_flow(45, 61, seed=1)
    r = to.turbulence_map(flow, 45, 61, 25)
    assert r["bgr"].shape == (45, 61, 3) and r["bgr"].dtype == np.uint8
    assert r["lohi"][0] < r["lohi"][1]
    assert (r["index"] == 0).mean() >= 0.05 - 1e-3 and (r["index"] == 255).mean() >= 0.05 - 1e-3
    assert (r["bgr"] == to.JET_BGR[r["index"]]).all()
    flat = to.turbulence_map(np.full((20, 30, 2), 1.5, np.float32), 20, 30, 25)
    assert (flat["tv"] == 0).all() and (flat["index"] == 0).all() and (flat["bgr"] == to.JET_BGR[0]).all()
    # a field at half the resolution goes through the quality map's resize and the vector rescale
    lod = to.turbulence_map(to.quantised_flow(10, 15, seed=2), 20, 30, 5)
    assert lod["tv"].shape == (20, 30)


def test_committed_jet_table_equals_its_generator():
    jet = to._jet_module()
    text = open(os.path.join(CSRC, "jet_table.inc")).read()
    assert text == jet.render()
    table = jet.parse(text)
    assert table == jet.jet_table() and len(table) == 256
    t = np.array(table)
    # the landmarks of JET: dark blue, blue, cyan, yellow, red, dark red
    assert t[0].tolist() == [0, 0, 143] and t[255].tolist() == [128, 0, 0]
    # where an abscissa i / 255 falls on a stop (i = 85 k / 21), the entry is that stop
    assert t[85].tolist() == [0, 223, 255] and t[170].tolist() == [255, 207, 0]
    assert (np.diff(t[:, 0].astype(int))[:200] >= 0).all() and (np.diff(t[:, 2].astype(int))[60:] <= 0).all()
    stops = jet.jet_stops()
    assert [float(v) for v in stops[0]] == [0.0, 0.0, 0.5625] and [float(v) for v in stops[63]] == [0.5, 0.0, 0.0]


def test_header_declares_and_library_exports_the_symbols():
    from vfml import hip
    text = open(os.path.join(ROOT, "include", "vfml.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/vfml.h"
        assert name in hip.EXPORTS
    assert "turbulence.hip" in hip.SOURCES
    lib = ctypes.CDLL(hip.build())
    for name in SYMBOLS:
        assert hasattr(lib, name)
    lib.vfml_abi_version.restype = ctypes.c_int
    assert lib.vfml_abi_version() == 27


def test_kernel_size_is_rejected_before_any_launch():
    from vfml import hip
    L = hip.lib()
    for k in (0, 2, 24, 64, 65, -3):
        assert L.vfml_flow_turbulence_map(None, 4, 4, 4, 4, k, None, None, None, None, None, None) != 0
        assert b"ksize" in L.vfml_last_error()
    assert L.vfml_flow_turbulence_map(None, 4, 4, 4, 4, 25, None, None, None, None, None, None) != 0    # null pointers
    assert L.vfml_flow_turbulence_workspace_bytes(1080, 1920) >= 4 * 1080 * 1920
    assert L.vfml_flow_turbulence_workspace_bytes(0, 5) == 0


def test_flow_maps_error_contract():
    import flow_maps
    flow = np.zeros((8, 8, 2), np.float32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        flow_maps.generate_turbulence_map(flow, (8, 8, 3), device="cpu")
    for k in (24, 0, 2):
        with pytest.raises(ValueError):
            flow_maps.generate_turbulence_map(flow, (8, 8, 3), kernel_size=k)
    with pytest.raises(ValueError):
        flow_maps.generate_turbulence_map(flow, (8, 8, 3), kernel_size=65)
    # no field, or an empty one: a zero picture, as the reference returns
    for empty in (None, np.zeros((0, 8, 2), np.float32), np.zeros((8, 0, 2), np.float32)):
        out = flow_maps.generate_turbulence_map(empty, (6, 9, 3))
        assert out.shape == (6, 9, 3) and out.dtype == np.uint8 and not out.any()


def test_cli_parser_accepts_the_options():
    import flow_maps
    a = flow_maps.build_parser().parse_args(["--input", "synthetic:64x48x4", "--flow-cache", "cache", "--output", "qa.avi"])
    assert (a.start_frame, a.frames, a.kernel_size, a.threshold, a.uncompressed) == (0, None, 25, 0.8, False)
    a = flow_maps.build_parser().parse_args(["--input", "clip.npy", "--flow-cache", "cache", "--output", "qa.avi",
                                             "--start-frame", "2", "--frames", "3", "--kernel-size", "9",
                                             "--threshold", "0.7", "--uncompressed"])
    assert (a.input, a.flow_cache, a.output) == ("clip.npy", "cache", "qa.avi")
    assert (a.start_frame, a.frames, a.kernel_size, a.threshold, a.uncompressed) == (2, 3, 9, 0.7, True)
    with pytest.raises(SystemExit):
        flow_maps.build_parser().parse_args(["--input", "clip.npy"])
    with pytest.raises(ValueError):
        flow_maps.main(["--input", "synthetic:64x48x4", "--flow-cache", "cache", "--output", "qa.avi", "--kernel-size", "8"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        flow_maps.main(["--input", "synthetic:64x48x4", "--flow-cache", "cache", "--output", "qa.avi", "--device", "cpu"])
