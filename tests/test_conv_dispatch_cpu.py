"""Which kernel a convolution call becomes: vfml_conv2d_variant / vfml_conv2d_split_variant against a recorded fixture.

tests/golden/conv_dispatch.json holds, per call, the name of the template instantiation (or the error text) that the
dispatcher of commit `parent` chose - recorded from that commit's C++ with launchers that wrote down their own template
arguments instead of launching.  The plan function (csrc/conv_split_plan.hip) must choose the same for every row.
No GPU: the addresses are made up, the library compares them and checks their alignment, nothing more."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_dispatch.json")

# made-up, 32-byte aligned, far enough apart for every operand of the table
IN0, W_HI, OUT, BIAS, AUX0, ADDEND, OUT_T, STATS, KSPLIT_WS, PROJ_W, PROJ_OUT = (0x10000000 * i for i in range(1, 12))
IN1_FAR = IN0 + (1 << 24)       # a second source with a row stride of its own, in the same buffer


def make_call(row):
    """(ConvDesc, weight arguments or None) of a fixture row: `call` holds the fields that differ from a 1x1 stride-1
    convolution of one 16 x 16 image; in1 is the channel slice behind in0 of one pixel row (ld0 = ld1 = c0 + c1) unless
    `in1_far` gives it rows of its own (ld0 = c0, ld1 = c1) 16 MiB further on."""
    from vfml import hip
    c = dict(n=1, h=16, w=16, c0=32, c1=0, cout=32, kh=1, kw=1, stride=1, pad_h=0, pad_w=0, epilogue=0, split=0, flags=0,
             in_fmt=0, out_fmt=0, aux_fmt=0, k_order=0, w_lo=True, split_api=True, in1_far=False, bias=0, aux0=False, addend=False,
             out_t=False, stats_part=False, ksplit_ws=False, proj_n=0)
    c.update(row["call"])
    ctot = c["c0"] + c["c1"]
    d = hip.ConvDesc()
    d.in0, d.c0 = IN0, c["c0"]
    d.ld0 = c.get("ld0", c["c0"] if c["in1_far"] else ctot)
    if c["c1"]:
        d.in1, d.c1 = (IN1_FAR if c["in1_far"] else IN0 + 4 * c["c0"]), c["c1"]
        d.ld1 = c.get("ld1", c["c1"] if c["in1_far"] else ctot)
    d.n, d.h, d.w = c["n"], c["h"], c["w"]
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w = c["cout"], c["kh"], c["kw"], c["stride"], c["pad_h"], c["pad_w"]
    d.out, d.ldo = OUT, c.get("ldo", c["cout"])
    d.epilogue, d.split, d.out_scale, d.flags = c["epilogue"], c["split"], 1.0, c["flags"]
    if c["bias"]:
        d.bias = BIAS + c["bias"] - 1         # (bias = 1: aligned; 5: four bytes off a 16-byte boundary)
    if c["aux0"]:
        d.aux0, d.ld_aux0 = AUX0, c["cout"]
    if c["addend"]:
        d.addend, d.ld_addend = ADDEND, c["cout"]
    ho = (c["h"] + 2 * c["pad_h"] - c["kh"]) // c["stride"] + 1
    wo = (c["w"] + 2 * c["pad_w"] - c["kw"]) // c["stride"] + 1
    if c["out_t"]:
        d.out_t, d.ld_out_t = OUT_T, c["n"] * ho * wo
    if c["stats_part"]:
        d.stats_part = STATS
    if c["ksplit_ws"]:
        d.ksplit_ws = KSPLIT_WS
    if c["proj_n"]:
        d.proj_hi, d.proj_lo = PROJ_W, PROJ_W + 2 * c["proj_n"] * c["cout"]
        d.proj_n, d.proj_kp, d.proj_scale, d.proj_out, d.ld_proj = c["proj_n"], c["cout"], 1.0, PROJ_OUT, c["proj_n"]
    if not c["split_api"]:
        d.weight = W_HI
        return d, None
    taps = c["kh"] * c["kw"]
    kp = c.get("kp", {0: (taps * ctot + 31) // 32 * 32, 1: taps * ((ctot + 31) // 32 * 32), 2: taps * ctot}[c["k_order"]])
    return d, (W_HI, (W_HI + 2 * c["cout"] * kp) if c["w_lo"] else None, kp, 1.0, c["in_fmt"], c["out_fmt"], c["aux_fmt"], c["k_order"])


def _rows():
    with open(FIXTURE) as f:
        return json.load(f)["rows"]


def test_the_fixture_covers_every_kernel_family_and_the_refusals():
    rows = _rows()
    names = [r["name"] for r in rows if "name" in r]
    for family in ("conv_gemm_kernel<", "conv_gemm_split_kernel<", "conv_gemm_dma_kernel<", "conv_gemm_tapx_kernel<"):
        assert any(n.startswith(family) for n in names), family
    assert sum("error" in r for r in rows) >= 4 and sum(bool(r.get("tile")) for r in rows) >= 7
    assert len({r["id"] for r in rows}) == len(rows) >= 60


@pytest.mark.parametrize("row", _rows(), ids=lambda r: r["id"])
def test_variant_is_what_the_recorded_dispatcher_chose(row, monkeypatch):
    from vfml import hip
    L = hip.lib()
    if row.get("tile"):
        monkeypatch.setenv("VFML_DMA_TILE", row["tile"])
    else:
        monkeypatch.delenv("VFML_DMA_TILE", raising=False)
    d, wargs = make_call(row)
    buf = ctypes.create_string_buffer(160)
    if wargs is None:
        rc = L.vfml_conv2d_variant(ctypes.byref(d), buf, len(buf))
    else:
        rc = L.vfml_conv2d_split_variant(ctypes.byref(d), *wargs, buf, len(buf))
    if "error" in row:
        assert rc != 0 and L.vfml_last_error().decode() == row["error"]
    else:
        assert rc == 0, L.vfml_last_error().decode()
        assert buf.value.decode() == row["name"]
