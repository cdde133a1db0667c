"""The coverage ledger of the split-row convolution kernels: which template instantiation each call of
tests/conv_tile_cases.py becomes (vfml_conv2d_split_variant through hip.conv2d(variant_only=True): validated and planned,
nothing launched), held against the instantiations that exist (vfml_conv2d_split_variant_at walks REG_VARIANTS,
DMA_VARIANTS and TAPX_VARIANTS).  Every non-persistent row of DMA_VARIANTS and every row of TAPX_VARIANTS must be reached
by a case - tests/test_gpu_conv_tiles.py runs each case against float64 PyTorch - or stand in UNREACHED with the reason
no accepted call plans it.  No GPU: the addresses are made up, the library compares them and checks their alignment."""
import ctypes
import re

import pytest

from conv_tile_cases import CASES, planned_variant

# name of a row no accepted call plans -> why, from plan_split() and the validation in vfml_conv2d_split.  At most 6.
UNREACHED = {}


def table_rows():
    from vfml import hip
    L = hip.lib()
    rows, buf = [], ctypes.create_string_buffer(160)
    while L.vfml_conv2d_split_variant_at(len(rows), buf, len(buf)) == 0:
        rows.append(buf.value.decode())
        assert len(rows) < 1000
    return rows


@pytest.fixture(scope="module")
def ledger():
    """{case id: planned kernel name}, each case under its own forced tile."""
    names = {}
    with pytest.MonkeyPatch.context() as mp:
        for c in CASES:
            if c.tile:
                mp.setenv("VFML_DMA_TILE", c.tile)
            else:
                mp.delenv("VFML_DMA_TILE", raising=False)
            names[c.id] = planned_variant(c)
    return names


def _in_scope(name):
    """Rows the ledger answers for: the per-tap forms of conv_gemm_dma_kernel (PERSIST false) and conv_gemm_tapx_kernel."""
    return name.startswith("conv_gemm_tapx_kernel<") or re.match(r"conv_gemm_dma_kernel<\d, \d, \d, \d, false,", name) is not None


def test_the_walk_lists_each_table_once():
    from vfml import hip
    rows = table_rows()
    assert len(set(rows)) == len(rows)
    for family in ("conv_gemm_split_kernel<", "conv_gemm_dma_kernel<", "conv_gemm_tapx_kernel<"):
        assert any(r.startswith(family) for r in rows), family
    order = [r.split("<")[0] for r in rows]
    assert order == sorted(order, key=["conv_gemm_split_kernel", "conv_gemm_dma_kernel", "conv_gemm_tapx_kernel"].index)
    buf = ctypes.create_string_buffer(160)
    assert hip.lib().vfml_conv2d_split_variant_at(-1, buf, len(buf)) != 0
    assert hip.lib().vfml_conv2d_split_variant_at(len(rows), buf, len(buf)) != 0


def test_every_planned_name_is_a_row(ledger):
    rows = set(table_rows())
    assert not {cid: nm for cid, nm in ledger.items() if nm not in rows}


def test_every_per_tap_and_shared_stage_row_is_reached(ledger):
    rows = [r for r in table_rows() if _in_scope(r)]
    reached = set(ledger.values())
    assert len(UNREACHED) <= 6
    assert all(r in rows and r not in reached for r in UNREACHED), "UNREACHED names a row that does not exist, or that a case reaches"
    missing = [r for r in rows if r not in reached and r not in UNREACHED]
    assert not missing, "no case of tests/conv_tile_cases.py reaches:\n" + "\n".join(missing)
    others = sorted(nm for nm in reached if not _in_scope(nm))
    print(f"{len(rows)} rows in scope, {len(rows) - len(UNREACHED)} reached by {len(ledger)} cases; out of scope and touched: {others}")


def test_unforced_cases_get_the_smallest_tiles(ledger):
    """At these sizes the cost model never picks a large tile by itself (dma_cost is mf / eff up to 512 tiles: 2.86 for
    128 x 64 against 4.3 and 6.0): what the large tiles do is only seen with VFML_DMA_TILE."""
    auto = {c.id: ledger[c.id] for c in CASES if c.tile is None}
    assert len(auto) >= 10
    for cid, nm in auto.items():
        assert nm.startswith("conv_gemm_dma_kernel<2, 1, 2, 2, false,") or nm.startswith("conv_gemm_dma_kernel<1, 1, 4, 1, false,"), (cid, nm)


def test_forced_cases_run_on_the_tile_and_kernel_they_are_there_for(ledger):
    for c in CASES:
        nm = ledger[c.id]
        if c.kernel:
            assert nm.startswith({"dma": "conv_gemm_dma_kernel<", "tapx": "conv_gemm_tapx_kernel<"}[c.kernel]), (c.id, nm)
        if c.tile and not (c.kernel == "dma" and c.tile in ("2,2,4,1", "2,3,4,1")):
            assert "<" + c.tile.replace(",", ", ") + "," in nm, (c.id, nm)
