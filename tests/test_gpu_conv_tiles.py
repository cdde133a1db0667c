"""conv_gemm_dma_kernel / conv_gemm_tapx_kernel on the tile shapes the 1080p engine runs (192 x 128, 128 x 192, 128 x 128 and
the shared-stage kernel's 256 x 64 / 256 x 96), forced per call with VFML_DMA_TILE on launches of a few hundred pixels:
every case of tests/conv_tile_cases.py against a float64 PyTorch reference of the same operation.

Per case: the whole map, then the rows of the last row tile and the columns of the last column tile by themselves (and
each of the z, r*h and h slices of a gate), so that a defect confined to a tail is not diluted; nothing outside [M][cout] of
a strided output with guard rows behind it may change; and the forced-tile result must be BIT-identical to the same call on
the tile the planner picks by itself (each output element is accumulated over K in the same order whatever the tile).
tests/test_conv_tile_coverage_cpu.py holds the table against the instantiations that exist."""
import dataclasses
import functools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from conv_tile_cases import CASES, GUARD_ROWS, STATE_LD, conv_args, geometry, k_order, tile_dims
from test_gpu_kernels import CONV_TOL, _f16, as_weight, nhwc, rel_err, s16_decode

pytestmark = pytest.mark.gpu

# bounds of the gate epilogues: those of test_gpu_kernels.py::test_gru_epilogues_in_split_rows (z and r*h; h)
GATE_TOL = {"z": 3e-6, "rh": 3e-6, "h": 5e-6}
S16_SENTINEL = 0x4248          # every half of a split-row output before the launch (3.14 as f16)


def _by_group(*groups):
    return [pytest.param(c, id=c.id) for c in CASES if c.group in groups]


@functools.lru_cache(maxsize=None)
def _problem(key):
    """Seeded operands of a case and its float64 pre-activation map, shared by the cases that differ only in tile, kernel
    and addend mode (`key`: the case with those fields blanked).  Never modified by a test."""
    from vfml import hip
    from vfml.weights import pack_conv_weight
    c = key
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    geo = geometry(c)
    M, ctot = geo["M"], c.c0 + c.c1
    p = {}
    if c.state:
        z, r, h = torch.sigmoid(torch.randn(M, 128, generator=g)), torch.sigmoid(torch.randn(M, 128, generator=g)), \
            torch.tanh(torch.randn(M, 128, generator=g))
        xs = torch.randn(M, 384, generator=g)
        p["state"] = torch.cat([z, r * h, h, xs], 1)                      # [ z | r*h | h | x ]
        src = torch.cat([h if c.epi == "gru_zr" else r * h, xs], 1)
        x = src.view(c.n, c.H, c.W, ctot).permute(0, 3, 1, 2).contiguous()
        p["aux0"], p["aux1"] = (h, None) if c.epi == "gru_zr" else (z, h)
    else:
        x = torch.randn(c.n, ctot, c.H, c.W, generator=g)
        na = c.cout - c.split if c.epi == "gru_zr" else c.cout
        p["aux0"] = p["aux1"] = None
        if c.epi == "gru_zr":
            p["aux0"] = torch.tanh(torch.randn(M, na, generator=g))
        elif c.epi == "gru_q":
            p["aux0"], p["aux1"] = torch.sigmoid(torch.randn(M, na, generator=g)), torch.tanh(torch.randn(M, na, generator=g))
        elif c.epi == "add_aux":
            p["aux0"] = torch.randn(M, na, generator=g)
    wt = torch.randn(c.cout, ctot, c.kh, c.kw, generator=g) / math.sqrt(ctot * c.kh * c.kw)
    b = torch.randn(c.cout, generator=g) * (0.1 if c.epi.startswith("gru") else 1.0)
    p["addend"] = torch.randn(M, c.cout, generator=g) * 0.5
    blk = {"tap": False, "cblock": True, "cblock64": 64}[c.korder]
    p["weight"] = as_weight(pack_conv_weight(wt, cblock=blk), c.cout, "f16x3", order=k_order(c))
    p["x"], p["bias"] = x, b.cuda()
    # what the reduced products see: the weights times the power-of-two split scale and / or the activations rounded to ONE f16
    scale = p["weight"].scale
    wq = _f16(wt * scale) / scale if c.mfma in (2, 1) else wt.double()
    xq = _f16(x) if c.mfma in ("2a", 1) else x.double()

    def rows(t):
        return t.permute(0, 2, 3, 1).reshape(M, c.cout)
    pad = (geo["ph"], geo["pw"])
    p["acc"] = rows(F.conv2d(xq, wq, b.double(), stride=c.stride, padding=pad))
    p["full"] = rows(F.conv2d(x.double(), wt.double(), b.double(), stride=c.stride, padding=pad)) if c.mfma != 3 else p["acc"]
    return p


def _key(c):
    return dataclasses.replace(c, group="", tile=None, per_tap=False, addend="none", stats=False, kernel=None)


def _expected(c, p, acc, addend):
    """float64 [M][cout] of the epilogue of case `c` over the pre-activation map `acc`."""
    v = acc + (p["addend"].double() if addend != "none" else 0.0)
    a0 = p["aux0"].double() if p["aux0"] is not None else None
    a1 = p["aux1"].double() if p["aux1"] is not None else None
    if c.epi == "relu":
        return F.relu(v)
    if c.epi == "tanh":
        return torch.tanh(v)
    if c.epi == "sigmoid":
        return torch.sigmoid(v)
    if c.epi == "tanh_relu":
        return torch.cat([torch.tanh(v[:, :c.split]), F.relu(v[:, c.split:])], 1)
    if c.epi == "add_aux":
        return a0 + v
    if c.epi == "gru_zr":
        s = torch.sigmoid(v)
        return torch.cat([s[:, :c.split], s[:, c.split:] * a0], 1)
    if c.epi == "gru_q":
        return (1.0 - a0) * a1 + a0 * torch.tanh(v)
    return v


def _buffers(c, p, gpu):
    """Fresh device buffers of a case: sources and aux operands filled, outputs and guard rows holding the sentinel."""
    from vfml import hip
    geo = geometry(c)
    P, M, sizes = geo["P"], geo["M"], geo["sizes"]
    bufs = {}
    if c.state:
        st = torch.zeros(sizes["state"], device=gpu)
        st.view(torch.int16)[:] = S16_SENTINEL
        hip.to_s16(p["state"].cuda().reshape(-1), P, STATE_LD, STATE_LD, st, STATE_LD)
        bufs["state"] = st
    else:
        src = torch.zeros(sizes["src"], device=gpu)
        xs = nhwc(p["x"]).view(P, c.c0 + c.c1)
        for operand, lo, n in ((geo["in0"], 0, c.c0), (geo["in1"], c.c0, c.c1)):
            if operand:
                _, off, ld = operand
                hip.to_s16(xs[:, lo:lo + n].contiguous().reshape(-1), P, n, n, src, ld, dst_off=off)
        bufs["src"] = src
        if c.out_fmt == "s16":
            out = torch.zeros(sizes["out"], device=gpu)
            out.view(torch.int16)[:] = S16_SENTINEL
        else:
            out = torch.full((sizes["out"],), float("nan"), device=gpu)
        bufs["out"] = out
        if "aux" in sizes:
            aux = torch.zeros(sizes["aux"], device=gpu)
            for k in ("aux0", "aux1"):
                if geo[k]:
                    _, off, ld = geo[k]
                    t = p[k].cuda().contiguous()
                    if c.aux_fmt == "s16":
                        hip.to_s16(t.reshape(-1), M, t.shape[1], t.shape[1], aux, ld, dst_off=off)
                    else:
                        aux[off:off + M * ld].view(M, ld)[:, :t.shape[1]] = t
            bufs["aux"] = aux
    if "addend" in sizes:
        _, off, ld = geo["addend"]
        add = torch.full((sizes["addend"],), float("nan"), device=gpu)
        add[off:off + M * ld].view(M, ld)[:, :c.cout] = p["addend"].cuda()
        bufs["addend"] = add
        bufs["decoy"] = torch.full((sizes["addend"],), 1000.0, device=gpu)    # (what a kernel that ignored addend_ind would add)
    return bufs


def _launch(c, p, gpu, monkeypatch, tile, *, per_tap=None, addend=None, stats_part=None):
    """One run of case `c` on tile `tile` (None: the planner's own) -> (buffers before, buffers after)."""
    from vfml import hip
    bufs = _buffers(c, p, gpu)
    before = {k: v.clone() for k, v in bufs.items()}
    mode = c.addend if addend is None else addend
    ind = None
    if mode == "ind":
        _, off, _ = geometry(c)["addend"]
        table = torch.zeros(4, dtype=torch.int64, device=gpu)
        hip.ptr_table_set(table, [0, bufs["addend"].data_ptr() + 4 * off])
        ind = (table, 1)         # (the cell holds the pointer itself, offset included)
    args, kw = conv_args(c, bufs, p["weight"], p["bias"], per_tap=per_tap, addend=mode, stats_part=stats_part, addend_ind=ind)
    if tile:
        monkeypatch.setenv("VFML_DMA_TILE", tile)
    else:
        monkeypatch.delenv("VFML_DMA_TILE", raising=False)
    hip.conv2d(*args, **kw)
    monkeypatch.delenv("VFML_DMA_TILE", raising=False)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault: nothing that runs after it on this device means anything
        pytest.exit(f"{c.id} on tile {tile}: {e}", returncode=3)
    return before, bufs


def _output(c, before, after):
    """Decoded [M][cout] f32 output of a run on the host, after checking that nothing outside it changed: the other
    columns of the strided rows, the guard rows behind, and every other buffer of the call."""
    geo = geometry(c)
    M = geo["M"]
    name, off, ldo = geo["out"]
    for k in after:
        if k != name:
            assert torch.equal(after[k].view(torch.int32), before[k].view(torch.int32)), f"the launch changed {k}"
    rows = M + GUARD_ROWS
    if c.out_fmt == "s16":
        # units of 8 channels (16 bytes of hi halves, 16 of lo halves): written where row < M and channel < cout
        # (cout % 4 == 0: whole quads), every other half as it was
        a = after[name].view(torch.int16).view(rows, ldo // 8, 2, 8).cpu()
        b = before[name].view(torch.int16).view(rows, ldo // 8, 2, 8).cpu()
        ch = (torch.arange(ldo // 8).view(-1, 1, 1) * 8 + torch.arange(8).view(1, 1, -1)).expand(ldo // 8, 2, 8)
        inside = ((ch >= off) & (ch < off + c.cout)).unsqueeze(0) & (torch.arange(rows) < M).view(-1, 1, 1, 1)
        assert torch.equal(a[~inside], b[~inside]), "split-row output: halves outside [M][cout] changed"
        got = s16_decode(after[name], rows, ldo, ldo)[:M, off:off + c.cout]
    else:
        a = after[name].view(rows, ldo).cpu()
        assert torch.isnan(a[M:]).all() and torch.isnan(a[:M, c.cout:]).all(), "f32 output: written outside [M][cout]"
        got = a[:M, :c.cout]
    assert torch.isfinite(got).all()
    return got


def _regions(c, tile):
    """(name, row slice, column slice, bound) of what is compared by itself: the whole map, the last row tile's rows, the last
    column tile's columns, and the slices of a gate."""
    M, tol = geometry(c)["M"], CONV_TOL["f16x3"]
    tbm, tbn = tile_dims(tile)
    r0, c0 = (M - 1) // tbm * tbm, (c.cout - 1) // tbn * tbn
    if c.epi == "gru_zr":
        zt, rt = (GATE_TOL["z"], GATE_TOL["rh"]) if c.state else (tol, tol)
        reg = [("z", slice(None), slice(0, c.split), zt), ("r*h", slice(None), slice(c.split, None), rt),
               ("z, last row tile", slice(r0, None), slice(0, c.split), zt), ("r*h, last row tile", slice(r0, None), slice(c.split, None), rt)]
        if c0 > c.split:
            reg.append(("r*h, last column tile", slice(None), slice(c0, None), rt))
        return reg
    if c.epi == "gru_q" and c.state:
        tol = GATE_TOL["h"]
    return [("map", slice(None), slice(None), tol), ("last row tile", slice(r0, None), slice(None), tol),
            ("last column tile", slice(None), slice(c0, None), tol)]


def _check(c, tile, got, want):
    errs = {nm: rel_err(got[rs, cs], want[rs, cs].float()) for nm, rs, cs, _ in _regions(c, tile)}
    print(c.id, " ".join(f"{nm}: {e:.2e}" for nm, e in errs.items()))
    for nm, _, _, bound in _regions(c, tile):
        assert errs[nm] < bound, (nm, errs[nm], bound)


def _same_bits(c, a, b, what):
    name = geometry(c)["out"][0]
    x, y = a[name].view(torch.int32), b[name].view(torch.int32)
    if not torch.equal(x, y):
        d = (x.long() - y.long()).abs()
        pytest.fail(f"{what}: {int((d != 0).sum())} words differ, by up to {int(d.max())} (f32: ulps)")


def _run(c, gpu, monkeypatch):
    """Case `c` on its forced tile against float64, and against the same call on the planner's own tile."""
    p = _problem(_key(c))
    before, after = _launch(c, p, gpu, monkeypatch, c.tile)
    got = _output(c, before, after)
    want = _expected(c, p, p["acc"], c.addend)
    _check(c, c.tile, got, want)
    if c.tile:
        _, auto = _launch(c, p, gpu, monkeypatch, None)
        _same_bits(c, after, auto, f"tile {c.tile} against the planner's own")
    return p, got, after


@pytest.mark.parametrize("c", _by_group("uniform", "general", "steps64", "stride2", "auto"))
def test_loaders_and_products_on_forced_tiles(gpu, monkeypatch, c):
    """Both loaders x 3 / 2 / "2a" / 1 MFMAs per product (and the 64-channel steps) x 3x3, 5x1, 1x5, 1x1 taps, stride 1
    and 2.  The reduced products equal the float64 convolution of the f16-rounded operands (exactly the lo terms are gone),
    and differ from the full-precision one by that rounding and no more - as in
    test_gpu_kernels.py::test_conv2d_reduced_mfma_counts_drop_exactly_the_lo_terms."""
    p, got, _ = _run(c, gpu, monkeypatch)
    if c.mfma != 3:
        d = rel_err(got, p["full"].float())
        assert 5e-6 < d < 3e-3, d


@pytest.mark.parametrize("c", _by_group("shared"))
def test_shared_stage_kernel_with_relu_into_split_rows(gpu, monkeypatch, c):
    """conv_gemm_tapx_kernel on each of its four tiles, ReLU into split rows: against float64, and BIT-identical to
    conv_gemm_dma_kernel (VFML_CONV_PER_TAP) on the same tile."""
    p, _, after = _run(c, gpu, monkeypatch)
    _, per_tap = _launch(c, p, gpu, monkeypatch, c.tile, per_tap=True)
    _same_bits(c, after, per_tap, "shared stage against per-tap stages")


@pytest.mark.parametrize("c", _by_group("gate", "gate-ragged"))
def test_gru_gates_on_forced_tiles(gpu, monkeypatch, c):
    """EPI_GRU_ZR / EPI_GRU_Q as the engine issues them - the state buffer in split rows, the gate written in place, the
    batched epilogue (epilogue_rows_fast_k) - without addend, with a per-pixel addend, and with the addend's pointer in a
    device cell (addend_ind; the descriptor's own addend field then names a decoy).  Float64 end to end; z, r*h and h
    each by itself.  The ragged variant (f32 aux operands, the z / r*h boundary at 68 of 132) takes epilogue_rows."""
    p, _, after = _run(c, gpu, monkeypatch)
    if c.addend == "ind":
        _, direct = _launch(c, p, gpu, monkeypatch, c.tile, addend="direct")
        _same_bits(c, after, direct, "addend_ind against addend")
        if c.state:     # (every slice of the state, not only the gate's)
            assert torch.equal(after["state"].view(torch.int32), direct["state"].view(torch.int32))
    if c.kernel == "tapx" and c.addend == "none":
        _, per_tap = _launch(c, p, gpu, monkeypatch, c.tile, per_tap=True)
        _same_bits(c, after, per_tap, "shared stage against per-tap stages")


@pytest.mark.parametrize("c", _by_group("epilogue"))
def test_other_epilogues_on_forced_tiles(gpu, monkeypatch, c):
    """EPI_TANH_RELU (split 128: the context encoder's last layer), EPI_ADD_AUX over a split-row aux operand (the GMA read-out,
    the SK blocks), EPI_TANH and EPI_SIGMOID, into f32 and into split rows."""
    _run(c, gpu, monkeypatch)


@pytest.mark.parametrize("c", _by_group("stats"))
def test_instnorm_partials_on_forced_tiles(gpu, monkeypatch, c):
    """stats_part on the per-tap and the shared-stage kernel's large tiles, as test_conv_leaves_instnorm_partials asserts it
    on the planner's own: the output is the one of the run without statistics, NaN stays behind the partials, and the
    finalised statistics are instnorm_stats of the stored map."""
    from vfml import hip
    p = _problem(_key(c))
    geo = geometry(c)
    hw, chunks = geo["M"], geo["chunks"]
    assert c.n == 1 and chunks == (hw + hip.STATS_ROWS_S16 - 1) // hip.STATS_ROWS_S16
    part = torch.full((chunks * c.cout * 2 + 8,), float("nan"), device=gpu, dtype=torch.float64)
    before, after = _launch(c, p, gpu, monkeypatch, c.tile, stats_part=part)
    got = _output(c, before, after)
    _check(c, c.tile, got, p["acc"])
    plain = dataclasses.replace(c, stats=False)
    _, without = _launch(plain, p, gpu, monkeypatch, c.tile)
    _same_bits(c, after, without, "with statistics against without")
    assert torch.isnan(part[chunks * c.cout * 2:]).all() and not torch.isnan(part[:chunks * c.cout * 2]).any()
    st_a = torch.empty(c.cout * 2, device=gpu)
    st_b = torch.empty_like(st_a)
    hip.instnorm_finalize(part, 1, chunks, c.cout, hw, st_a)
    stored = got.cuda().contiguous().reshape(-1)
    ws = torch.empty(hip.instnorm_workspace_bytes(1, hw, c.cout) // 8 + 1, device=gpu, dtype=torch.float64)
    hip.instnorm_stats(stored, 1, hw, c.cout, st_b, ws)
    assert torch.allclose(st_a, st_b, rtol=2e-7, atol=1e-9), (st_a - st_b).abs().max().item()
    assert torch.allclose(st_a.view(c.cout, 2)[:, 0].cpu().double(), got.double().mean(0), rtol=1e-5, atol=1e-6)
