"""The split-row convolution calls that pin conv_gemm_dma_kernel / conv_gemm_tapx_kernel to the tile shapes the 1080p engine
runs - one table, read by the CPU ledger (tests/test_conv_tile_coverage_cpu.py: which instantiation does each call become,
is every instantiation reached) and by the numeric tests (tests/test_gpu_conv_tiles.py: each call against float64 PyTorch).

The planner's cost model (csrc/conv_split_plan.hip) gives every problem of a few hundred pixels the 128 x 64 tile, so the
larger tiles are forced per call with VFML_DMA_TILE; the shapes are the smallest at which the kernels can still go wrong:

  pixels  (2, 13, 21) = 546 = 2 x 192 + 162 (5 slabs + 2 rows); (3, 9, 14) = 378, two image boundaries inside one tile;
          (1, 5, 7) = 35, less than one slab; (1, 40, 7) = 280, image rows far narrower than a slab.  None is a multiple of 32.
  cout    256; 260 (a 68-wide second 192-column tile, a 4-wide third 128-column tile); 196 (the last 8-channel unit is one
          quad); 136; 100; and 64 / 40, 96 / 72 on the 256 x 64 and 256 x 96 tiles of the shared-stage kernel.

Both readers build their calls with conv_args(); the ledger hands it made-up addresses (fake_buffers) and variant_only=True.
A new instantiation in DMA_VARIANTS / TAPX_VARIANTS comes with a case here: the ledger fails until one reaches it."""
import dataclasses
import itertools

T3222, T2322, T2222, T2241, T2341 = "3,2,2,2", "2,3,2,2", "2,2,2,2", "2,2,4,1", "2,3,4,1"
LARGE_TILES = (T3222, T2322, T2222)
PIXELS = ((2, 13, 21), (3, 9, 14), (1, 5, 7), (1, 40, 7))
COUTS = (256, 260, 196, 136, 100)

# the GRU state buffer of the engine (and of test_gru_epilogues_in_split_rows): [ z | r*h | h | x ] per pixel
STATE_LD, Z, RH, HH, X = 768, 0, 128, 256, 384
GUARD_ROWS = 3          # rows behind the last output row that must stay as they were


@dataclasses.dataclass(frozen=True)
class Case:
    group: str
    tile: str           # forced VFML_DMA_TILE, or None
    c0: int
    c1: int
    strides: int        # 1: both sources are channel slices of one buffer (one row stride); 2: rows of their own
    cout: int
    kh: int
    kw: int
    n: int
    H: int
    W: int
    stride: int = 1
    pad: tuple = None   # None: (kh // 2, kw // 2)
    korder: str = "cblock"      # "tap", "cblock", "cblock64"
    mfma: object = 3            # 3, 2, "2a", 1
    epi: str = "none"           # none relu tanh sigmoid tanh_relu add_aux gru_zr gru_q
    split: int = 0
    out_fmt: str = "f32"        # f32 / s16
    aux_fmt: str = "f32"
    addend: str = "none"        # none / direct / ind
    per_tap: bool = False
    stats: bool = False
    state: bool = False         # operands are slices of the GRU state buffer, the gate written in place
    kernel: str = None          # the kernel family this case is there for ("dma", "tapx"): the ledger asserts it

    @property
    def id(self):
        f = [self.group, self.tile.replace(",", "") if self.tile else "auto", f"{self.c0}+{self.c1}x{self.strides}",
             f"o{self.cout}", f"{self.kh}x{self.kw}s{self.stride}", f"n{self.n}x{self.H}x{self.W}", self.korder, f"m{self.mfma}",
             self.epi, self.out_fmt]
        if self.aux_fmt != "f32":
            f.append("aux" + self.aux_fmt)
        if self.addend != "none":
            f.append("add-" + self.addend)
        if self.per_tap:
            f.append("pertap")
        if self.stats:
            f.append("stats")
        return "-".join(f)


def tile_dims(tile):
    """(rows, columns) of a forced tile; the unforced 128 x 64 for None."""
    if tile is None:
        return 128, 64
    tm, tn, wm, wn = (int(v) for v in tile.split(","))
    return 32 * tm * wm, 32 * tn * wn


def geometry(c):
    """Derived sizes of a case: padding, output size, pixel counts, and every operand as (buffer, float offset, row stride)."""
    ph, pw = c.pad if c.pad is not None else (c.kh // 2, c.kw // 2)
    ho, wo = (c.H + 2 * ph - c.kh) // c.stride + 1, (c.W + 2 * pw - c.kw) // c.stride + 1
    P, M = c.n * c.H * c.W, c.n * ho * wo
    g = dict(ph=ph, pw=pw, ho=ho, wo=wo, P=P, M=M, sizes={})
    c8 = (c.cout + 7) // 8 * 8
    if c.state:
        assert P == M
        g["sizes"]["state"] = (P + GUARD_ROWS) * STATE_LD
        if c.epi == "gru_zr":
            g.update(in0=("state", HH, STATE_LD), in1=("state", X, STATE_LD), out=("state", Z, STATE_LD),
                     aux0=("state", HH, STATE_LD), aux1=None)
        else:
            g.update(in0=("state", RH, STATE_LD), in1=("state", X, STATE_LD), out=("state", HH, STATE_LD),
                     aux0=("state", Z, STATE_LD), aux1=("state", HH, STATE_LD))
    else:
        if c.strides == 1:
            ld = c.c0 + c.c1 + 64
            g.update(in0=("src", 32, ld), in1=("src", 32 + c.c0, ld) if c.c1 else None)
            g["sizes"]["src"] = P * ld
        else:
            ld0, ld1 = c.c0, c.c1 + 8
            g.update(in0=("src", 0, ld0), in1=("src", P * ld0, ld1) if c.c1 else None)
            g["sizes"]["src"] = P * (ld0 + (ld1 if c.c1 else 0))
        ldo = c8 + 8
        g["out"] = ("out", 0, ldo)
        g["sizes"]["out"] = (M + GUARD_ROWS) * ldo
        g["aux0"] = g["aux1"] = None
        naux = {"add_aux": 1, "gru_zr": 1, "gru_q": 2}.get(c.epi, 0)
        if naux:
            lda = c8 + 16
            g["aux0"] = ("aux", 8, lda)
            if naux == 2:
                g["aux1"] = ("aux", 8 + M * lda, lda)
            g["sizes"]["aux"] = 8 + naux * M * lda
    g["addend"] = None
    if c.addend != "none":
        lda = c.cout + 12
        g["addend"] = ("addend", 4, lda)           # wider than cout, a non-zero offset
        g["sizes"]["addend"] = 4 + M * lda
    if c.stats:
        g["chunks"] = (ho * wo + 31) // 32          # hip.STATS_ROWS_S16
    return g


def conv_args(c, bufs, weight, bias, *, per_tap=None, addend=None, stats_part=None, addend_ind=None, variant_only=False):
    """(args, kwargs) of the hip.conv2d call of case `c` over the buffers `bufs` (name -> flat f32 tensor).  `addend`
    overrides c.addend ("none" / "direct" / "ind": with "ind" the descriptor's own addend field names bufs["decoy"], the
    pointer that counts sits in the cell addend_ind = (table, entry))."""
    from vfml import hip
    g = geometry(c)
    fmt = {"f32": hip.FMT_F32, "s16": hip.FMT_S16}
    epi = {"none": hip.EPI_NONE, "relu": hip.EPI_RELU, "tanh": hip.EPI_TANH, "sigmoid": hip.EPI_SIGMOID,
           "tanh_relu": hip.EPI_TANH_RELU, "add_aux": hip.EPI_ADD_AUX, "gru_zr": hip.EPI_GRU_ZR, "gru_q": hip.EPI_GRU_Q}[c.epi]
    b0, o0, ld0 = g["in0"]
    bo, oo, ldo = g["out"]
    args = (bufs[b0], c.c0, ld0, c.n, c.H, c.W, weight, bias, c.cout, c.kh, c.kw, bufs[bo], ldo)
    kw = dict(stride=c.stride, pad_h=g["ph"], pad_w=g["pw"], in0_off=o0, out_off=oo, epilogue=epi, split=c.split,
              in_fmt=hip.FMT_S16, out_fmt=fmt[c.out_fmt], aux_fmt=fmt[c.aux_fmt], mfma=c.mfma,
              per_tap=c.per_tap if per_tap is None else per_tap, variant_only=variant_only)
    if g["in1"]:
        b1, o1, ld1 = g["in1"]
        kw.update(in1=bufs[b1], c1=c.c1, ld1=ld1, in1_off=o1)
    for k in ("aux0", "aux1"):
        if g[k]:
            ba, oa, lda = g[k]
            kw.update({k: bufs[ba], "ld_" + k: lda, k + "_off": oa})
    mode = c.addend if addend is None else addend
    if mode != "none":
        ba, oa, lda = g["addend"]
        kw.update(addend=bufs["decoy" if mode == "ind" else ba], ld_addend=lda, addend_off=oa)
        if mode == "ind":
            kw.update(addend_ind=addend_ind)
    if c.stats:
        kw.update(stats_part=stats_part)
    return args, kw


def k_order(c):
    from vfml import hip
    return {"tap": hip.KORDER_TAP, "cblock": hip.KORDER_CBLOCK, "cblock64": hip.KORDER_CBLOCK64}[c.korder]


# -- made-up operands for the ledger: the library compares addresses and checks their alignment, nothing more ----------------
class FakeTensor:
    """Stands where hip.conv2d expects a flat device tensor: an address, never followed."""
    is_cuda = True

    def __init__(self, address, dtype=None):
        import torch
        self._address, self.dtype = address, dtype or torch.float32

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self._address


def fake_buffers(c):
    """(bufs, weight, bias, stats_part, addend_ind) of case `c` at made-up 32-byte aligned addresses: each buffer name in
    its own 256 MiB window, the two weight planes in one."""
    import torch
    from vfml import hip
    names = ["src", "out", "aux", "addend", "decoy", "state"]
    bufs = {nm: FakeTensor(0x10000000 * (i + 1)) for i, nm in enumerate(names)}
    ctot, taps = c.c0 + c.c1, c.kh * c.kw
    w = object.__new__(hip.SplitWeight)
    w.rows, w.k, w.scale, w.order = c.cout, taps * ctot, 1.0, k_order(c)
    w.kp = {"tap": (taps * ctot + 31) // 32 * 32, "cblock": taps * ((ctot + 31) // 32 * 32), "cblock64": taps * ctot}[c.korder]
    w.hi = FakeTensor(0x90000000, torch.float16)
    w.lo = FakeTensor(0x90000000 + 2 * c.cout * w.kp, torch.float16)
    return bufs, w, FakeTensor(0xA0000000), FakeTensor(0xB0000000, torch.float64), (FakeTensor(0xC0000000, torch.int64), 1)


def planned_variant(c):
    """Name of the kernel the library plans for case `c` (with c.tile forced by the caller's environment): no GPU."""
    from vfml import hip
    bufs, w, bias, stats, ind = fake_buffers(c)
    args, kw = conv_args(c, bufs, w, bias, stats_part=stats, addend_ind=ind, variant_only=True)
    return hip.conv2d(*args, **kw)


# -- the table -------------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    px = itertools.cycle(PIXELS)
    co = itertools.cycle(COUTS)

    def add(group, tile, c0, c1, strides, cout, kh, kw, shape=None, **kwargs):
        n, H, W = shape or next(px)
        out.append(Case(group, tile, c0, c1, strides, cout, kh, kw, n, H, W, **kwargs))

    # Loaders and products: the uniform-step loader (channel-block order, one row stride) and the general loader (tap
    # order over channel counts off the 32-channel grid, or two row strides) x 3, 2, "2a", 1 MFMAs per product x taps.
    # 96 channels: whole 32-channel blocks (uniform steps) but no whole 64-channel ones, so mfma = 1 stays NM 1 - the
    # 64-channel steps (NM 5) come with the cblock64 rows behind.
    for tile in LARGE_TILES:
        for mfma in (3, 2, "2a", 1):
            for kh, kw in ((3, 3), (5, 1), (1, 5), (1, 1)):
                add("uniform", tile, 64, 32, 1, next(co), kh, kw, mfma=mfma, per_tap=kw > 1 and mfma == 3, kernel="dma")
                if (kh, kw) == (1, 1):
                    add("general", tile, 72, 0, 1, next(co), kh, kw, korder="tap", mfma=mfma, kernel="dma")
                else:
                    add("general", tile, 32, 64, 2, next(co), kh, kw, korder="tap" if kh == 3 else "cblock", mfma=mfma,
                        kernel="dma")
        for kh, kw in ((3, 3), (5, 1), (1, 1)):
            add("steps64", tile, 64, 64, 1, next(co), kh, kw, korder="cblock64" if kh * kw > 1 else "tap", mfma=1,
                per_tap=kh == 3, kernel="dma")
    # Stride 2: 3x3 and 1x1 on both loaders (a strided 1x1 is not the GEMM-rows case)
    for tile in LARGE_TILES:
        for kh in (3, 1):
            add("stride2", tile, 96, 0, 1, next(co), kh, kh, stride=2, kernel="dma")
            add("stride2", tile, 72, 0, 1, next(co), kh, kh, stride=2, korder="tap", kernel="dma")
    # The shared-stage kernel: ReLU into split rows; every case also runs with per_tap and must be bit-identical.
    # (2x4: padding 1 / 2 on an even filter is not "same" - the per-tap kernel in both runs)
    for tile, couts in ((T3222, (256, 196)), (T2322, (260, 136)), (T2241, (64, 40)), (T2341, (96, 72))):
        cc = itertools.cycle(couts)
        for mfma in (3, 1):
            for kh, kw in ((1, 5), (3, 3), (2, 4), (1, 3)):
                add("shared", tile, 64, 64, 1, next(cc), kh, kw, korder="cblock64" if mfma == 1 else "cblock", mfma=mfma,
                    epi="relu", out_fmt="s16", kernel="dma" if kh == 2 else "tapx")
    # GRU gates as the engine issues them: the state buffer in split rows, gates written in place; 1x5 on the shared-stage
    # kernel under 192 x 128 / 128 x 192, 5x1 on the per-tap kernel; without addend, with one, and with it behind addend_ind
    for tile in LARGE_TILES:
        for kh, kw in ((1, 5), (5, 1)):
            for mfma in (3, 1):
                for gate, cout in (("gru_zr", 256), ("gru_q", 128)):
                    shape = next(px)
                    for addend in ("none", "direct", "ind"):
                        add("gate", tile, 128, 384, 1, cout, kh, kw, shape=shape, korder="cblock64" if mfma == 1 else "cblock",
                            mfma=mfma, epi=gate, split=128 if gate == "gru_zr" else 0, out_fmt="s16", aux_fmt="s16",
                            addend=addend, state=True, kernel="tapx" if kw == 5 and tile != T2222 else "dma")
        # the general epilogue's gates: f32 aux operands, a z / r*h boundary off the 8-channel grid
        for kh, kw in ((1, 5), (5, 1)):
            add("gate-ragged", tile, 64, 32, 1, 132, kh, kw, epi="gru_zr", split=68, addend="direct")
            add("gate-ragged", tile, 64, 32, 1, 132, kh, kw, epi="gru_q", addend="direct")
    # The other epilogues on the large tiles (all of them the general epilogue_rows)
    for tile in LARGE_TILES:
        for out_fmt in ("f32", "s16"):
            add("epilogue", tile, 64, 32, 1, 256, 3, 3, epi="tanh_relu", split=128, out_fmt=out_fmt, per_tap=out_fmt == "f32")
            add("epilogue", tile, 72, 0, 1, next(co), 3, 3, korder="tap", epi="add_aux", out_fmt=out_fmt, aux_fmt="s16")
            add("epilogue", tile, 64, 32, 1, next(co), 1, 1, epi="tanh", out_fmt=out_fmt)
            add("epilogue", tile, 32, 64, 2, next(co), 5, 1, epi="sigmoid", out_fmt=out_fmt)
    # stats_part on forced tiles: one image, so no 32-pixel block straddles two
    for tile, cout in ((T3222, 196), (T2322, 260), (T2222, 136)):
        for per_tap in (False, True):
            add("stats", tile, 64, 0, 1, cout, 3, 3, shape=(1, 5, 7) if per_tap and tile == T2222 else (1, 40, 7), per_tap=per_tap, stats=True,
                kernel="dma" if per_tap or tile == T2222 else "tapx")
    add("stats", T2241, 64, 0, 1, 40, 3, 3, shape=(1, 40, 7), stats=True, kernel="tapx")
    add("stats", T2341, 64, 0, 1, 72, 3, 3, shape=(1, 5, 7), stats=True, kernel="tapx")
    # What the planner picks by itself at these sizes: 128 x 64 tiles (128 x 32 up to 32 output channels)
    for mfma in (3, 2, "2a", 1):
        add("auto", None, 64, 32, 1, next(co), 3, 3, mfma=mfma)
        add("auto", None, 72, 0, 1, 64, 3, 3, korder="tap", mfma=mfma)
        add("auto", None, 64, 32, 1, 20, 3, 3, mfma=mfma)
    add("auto", None, 64, 64, 1, 40, 5, 1, korder="cblock64", mfma=1)
    add("auto", None, 128, 384, 1, 256, 1, 5, mfma=3)      # the gate shape: no shared stage by itself at this size
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)
