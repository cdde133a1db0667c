"""Level 0 of the correlation pyramids on demand (csrc/corr_ensure.hip, vfml_corr_level0_ensure):
the pass in front of a lookup computes the 128 x 64 tiles of the level-0 volumes that the lookup's windows read and that
a pair's bitmap does not have yet, instead of the dense level-0 GEMM.

Oracle: the dense GEMM (hip.conv2d, the resident-A walk) on the same operands.  The pass runs the same walk over chosen
tiles, so every computed value must be the dense one bit for bit, and a lookup must not be able to tell the two apart:
its output over a NaN-filled level 0 that only the pass wrote is BYTE-equal to its output over the dense volume.

Geometry of the kernel tests: a 30 x 38 feature map, in 4 x 8 tiles 32 x 40 = 1280 volume rows and columns (just above
the GEMM form's 1024): 10 row tiles of 128, 20 column tiles of 64; the height is no multiple of 8 and the width none of 4,
so both tile edges carry rows and columns that no cell owns."""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, D, R, L = 30, 38, 256, 4, 4
M = 2                      # centre frames 1 and 2 of the frames 0 .. 3: problems f (1 -> 2, 2 -> 3) and b (1 -> 0, 2 -> 1)
SC = 16.0
NAN_BITS = 0x7FC0BEEF      # the pattern an uncomputed level-0 texel holds


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tiled(y, x, w, tws=2, ths=3):
    """hip.VolTile.position / the kernels' tiled_at, on NumPy integers"""
    tpr = ((w - 1) >> tws) + 1
    return ((((y >> ths) * tpr + (x >> tws)) << (tws + ths)) + ((y & ((1 << ths) - 1)) << tws) + (x & ((1 << tws) - 1)))


class _Setup:
    """Four frames' operands, the four problems' dense level 0, shared levels 1-3, and the device tables of both routes."""

    def __init__(self, gpu):
        from vfml import hip
        from vfml.network import cor_pad
        g = torch.Generator().manual_seed(4100)
        self.vt = vt = hip.VolTile(2, 3)
        self.hl, self.wl = [H, H // 2, H // 4, H // 8], [W, W // 2, W // 4, W // 8]
        self.Nl = [vt.count(self.hl[l], self.wl[l]) for l in range(L)]
        self.Pv, self.Pn = self.Nl[0], H * W
        assert self.Pv == 1280 and self.Pv >= 1024                       # the GEMM form, 10 x 20 tiles
        self.mtiles, self.ntiles = self.Pv // 128, self.Pv // 64
        self.ld = [(n + 31) // 32 * 32 + 32 for n in self.Nl]
        self.scale = 1.0 / 16.0 / SC
        self.rows, self.planes = [], []
        for _ in range(4):
            f = torch.randn(self.Pn, D, generator=g).cuda()
            ft = vt.rows(f.reshape(-1), H, W, D)                         # tile order, zero rows where no cell lands
            r = torch.empty(self.Pv * D, device="cuda")
            hip.to_s16(ft * SC, self.Pv, D, D, r, D)
            self.rows.append(r)
            self.planes.append(hip.SplitWeight(self.Pv, D, torch.device("cuda")).fill(ft.contiguous(), scale=SC))
        self.problems = [(1, 2), (2, 3), (1, 0), (2, 1)]                 # (query frame, target frame): direction-major
        # levels 1-3: any values, the same buffers on both routes (level 0 alone is under test)
        self.upper = [[torch.randn(self.Pv * self.ld[l], generator=g).cuda() for l in range(1, L)] for _ in self.problems]
        self.dense = []
        for c, t in self.problems:
            v = torch.empty(self.Pv * self.ld[0], device="cuda")
            hip.conv2d(self.rows[c], D, D, 1, 1, self.Pv, self.planes[t], None, self.Pv, 1, 1, v, self.ld[0],
                       out_scale=self.scale, in_fmt=hip.FMT_S16, mfma=1)
            self.dense.append(v)
        self.cor_p = cor_pad(L * (2 * R + 1) ** 2, True)
        self.counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def sparse(self):
        """NaN-filled level-0 buffers with empty bitmaps, and the pass's cells"""
        from vfml import hip
        lvl0 = [torch.full((self.Pv * self.ld[0],), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
                for _ in self.problems]
        bits = [torch.zeros(hip.corr_bitmap_words(self.Pv, self.Pv), dtype=torch.int32, device="cuda") for _ in self.problems]
        cells = torch.zeros(64, dtype=torch.int64, device="cuda")
        hip.ptr_table_set(cells, [p for i, (c, t) in enumerate(self.problems)
                                  for p in (self.rows[c], self.planes[t].hi, lvl0[i], bits[i])])
        return lvl0, bits, cells

    def ensure(self, cells, coords, n=M, c0=0):
        from vfml import hip
        self.counter.zero_()
        hip.corr_level0_ensure(self.rows[1], D, self.planes[2], self.dense[0], self.Pv, self.Pv, self.ld[0], self.scale,
                               cells[4 * c0:], n, 2, M, coords, c0 * self.Pn * 4, 4, 2, H, W, R, self.vt.code, counter=self.counter)
        return int(self.counter.item())

    def lookup(self, level0, coords):
        from vfml import hip
        tab = torch.zeros(64, dtype=torch.int64, device="cuda")
        hip.ptr_table_set(tab, [p for i in range(len(self.problems)) for p in [level0[i]] + self.upper[i]])
        out = torch.zeros(M * self.Pn * 2 * self.cor_p, device="cuda")
        hip.corr_lookup(None, self.hl, self.wl, self.ld, R, self.Pn, coords, 0, 4, out, 0, 2 * self.cor_p, out_fmt=hip.FMT_S16,
                        table=tab, nmaps=M, vol_tile=self.vt.code, bidir=(2, self.cor_p, M))
        torch.cuda.synchronize()
        return out

    def coords(self, seed=7):
        """[M * Pn][4] (forward x, y, backward x, y): the grid plus sub-cell flow; a block of queries displaced by about 12
        cells; windows that straddle every image edge (the border cells' own, and rows pushed out by up to 7 cells); queries
        far outside."""
        g = torch.Generator().manual_seed(seed)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        grid = torch.stack([xs, ys, xs, ys], -1).reshape(1, self.Pn, 4).repeat(M, 1, 1)
        c = grid + (torch.rand(M, self.Pn, 4, generator=g) - 0.5) * 3.0
        c = c.view(M, H, W, 4)
        c[0, 8:20, 10:24] += torch.tensor([12.3, -11.6, -12.7, 11.2])
        c[1, 0:3, :, 1] -= 6.6                                 # over the top edge
        c[1, -3:, :, 3] += 7.4                                 # over the bottom edge
        c[0, :, 0:2, 0] -= 5.5                                 # over the left edge
        c[0, :, -2:, 2] += 6.5                                 # over the right edge
        c[1, 12, 5] = torch.tensor([1e6, 3.0, -1e6, 4.0])      # far outside
        c[1, 13, 6] = torch.tensor([7.0, -1e6, 9.0, 1e6])
        c[0, 5, 30] = torch.tensor([-3.2, -2.1, W + 2.3, H + 1.7])    # window partly / wholly past a corner
        return c.reshape(-1).cuda().contiguous()

    def want_tiles(self, coords):
        """The window rule restated on the CPU: per problem the set of (row tile, column tile) its queries' level-0 windows
        touch - the in-image part of the (2R+2)^2 integer grid from floor(coordinate) - R on."""
        c = coords.cpu().view(M, H, W, 4).numpy()
        want = [set() for _ in self.problems]
        for d in range(2):
            for m in range(M):
                for y in range(H):
                    for x in range(W):
                        x0 = int(np.clip(np.floor(c[m, y, x, 2 * d]), -65536.0, 65536.0)) - R
                        y0 = int(np.clip(np.floor(c[m, y, x, 2 * d + 1]), -65536.0, 65536.0)) - R
                        xa, xb = max(x0, 0), min(x0 + 2 * R + 1, W - 1)
                        ya, yb = max(y0, 0), min(y0 + 2 * R + 1, H - 1)
                        mt = int(_tiled(y, x, W)) >> 7
                        if xa > xb or ya > yb:
                            continue
                        for ty in range(ya >> 3, (yb >> 3) + 1):           # the 4 x 8 texel tiles of the window
                            for tx in range(xa >> 2, (xb >> 2) + 1):
                                want[d * M + m].add((mt, int(_tiled(8 * ty, 4 * tx, W)) >> 6))
        return want

    def marked(self, bits):
        out = []
        for b in bits:
            w = b.cpu().numpy().view(np.uint32).reshape(self.mtiles, -1)
            out.append({(mt, 32 * k + j) for mt in range(self.mtiles) for k in range(w.shape[1]) for j in range(32)
                        if (int(w[mt, k]) >> j) & 1})
        return out


@pytest.fixture(scope="module")
def setup(gpu):
    return _Setup(gpu)


def test_lookup_over_ensured_tiles_is_byte_equal_to_the_dense_volume(setup):
    s = setup
    coords = s.coords()
    ref = s.lookup(s.dense, coords)
    lvl0, bits, cells = s.sparse()
    n = s.ensure(cells, coords)
    got = s.lookup(lvl0, coords)
    assert torch.equal(_bits(got), _bits(ref))                  # both directions, both centres, every channel
    # what was computed is the dense volume's bits; everything else still holds the pattern
    marked = s.marked(bits)
    assert n == sum(len(m) for m in marked) and 0 < n < len(s.problems) * s.mtiles * s.ntiles
    for i in range(len(s.problems)):
        a, b = _bits(lvl0[i]).view(s.Pv, s.ld[0]), _bits(s.dense[i]).view(s.Pv, s.ld[0])
        done = torch.zeros(s.mtiles, s.ntiles, dtype=torch.bool)
        for mt, ct in marked[i]:
            done[mt, ct] = True
        done = done.cuda().repeat_interleave(128, 0).repeat_interleave(64, 1)
        assert torch.equal(a[:, :s.Pv][done], b[:, :s.Pv][done])
        assert (a[:, :s.Pv][~done] == NAN_BITS).all() and (a[:, s.Pv:] == NAN_BITS).all()
    # the warm iteration 0 of the engine looks up the newest centre alone: its row range, on fresh buffers
    lvl0, bits, cells = s.sparse()
    n1 = s.ensure(cells, coords, n=1, c0=1)
    m1 = s.marked(bits)
    assert not m1[0] and not m1[2] and m1[1] == marked[1] and m1[3] == marked[3] and n1 == len(m1[1]) + len(m1[3])


def test_bookkeeping_of_the_bitmap(setup):
    s = setup
    coords = s.coords(seed=8)
    lvl0, bits, cells = s.sparse()
    first = s.ensure(cells, coords)
    want = s.want_tiles(coords)
    assert s.marked(bits) == want and first == sum(len(w) for w in want)
    assert s.ensure(cells, coords) == 0                         # nothing new: the pass only checks
    # one block of centre 0's queries moves by 9 cells: only its row tiles gain tiles, exactly the new windows'
    moved = coords.clone().view(M, H, W, 4)
    moved[0, 16:24, 4:20, 0] += 9.0
    moved[0, 16:24, 4:20, 3] -= 9.0
    moved = moved.reshape(-1).contiguous()
    rows = {int(_tiled(y, x, W)) >> 7 for y in range(16, 24) for x in range(4, 20)}
    added = s.ensure(cells, moved)
    now, want2 = s.marked(bits), s.want_tiles(moved)
    assert added > 0 and added == sum(len(a - b) for a, b in zip(now, want))
    for i, (a, b) in enumerate(zip(now, want)):
        assert a == b | want2[i]
        assert {mt for mt, _ in a - b} <= (rows if i in (0, 2) else set())
    got = s.lookup(lvl0, moved)
    assert torch.equal(_bits(got), _bits(s.lookup(s.dense, moved)))
    for b in bits:
        b.zero_()
    assert s.ensure(cells, coords) == first


# ---------------------------------------------------------------------------------------------- the engine
def _net(sd=None, **over):
    from vfml import build_network, get_cfg
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    cfg.precision = "mixed"
    for k, v in over.items():
        setattr(cfg, k, v)
    net = build_network(cfg)
    net.load_state_dict(sd(cfg) if sd is not None else seeded_state_dict(cfg, 0))
    net.cuda().eval()
    return net


def _job(net, clip, T=5):
    from processing.videoflow_processor import VideoFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        proc = VideoFlowProcessor("cuda", sequence_length=T)
    proc.core.model = net
    return [proc.compute_optical_flow_resident(clip, i).clone() for i in range(clip.shape[0])]


_TILES = {}


@pytest.mark.parametrize("weights", ["seeded", "drift13"])
def test_sliding_job_is_byte_equal_to_the_dense_build(gpu, weights):
    """Eight fields of a keyed sliding job at 240 x 304 px, T = 5, mixed plan: pyramid buffers are recycled (asserted: more
    pyramids are built than buffer sets handed out), the cold launch sequence runs (eagerly) and the warm one is captured
    and replayed (asserted on the engine's window statistics and graph table).  drift13: the flow head adds a cell per iteration, flows
    of about 13 cells, so tiles keep being added in the later iterations (asserted: more tiles than the seeded job's)."""
    import tests_support as ts
    from vfml.synth import synthetic_clip
    from vfml.weights import seeded_state_dict
    sd = None if weights == "seeded" else (lambda cfg: ts.drift_state_dict(seeded_state_dict(cfg, 0), 1))
    clip = torch.from_numpy(np.stack(synthetic_clip(8, 240, 304))).cuda()
    net = _net(sd)
    assert net.corr_on_demand
    handed, inner = [], net._pyramid_buffers

    def counting(sizes, dev, limit):
        bufs = inner(sizes, dev, limit)
        handed.append(bufs[0].data_ptr())
        return bufs
    net._pyramid_buffers = counting
    got = _job(net, clip)
    net._pyramid_buffers = inner
    assert len(handed) > 8 and len(set(handed)) < len(handed)             # (8: the cache's limit at T = 5) recycled buffers
    # the cold launch sequence ran (window 0), the warm one was captured with the passes in it and replayed
    assert net.iter0_stats["cold"] >= 1 and net.iter0_stats["warm"] >= 3
    warm = [v for k, v in net._graphs.items() if k[-1] is True and k[-3] is True]   # key: (..., warm, att_slots, on_demand)
    assert warm and isinstance(warm[0], torch.cuda.CUDAGraph)
    tiles = net.corr_tiles_computed()
    pairs = sum(1 for k in net._feat_cache if k[0] == "p")
    assert pairs and all(k[1][-1] == "od" for k in net._feat_cache if k[0] == "p")        # the job did run on demand
    net.corr_on_demand = False
    net.clear_feature_cache()
    ref = _job(net, clip)
    assert net.corr_tiles_computed() == 0
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(_bits(a), _bits(b)), (weights, i)
    print(f"[{weights}] level-0 tiles computed over the job: {tiles} (a dense pair has {10 * 20})")
    assert tiles > 0
    _TILES[weights] = tiles
    if weights == "drift13":
        assert tiles > _TILES["seeded"]
