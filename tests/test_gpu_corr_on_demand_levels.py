"""Pooled levels of the correlation pyramids on demand, in the level-0 pass (csrc/corr_ensure.hip, vfml_corr_levels_ensure;
DESIGN.md section 4b): ONE launch in front of a lookup computes, for every listed level, the 128 x 64 tiles of that level's
volumes that the lookup's windows read and that the level's bitmap does not have yet, instead of the level's dense GEMM.

Oracle: the dense GEMM of each level (hip.conv2d, the resident-A walk) on the same operands.  The pass runs the same walk
over chosen tiles, so every computed value must be the dense one bit for bit, and a lookup must not be able to tell the two
apart: its output over NaN-filled levels that only the pass wrote is BYTE-equal to its output over the dense volumes.

Geometry, in 4 x 8 tiles (hip.VolTile(2, 3): count(h, w) = ceil(h / 8) * ceil(w / 4) * 32):
  levels 0 + 1   query map 49 x 89: 5152 volume rows = 40.25 row tiles (the last one ragged), level 0 has 80.5 column tiles;
                 level 1 is 24 x 44: 1056 columns, just above the GEMM form's 1024, 16.5 column tiles (ragged)
  level 2 alone  query map 97 x 177: 18720 rows; level 2 is 24 x 44 again"""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, R, SC = 256, 4, 16.0
NAN_BITS = 0x7FC0BEEF      # the pattern an uncomputed texel holds


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tiled(y, x, w, tws=2, ths=3):
    """hip.VolTile.position / the kernels' tiled_at, on NumPy integers"""
    tpr = ((w - 1) >> tws) + 1
    return ((((y >> ths) * tpr + (x >> tws)) << (tws + ths)) + ((y & ((1 << ths) - 1)) << tws) + (x & ((1 << tws) - 1)))


class _Kernel:
    """Operands of `frames` frames for a query map H x W and the pyramid levels `levels` under test: the problems' dense
    volumes of those levels, NaN-filled twins with empty bitmaps, the pass's cells, and the window rule on the CPU."""

    def __init__(self, H, W, levels, problems, frames, seed):
        from vfml import hip
        g = torch.Generator().manual_seed(seed)
        self.H, self.W, self.levels, self.problems = H, W, levels, problems
        self.M = len(problems) // 2                                      # centres (direction-major problems)
        self.vt = vt = hip.VolTile(2, 3)
        self.hl, self.wl = [H >> l for l in range(4)], [W >> l for l in range(4)]
        self.Nl = [vt.count(self.hl[l], self.wl[l]) for l in range(4)]
        self.Pv, self.Pn = self.Nl[0], H * W
        self.mtiles = (self.Pv + 127) // 128
        self.ntiles = [(n + 63) // 64 for n in self.Nl]
        self.ld = [(n + 31) // 32 * 32 + 32 for n in self.Nl]
        self.scale = 1.0 / 16.0 / SC
        queries = {c for c, _ in problems}
        self.rows, self.planes = {}, {}
        for fr in range(frames):
            if fr in queries:
                f = torch.randn(self.Pn, D, generator=g).cuda()
                ft = vt.rows(f.reshape(-1), H, W, D)                     # tile order, zero rows where no cell lands
                r = torch.empty(self.Pv * D, device="cuda")
                hip.to_s16(ft * SC, self.Pv, D, D, r, D)
                self.rows[fr] = r
            for l in levels:                                             # (any values: the pooling is not under test)
                f = torch.randn(self.hl[l] * self.wl[l], D, generator=g).cuda()
                ft = vt.rows(f.reshape(-1), self.hl[l], self.wl[l], D)
                self.planes[fr, l] = hip.SplitWeight(self.Nl[l], D, torch.device("cuda")).fill(ft.contiguous(), scale=SC)
        self.dense = {}
        for i, (c, t) in enumerate(problems):
            for l in levels:
                v = torch.empty(self.Pv * self.ld[l], device="cuda")
                hip.conv2d(self.rows[c], D, D, 1, 1, self.Pv, self.planes[t, l], None, self.Nl[l], 1, 1, v, self.ld[l],
                           out_scale=self.scale, in_fmt=hip.FMT_S16, mfma=1)
                self.dense[i, l] = v
        self.words = [hip.corr_bitmap_words(self.Pv, self.Nl[l]) for l in levels]
        self.per = 1 + 3 * len(levels)
        self.counter = torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def sparse(self):
        """NaN-filled level buffers, one bitmap buffer per problem (a section per level), and the pass's cells"""
        from vfml import hip
        vols = {(i, l): torch.full((self.Pv * self.ld[l],), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
                for i in range(len(self.problems)) for l in self.levels}
        bits = [torch.zeros(sum(self.words), dtype=torch.int32, device="cuda") for _ in self.problems]
        cells = torch.zeros(64, dtype=torch.int64, device="cuda")
        ptrs = []
        for i, (c, t) in enumerate(self.problems):
            ptrs.append(self.rows[c])
            for j, l in enumerate(self.levels):
                ptrs += [self.planes[t, l].hi, vols[i, l], bits[i].data_ptr() + 4 * sum(self.words[:j])]
        hip.ptr_table_set(cells, ptrs)
        return vols, bits, cells

    def ensure(self, cells, coords, n=None, c0=0):
        """-> tiles computed per pyramid level"""
        from vfml import hip
        self.counter.zero_()
        c, t = self.problems[0]
        lv = [(l, self.planes[t, l], self.dense[0, l], self.Nl[l], self.ld[l], self.hl[l], self.wl[l]) for l in self.levels]
        hip.corr_levels_ensure(self.rows[c], D, self.Pv, lv, self.scale, cells[self.per * c0:], self.M if n is None else n, 2,
                               self.M, coords, c0 * self.Pn * 4, 4, 2, self.H, self.W, R, self.vt.code, counters=self.counter)
        return self.counter.tolist()

    def coords(self, seed):
        """[M * Pn][4] (forward x, y, backward x, y): the grid plus sub-cell flow; a block of queries displaced by about 12
        cells; windows that straddle every image edge (the border cells' own, and rows pushed out by up to 7 cells); queries
        far outside; a block on odd integers (level 1: floor(c / 2) of an odd number, of a negative odd number)."""
        H, W, M = self.H, self.W, self.M
        g = torch.Generator().manual_seed(seed)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        grid = torch.stack([xs, ys, xs, ys], -1).reshape(1, self.Pn, 4).repeat(M, 1, 1)
        c = grid + (torch.rand(M, self.Pn, 4, generator=g) - 0.5) * 3.0
        c = c.view(M, H, W, 4)
        m1 = M - 1
        c[0, 8:20, 10:24] += torch.tensor([12.3, -11.6, -12.7, 11.2])
        c[m1, 0:3, :, 1] -= 6.6                                # over the top edge
        c[m1, -3:, :, 3] += 7.4                                # over the bottom edge
        c[0, :, 0:2, 0] -= 5.5                                 # over the left edge
        c[0, :, -2:, 2] += 6.5                                 # over the right edge
        c[m1, 12, 5] = torch.tensor([1e6, 3.0, -1e6, 4.0])     # far outside
        c[m1, 13, 6] = torch.tensor([7.0, -1e6, 9.0, 1e6])
        c[0, 5, 30] = torch.tensor([-3.2, -2.1, W + 2.3, H + 1.7])    # window partly / wholly past a corner
        blk = grid.view(M, H, W, 4)[m1, 24:32, 40:56]
        c[m1, 24:32, 40:56] = torch.floor(blk / 2) * 2 + 1.0   # odd integers
        c[m1, 33:35, 0:4, 0] = -3.0                            # negative odd: -1.5 at level 1, floor -2
        c[m1, 33:35, 0:4, 3] = -5.0
        return c.reshape(-1).cuda().contiguous()

    def want_tiles(self, coords, l):
        """The window rule restated on the CPU: per problem the set of (row tile, column tile) its queries' level-l windows
        touch - the in-image part of the (2R+2)^2 integer grid from floor(coordinate * 2^-l) - R on."""
        H, W, M = self.H, self.W, self.M
        hl, wl = self.hl[l], self.wl[l]
        c = coords.cpu().view(M, H, W, 4).numpy() * np.float32(2.0 ** -l)
        org = np.clip(np.floor(c), -65536.0, 65536.0).astype(np.int64) - R
        want = [set() for _ in self.problems]
        for d in range(2):
            for m in range(M):
                for y in range(H):
                    for x in range(W):
                        x0, y0 = int(org[m, y, x, 2 * d]), int(org[m, y, x, 2 * d + 1])
                        xa, xb = max(x0, 0), min(x0 + 2 * R + 1, wl - 1)
                        ya, yb = max(y0, 0), min(y0 + 2 * R + 1, hl - 1)
                        if xa > xb or ya > yb:
                            continue
                        mt = int(_tiled(y, x, W)) >> 7
                        for ty in range(ya >> 3, (yb >> 3) + 1):           # the 4 x 8 texel tiles of the window
                            for tx in range(xa >> 2, (xb >> 2) + 1):
                                want[d * M + m].add((mt, int(_tiled(8 * ty, 4 * tx, wl)) >> 6))
        return want

    def marked(self, bits, l):
        j = self.levels.index(l)
        at, n = sum(self.words[:j]), self.words[j]
        out = []
        for b in bits:
            w = b[at:at + n].cpu().numpy().view(np.uint32).reshape(self.mtiles, -1)
            out.append({(mt, 32 * k + i) for mt in range(self.mtiles) for k in range(w.shape[1]) for i in range(32)
                        if (int(w[mt, k]) >> i) & 1})
        return out

    def check_volumes(self, vols, marked, l):
        """computed tiles hold the dense volume's bits, everything else - ragged edges and padding included - the pattern"""
        N = self.Nl[l]
        for i in range(len(self.problems)):
            a, b = _bits(vols[i, l]).view(self.Pv, self.ld[l]), _bits(self.dense[i, l]).view(self.Pv, self.ld[l])
            done = torch.zeros(self.mtiles, self.ntiles[l], dtype=torch.bool)
            for mt, ct in marked[i]:
                assert mt < self.mtiles and ct < self.ntiles[l]              # no bit at or beyond the tile counts
                done[mt, ct] = True
            done = done.cuda().repeat_interleave(128, 0).repeat_interleave(64, 1)[:self.Pv, :N]
            want = torch.where(done, b[:, :N], torch.full_like(b[:, :N], NAN_BITS))
            assert torch.equal(a[:, :N], want), (l, i)
            assert (a[:, N:] == NAN_BITS).all(), (l, i)


# ------------------------------------------------------------------------------- levels 0 and 1 in one launch
H1, W1, L = 49, 89, 4


class _Setup01(_Kernel):
    def __init__(self):
        from vfml.network import cor_pad
        # centre frames 1 and 2 of the frames 0 .. 3: problems f (1 -> 2, 2 -> 3) and b (1 -> 0, 2 -> 1)
        super().__init__(H1, W1, [0, 1], [(1, 2), (2, 3), (1, 0), (2, 1)], 4, 4200)
        assert self.Pv == 5152 and self.Nl[1] == 1056 and self.mtiles == 41 and self.ntiles[:2] == [81, 17]
        g = torch.Generator().manual_seed(4201)
        # levels 2 and 3: any values, the same buffers on both routes
        self.upper = [[torch.randn(self.Pv * self.ld[l], generator=g).cuda() for l in (2, 3)] for _ in self.problems]
        self.cor_p = cor_pad(L * (2 * R + 1) ** 2, True)

    def lookup(self, vols, coords):
        from vfml import hip
        tab = torch.zeros(64, dtype=torch.int64, device="cuda")
        hip.ptr_table_set(tab, [p for i in range(len(self.problems)) for p in [vols[i, 0], vols[i, 1]] + self.upper[i]])
        out = torch.zeros(self.M * self.Pn * 2 * self.cor_p, device="cuda")
        hip.corr_lookup(None, self.hl, self.wl, self.ld, R, self.Pn, coords, 0, 4, out, 0, 2 * self.cor_p, out_fmt=hip.FMT_S16,
                        table=tab, nmaps=self.M, vol_tile=self.vt.code, bidir=(2, self.cor_p, self.M))
        torch.cuda.synchronize()
        return out


@pytest.fixture(scope="module")
def setup01(gpu):
    return _Setup01()


def test_lookup_over_ensured_levels_is_byte_equal_to_the_dense_volumes(setup01):
    s = setup01
    coords = s.coords(7)
    ref = s.lookup(s.dense, coords)
    vols, bits, cells = s.sparse()
    n = s.ensure(cells, coords)
    got = s.lookup(vols, coords)
    assert torch.equal(_bits(got), _bits(ref))                  # both directions, both centres, every channel
    marked = {l: s.marked(bits, l) for l in (0, 1)}
    for l in (0, 1):
        total = len(s.problems) * s.mtiles * s.ntiles[l]
        assert n[l] == sum(len(m) for m in marked[l]) and 0 < n[l] < total // 2       # the pass is selective
        s.check_volumes(vols, marked[l], l)
    assert n[2] == 0 and n[3] == 0
    # the warm iteration 0 of the engine looks up the newest centre alone: its row range, on fresh buffers
    vols, bits, cells = s.sparse()
    n1 = s.ensure(cells, coords, n=1, c0=1)
    for l in (0, 1):
        m1 = s.marked(bits, l)
        assert not m1[0] and not m1[2] and m1[1] == marked[l][1] and m1[3] == marked[l][3]
        assert n1[l] == len(m1[1]) + len(m1[3])


def test_bitmaps_of_both_levels_follow_the_window_rule(setup01):
    s = setup01
    coords = s.coords(8)
    vols, bits, cells = s.sparse()
    first = s.ensure(cells, coords)
    for l in (0, 1):
        want = s.want_tiles(coords, l)
        assert s.marked(bits, l) == want and first[l] == sum(len(w) for w in want)
        share = first[l] / (len(s.problems) * s.mtiles * s.ntiles[l])
        print(f"level {l}: {first[l]} tiles, {100 * share:.1f} % of the dense volumes")
    assert s.ensure(cells, coords) == [0, 0, 0, 0]              # nothing new: the pass only checks
    got = s.lookup(vols, coords)
    assert torch.equal(_bits(got), _bits(s.lookup(s.dense, coords)))


# ------------------------------------------------------------------------------- level 2 alone
def test_level2_alone_over_a_larger_query_map(gpu):
    """Level set {2}: the rows' order is the 97 x 177 query map's, the windows lie around coordinate / 4 in the 24 x 44
    level image.  No lookup: level 0 of this map would be 1.4 GB per problem."""
    s = _Kernel(97, 177, [2], [(1, 2), (1, 0)], 3, 4300)
    assert s.Pv == 18720 and s.Nl[2] == 1056 and s.ntiles[2] == 17
    coords = s.coords(9)
    vols, bits, cells = s.sparse()
    n = s.ensure(cells, coords)
    marked = s.marked(bits, 2)
    want = s.want_tiles(coords, 2)
    assert marked == want and n == [0, 0, sum(len(w) for w in want), 0]
    assert 0 < n[2] < len(s.problems) * s.mtiles * s.ntiles[2]
    s.check_volumes(vols, marked, 2)
    assert s.ensure(cells, coords) == [0, 0, 0, 0]


def test_cell_table_of_a_five_frame_window_with_three_levels(gpu):
    """T = 5 with three on-demand levels names 2 x 3 x (1 + 3 x 3) = 60 cells, more than one vfml_ptr_table_set launch
    carries: hip.ptr_table_set writes them in several."""
    from vfml import hip
    vals = [0x1000 + 8 * i for i in range(60)]
    cells = torch.full((128,), -1, dtype=torch.int64, device="cuda")
    hip.ptr_table_set(cells, vals)
    assert cells[:60].tolist() == vals and (cells[60:] == -1).all()


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


def _job(net, clip, T):
    from processing.videoflow_processor import VideoFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        proc = VideoFlowProcessor("cuda", sequence_length=T)
    proc.core.model = net
    return [proc.compute_optical_flow_resident(clip, i).clone() for i in range(clip.shape[0])]


def _od_levels(net):
    """the on-demand level sets of the cached pyramids (the cache key's part in front of its "od" tail)"""
    keys = [k[1] for k in net._feat_cache if k[0] == "p"]
    assert keys and all(k[-1] == "od" for k in keys)
    return {k[-2] for k in keys}


_TILES = {}


@pytest.mark.parametrize("weights", ["seeded", "drift13"])
def test_sliding_job_with_level1_on_demand_is_byte_equal_to_the_dense_build(gpu, weights):
    """Six fields of a keyed sliding job at 480 x 608 px, T = 5, mixed plan: the 60 x 76 map's level 1 (30 x 38) has 1280
    columns and is on demand, its level 2 has 320 and stays dense.  The cold launch sequence runs eagerly, the warm one is
    captured with the pass in it and replayed.  drift13: the flow head adds a cell per iteration, flows of about 13 cells, so
    tiles keep being added in the later iterations (asserted: more level-1 tiles than the seeded job's)."""
    import tests_support as ts
    from vfml.synth import synthetic_clip
    from vfml.weights import seeded_state_dict
    sd = None if weights == "seeded" else (lambda cfg: ts.drift_state_dict(seeded_state_dict(cfg, 0), 1))
    clip = torch.from_numpy(np.stack(synthetic_clip(6, 480, 608))).cuda()
    net = _net(sd)
    assert net.corr_on_demand and 1 in net.corr_on_demand_levels
    got = _job(net, clip, 5)
    assert net.iter0_stats["cold"] >= 1 and net.iter0_stats["warm"] >= 3       # eager, captured, replayed
    warm = [v for k, v in net._graphs.items() if k[-1] is True and k[-3] is True]   # key: (..., warm, att_slots, on_demand)
    assert warm and isinstance(warm[0], torch.cuda.CUDAGraph)
    assert _od_levels(net) == {(0, 1)}
    tiles = net.corr_level_tiles_computed()
    net.corr_on_demand = False
    net.clear_feature_cache()
    ref = _job(net, clip, 5)
    assert net.corr_level_tiles_computed() == [0, 0, 0, 0]
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(_bits(a), _bits(b)), (weights, i)
    print(f"[{weights}] tiles computed over the job, per level: {tiles} (a dense pair has {60 * 120} and {60 * 20})")
    assert tiles[0] > 0 and tiles[1] > 0 and tiles[2] == 0 and tiles[3] == 0
    _TILES[weights] = tiles
    if weights == "drift13":
        assert tiles[1] > _TILES["seeded"][1]


def test_sliding_job_with_levels_1_and_2_on_demand_is_byte_equal_to_the_dense_build(gpu):
    """Four fields at 960 x 1216 px, T = 3: the 120 x 152 map's level 1 has 4864 columns, its level 2 (30 x 38) 1280 - all
    three f32 levels are on demand."""
    from vfml.synth import synthetic_clip
    clip = torch.from_numpy(np.stack(synthetic_clip(4, 960, 1216))).cuda()
    net = _net()
    net.corr_on_demand_levels = (1, 2)                          # (level 2 is not in the default set)
    got = _job(net, clip, 3)
    assert _od_levels(net) == {(0, 1, 2)}
    tiles = net.corr_level_tiles_computed(reset=False)
    assert net.corr_tiles_computed() == tiles[0]                # (the level-0 reading, as before)
    net.corr_on_demand = False
    net.clear_feature_cache()
    ref = _job(net, clip, 3)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(_bits(a), _bits(b)), i
    print(f"tiles computed over the job, per level: {tiles}")
    assert tiles[0] > 0 and tiles[1] > 0 and tiles[2] > 0 and tiles[3] == 0
