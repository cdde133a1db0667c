"""vfml/update_block.py is the one place the update block's launches stand (no GPU needed): MemFlow's volume geometry out of
the MOF engine's `_volume_geometry`, and each layer's launch in one launch site."""
import os

import pytest

VFML = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-flow-ml_amd", "vfml")


@pytest.mark.parametrize("H,W", [(128, 192), (256, 320), (1080, 1920)])
def test_memflow_takes_the_geometry_it_computed_by_hand(H, W):
    """Level sizes, tile counts and f32 row strides (whole 128-byte lines, an odd number of them) as forward_pairs spelled
    them out before it called _volume_geometry: host arithmetic only."""
    from vfml import hip
    from vfml.memflow_net import build_memflow_network, memflow_cfg
    cfg = memflow_cfg()
    net = build_memflow_network(cfg)
    L = cfg.corr_levels
    h, w = H // 8, W // 8
    hl, wl = [h], [w]
    for l in range(1, L):
        hl.append(hl[-1] // 2)
        wl.append(wl[-1] // 2)
    VT = net._tile()
    assert VT is not None
    Nl = [VT.count(hl[l], wl[l]) for l in range(L)]
    ldl = [(s + 31) // 32 * 32 for s in Nl]
    ldl = [n if (n // 32) % 2 else n + 32 for n in ldl]
    geo = net._volume_geometry(H, W, L, hip.FMT_S16)
    assert (geo.hl, geo.wl, geo.Sl) == (hl, wl, [hl[l] * wl[l] for l in range(L)])
    assert (geo.Nl, geo.Pv, geo.TILE, geo.ldl) == (Nl, Nl[0], VT.code, ldl)
    assert geo.psz == [Nl[0] * ldl[l] for l in range(L)]
    assert geo.VF == hip.FMT_F32 and geo.vol16 == 0            # corr_lookup's default volume format: what MemFlow passed


def _code(name):
    """The file's lines that are neither blank nor comments."""
    with open(os.path.join(VFML, name)) as f:
        return [ln for ln in f.read().split("\n") if ln.strip() and not ln.strip().startswith("#")]


# (vfml/torch_ops.py wraps single kernels as stand-alone operators, the lookup among them: no engine, no update block)
ENGINE_FILES = sorted(f for f in os.listdir(VFML) if f.endswith(".py") and f not in ("hip.py", "torch_ops.py"))


@pytest.mark.parametrize("needle,per_site", [("EPI_GRU_ZR", 1), ("EPI_GRU_Q", 1), ("transpose_to_s16(", 1), ('.tprop"]', 1),
                                             ('P[f"{UB}.flow_head.conv1"]', 1), ('P[f"{UB}.mask.0"]', 1),
                                             ('P[f"{UB}.encoder.convf2"]', 1), ("hip.corr_lookup(", 2)])
def test_one_launch_site_per_layer(needle, per_site):
    """Each of the update block's layers is launched from one function of update_block.py (the lookup: its list and its
    table form), and from no other engine file."""
    hits = {f: sum(ln.count(needle) for ln in _code(f)) for f in ENGINE_FILES}
    assert hits.pop("update_block.py") == per_site, needle
    assert not any(hits.values()), (needle, hits)
