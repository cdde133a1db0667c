"""The engine with the lookup's patch cache (MOFNetHIP.lookup_cache) gives the fields of the uncached
lookup, bit for bit: a keyed sliding job at 240 x 304 px, T = 5, mixed plan, graph replay on.  The job runs twice with the
frame caches cleared in between: the cold launch sequence (every centre's iteration 0; the engine runs it eagerly, its
workspaces differ from the warm one's) runs twice, the warm one (the newest centre's iteration 0 alone: a lookup on a row
range) is captured and replayed, with the key reset inside the graph."""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIELDS = 6


def _bits(t):
    return t.contiguous().view(torch.int32)


def _net(sd, cache, count):
    from vfml import build_network, get_cfg
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    cfg.precision = "mixed"
    cfg.use_graph = True
    net = build_network(cfg)
    net.load_state_dict(sd(cfg) if sd is not None else seeded_state_dict(cfg, 0))
    net.cuda().eval()
    net.lookup_cache, net.lookup_cache_count = cache, count
    return net


def _job(net, clip, pick_only):
    from processing.videoflow_processor import VideoFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        proc = VideoFlowProcessor("cuda", sequence_length=5)
    proc.PICK_ONLY = pick_only
    proc.core.model = net
    return [proc.compute_optical_flow_resident(clip, i).clone() for i in range(clip.shape[0])]


def _twice(net, clip, pick_only):
    first = _job(net, clip, pick_only)
    net.clear_feature_cache()
    return first + _job(net, clip, pick_only)


@pytest.mark.parametrize("weights,pick_only,count", [("seeded", True, False), ("seeded", False, True), ("drift13", True, True)])
def test_sliding_job_is_byte_equal_to_the_uncached_lookup(gpu, weights, pick_only, count):
    """drift13: the flow head adds a cell per iteration, so windows keep moving and late iterations still miss."""
    import tests_support as ts
    from vfml.synth import synthetic_clip
    from vfml.weights import seeded_state_dict
    sd = None if weights == "seeded" else (lambda cfg: ts.drift_state_dict(seeded_state_dict(cfg, 0), 1))
    clip = torch.from_numpy(np.stack(synthetic_clip(FIELDS, 240, 304))).cuda()
    net = _net(sd, True, count)
    got = _twice(net, clip, pick_only)
    assert "lookup_patches" in net._ws and "lookup_keys" in net._ws                  # the cached launch did run
    assert net.iter0_stats["cold"] >= 2 and net.iter0_stats["warm"] >= 4
    # the warm sequence was captured and replayed; key: (..., warm, att_slots, on_demand)
    assert any(isinstance(g, torch.cuda.CUDAGraph) for k, g in net._graphs.items() if k[-3] is True)
    counts = net.lookup_cache_counts()
    ref_net = _net(sd, False, False)
    ref = _twice(ref_net, clip, pick_only)
    assert "lookup_patches" not in ref_net._ws
    assert len(got) == len(ref) == 2 * FIELDS
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(_bits(a), _bits(b)), (weights, pick_only, i)
    if count:
        print(f"[{weights}, pick_only={pick_only}] (hits, misses) per iteration over the job: {counts}")
        depth = net.cfg.decoder_depth
        assert len(counts) == depth and all(h + m > 0 for h, m in counts)
        assert counts[0][0] == 0                                 # the keys start every field empty
        if weights == "seeded":
            assert sum(h for h, _ in counts[2:]) > 0             # sub-cell updates: the windows stay where they were
        else:
            assert sum(m for _, m in counts[depth // 2:]) > 0    # real misses in late iterations
