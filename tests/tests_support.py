"""Helpers shared by the GPU test modules.

Noise-floor helpers (no GPU needed): the oracle in float64, the statistics of the difference of two flow fields
(`error_stats`), and the float32 oracle's own rounding noise against the float64 oracle on a given input (`noise_floor`,
"N").  The elementwise tests bound the engine's error by a fixed multiple of N computed for the very input they run:
nothing in a bound comes from the engine."""
import hashlib
import time

import numpy as np
import torch
import torch.nn.functional as F

EPE_TOL = 1e-3            # px: the mean-EPE tolerance of the older end-to-end tests (tests/test_gpu_e2e.py)
STAT_KEYS = ("mean", "p999", "max", "block", "ring")
K_OF = {"f32": 4.0, "f16x3": 8.0, "mixed": 8.0}     # engine error <= K x N, per statistic (fixed, not fitted)
# max / mean of the end-point deviation of the default mixed plan's oracle (float64) from the plain oracle: the largest
# value test_noise_floor.py measures on the CPU (3.56 at T3 128x128, 3.26 at T5 128x192), rounded up.  The shape of a
# field of rounding errors, taken from the reference side alone.
MIXED_MAX_OVER_MEAN_CPU = 4.0


def s16_decode(flat, rows, ld, c):
    """split rows (FMT_S16) device buffer -> f32 [rows, c] on the host."""
    u = flat.view(torch.float16).view(rows, ld // 8, 2, 8).float().cpu()
    return (u[:, :, 0] + u[:, :, 1]).reshape(rows, ld)[:, :c]


# ----------------------------------------------------------------------------- statistics of a field difference
def epe_map(got, ref):
    """[1, F, 2, H, W] x 2 -> float64 end-point error [F, H, W]."""
    return (got.double() - ref.double()).pow(2).sum(2).sqrt()[0]


def _stats_of_map(e, block, ring):
    H, W = e.shape
    flat = e.reshape(-1)
    k = max(1, int(np.ceil(0.999 * flat.numel())))
    # means over block x block tiles anchored at (0, 0); the ragged tiles of the last row / column are means over
    # the pixels they do have
    ph, pw = -H % block, -W % block
    s = F.avg_pool2d(F.pad(e[None, None], (0, pw, 0, ph)), block, divisor_override=1)
    cnt = F.avg_pool2d(F.pad(torch.ones_like(e)[None, None], (0, pw, 0, ph)), block, divisor_override=1)
    inner = torch.zeros_like(e, dtype=torch.bool)
    inner[ring:H - ring, ring:W - ring] = True
    outer = e[~inner]
    return {"mean": float(flat.mean()), "p999": float(flat.kthvalue(k).values), "max": float(flat.max()),
            "block": float((s / cnt).max()), "ring": float(outer.mean()) if outer.numel() else 0.0}


def error_stats(got, ref, block=64, ring=8):
    """Statistics of the end-point error between two stacks of flow fields [1, F, 2, H, W], in the fields' units:
    mean, 99.9th percentile and maximum; the worst mean over block x block tiles (ragged edge tiles included); the mean
    over the outer `ring` pixels.  Returns {"per_flow": [dict per flow], and each statistic's worst value over the flows}."""
    if got.shape != ref.shape or got.dim() != 5 or got.shape[0] != 1 or got.shape[2] != 2:
        raise ValueError(f"error_stats: two [1, F, 2, H, W] fields expected, got {tuple(got.shape)} / {tuple(ref.shape)}")
    per = [_stats_of_map(e, block, ring) for e in epe_map(got, ref)]
    out = {k: max(p[k] for p in per) for k in STAT_KEYS}
    out["per_flow"] = per
    return out


def low_stats(got, ref):
    """error_stats of 1/8-resolution fields (in cells): tiles of 8 x 8 cells and a one-cell ring - the same areas of the
    frame as 64 x 64 pixels and 8 pixels at full resolution."""
    return error_stats(got, ref, block=8, ring=1)


def engine_low(low):
    """The engine's low-resolution flows [M, h, w, 4] (forward xy | backward xy per cell) in the oracle's layout
    [1, 2M, 2, h, w] (forward flows first)."""
    f = low[..., 0:2].permute(0, 3, 1, 2)
    b = low[..., 2:4].permute(0, 3, 1, 2)
    return torch.cat([f, b], dim=0)[None]


def fmt_stats(s):
    return " ".join(f"{k} {s[k]:.2e}" for k in STAT_KEYS)


def assert_within(got, floor, K, what):
    """Every statistic of `got` at most K times the same statistic of `floor`; prints the ratios first.  Returns them."""
    ratios = {k: got[k] / floor[k] if floor[k] > 0 else (0.0 if got[k] == 0 else float("inf")) for k in STAT_KEYS}
    print(f"{what}: engine {fmt_stats(got)} | N {fmt_stats(floor)} | ratio " +
          " ".join(f"{k} {ratios[k]:.2f}" for k in STAT_KEYS) + f" (K = {K:g})")
    bad = {k: round(r, 2) for k, r in ratios.items() if not r <= K}
    assert not bad, f"{what}: above {K:g} x N in {bad}: engine {fmt_stats(got)} | N {fmt_stats(floor)}"
    return ratios


# ----------------------------------------------------------------------------- oracles and their noise floor
def oracle_cfg(**over):
    from oracle import mof_oracle as mo
    cfg = mo.get_cfg()
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def oracle_f32(cfg, state_dict):
    from oracle import mof_oracle as mo
    ora = mo.build_network(cfg)
    ora.load_state_dict(state_dict)
    return ora.eval()


def oracle_f64(cfg, state_dict):
    """The oracle in float64: same modules, parameters converted exactly; feed it a float64 tensor."""
    return oracle_f32(cfg, state_dict).double()


_PAIRS = {}


def _networks(cfg, state_dict, plan, corr_volume, builder, n):
    """n fresh float32 oracles (eval mode, weights loaded) from `builder`, a module with build_network: oracle.mof_oracle (the
    default), tests/mof_gma_oracle.py, tests/mof_sk_oracle.py, or oracle.plan_oracle (the default with a `plan`), whose
    build_network also takes the plan and the correlation volume's format."""
    from oracle import plan_oracle as po
    if builder is None:
        from oracle import mof_oracle as mo
        builder = mo if plan is None else po
    if builder is po:
        nets = [po.build_network(cfg, {} if plan is None else plan, corr_volume) for _ in range(n)]
    elif plan is not None:
        raise ValueError(f"{builder.__name__} builds no oracle of a plan: there is none for this variant")
    else:
        nets = [builder.build_network(cfg) for _ in range(n)]
    for net in nets:
        net.load_state_dict(state_dict)
        net.eval()
    return nets


def _key(x, cfg, state_dict, plan, corr_volume, builder):
    return (_digest(x), repr(sorted(vars(cfg).items())), _digest(*state_dict.values()),
            None if plan is None else repr(sorted((k, str(v)) for k, v in plan.items())), corr_volume,
            None if builder is None else builder.__name__)


def _digest(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(str(tuple(t.shape)).encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def oracle_pair(x, cfg, state_dict, plan=None, corr_volume="f32", builder=None):
    """The oracle's fields for frames x [1, T, 3, H, W] (float32) in float32 and in float64, computed once per session and
    input: {"f32": (flow, low), "f64": (flow, low), "seconds": (t32, t64)}.  With `plan` (an mfma_plan dict; {} counts) the
    oracle of that plan (oracle/plan_oracle.py) instead of the plain one; with `builder` (a module with build_network, see
    _networks) that variant's oracle."""
    key = _key(x, cfg, state_dict, plan, corr_volume, builder)
    ent = _PAIRS.get(key)
    if ent is None:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        nets = _networks(cfg, state_dict, plan, corr_volume, builder, 2)
        nets[1].double()
        ent, secs = {}, []
        for name, net, xin in (("f32", nets[0], x.float()), ("f64", nets[1], x.double())):
            t0 = time.time()
            ent[name] = net(xin, {}, return_lowres=True)
            secs.append(time.time() - t0)
        ent["seconds"] = tuple(secs)
        _PAIRS[key] = ent
    return ent


def noise_floor(x, cfg, state_dict, plan=None, corr_volume="f32", builder=None):
    """N: the statistics of the float32 oracle's field against the float64 oracle's, on input x.  Every bound of the
    elementwise tests is a multiple of this; nothing in it comes from the engine."""
    p = oracle_pair(x, cfg, state_dict, plan, corr_volume, builder)
    return error_stats(p["f32"][0], p["f64"][0])


def noise_floor_low(x, cfg, state_dict, plan=None, corr_volume="f32", builder=None):
    p = oracle_pair(x, cfg, state_dict, plan, corr_volume, builder)
    return low_stats(p["f32"][1], p["f64"][1])


# ----------------------------------------------------------------------------- large flow from the seeded weights
DRIFT_DIRECTION = (1.0, -0.5, -1.0, 0.75)       # forward x, forward y, backward x, backward y: cells per iteration and unit c
DRIFT_KEY = "update_block.flow_head.conv2.bias"
DRIFT_KEY_SK = "update_block.flow_head.ffn2.2.bias"     # the SK flow head is a PCBlock: its last 1x1's bias


def drift_state_dict(sd, c, key=DRIFT_KEY):
    """A copy of state dict `sd` whose flow head adds c * DRIFT_DIRECTION cells to the flow in every iteration: the seeded
    weights' own flow stays near one cell, with this the 1/8-resolution flow reaches about depth * c cells (forward and
    backward, x and y each another way).  `key` names the bias of the flow head's last convolution (DRIFT_KEY_SK for an SK
    checkpoint).  A bias of two entries (MemFlow's flow head: one flow) takes the first two components.  Every other entry is
    the same tensor's clone; oracle and engine load the same dict."""
    out = {k: v.clone() for k, v in sd.items()}
    b = out[key]
    if b.numel() not in (2, 4):
        raise ValueError(f"drift_state_dict: {key} has {b.numel()} entries, a flow head has 2 (one flow) or 4")
    # (MemFlow's flow head gives one flow: the forward components)
    out[key] = b + float(c) * torch.tensor(DRIFT_DIRECTION[:b.numel()], dtype=b.dtype, device=b.device)
    return out


_F64 = {}


def oracle_f64_fields(x, cfg, state_dict, plan=None, corr_volume="f32", builder=None):
    """(flow, low) of the float64 oracle alone - the plain one, with `plan` the plan oracle, with `builder` that variant's (see
    _networks) - for frames x [1, T, 3, H, W], computed once per session and input (half the work of oracle_pair where no
    float32 run is needed)."""
    key = _key(x, cfg, state_dict, plan, corr_volume, builder)
    ent = _F64.get(key)
    if ent is None and key in _PAIRS:          # (the same network on the same input: oracle_pair has run it already)
        ent = _F64[key] = _PAIRS[key]["f64"]
    if ent is None:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        net = _networks(cfg, state_dict, plan, corr_volume, builder, 1)[0].double()
        ent = _F64[key] = net(x.double(), {}, return_lowres=True)
    return ent


def plan_deviation(x, cfg, state_dict, plan, corr_volume="f32"):
    """error_stats of the plan oracle's field against the plain oracle's, both in float64: what the plan's roundings cost
    on this input with these weights, no engine involved.  Returns (stats, max |low| of the plain oracle in cells)."""
    ref, low = oracle_f64_fields(x, cfg, state_dict)
    got, _ = oracle_f64_fields(x, cfg, state_dict, plan, corr_volume)
    return error_stats(got, ref), float(low.abs().max())


# ----------------------------------------------------------------------------- the MemFlow oracles
# Another call shape than the MOF oracles': forward(pair) -> (low, flow), frames already in [-1, 1], a stream of fields
# through tests/memflow_memory_oracle.py.
_MEMFLOW = {}


def memflow_oracle_net(depth, state_dict, double=False):
    """oracle.memflow_oracle's network at `depth` iterations with `state_dict` loaded, eval mode; `double`: the same modules
    in float64 (parameters converted exactly; feed it float64 frames)."""
    from oracle import memflow_oracle as mm
    cfg = mm.get_cfg()
    cfg.decoder_depth = depth
    net = mm.build_network(cfg)
    net.load_state_dict(state_dict)
    net.eval()
    return net.double() if double else net


def memflow_stack(fields):
    """[(low [1, 2, h, w], flow [1, 2, H, W]) per field] -> (flow [1, F, 2, H, W], low [1, F, 2, h, w]): the layout of
    error_stats / low_stats, in oracle_pair's order."""
    return torch.stack([f[1][0] for f in fields])[None], torch.stack([f[0][0] for f in fields])[None]


def memflow_stream_fields(net, clip, M, alter=None):
    """The fields (i, i+1) of clip [1, F+1, 3, H, W] (in [-1, 1], the network's dtype) through ONE
    memflow_memory_oracle.Stream of capacity M (M = 0: MemFlowNetOracle.forward on every pair), stacked by memflow_stack.
    `alter`: applied to every field's attention rows [1, P, (n + 1) P] - the mutants of tests/test_memflow_noise_cpu.py."""
    import memflow_memory_oracle as mo
    st = mo.Stream(net, M, alter)
    return memflow_stack([st.step(clip[:, i:i + 2]) for i in range(clip.shape[1] - 1)])


def memflow_oracle_fields(clip, depth, state_dict, M):
    """The MemFlow oracle's fields of clip [1, F+1, 3, H, W] (float32, in [-1, 1]) through one stream of capacity M, in
    float32 and in float64 (the same modules and state dict, .double()), computed once per session and (clip, depth, weights,
    M): {"f32": (flow [1, F, 2, H, W], low [1, F, 2, h, w]), "f64": (flow, low), "seconds": (t32, t64)}."""
    key = (_digest(clip), int(depth), _digest(*state_dict.values()), int(M))
    ent = _MEMFLOW.get(key)
    if ent is None:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        ent, secs = {}, []
        for name, double in (("f32", False), ("f64", True)):
            net = memflow_oracle_net(depth, state_dict, double)
            t0 = time.time()
            ent[name] = memflow_stream_fields(net, clip.double() if double else clip.float(), M)
            secs.append(time.time() - t0)
        ent["seconds"] = tuple(secs)
        _MEMFLOW[key] = ent
    return ent


def field_of(t, f):
    """Field f of a stack [1, F, 2, H, W], as a stack of one."""
    return t[:, f:f + 1]


# ----------------------------------------------------------------------------- input kinds
INPUT_KINDS = ("rand", "clip", "letterbox", "patch", "black", "white")


def make_frames(kind, T, H, W, seed=0):
    """uint8 frames [T, H, W, 3] of one of INPUT_KINDS: uniform noise; the synthetic clip; the clip with 24 black rows
    at the top and the bottom; flat grey with one textured, moving 32 x 48 patch; all black; all white."""
    from vfml.synth import synthetic_clip
    if kind == "rand":
        g = torch.Generator().manual_seed(1000 * T + H + seed)
        return torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, generator=g)
    if kind in ("clip", "letterbox", "patch"):
        clip = torch.from_numpy(np.stack(synthetic_clip(T, H, W)))
        if kind == "letterbox":
            clip[:, :24] = 0
            clip[:, H - 24:] = 0
        if kind == "patch":
            flat = torch.full_like(clip, 128)
            for t in range(T):
                y, x = H // 2 - 16 + 2 * t, W // 2 - 24 - 3 * t
                flat[t, y:y + 32, x:x + 48] = clip[t, y:y + 32, x:x + 48]
            clip = flat
        return clip
    if kind in ("black", "white"):
        return torch.full((T, H, W, 3), 0 if kind == "black" else 255, dtype=torch.uint8)
    raise ValueError(kind)


def to_float_frames(u8):
    """uint8 [T, H, W, 3] -> float32 [1, T, 3, H, W] in [0, 1]: the reference's host-side conversion."""
    return (u8.float() / 255.0).permute(0, 3, 1, 2)[None].contiguous()
