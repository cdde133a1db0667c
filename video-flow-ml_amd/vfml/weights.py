"""Parameter table of the MOF network, seeded checkpoints, and NHWC weight packing.

The reference loads `VideoFlow_ckpt/{ARCH}_{dataset}[_288960noise].pth` with
`torch.load` + strict `load_state_dict` after stripping a `module.` prefix
(processing/videoflow_core.py:79-85,104-110).  The published checkpoints are not available
(.MISSING_LARGE_BLOBS), so `write_seeded_checkpoint` produces a deterministic stand-in with the
same file name and key layout (`fnet.*`, `cnet.*`, `update_block.{encoder,tprop,gru,flow_head,mask}.*`).
"""
import math
import os

import torch


def _encoder_spec(prefix, out_dim):
    s = [(f"{prefix}.conv1", 64, 3, 7, 7)]
    cin = 64
    for li, (planes, stride) in enumerate([(64, 1), (96, 2), (128, 2)], start=1):
        for bi in range(2):
            st = stride if bi == 0 else 1
            s.append((f"{prefix}.layer{li}.{bi}.conv1", planes, cin, 3, 3))
            s.append((f"{prefix}.layer{li}.{bi}.conv2", planes, planes, 3, 3))
            if st != 1:
                s.append((f"{prefix}.layer{li}.{bi}.downsample.0", planes, cin, 1, 1))
            cin = planes
    s.append((f"{prefix}.conv2", out_dim, 128, 1, 1))
    return s


BASE_CORR_LEVELS, BASE_CORR_RADIUS = 4, 4   # what a checkpoint's correlation-input weights are shaped for


def corr_channel_subset(levels, radius, base_levels=BASE_CORR_LEVELS, base_radius=BASE_CORR_RADIUS):
    """Channels of a base (4-level, radius-4) lookup that a smaller lookup produces, in its own order:
    level l < levels, window offsets within +-radius (the centred sub-window).  The reference's --fast
    mode lowers corr_levels / corr_radius on the cfg of an already-trained network
    (processing/videoflow_core.py:91-94); the checkpoint keeps its shapes, the engine uses the matching
    input columns of the first motion-encoder convolution."""
    if levels > base_levels or radius > base_radius:
        raise ValueError(f"corr_levels <= {base_levels} and corr_radius <= {base_radius} required")
    bw, d = 2 * base_radius + 1, base_radius - radius
    return [l * bw * bw + (i + d) * bw + (j + d)
            for l in range(levels) for i in range(2 * radius + 1) for j in range(2 * radius + 1)]


# The SK ("super kernel") update block (cfg.sk): its first depthwise weight names the family in a
# checkpoint.  A depthwise entry of the table is (name, C, 1, k, k) - PyTorch's shape of a grouped convolution's weight.
SK_KEY = "update_block.encoder.convc1.conv_list.0.weight"


def is_depthwise(name):
    return ".conv_list." in name


def pcblock_hidden(cin):
    return int(1.5 * cin)


def _pcblock_spec(name, cin, cout, k):
    """PCBlock(cin, cout, k) of SKFlow in state-dict order: two depthwise convolutions, the first feed-forward pair, the
    pointwise convolution, the second feed-forward pair (every convolution biased)."""
    hid = pcblock_hidden(cin)
    return [(f"{name}.conv_list.0", cin, 1, k[0], k[0]), (f"{name}.conv_list.1", cin, 1, k[1], k[1]),
            (f"{name}.ffn1.0", hid, cin, 1, 1), (f"{name}.ffn1.2", cin, hid, 1, 1), (f"{name}.pw", cin, cin, 1, 1),
            (f"{name}.ffn2.0", hid, cin, 1, 1), (f"{name}.ffn2.2", cout, hid, 1, 1)]


def sk_blocks(cfg):
    """[(name, cin, cout, (k0, k1))] of the seven PCBlocks of the SK update block, in state-dict order."""
    cor = BASE_CORR_LEVELS * (2 * BASE_CORR_RADIUS + 1) ** 2
    hid = cfg.feat_dim // 2
    gin = hid + (4 if getattr(cfg, "gma", False) else 3) * 128
    ub = "update_block"
    return [(f"{ub}.encoder.convc1", 2 * cor, 256, (1, 15)), (f"{ub}.encoder.convc2", 256, 192, (1, 15)),
            (f"{ub}.encoder.convf2", 128, 64, (1, 15)), (f"{ub}.encoder.conv", 192 + 64, 128 - 4, (1, 15)),
            (f"{ub}.gru", gin, hid, (1, 7)), (f"{ub}.flow_head", hid, 4, (1, 15))]


def _sk_spec(cfg):
    hid = cfg.feat_dim // 2
    ub = "update_block"
    blocks = {n: _pcblock_spec(n, ci, co, k) for n, ci, co, k in sk_blocks(cfg)}
    s = _encoders_spec(cfg)
    s += blocks[f"{ub}.encoder.convc1"] + blocks[f"{ub}.encoder.convc2"]
    s += [(f"{ub}.encoder.convf1", 128, 4, 1, 1)]
    s += blocks[f"{ub}.encoder.convf2"] + blocks[f"{ub}.encoder.conv"]
    s += [(f"{ub}.tprop", 128, 3 * 128, 1, 1)]
    s += blocks[f"{ub}.gru"] + blocks[f"{ub}.flow_head"]
    s += [(f"{ub}.mask.0", 256, hid, 3, 3), (f"{ub}.mask.2", 2 * 64 * 9, 256, 1, 1)]
    if getattr(cfg, "gma", False):
        s += [(n, co, ci, 1, 1) for n, (co, ci) in GMA_NO_BIAS.items()]
    return s


# The Twins-SVT encoders (cfg.twins): timm's twins_svt_large cut to two stages, `<prefix>.svt.*`.  The
# first patch embedding of fnet names the family in a checkpoint.
TWINS_KEY = "fnet.svt.patch_embeds.0.proj.weight"
TWINS_WS = 7                                      # window of the locally-grouped attention
# per stage: (patch, channels in, channels, heads, reduction of the sub-sampled attention)
TWINS_STAGES = ((4, 3, 128, 4, 8), (2, 128, 256, 8, 4))
TWINS_FINAL_NORM = 1024                           # timm's final norm of the four-stage backbone: carried, loaded, unused
TWINS_LN_SEEDED = ((0.75, 1.25), (-0.1, 0.1))     # seeded LayerNorm weight / bias ranges (PyTorch's 1 / 0 would test nothing)


def twins_encoder_spec(prefix):
    """[(name, kind, weight shape)] of one Twins-SVT encoder in state-dict order; every entry has a bias of shape[0] values.
    kind: "conv" (Conv2d, kernel = stride), "linear", "dw" (depthwise 3 x 3) or "ln" (LayerNorm weight and bias)."""
    sv = f"{prefix}.svt"
    s = []
    for i, (p, cin, c, _, _) in enumerate(TWINS_STAGES):
        s += [(f"{sv}.patch_embeds.{i}.proj", "conv", (c, cin, p, p)), (f"{sv}.patch_embeds.{i}.norm", "ln", (c,))]
    for i, (_, _, c, _, sr) in enumerate(TWINS_STAGES):
        b = f"{sv}.blocks.{i}.0"
        s += [(f"{b}.norm1", "ln", (c,)), (f"{b}.attn.qkv", "linear", (3 * c, c)), (f"{b}.attn.proj", "linear", (c, c)),
              (f"{b}.norm2", "ln", (c,)), (f"{b}.mlp.fc1", "linear", (4 * c, c)), (f"{b}.mlp.fc2", "linear", (c, 4 * c))]
        b = f"{sv}.blocks.{i}.1"
        s += [(f"{b}.norm1", "ln", (c,)), (f"{b}.attn.q", "linear", (c, c)), (f"{b}.attn.kv", "linear", (2 * c, c)),
              (f"{b}.attn.proj", "linear", (c, c)), (f"{b}.attn.sr", "conv", (c, c, sr, sr)), (f"{b}.attn.norm", "ln", (c,)),
              (f"{b}.norm2", "ln", (c,)), (f"{b}.mlp.fc1", "linear", (4 * c, c)), (f"{b}.mlp.fc2", "linear", (c, 4 * c))]
    for i, (_, _, c, _, _) in enumerate(TWINS_STAGES):
        s.append((f"{sv}.pos_block.{i}.proj.0", "dw", (c, 1, 3, 3)))
    s.append((f"{sv}.norm", "ln", (TWINS_FINAL_NORM,)))
    return s


def twins_spec(cfg):
    """The non-BasicEncoder parameters of a cfg.twins network: both encoders' tables (empty without cfg.twins)."""
    if not getattr(cfg, "twins", False):
        return []
    return twins_encoder_spec("fnet") + twins_encoder_spec("cnet")


def _encoders_spec(cfg):
    """The two BasicEncoders' convolutions - none with cfg.twins, whose encoders are twins_spec's."""
    if getattr(cfg, "twins", False):
        return []
    return _encoder_spec("fnet", cfg.feat_dim) + _encoder_spec("cnet", cfg.feat_dim)


def conv_spec(cfg):
    """[(name, cout, cin, kh, kw)] for every convolution, in state-dict order (checkpoint shapes: the
    correlation input is always the base 4-level radius-4 lookup).  cfg.sk: the SK update block's table (_sk_spec).
    cfg.twins: without the encoders' convolutions - twins_spec lists the Twins-SVT encoders' parameters, which come first."""
    if getattr(cfg, "sk", False):
        return _sk_spec(cfg)
    cor = BASE_CORR_LEVELS * (2 * BASE_CORR_RADIUS + 1) ** 2
    hid = cfg.feat_dim // 2
    s = _encoders_spec(cfg)
    ub = "update_block"
    s += [
        (f"{ub}.encoder.convc1", 256, 2 * cor, 1, 1),
        (f"{ub}.encoder.convc2", 192, 256, 3, 3),
        (f"{ub}.encoder.convf1", 128, 4, 7, 7),
        (f"{ub}.encoder.convf2", 64, 128, 3, 3),
        (f"{ub}.encoder.conv", 128 - 4, 192 + 64, 3, 3),
        (f"{ub}.tprop", 128, 3 * 128, 1, 1),
    ]
    gma = bool(getattr(cfg, "gma", False))
    gin = hid + (4 if gma else 3) * 128      # GMA: [inp | mf | mt | mg], the aggregated motion features last
    for nm, kh, kw in (("z1", 1, 5), ("r1", 1, 5), ("q1", 1, 5), ("z2", 5, 1), ("r2", 5, 1), ("q2", 5, 1)):
        s.append((f"{ub}.gru.conv{nm}", hid, gin, kh, kw))
    s += [
        (f"{ub}.flow_head.conv1", 256, hid, 3, 3),
        (f"{ub}.flow_head.conv2", 4, 256, 3, 3),
        (f"{ub}.mask.0", 256, hid, 3, 3),
        (f"{ub}.mask.2", 2 * 64 * 9, 256, 1, 1),
    ]
    if gma:
        s += [(n, co, ci, 1, 1) for n, (co, ci) in GMA_NO_BIAS.items()]
    return s


# The two 1x1 convolutions of the GMA aggregator (cfg.gma), neither with a bias: `att.to_qk` maps the
# context half `inp` onto q | k (one head, d = 128), `aggregator.to_v` the motion features onto the values.
GMA_NO_BIAS = {"att.to_qk": (256, 128), "update_block.aggregator.to_v": (128, 128)}
GMA_GAMMA = "update_block.aggregator.gamma"
GMA_SEEDED_GAMMA = 0.5      # upstream initialises 0, which would switch the block off (seeded_memflow_state_dict chooses alike)


def seeded_state_dict(cfg, seed=0):
    """PyTorch's default Conv2d initialisation (uniform +-1/sqrt(fan_in) for weight and bias),
    drawn layer by layer from one seeded generator, so the values depend only on (cfg, seed).  (A depthwise entry's fan-in
    is k * k: its bound is 1 / k, PyTorch's default for a grouped convolution.)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, kind, shape in twins_spec(cfg):
        # Linear and convolution weights by the same rule (fan-in = the weight's other dimensions); LayerNorm weights and
        # biases from TWINS_LN_SEEDED
        if kind == "ln":
            (w0, w1), (b0, b1) = TWINS_LN_SEEDED
            sd[f"{name}.weight"] = w0 + (w1 - w0) * torch.rand(shape, generator=g)
            sd[f"{name}.bias"] = b0 + (b1 - b0) * torch.rand(shape, generator=g)
            continue
        bound = 1.0 / math.sqrt(math.prod(shape[1:]))
        sd[f"{name}.weight"] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        sd[f"{name}.bias"] = (torch.rand(shape[0], generator=g) * 2 - 1) * bound
    for name, cout, cin, kh, kw in conv_spec(cfg):
        bound = 1.0 / math.sqrt(cin * kh * kw)
        sd[f"{name}.weight"] = (torch.rand(cout, cin, kh, kw, generator=g) * 2 - 1) * bound
        if name not in GMA_NO_BIAS:
            sd[f"{name}.bias"] = (torch.rand(cout, generator=g) * 2 - 1) * bound
    if getattr(cfg, "gma", False):
        sd[GMA_GAMMA] = torch.tensor([GMA_SEEDED_GAMMA])
    return sd


def load_checked(model, state, what):
    """Strict `load_state_dict` (reference processing/videoflow_core.py:110) with an error that names what does not
    fit, its unexpected key FAMILIES listed instead of hundreds of raw keys.  The encoders are the RAFT BasicEncoder
    (`fnet.conv1`, `fnet.layer1.0.conv1`, ...) or, with cfg.twins - which VideoFlowCore.load_model sets from the checkpoint -
    the Twins-SVT encoders cut to two stages that the released MOF / BOF configurations select (`fnet.svt.*`, SURVEY.md
    App. A); a full four-stage backbone (`svt.patch_embeds.2`, ...) is refused.  The GMA aggregator's keys
    (`att.to_qk`, `update_block.aggregator.*`) belong to the network when cfg.gma is set, which VideoFlowCore.load_model
    does from the checkpoint: they are named as unexpected only for a network built without it; the SK update block's
    keys (`update_block.*.conv_list.*`, `.ffn1.*`, `.pw`, `.ffn2.*`) likewise with cfg.sk.  Numerical parity with the
    published checkpoints is unverified: they are not available here (.MISSING_LARGE_BLOBS)."""
    want = set(model.state_dict().keys())
    have = set(state.keys())
    if want != have:
        def families(keys):
            fam = {}
            for k in keys:
                parts = k.split(".")
                f = ".".join(parts[:2]) + ".*" if len(parts) > 2 else k
                fam[f] = fam.get(f, 0) + 1
            return ", ".join(f"{f} ({n})" for f, n in sorted(fam.items())) or "none"
        raise RuntimeError(
            f"{what}: checkpoint does not match the network this engine builds ({'Twins-SVT (two stages)' if TWINS_KEY in want else 'CNN BasicEncoder'} fnet/cnet, "
            f"{'SK' if SK_KEY in want else 'SepConvGRU'} update block{', GMA aggregator' if GMA_GAMMA in want else ''}).  Unexpected key families: {families(have - want)}.  Missing key families: "
            f"{families(want - have)}.  A full four-stage timm Twins-SVT backbone (svt.patch_embeds.2, svt.blocks.2, ...) "
            f"is the one family that is not supported; Twins-SVT encoders cut to two stages (fnet.svt.* / cnet.svt.*) are, "
            f"through cfg.twins; the GMA aggregator (att.to_qk, update_block.aggregator.*) is, "
            f"through cfg.gma, and the SK update block (update_block.*.conv_list.*) is, through cfg.sk.")
    bad = [f"{k}: checkpoint {tuple(state[k].shape)} vs network {tuple(v.shape)}"
           for k, v in model.state_dict().items() if tuple(state[k].shape) != tuple(v.shape)]
    if bad:
        raise RuntimeError(f"{what}: parameter shapes differ: " + "; ".join(bad[:8]) + (" ..." if len(bad) > 8 else ""))
    model.load_state_dict(state)


def checkpoint_name(architecture="mof", dataset="sintel", variant="standard"):
    """File name rule of reference processing/videoflow_core.py:79-85."""
    arch = architecture.upper()
    if variant == "noise" and dataset == "things":
        return f"{arch}_{dataset}_288960noise.pth"
    return f"{arch}_{dataset}.pth"


def write_seeded_checkpoint(root, cfg, seed=0, architecture="mof", dataset="sintel", variant="standard",
                            dataparallel_prefix=False):
    """Write `<root>/VideoFlow_ckpt/<name>.pth`; returns the path."""
    d = os.path.join(root, "VideoFlow_ckpt")
    os.makedirs(d, exist_ok=True)
    sd = seeded_state_dict(cfg, seed)
    if dataparallel_prefix:
        sd = {"module." + k: v for k, v in sd.items()}
    path = os.path.join(d, checkpoint_name(architecture, dataset, variant))
    torch.save(sd, path)
    return path


def pack_conv_weight(w, cin_pad=None, cblock=False):
    """[cout, cin, kh, kw] -> flat [cout][kh][kw][cin(+pad)] float32 (the kernels' K order), or with
    `cblock` the channel-block order [cout][cin/32][kh][kw][32] (cin zero padded to a multiple of 32;
    include/vfml.h VFML_KORDER_CBLOCK)."""
    cout, cin, kh, kw = w.shape
    if cblock:
        blk = 64 if cblock == 64 else 32       # cblock=64: VFML_KORDER_CBLOCK64 (cin a multiple of 64)
        cp = (cin + blk - 1) // blk * blk
        w = torch.nn.functional.pad(w.detach().to(torch.float32), (0, 0, 0, 0, 0, cp - cin))
        return w.reshape(cout, cp // blk, blk, kh, kw).permute(0, 1, 3, 4, 2).contiguous().reshape(-1)
    w = w.detach().to(torch.float32).permute(0, 2, 3, 1)
    if cin_pad is not None and cin_pad > cin:
        w = torch.nn.functional.pad(w, (0, cin_pad - cin))
    return w.contiguous().reshape(-1)
