"""CPU oracle of a MemFlow stream WITH the warm start (TEST INFRASTRUCTURE ONLY).  Parity with upstream
unpinned, as tests/memflow_memory_oracle.py, whose `step` is restated here with a starting flow:

    coords1 = coords0 + flow_init        (flow_init None: zero, and the step is memflow_memory_oracle.step bit for bit)

and a stream that feeds every field forward_interpolate_oracle.forward_interpolate of the previous field's final
1/8-resolution flow, in the network's own dtype (float32 or float64).  The first field and the first after end=True or reset()
start cold.  The bank logic is memflow_memory_oracle's, unchanged."""
import math
import time

import numpy as np
import torch

import forward_interpolate_oracle as fio
from memflow_memory_oracle import CorrBlock, coords_grid, epe, fixture_clip, upsample_flow  # noqa: F401


@torch.no_grad()
def step(net, pair, bank, M, flow_init=None):
    """memflow_memory_oracle.step with flow_init [1, 2, h, w] (cells, the network's dtype) as the recurrence's start."""
    cfg, ub = net.cfg, net.update_block
    B, _, _, H, W = pair.shape
    h, w = H // 8, W // 8
    fm = net.fnet(pair.reshape(2 * B, 3, H, W)).reshape(B, 2, -1, h, w)
    corr_fn = CorrBlock(fm[:, 0], fm[:, 1], cfg.corr_levels, cfg.corr_radius)
    cn = net.cnet(pair[:, 0])
    hid, inp = torch.split(cn, [net.hidden_dim, net.context_dim], dim=1)
    hid, inp = torch.tanh(hid), torch.relu(inp)
    q = net.query(inp).flatten(2).transpose(1, 2)
    k = net.key(inp).flatten(2)
    held = list(bank) if M > 0 else []
    keys = torch.cat([e[0] for e in held] + [k], dim=2) if held else k
    attn = torch.softmax(torch.matmul(q, keys) / math.sqrt(cfg.att_dim), dim=-1)
    coords0 = coords_grid(B, h, w, pair.dtype)
    coords1 = coords0.clone() if flow_init is None else coords0 + flow_init
    v = None
    for _ in range(cfg.decoder_depth):
        corr = corr_fn(coords1)
        motion = ub.encoder(coords1 - coords0, corr)
        v = ub.value(motion).flatten(2).transpose(1, 2)
        values = torch.cat([e[1] for e in held] + [v], dim=1) if held else v
        readout = torch.matmul(attn, values).transpose(1, 2).reshape(B, -1, h, w)
        motion_global = motion + ub.gamma * readout
        hid = ub.gru(hid, torch.cat([inp, motion, motion_global], dim=1))
        coords1 = coords1 + ub.flow_head(hid)
    if M > 0:
        bank.append((k.clone(), v.clone()))
        del bank[:max(0, len(bank) - M)]
    else:
        del bank[:]
    up = upsample_flow(coords1 - coords0, 0.25 * ub.mask(hid))
    return coords1 - coords0, up


def project(low):
    """forward_interpolate of low [1, 2, h, w] in its own dtype -> (flow_init [1, 2, h, w], index [h, w] int32, margin [h, w])."""
    out, index, margin = fio.forward_interpolate(np.ascontiguousarray(low[0].permute(1, 2, 0).numpy()))
    return torch.from_numpy(out).permute(2, 0, 1)[None].contiguous(), index, margin


class Stream:
    """The interface of vfml.memflow_net.MemFlowStream(net, memory_frames, warm_start) over step().  After a step `init`,
    `index` and `margin` are the projection the field started from (None for a cold field)."""

    def __init__(self, net, memory_frames, warm_start=True):
        self.net, self.memory_frames, self.warm_start, self.bank = net, memory_frames, warm_start, []
        self.low = self.init = self.index = self.margin = None

    def step(self, pair, end=False):
        self.init = self.index = self.margin = None
        if self.warm_start and self.low is not None:
            self.init, self.index, self.margin = project(self.low)
        low, up = step(self.net, pair, self.bank, self.memory_frames, self.init)
        self.low = low
        if end:
            self.reset()
        return low, up

    def reset(self):
        del self.bank[:]
        self.low = None


_FIELDS = {}


def oracle_fields(clip, depth, state_dict, M, fields=3, warm=True):
    """The fields (i, i+1), i < fields, of clip [1, F, 3, H, W] through one warm stream of capacity M in float32 and float64,
    once per session and arguments, in tests_support.memflow_oracle_fields' layout plus the projections:
        {"f32": (flow [1, F, 2, H, W], low [1, F, 2, h, w]), "f64": the same, "seconds": (t32, t64),
         "init": {"f32": [None | [1, 2, h, w] per field], "f64": ...}, "index": {...: [None | int32 [h, w]]}, "margin": {...}}"""
    import tests_support as ts
    key = (ts._digest(clip), int(depth), ts._digest(*state_dict.values()), int(M), int(fields), bool(warm))
    ent = _FIELDS.get(key)
    if ent is None:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        ent = {"init": {}, "index": {}, "margin": {}}
        secs = []
        for name, double in (("f32", False), ("f64", True)):
            net = ts.memflow_oracle_net(depth, state_dict, double)
            x = clip.double() if double else clip.float()
            st = Stream(net, M, warm)
            t0 = time.time()
            out, ini, idx, mar = [], [], [], []
            for i in range(fields):
                out.append(st.step(x[:, i:i + 2]))
                ini.append(st.init)
                idx.append(st.index)
                mar.append(st.margin)
            secs.append(time.time() - t0)
            ent[name] = ts.memflow_stack(out)
            ent["init"][name], ent["index"][name], ent["margin"][name] = ini, idx, mar
        ent["seconds"] = tuple(secs)
        _FIELDS[key] = ent
    return ent


def stability(ent):
    """The condition under which a warm stream can be compared elementwise (a discontinuous selection): the float32 and float64
    oracle streams choose the same source in every cell of every warm field.  Returns the smallest margin (cells) over both."""
    least = float("inf")
    for a, b, ma, mb in zip(ent["index"]["f32"], ent["index"]["f64"], ent["margin"]["f32"], ent["margin"]["f64"]):
        assert (a is None) == (b is None)
        if a is None:
            continue
        flips = int((a != b).sum())
        assert flips == 0, f"the float32 and float64 oracle streams choose another source in {flips} cells"
        least = min(least, float(ma.min()), float(mb.min()))
    return least
