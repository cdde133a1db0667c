"""CPU oracle of MemFlow WITH its memory bank (TEST INFRASTRUCTURE ONLY).  Status: PARITY UNPINNED, as oracle/memflow_oracle.py.

oracle.memflow_oracle's network unchanged, run over a stream of fields in frame order with a bank of
capacity M, in plain PyTorch of any dtype:

    bank         pairs (k_j, v_j) of earlier fields, oldest first, n <= M of them
    q_t, k_t     the 1x1 convolutions of the context `inp` of field t
    attn         softmax(q_t [k_j ..., k_t]^T / sqrt(d))   JOINTLY over all (n + 1) P columns
    every iteration:  v_t = value(motion),  readout = attn . [v_j ..., v_t],  motion_global = motion + gamma * readout
    after the last iteration the bank takes (k_t, v_t of that iteration); beyond M entries the oldest goes

M = 0 (or an empty bank) is MemFlowNetOracle.forward, bit for bit.  Not built, and where upstream may differ: a bank-size
dependent score scale, top-k, long-term consolidation, a flow_init warm start.
"""
import math

import torch

from oracle.memflow_oracle import CorrBlock, MemFlowNetOracle, coords_grid, upsample_flow  # noqa: F401


@torch.no_grad()
def step(net, pair, bank, M, alter=None):
    """One field.  net: a MemFlowNetOracle; pair [1, 2, 3, H, W] in [-1, 1]; bank: the list of (k [1,d,P], v [1,P,d]) this
    field reads - and joins: it is updated in place.  Returns (flow_low [1,2,h,w], flow [1,2,H,W]).  alter: a function
    applied to the attention rows [1, P, (n + 1) P] before they are used (the mutants of tests/test_memflow_noise_cpu.py)."""
    cfg, ub = net.cfg, net.update_block
    B, _, _, H, W = pair.shape
    h, w = H // 8, W // 8
    fm = net.fnet(pair.reshape(2 * B, 3, H, W)).reshape(B, 2, -1, h, w)
    corr_fn = CorrBlock(fm[:, 0], fm[:, 1], cfg.corr_levels, cfg.corr_radius)
    cn = net.cnet(pair[:, 0])
    hid, inp = torch.split(cn, [net.hidden_dim, net.context_dim], dim=1)
    hid, inp = torch.tanh(hid), torch.relu(inp)
    q = net.query(inp).flatten(2).transpose(1, 2)                        # [B, P, d]
    k = net.key(inp).flatten(2)                                          # [B, d, P]
    held = list(bank) if M > 0 else []
    keys = torch.cat([e[0] for e in held] + [k], dim=2) if held else k
    attn = torch.softmax(torch.matmul(q, keys) / math.sqrt(cfg.att_dim), dim=-1)
    if alter is not None:
        attn = alter(attn)
    coords0 = coords_grid(B, h, w, pair.dtype)
    coords1 = coords0.clone()
    v = None
    for _ in range(cfg.decoder_depth):
        corr = corr_fn(coords1)
        motion = ub.encoder(coords1 - coords0, corr)
        v = ub.value(motion).flatten(2).transpose(1, 2)                  # [B, P, d]
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


class Stream:
    """The interface of vfml.memflow_net.MemFlowStream over step()."""

    def __init__(self, net, memory_frames, alter=None):
        self.net, self.memory_frames, self.bank, self.alter = net, memory_frames, [], alter

    def step(self, pair, end=False):
        out = step(self.net, pair, self.bank, self.memory_frames, self.alter)
        if end:
            self.reset()
        return out

    def reset(self):
        del self.bank[:]


def fixture_clip(H, W, frames=5, seed=5):
    """[1, frames, 3, H, W] in [-1, 1]: a crop of one random picture that moves by (2, 1) pixels per frame, plus noise."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(1, 1, 3, H + 16, W + 16, generator=g) * 2 - 1
    out = [(base[0, :, :, 2 * i:2 * i + H, i:i + W] + 0.05 * torch.randn(1, 3, H, W, generator=g)).clamp(-1, 1)
           for i in range(frames)]
    return torch.stack(out, dim=1)


def run_fields(net, clip, M):
    """The fields (i, i+1) of a clip through one stream of capacity M: [(flow_low, flow)]."""
    st = Stream(net, M)
    return [st.step(clip[:, i:i + 2]) for i in range(clip.shape[1] - 1)]


def epe(a, b):
    return (a.double() - b.double()).pow(2).sum(1).sqrt().mean().item()
