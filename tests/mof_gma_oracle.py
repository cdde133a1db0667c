"""CPU oracle of the MOF / BOF network WITH the GMA global-motion aggregator (TEST INFRASTRUCTURE ONLY).

oracle.mof_oracle's network with the block of DESIGN.md section 15 added, in plain PyTorch: parameter names are the
engine's (`att.to_qk`, `update_block.aggregator.to_v`, `update_block.aggregator.gamma`), so a state dict of
vfml.weights.seeded_state_dict(cfg with gma=True) loads into it strictly.

    q | k = att.to_qk(inp)                         1x1, 128 -> 256, no bias; one head, d = 128
    attn  = softmax_j(q_i . k_j / sqrt(128))       over the cells of the same centre frame, once per frame
    mg    = mf + gamma * attn @ to_v(mf)           to_v 1x1, 128 -> 128, no bias; every iteration
    GRU input [inp | mf | mt | mg]

Like the rest of the oracle this restates a published block (GMA, Jiang et al. 2021) as recalled; it is pinned by the
known answers of tests/test_gma_cpu.py, not against upstream code.
"""
import math

import torch
import torch.nn as nn

from oracle import mof_oracle as mo


class Attention(nn.Module):
    def __init__(self, dim=128, d=128):
        super().__init__()
        self.d = d
        self.to_qk = nn.Conv2d(dim, 2 * d, 1, bias=False)

    def forward(self, inp):
        """inp [n, 128, h, w] -> attention [n, P, P] (rows sum to one)."""
        n, _, h, w = inp.shape
        q, k = self.to_qk(inp).reshape(n, 2, self.d, h * w).unbind(1)
        return torch.softmax(q.transpose(1, 2) @ k / math.sqrt(self.d), dim=-1)


class Aggregate(nn.Module):
    def __init__(self, dim=128, d=128):
        super().__init__()
        self.to_v = nn.Conv2d(dim, d, 1, bias=False)
        self.gamma = nn.Parameter(torch.zeros(1))

    def forward(self, attn, mf):
        n, c, h, w = mf.shape
        v = self.to_v(mf).reshape(n, -1, h * w)                  # [n, d, P]
        out = (attn @ v.transpose(1, 2)).transpose(1, 2)         # [n, d, P]
        return mf + self.gamma * out.reshape(n, -1, h, w)


class GMAUpdateBlock(mo.MOFUpdateBlock):
    def __init__(self, cor_planes, hidden_dim=128):
        super().__init__(cor_planes, hidden_dim)
        self.gru = mo.SepConvGRU(hidden_dim, input_dim=4 * 128)
        self.aggregator = Aggregate(128, 128)

    def forward(self, net, inp, fcorr, bcorr, fflow, bflow, bs, attn=None):
        mf = self.encoder(fflow, bflow, fcorr, bcorr)
        mt = self.temporal(mf, bs)
        mg = self.aggregator(attn, mf)
        net = self.gru(net, torch.cat([inp, mf, mt, mg], dim=1))
        return net, 0.25 * self.mask(net), self.flow_head(net)


class MOFGMAOracle(mo.MOFNetOracle):
    def __init__(self, cfg):
        super().__init__(cfg)
        sel = self.update_block.encoder.sel
        self.update_block = GMAUpdateBlock(4 * 81, self.hidden_dim)
        self.update_block.encoder.sel = sel
        self.att = Attention(self.context_dim, 128)

    @torch.no_grad()
    def forward(self, images, data=None, return_lowres=False):
        cfg = self.cfg
        if getattr(cfg, "network", "MOFNetStack") == "BOFNet" and images.shape[1] > 3:
            lo = images.shape[1] // 2 - 1
            images = images[:, lo:lo + 3]
        B, N, _, H, W = images.shape
        M = N - 2
        h, w = H // 8, W // 8
        images = cfg.input_scale * images + cfg.input_shift
        fmaps = self.fnet(images.reshape(B * N, 3, H, W)).reshape(B, N, -1, h, w)
        centre = fmaps[:, 1:N - 1].reshape(B * M, -1, h, w)
        fcorr_fn = mo.CorrBlock(centre, fmaps[:, 2:N].reshape(B * M, -1, h, w), cfg.corr_levels, cfg.corr_radius)
        bcorr_fn = mo.CorrBlock(centre, fmaps[:, 0:N - 2].reshape(B * M, -1, h, w), cfg.corr_levels, cfg.corr_radius)
        cnet = self.cnet(images[:, 1:N - 1].reshape(B * M, 3, H, W))
        net, inp = torch.split(cnet, [self.hidden_dim, self.context_dim], dim=1)
        net, inp = torch.tanh(net), torch.relu(inp)
        attn = self.att(inp)                   # once per centre frame
        coords0 = mo.coords_grid(B * M, h, w, images.dtype)
        fcoords1, bcoords1 = coords0.clone(), coords0.clone()
        for _ in range(cfg.decoder_depth):
            fcorr, bcorr = fcorr_fn(fcoords1), bcorr_fn(bcoords1)
            net, up_mask, delta = self.update_block(net, inp, fcorr, bcorr, fcoords1 - coords0, bcoords1 - coords0, B,
                                                    attn=attn)
            fcoords1 = fcoords1 + delta[:, 0:2]
            bcoords1 = bcoords1 + delta[:, 2:4]
        fmask, bmask = torch.split(up_mask, [576, 576], dim=1)
        fup = mo.upsample_flow(fcoords1 - coords0, fmask).reshape(B, M, 2, H, W)
        bup = mo.upsample_flow(bcoords1 - coords0, bmask).reshape(B, M, 2, H, W)
        low = torch.cat([(fcoords1 - coords0).reshape(B, M, 2, h, w),
                         (bcoords1 - coords0).reshape(B, M, 2, h, w)], dim=1)
        return torch.cat([fup, bup], dim=1), low


def build_network(cfg):
    return MOFGMAOracle(cfg)
