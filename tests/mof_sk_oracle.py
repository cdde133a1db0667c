"""CPU oracle of the MOF / BOF network WITH the SK ("super kernel") update block (TEST INFRASTRUCTURE ONLY).

oracle.mof_oracle's network with the update block of DESIGN.md section 16, in plain PyTorch: parameter names are the
engine's (`update_block.encoder.convc1.conv_list.0`, ...), so a state dict of vfml.weights.seeded_state_dict(cfg with
sk=True) loads into it strictly; with cfg.gma as well the aggregator of tests/mof_gma_oracle.py is part of it.

    PCBlock(C, C_out, (k0, k1)), hid = int(1.5 C), every convolution biased:
        x = gelu(x + ffn1.2(gelu(ffn1.0(x))))         1x1 C -> hid -> C
        x = gelu(x + conv_list.0(x))                  depthwise k0 x k0, zero padding k0 // 2
        x = gelu(x + conv_list.1(x))                  depthwise k1 x k1
        x = gelu(x + pw(x))                           1x1 C -> C
        y = ffn2.2(gelu(ffn2.0(x)))                   1x1 C -> hid -> C_out
    gelu is the exact one (erf), the depthwise convolutions cross-correlations (nn.Conv2d).

Like the rest of the oracle this restates a published block (SKFlow, Sun et al. 2022, as VideoFlow uses it) as recalled; it
is pinned by the known answers of tests/test_sk_cpu.py, not against upstream code.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import mof_gma_oracle as go
from oracle import mof_oracle as mo


class PCBlock(nn.Module):
    def __init__(self, c, c_out, k):
        super().__init__()
        hid = int(1.5 * c)
        self.conv_list = nn.ModuleList([nn.Conv2d(c, c, kk, padding=kk // 2, groups=c) for kk in k])
        self.ffn1 = nn.Sequential(nn.Conv2d(c, hid, 1), nn.GELU(), nn.Conv2d(hid, c, 1))
        self.pw = nn.Conv2d(c, c, 1)
        self.ffn2 = nn.Sequential(nn.Conv2d(c, hid, 1), nn.GELU(), nn.Conv2d(hid, c_out, 1))

    def forward(self, x):
        x = F.gelu(x + self.ffn1(x))
        for conv in self.conv_list:
            x = F.gelu(x + conv(x))
        x = F.gelu(x + self.pw(x))
        return self.ffn2(x)


class SKMotionEncoder(nn.Module):
    def __init__(self, cor_planes):
        super().__init__()
        self.convc1 = PCBlock(2 * cor_planes, 256, (1, 15))
        self.convc2 = PCBlock(256, 192, (1, 15))
        self.convf1 = nn.Conv2d(4, 128, 1)
        self.convf2 = PCBlock(128, 64, (1, 15))
        self.conv = PCBlock(192 + 64, 128 - 4, (1, 15))

    def forward(self, fflow, bflow, fcorr, bcorr):
        flow = torch.cat([fflow, bflow], dim=1)
        cor = F.gelu(self.convc1(torch.cat([fcorr, bcorr], dim=1)))
        cor = self.convc2(cor)
        flo = self.convf2(self.convf1(flow))
        out = self.conv(torch.cat([cor, flo], dim=1))
        return torch.cat([out, flow], dim=1)


class SKUpdateBlock(nn.Module):
    """The MOF / BOF update block with its motion encoder, GRU and flow head replaced by PCBlocks; the temporal fusion and
    the mask head are oracle.mof_oracle's, the aggregator (gma) tests/mof_gma_oracle.py's."""

    def __init__(self, cor_planes, hidden_dim=128, gma=False):
        super().__init__()
        self.encoder = SKMotionEncoder(cor_planes)
        self.tprop = nn.Conv2d(3 * 128, 128, 1)
        self.gru = PCBlock(hidden_dim + (4 if gma else 3) * 128, hidden_dim, (1, 7))
        self.flow_head = PCBlock(hidden_dim, 4, (1, 15))
        self.mask = nn.Sequential(nn.Conv2d(hidden_dim, 256, 3, padding=1), nn.ReLU(inplace=False),
                                  nn.Conv2d(256, 2 * 64 * 9, 1))
        if gma:
            self.aggregator = go.Aggregate(128, 128)

    temporal = mo.MOFUpdateBlock.temporal

    def forward(self, net, inp, fcorr, bcorr, fflow, bflow, bs, attn=None):
        mf = self.encoder(fflow, bflow, fcorr, bcorr)
        mt = self.temporal(mf, bs)
        parts = [net, inp, mf, mt]
        if attn is not None:
            parts.append(self.aggregator(attn, mf))
        net = self.gru(torch.cat(parts, dim=1))
        return net, 0.25 * self.mask(net), self.flow_head(net)


class MOFSKOracle(mo.MOFNetOracle):
    def __init__(self, cfg):
        if (cfg.corr_levels, cfg.corr_radius) != (4, 4):
            raise ValueError(f"the SK update block needs the base lookup (corr_levels, corr_radius) = (4, 4), got "
                             f"({cfg.corr_levels}, {cfg.corr_radius})")
        super().__init__(cfg)
        self.gma = bool(getattr(cfg, "gma", False))
        self.update_block = SKUpdateBlock(4 * 81, self.hidden_dim, gma=self.gma)
        if self.gma:
            self.att = go.Attention(self.context_dim, 128)

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
        attn = self.att(inp) if self.gma else None
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
    return MOFSKOracle(cfg)
