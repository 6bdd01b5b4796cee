"""What the engines and the checkpoint checks share of the models: the parameter specs (the reference's state_dict names and
shapes), FlatParams and the initial BatchNorm buffers.  torch and the standard library only."""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict

import torch

Tensor = torch.Tensor
BN_EPS, BN_MOM, P_DROP = 1e-5, 0.1, 0.2


def feature_encoder_spec(in_dim=6, hidden_dims=(256, 128), out_dim=128):
    """src/gan/feature_encoder.py:16-42."""
    spec = OrderedDict([("net.0.weight", (in_dim,)), ("net.0.bias", (in_dim,))])
    prev, idx = in_dim, 1
    for h in hidden_dims:
        spec[f"net.{idx}.weight"] = (h, prev)
        spec[f"net.{idx}.bias"] = (h,)
        prev, idx = h, idx + 3
    spec[f"net.{idx}.weight"] = (out_dim, prev)
    spec[f"net.{idx}.bias"] = (out_dim,)
    return spec


def generator_spec(noise_dim, latent_dim, mode, hidden, max_notes, note_dim, numeric_embed_dim):
    """src/gan/models.py:86-106, :20-27, :33-64."""
    in_dim = noise_dim + numeric_embed_dim + (latent_dim if mode == "conditioning" else 0)
    red = max(1, max_notes // 8)
    return OrderedDict([
        ("noise_to_latent.net.0.weight", (hidden, in_dim)), ("noise_to_latent.net.0.bias", (hidden,)),
        ("noise_to_latent.net.2.weight", (latent_dim, hidden)), ("noise_to_latent.net.2.bias", (latent_dim,)),
        ("decoder.pre.0.weight", (512, latent_dim)), ("decoder.pre.0.bias", (512,)),
        ("decoder.pre.2.weight", (256 * red, 512)), ("decoder.pre.2.bias", (256 * red,)),
        ("decoder.deconv.0.weight", (256, 128, 5)), ("decoder.deconv.0.bias", (128,)),
        ("decoder.deconv.1.weight", (128,)), ("decoder.deconv.1.bias", (128,)),
        ("decoder.deconv.3.weight", (128, 64, 5)), ("decoder.deconv.3.bias", (64,)),
        ("decoder.deconv.4.weight", (64,)), ("decoder.deconv.4.bias", (64,)),
        ("decoder.deconv.6.weight", (64, note_dim, 5)), ("decoder.deconv.6.bias", (note_dim,)),
    ])


def discriminator_spec(note_dim, emb_dim=256, numeric_embed_dim=0):
    """src/gan/models.py:137-157."""
    return OrderedDict([
        ("conv.0.weight", (64, note_dim, 5)), ("conv.0.bias", (64,)),
        ("conv.2.weight", (128, 64, 5)), ("conv.2.bias", (128,)),
        ("conv.4.weight", (256, 128, 5)), ("conv.4.bias", (256,)),
        ("fc.1.weight", (emb_dim, 256)), ("fc.1.bias", (emb_dim,)),
        ("real_fake.weight", (1, emb_dim + numeric_embed_dim)), ("real_fake.bias", (1,)),
    ])


def emotion_disc_spec(cfg: dict):
    """src/emotion_discriminator/ed_model.py:52-58,115-145.  Returns (params, buffers, conv channel list)."""
    spec, bufs, chans = OrderedDict(), OrderedDict(), []
    prev = cfg.get("latent_dim", 128)
    if cfg.get("input_mode", "latent") == "notes":
        hid = cfg.get("notes_hidden", 256)
        in_ch, ch = cfg.get("note_dim", 4), 64
        for i in range(cfg.get("notes_blocks", 4)):
            k = 5 if i == 0 else 3
            chans.append((in_ch, ch, k))
            spec[f"encoder.conv.{i}.net.0.weight"] = (ch, in_ch, k)
            spec[f"encoder.conv.{i}.net.0.bias"] = (ch,)
            spec[f"encoder.conv.{i}.net.1.weight"] = (ch,)
            spec[f"encoder.conv.{i}.net.1.bias"] = (ch,)
            bufs[f"encoder.conv.{i}.net.1.running_mean"] = (ch,)
            bufs[f"encoder.conv.{i}.net.1.running_var"] = (ch,)
            in_ch, ch = ch, min(ch * 2, hid)
        spec["encoder.project.weight"] = (hid, in_ch)
        spec["encoder.project.bias"] = (hid,)
        prev = hid
    idx = 0
    for h in tuple(cfg.get("mlp_hidden", (256, 128))):
        spec[f"classifier.net.{idx}.weight"] = (h, prev)
        spec[f"classifier.net.{idx}.bias"] = (h,)
        prev, idx = h, idx + 3
    spec["classifier.head.weight"] = (cfg.get("n_classes", 4), prev)
    spec["classifier.head.bias"] = (cfg.get("n_classes", 4),)
    return spec, bufs, chans


class FlatParams:
    """All tensors of one optimiser in a single flat fp32 buffer (+ grads, Adam m/v, step state)."""

    def __init__(self, spec: "OrderedDict[str, tuple]", device, with_opt: bool = True, first=None):
        """`first`: tensor (or list of tensors) placed at offset 0 of the flat buffers (the dict order stays the spec's) -- the data-parallel
        wrapper all-reduces that tensor's gradient early and everything behind it as ONE contiguous range."""
        self.spec = spec
        self.n = sum(math.prod(s) for s in spec.values())
        pad = (-self.n) % 4
        self.data = torch.zeros(self.n + pad, device=device)
        self.p: Dict[str, Tensor] = OrderedDict()
        self.offsets = {}
        off = 0
        first = [first] if isinstance(first, str) else list(first or [])
        for k in first + [k for k in spec if k not in first]:
            n = math.prod(spec[k])
            self.offsets[k] = (off, n)
            off += n
        for k, s in spec.items():
            o, n = self.offsets[k]
            self.p[k] = self.data[o:o + n].view(s)
        self.g: Dict[str, Tensor] = OrderedDict()
        self.ticked = False      # Adam state already advanced by the sub-step's Philox draw (GanEngine.draw_randoms)
        if with_opt:
            self.grad = torch.zeros_like(self.data)
            self.m = torch.zeros_like(self.data)
            self.v = torch.zeros_like(self.data)
            self.state = torch.zeros(4, dtype=torch.float64, device=device)
            for k, s in spec.items():
                o, n = self.offsets[k]
                self.g[k] = self.grad[o:o + n].view(s)

    def load(self, params: Dict[str, Tensor], prefix: str = ""):
        for k in self.spec:
            src = params[prefix + k] if (prefix + k) in params else params[k]
            if tuple(src.shape) != tuple(self.spec[k]):
                raise ValueError(f"{k}: shape {tuple(src.shape)} != {self.spec[k]}")
            self.p[k].copy_(src.to(torch.float32))

    def state_dict(self) -> "OrderedDict[str, Tensor]":
        return OrderedDict((k, v.detach().cpu().clone()) for k, v in self.p.items())


def norm_buffers(bufs: "Dict[str, tuple]", device) -> "OrderedDict[str, Tensor]":
    """BatchNorm running statistics at their initial values: running_var one, everything else zero."""
    return OrderedDict((k, torch.ones(s, device=device) if k.endswith("running_var") else torch.zeros(s, device=device))
                       for k, s in bufs.items())
