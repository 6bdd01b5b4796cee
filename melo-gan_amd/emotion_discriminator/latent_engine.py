"""Pre-training of the latent-mode emotion discriminator on MI355X (`input_mode: latent`): the reference's
MLPClassifier (src/emotion_discriminator/ed_model.py:72-95) on (B, latent_dim) encoder latents, one step of train_ed.py:51-82
-- train-mode forward (dropout), mean cross-entropy, backward, AdamW.

The step is a chain of three small dependent layers at batch 64; launched layer by layer it is all launch gaps.  The fused
engine runs it as TWO launches (csrc/mlp_train.hip):
  A  ops.mlp_cls_fwd_bwd       per row block: [stage the batch,] [draw the masks,] forward, cross-entropy, data gradients
  B  ops.mlp_cls_wgrad_update  per parameter tile: weight / bias gradient, [AdamW,] loss, [epoch metrics]
    backward()    = A + B(gradients only)          update() = ops.adam_flat
    step_rng()    = A(draw, tick) + B(apply)       step_staged() = A(stage, draw, tick) + B(apply, metrics)
With `use_spectral_norm` (ed_model.py:79-82) the step is spectral_norm_fwd -> A on w_eff -> B(gradients only) ->
spectral_norm_bwd -> adam_flat.

EdLatentEngine(..., fused=False) (or MELO_ED_LATENT_FUSED=0) runs the same step on the per-layer launches EdEngine's
classifier tail uses (linear_fwd / softmax_ce / linear_dgrad / wgrad_multi / rng_fill / adam_flat): the comparator of the
tests and of tools/ed_latent_bench.py.  The public surface is EdEngine's, so train_ed's epoch loops and checkpoints work on
either.  There is no augmentation in latent mode: the reference applies none (ed_dataset.py:322-323).
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict
from typing import Dict, Optional

import torch

from .. import ops
from ..ops import ACT_GELU
from ..gan.engine import FlatParams, emotion_disc_spec
from .engine import EdEngine

Tensor = torch.Tensor

# The fused step is the default only once it has been measured no slower than the comparator in every alternation of
# tools/ed_latent_bench.py on the MI355X (DESIGN 9 f-2 holds the table, or says that there is none yet).
FUSED_DEFAULT = "0"


class EdLatentEngine(EdEngine):
    """One replica of the latent-mode emotion discriminator's training state on one GPU (input_mode == 'latent')."""

    def __init__(self, cfg: dict, device="cuda", batch_size: Optional[int] = None, max_notes: Optional[int] = None,
                 share: Optional["EdLatentEngine"] = None, fused: Optional[bool] = None):
        """max_notes is accepted for EdEngine's signature and unused.  share: see EdEngine.  fused: None = MELO_ED_LATENT_FUSED
        ('1' the two-launch step, '0' the per-layer comparator), which defaults to FUSED_DEFAULT."""
        if cfg.get("input_mode", "latent") != "latent":
            raise ValueError("EdLatentEngine: input_mode must be 'latent' (EdEngine pre-trains the 'notes' encoder)")
        self.cfg = cfg
        self.dev = d = torch.device(device)
        self.B = B = int(batch_size or cfg.get("batch_size", 64))
        self.D = D = int(cfg.get("latent_dim", 128))
        self.T = self.C = None
        self.n_classes = int(cfg.get("n_classes", 4))
        self.p_drop = float(cfg.get("dropout", 0.2))
        opt = cfg.get("optimizer", {})
        self.lr = float(opt.get("lr", 2e-4))
        self.betas = tuple(float(b) for b in opt.get("betas", (0.9, 0.999)))
        self.weight_decay = float(opt.get("weight_decay", 0.0))
        self.decoupled = str(opt.get("name", "adamw")).lower() == "adamw"
        self.fused = (os.environ.get("MELO_ED_LATENT_FUSED", FUSED_DEFAULT) != "0") if fused is None else bool(fused)
        spec, _, _ = emotion_disc_spec(cfg)
        self.mlp = tuple(int(h) for h in cfg.get("mlp_hidden", (256, 128)))
        self.chans = []
        if share is not None:
            if share.P.spec != spec or share.fused != self.fused:
                raise ValueError("EdLatentEngine(share=...): the two engines must have the same model configuration")
            self.P, self.buf = share.P, share.buf
        else:
            self.P = FlatParams(spec, d)
            self.buf: Dict[str, Tensor] = OrderedDict()
        self.sn_names = [f"classifier.net.{3 * j}" for j in range(len(self.mlp))] if cfg.get("use_spectral_norm", False) else []
        if share is not None:
            self.w_eff, self.sn_sigma = share.w_eff, share.sn_sigma
        else:
            self.w_eff, self.sn_sigma = {}, {}
            for nm in self.sn_names:
                shp = spec[nm + ".weight"]
                self.buf[nm + ".weight_u"] = torch.zeros(shp[0], device=d)
                self.buf[nm + ".weight_v"] = torch.zeros(math.prod(shp[1:]), device=d)
                self.w_eff[nm] = torch.zeros(shp, device=d)
                self.sn_sigma[nm] = torch.ones(1, device=d)
        f = lambda *s: torch.empty(*s, device=d)      # noqa: E731
        self.x = f(B, D)
        self.y = torch.zeros(B, dtype=torch.int64, device=d)
        self.cz = [f(B, h) for h in self.mlp]                    # pre-activations
        self.ca = [f(B, h) for h in self.mlp]                    # after GELU and dropout
        self.dcz = [f(B, h) for h in self.mlp]
        self.dmask = [torch.ones(B, h, device=d) for h in self.mlp]      # keep-mask / (1 - p)
        self.logits, self.dlogits = f(B, self.n_classes), f(B, self.n_classes)
        self.loss_rows = f(B)
        self.loss = torch.zeros(1, device=d)
        self.rng_step = share.rng_step if share is not None else torch.zeros(1, dtype=torch.int64, device=d)
        self.rng_seed = int(cfg.get("seed", 42))
        self.stream = share.stream if share is not None else torch.cuda.Stream(device=d)
        self._graphs = {}
        self._tails: Dict[int, "EdLatentEngine"] = {}
        self._owner = share if share is not None else self
        self.split_x = self.split_y = self.order = self.batch_base = self.serial_base = self.metrics = self.aug = None
        self.names = [f"classifier.net.{3 * j}" for j in range(len(self.mlp))] + ["classifier.head"]
        self.net = None
        if self.fused:      # the kernels' domain (layer count, widths, classes) is checked here: ValueError
            self.net = ops.MlpNet(B, [self._w(nm) for nm in self.names], [self.P.p[nm + ".bias"] for nm in self.names],
                                  self.cz, self.ca, self.dcz, self.dmask)
            self.w_off = [self.P.offsets[nm + ".weight"][0] for nm in self.names]
            self.b_off = [self.P.offsets[nm + ".bias"][0] for nm in self.names]

    # ---- state in / out ---------------------------------------------------------------------------------
    def tail(self, rows: int) -> "EdLatentEngine":
        """The same model (shared parameters / optimiser state / buffers) at a batch of `rows` < B samples."""
        if not 0 < rows < self.B:
            raise ValueError(f"tail: rows={rows} must be in (0, {self.B})")
        if rows not in self._tails:
            self._tails[rows] = EdLatentEngine(self.cfg, self.dev, rows, share=self, fused=self.fused)
            self._tails[rows].lr = self.lr
        return self._tails[rows]

    def state_dict(self) -> "OrderedDict[str, Tensor]":
        """Keys and shapes of EmotionDiscriminator.state_dict() in latent mode (ed_model.py:72-95,123-130):
        classifier.net.{0,3,...}.{weight,bias} and classifier.head.{weight,bias}; under spectral norm weight_orig / _u / _v."""
        sd = self.P.state_dict()
        for nm in self.sn_names:
            sd[nm + ".weight_orig"] = sd.pop(nm + ".weight")
            sd[nm + ".weight_u"] = self.buf[nm + ".weight_u"].cpu().clone()
            sd[nm + ".weight_v"] = self.buf[nm + ".weight_v"].cpu().clone()
        return sd

    def attach_split(self, x: Tensor, y: Tensor, aug=None):
        """Make (x, y) -- (n, latent_dim) fp32 and (n,) int64, resident on the device -- the split step_staged stages its
        batches from.  aug must be None: latent mode has no augmentation (ed_dataset.py:322-323).  Captured staged steps
        hold the old addresses and are dropped."""
        if self._owner is not self:
            raise ValueError("attach_split: attach to the full-batch engine; its tails share the split")
        if aug is not None:
            raise ValueError("attach_split: latent mode has no augmentation")
        ops._chk(x, "x")
        ops._chk(y, "y", (x.shape[0],), torch.int64)
        if x.dim() != 2 or x.shape[1] != self.D or x.shape[0] == 0:
            raise ValueError(f"attach_split: x must be (n > 0, {self.D}), got {tuple(x.shape)}")
        self.split_x, self.split_y = x, y
        self.order = torch.arange(x.shape[0], dtype=torch.int64, device=self.dev)
        self.batch_base = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.serial_base = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.metrics = torch.zeros(2, device=self.dev)
        self._plain = ops.augment_spec("ed", self.rng_seed)          # everything off: the comparator's staging is a plain copy
        for e in (self, *self._tails.values()):
            e._graphs.pop("step_staged", None)

    def draw_masks(self):
        """One Philox launch draws the keep-masks (scaled) and advances the AdamW state (EdEngine.draw_masks); the fused
        steps draw inside launch A instead.  mg_rng_fill carries two masks: more hidden layers are refused here."""
        if len(self.mlp) > 2:
            raise ValueError("draw_masks: mg_rng_fill draws two masks; with more hidden layers use the fused backward_rng / step_rng")
        super().draw_masks()

    # ---- the two launches -----------------------------------------------------------------------------------
    def _launch_a(self, train: bool, draw: bool = False, tick: bool = False, stage: bool = False):
        o = self._owner
        st = (o.split_x, o.split_y, o.order, o.order.numel(), o.batch_base, self is not o) if stage else None
        ops.mlp_cls_fwd_bwd(self.net, self.x, self.y, self.logits, self.loss_rows, self.dlogits if train else None, train=train,
                            draw=draw, p_drop=self.p_drop, seed=self.rng_seed, step_counter=self.rng_step if (draw or stage) else None,
                            tick_state=self.P.state if tick else None, betas=self.betas, stage=st)
        if tick:
            self.P.ticked = True

    def _launch_b(self, apply: bool, metrics: bool = False):
        fp = self.P
        adam = None
        if apply:
            adam = dict(p=fp.data, m=fp.m, v=fp.v, state=fp.state, lr=self.lr, betas=self.betas,
                        weight_decay=self.weight_decay if self.decoupled else 0.0)
            fp.ticked = False
        ops.mlp_cls_wgrad_update(self.net, self.x, self.dlogits, self.w_off, self.b_off, fp.grad, self.loss_rows, self.loss, adam=adam,
                                 metrics=self._owner.metrics if metrics else None, logits=self.logits, y=self.y,
                                 rng_step=self.rng_step if apply else None)

    def _fused_step(self, draw: bool, tick: bool, stage: bool, apply: bool, metrics: bool):
        """[spectral_norm_fwd] A B [spectral_norm_bwd, adam_flat]: under spectral norm the gradient of w_eff has to pass
        through mg_spectral_norm_bwd before the update, so B stops after the gradients."""
        if self.sn_names:
            ops.spectral_norm_fwd(self._sn_layers(), True)
        self._launch_a(True, draw, tick, stage)
        self._launch_b(apply and not self.sn_names, metrics)
        if self.sn_names:
            ops.spectral_norm_bwd(self._sn_layers(with_grad=True))
            if apply:
                self.update()

    # ---- the step ---------------------------------------------------------------------------------------
    def forward(self, train: bool = True):
        """Eval: logits (and per-row cross-entropy terms).  Train, fused: launch A, which carries the data gradients too."""
        if self.fused:
            if self.sn_names:
                ops.spectral_norm_fwd(self._sn_layers(), train)
            return self._launch_a(train)
        P = self.P.p
        if self.sn_names:
            ops.spectral_norm_fwd(self._sn_layers(), train)
        feat = self.x
        for j in range(len(self.mlp)):
            ops.linear_fwd(feat, self._w(self.names[j]), self.ca[j], bias=P[self.names[j] + ".bias"], zout=self.cz[j], act=ACT_GELU,
                           emul=self.dmask[j] if train else None)
            feat = self.ca[j]
        ops.linear_fwd(feat, P["classifier.head.weight"], self.logits, bias=P["classifier.head.bias"])

    def backward(self):
        """Train-mode forward + cross-entropy + gradients of every parameter into self.P.grad (masks as they are in dmask)."""
        if self.fused:
            return self._fused_step(False, False, False, False, False)
        G = self.P.g
        self.forward(train=True)
        ops.softmax_ce(self.logits, self.y, self.loss, self.dlogits, 1.0)
        n = len(self.mlp)
        g, jobs = self.dlogits, []
        for j in range(n, 0, -1):          # layer j: the head (j == n) or hidden layer j; its input is ca[j - 1]
            nm = self.names[j]
            jobs.append(ops.linear_wgrad(self.ca[j - 1], g, G[nm + ".weight"], db=G[nm + ".bias"], defer=True))
            ops.linear_dgrad(g, self._w(nm), self.dcz[j - 1], gref=self.cz[j - 1], gact=ACT_GELU, emul=self.dmask[j - 1])
            g = self.dcz[j - 1]
        jobs.append(ops.linear_wgrad(self.x, g, G[self.names[0] + ".weight"], db=G[self.names[0] + ".bias"], defer=True))
        ops.wgrad_multi(jobs)
        if self.sn_names:
            ops.spectral_norm_bwd(self._sn_layers(with_grad=True))

    def backward_rng(self):
        if self.fused:
            return self._fused_step(True, True, False, False, False)
        self.draw_masks()
        self.backward()

    def step_rng(self):
        """Mask draw + forward/backward + AdamW as ONE capturable sequence: two launches when fused."""
        if self.fused:
            return self._fused_step(True, True, False, True, False)
        self.backward_rng()
        self.update()

    def step_staged(self):
        """step_rng with its batch staged from the attached split by the device-side cursor and the epoch's metrics
        accumulated, as ONE capturable sequence (EdEngine.step_staged): still two launches when fused."""
        o = self._owner
        if o.split_x is None:
            raise ValueError("step_staged: no split attached (attach_split)")
        if self.fused:
            return self._fused_step(True, True, True, True, True)
        if self.D % 4:
            raise ValueError("step_staged(fused=False): mg_stage_augment moves 16-byte pieces: latent_dim must be a multiple of 4")
        ops.stage_augment(o.split_x.view(-1, 1, self.D), o.split_y, self.x.view(-1, 1, self.D), self.y, self.B, o.order,
                          o.order.numel(), self.rng_step, o.batch_base, o.serial_base, o._plain, last=self is not o)
        self.backward_rng()
        self.update()
        ops.ed_metrics_acc(self.logits, self.y, self.loss, self.B, o.metrics)


def make_engine(cfg: dict, device="cuda", batch_size: Optional[int] = None, max_notes: Optional[int] = None, **kw) -> EdEngine:
    """The pre-training engine `input_mode` names (ed_model.py:123-145; the reference's default is 'latent')."""
    mode = cfg.get("input_mode", "latent")
    if mode == "notes":
        return EdEngine(cfg, device, batch_size, max_notes)
    if mode == "latent":
        return EdLatentEngine(cfg, device, batch_size, max_notes, **kw)
    raise ValueError("input_mode must be 'latent' or 'notes'")
