"""Pre-training of the emotion discriminator on MI355X: one step of
/root/reference/src/emotion_discriminator/train_ed.py:51-82 -- train-mode forward (BatchNorm batch statistics, classifier
dropout), mean cross-entropy, backward, AdamW -- over libmelogan_hip.  The frozen, eval-mode use of the same network on
the GAN hot path lives in melo_gan_amd.gan.engine.GanEngine; the MLP tail's per-layer launches (layers.tail_fwd / tail_bwd)
are shared with it.  EdEngine's constructor builds what every classifier engine needs and then the input side (_init_input):
the convolutional encoder here, the batch of latents in latent_engine.EdLatentEngine.

Layout: activations (B, T, C) channels-last like everywhere else; parameters / gradients / Adam moments in one flat
fp32 buffer each (one fused AdamW launch); BatchNorm running statistics in `buf`.  Backward is hand-derived:
  logits -> classifier (Linear, GELU, Dropout)* -> project Linear -> mean over T -> [GELU, BatchNorm(train), Conv1d]*.

`use_spectral_norm: true` (ed_model.py:29-32,79-82: every encoder Conv1d and the classifier's hidden Linear layers wrapped in
torch.nn.utils.spectral_norm): the flat parameter buffer holds weight_orig, the buffers hold weight_u / weight_v; one launch
per forward runs the power iteration (training mode) and writes the effective weights w_orig / sigma the layers then use
(mg_spectral_norm_fwd), one launch after the weight gradients turns d w_eff into d w_orig (mg_spectral_norm_bwd).
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict
from typing import Dict, Optional, Sequence

import torch

from .. import ops
from ..ops import ACT_GELU
from ..params import FlatParams, emotion_disc_spec, norm_buffers
from .layers import tail_bwd, tail_fwd

Tensor = torch.Tensor


class EdEngine:
    """One replica of the emotion discriminator's training state on one GPU (input_mode == 'notes')."""

    input_mode = "notes"
    _mode_error = ("EdEngine pre-trains input_mode='notes' (the convolutional encoder); input_mode='latent' is "
                   "latent_engine.EdLatentEngine (latent_engine.make_engine picks by input_mode)")

    def __init__(self, cfg: dict, device="cuda", batch_size: Optional[int] = None, max_notes: Optional[int] = None,
                 share: Optional["EdEngine"] = None):
        """What every classifier engine needs -- parameters, optimiser settings, spectral-norm state, the MLP tail's
        activations, the Philox counter, the staged split's fields -- then the input side (_init_input).
        share: another engine of this class whose parameters, optimiser state, BatchNorm buffers and Philox counter this one
        uses as its own -- the same model at a different batch size (the trailing partial batch of an epoch: the
        reference's loaders have no drop_last, ed_dataset.py:542-558)."""
        if cfg.get("input_mode", "latent") != self.input_mode:
            raise ValueError(self._mode_error)
        self.cfg = cfg
        self.dev = d = torch.device(device)
        self.B = B = int(batch_size or cfg.get("batch_size", 64))
        self.n_classes = int(cfg.get("n_classes", 4))
        self.p_drop = float(cfg.get("dropout", 0.2))
        opt = cfg.get("optimizer", {})
        self.lr = float(opt.get("lr", 2e-4))
        self.betas = tuple(float(b) for b in opt.get("betas", (0.9, 0.999)))
        self.weight_decay = float(opt.get("weight_decay", 0.0))
        self.decoupled = str(opt.get("name", "adamw")).lower() == "adamw"
        spec, bufs, self.chans = emotion_disc_spec(cfg)          # latent mode: no buffers, no convolutions
        if share is not None:
            if share.P.spec != spec:
                raise ValueError(f"{type(self).__name__}(share=...): the two engines must have the same model configuration")
            self.P, self.buf = share.P, share.buf
        else:
            self.P = FlatParams(spec, d)
            self.buf: Dict[str, Tensor] = norm_buffers(bufs, d)
        self.mlp = tuple(int(h) for h in cfg.get("mlp_hidden", (256, 128)))
        self.names = [f"classifier.net.{3 * j}" for j in range(len(self.mlp))] + ["classifier.head"]      # the MLP tail's layers
        # spectral normalisation: which layers, their u / v buffers (module state), effective weights and sigmas (derived)
        self.sn_names = []
        if cfg.get("use_spectral_norm", False):
            self.sn_names = [f"encoder.conv.{i}.net.0" for i in range(len(self.chans))] + self.names[:-1]
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
        self.y = torch.zeros(B, dtype=torch.int64, device=d)
        self.cz = [f(B, h) for h in self.mlp]                    # classifier pre-activations
        self.ca = [f(B, h) for h in self.mlp]                    # after GELU and dropout
        self.dcz = [f(B, h) for h in self.mlp]
        self.dmask = [torch.ones(B, h, device=d) for h in self.mlp]      # keep-mask / (1 - p)
        self.logits, self.dlogits = f(B, self.n_classes), f(B, self.n_classes)
        self.loss = torch.zeros(1, device=d)
        self.rng_step = share.rng_step if share is not None else torch.zeros(1, dtype=torch.int64, device=d)
        self.rng_seed = int(cfg.get("seed", 42))
        self.stream = share.stream if share is not None else torch.cuda.Stream(device=d)
        self._graphs = {}
        self.updates = 0         # optimiser steps this engine issued: a graph that advances it baked the learning rate (set_lr)
        self._tails: Dict[int, "EdEngine"] = {}
        # the resident training split of the staged step (attach_split); a tail stages from its owner's
        self._owner = share if share is not None else self
        self.split_x = self.split_y = self.order = self.batch_base = self.serial_base = self.metrics = self.aug = None
        self._init_input(max_notes)

    def _init_input(self, max_notes: Optional[int]):
        """The convolutional encoder's side of the state: the batch of notes and everything up to the classifier's input."""
        cfg, d, B, chans = self.cfg, self.dev, self.B, self.chans
        self.T = T = int(max_notes or cfg.get("max_notes", 512))
        self.C = C = int(cfg.get("note_dim", 4))
        # three-tap layers by minimal filtering (csrc/conv_wino.hip: 2/3 of the direct form's matrix-pipe work) where the
        # problem is big enough to be bound by it: forward with >= 128 output columns, data-gradient with >= 128 input channels
        # (the GAN engine's rule); the weights change every step, so both filter images of every such layer are transformed
        # by ONE launch at the top of the step.  MELO_ED_WINO=0: the direct window GEMMs.
        wino = os.environ.get("MELO_ED_WINO", "1") == "1" and B * T >= 4096
        self.wino_f = [bool(wino and k == 3 and co >= 128 and ops.wino3_supported(B, T, ci, co)) for (ci, co, k) in chans]
        self.wino_d = [bool(wino and k == 3 and ci >= 128 and i > 0 and ops.wino3_supported(B, T, co, ci)) for i, (ci, co, k) in enumerate(chans)]
        wimg = lambda on, cin, n: torch.zeros(cin // 4, 4, n, 4, device=d) if on else None  # noqa: E731
        self.wino_wf = [wimg(f_, ci, co) for f_, (ci, co, _) in zip(self.wino_f, chans)]
        self.wino_wd = [wimg(f_, co, ci) for f_, (ci, co, _) in zip(self.wino_d, chans)]
        hid = cfg.get("notes_hidden", 256)
        f = lambda *s: torch.empty(*s, device=d)      # noqa: E731
        self.x = f(B, T, C)
        self.z = [f(B, T, co) for (_, co, _) in chans]           # conv output (bias included), BatchNorm input
        self.a = [f(B, T, co) for (_, co, _) in chans]           # GELU(BatchNorm(z))
        self.dz = [f(B, T, co) for (_, co, _) in chans]
        self.da = [f(B, T, co) for (_, co, _) in chans]
        self.bn_mean = [f(co) for (_, co, _) in chans]
        self.bn_invstd = [f(co) for (_, co, _) in chans]
        self.pool, self.dpool = f(B, chans[-1][1]), f(B, chans[-1][1])
        self.proj, self.dproj = f(B, hid), f(B, hid)

    # ---- state in / out ---------------------------------------------------------------------------------
    def init_weights(self, seed: int = 42):
        """torch's default initialisation of the reference module (the trainer applies no weights_init to the ED):
        Conv1d / Linear weight and bias ~ U(-1/sqrt(fan_in), 1/sqrt(fan_in)); BatchNorm gamma = 1, beta = 0."""
        g = torch.Generator().manual_seed(seed)
        for k, s in self.P.spec.items():
            if ".net.1." in k:                                   # BatchNorm1d affine
                self.P.p[k].fill_(1.0 if k.endswith("weight") else 0.0)
                continue
            wshape = self.P.spec[k[:-len("bias")] + "weight"] if k.endswith("bias") else s
            bound = 1.0 / math.sqrt(math.prod(wshape[1:]))
            self.P.p[k].copy_((torch.rand(s, generator=g) * 2 - 1) * bound)
        for k, v in self.buf.items():
            if k.endswith("weight_u") or k.endswith("weight_v"):      # torch: normalize(randn) (spectral_norm.py, SpectralNorm.apply)
                r = torch.randn(v.shape, generator=g)
                v.copy_(r / r.norm().clamp_min(1e-12))
            else:
                v.fill_(1.0 if k.endswith("running_var") else 0.0)

    def set_lr(self, lr: float):
        """ReduceLROnPlateau: the learning rate is a launch argument of the AdamW kernel, baked into every captured
        graph that contains the update -- those whose capture saw `updates` advance (ops.run_graphed's record): they are
        dropped and re-captured with the new rate on their next run.  Engines sharing this one's parameters (tail()) follow."""
        self.lr = float(lr)
        for k in [k for k, st in self._graphs.items() if st != "warm" and st.deltas[0]]:
            del self._graphs[k]
        for t in self._tails.values():
            t.set_lr(lr)

    def tail(self, rows: int) -> "EdEngine":
        """The same model (shared parameters / optimiser state / buffers) at a batch of `rows` < B samples."""
        if not 0 < rows < self.B:
            raise ValueError(f"tail: rows={rows} must be in (0, {self.B})")
        if rows not in self._tails:
            self._tails[rows] = type(self)(self.cfg, self.dev, rows, self.T, share=self, **self._tail_args())
            self._tails[rows].lr = self.lr
        return self._tails[rows]

    def _tail_args(self) -> dict:
        """Constructor arguments of a tail() engine beyond EdEngine's."""
        return {}

    def load_state(self, params: Dict[str, Tensor], buffers: Optional[Dict[str, Tensor]] = None):
        """params may be a torch state_dict of the reference module: a spectrally normalised layer's weight is `weight_orig`
        there, its `weight_u` / `weight_v` are buffers (taken from `params` too when `buffers` lacks them)."""
        params = dict(params)
        for nm in self.sn_names:
            if nm + ".weight_orig" in params:
                params[nm + ".weight"] = params[nm + ".weight_orig"]
        self.P.load(params)
        src = dict(params)
        src.update(buffers or {})
        for k, v in src.items():
            if k in self.buf:
                self.buf[k].copy_(v.to(torch.float32))

    def state_dict(self) -> "OrderedDict[str, Tensor]":
        """Keys and shapes of EmotionDiscriminator.state_dict() (ed_model.py), incl. num_batches_tracked."""
        sd = OrderedDict()
        P = self.P.state_dict()
        for i in range(len(self.chans)):
            pre = f"encoder.conv.{i}.net."
            sd[pre + "0.weight"], sd[pre + "0.bias"] = P[pre + "0.weight"], P[pre + "0.bias"]
            sd[pre + "1.weight"], sd[pre + "1.bias"] = P[pre + "1.weight"], P[pre + "1.bias"]
            sd[pre + "1.running_mean"] = self.buf[pre + "1.running_mean"].cpu().clone()
            sd[pre + "1.running_var"] = self.buf[pre + "1.running_var"].cpu().clone()
            sd[pre + "1.num_batches_tracked"] = torch.tensor(int(self.P.state[0].item()), dtype=torch.int64)
        for k, v in P.items():
            if k not in sd:
                sd[k] = v
        return self._sn_keys(sd)

    def _sn_keys(self, sd):
        """torch.nn.utils.spectral_norm's keys in a state_dict: weight_orig (parameter), weight_u, weight_v (buffers)."""
        for nm in self.sn_names:
            sd[nm + ".weight_orig"] = sd.pop(nm + ".weight")
            sd[nm + ".weight_u"] = self.buf[nm + ".weight_u"].cpu().clone()
            sd[nm + ".weight_v"] = self.buf[nm + ".weight_v"].cpu().clone()
        return sd

    def set_batch(self, x: Tensor, y: Tensor):
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)

    def attach_split(self, x: Tensor, y: Tensor, aug=None):
        """Make (x, y) -- (n, <a row of self.x>) fp32 and (n,) int64, resident on the device -- the split step_staged stages
        its batches from; `aug`: _split_aug.  Captured staged steps hold the old addresses and parameters and are dropped."""
        if self._owner is not self:
            raise ValueError("attach_split: attach to the full-batch engine; its tails share the split")
        aug = self._split_aug(aug)
        ops._chk(x, "x")
        ops._chk(y, "y", (x.shape[0],), torch.int64)
        row = tuple(self.x.shape[1:])
        if tuple(x.shape[1:]) != row or x.shape[0] == 0:
            raise ValueError(f"attach_split: x must be (n > 0, {', '.join(map(str, row))}), got {tuple(x.shape)}")
        self.split_x, self.split_y, self.aug = x, y, aug
        self.order = torch.arange(x.shape[0], dtype=torch.int64, device=self.dev)
        self.batch_base = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.serial_base = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.metrics = torch.zeros(2, device=self.dev)
        for e in (self, *self._tails.values()):
            e._graphs.pop("step_staged", None)

    def _split_aug(self, aug):
        """The split's augmentation (ops.augment_spec(...)); None: everything off, keyed by this engine's seed."""
        return aug if aug is not None else ops.augment_spec("ed", self.rng_seed)

    def set_epoch(self, order: Optional[Tensor], epoch_index: int):
        """Start an epoch of staged steps: `order` (n int64 row indices, host or device; None: the order buffer was written
        in place, e.g. by ops.weighted_order) becomes the epoch's order, the batch cursor restarts at the current step
        counter, the augmentation serials at epoch_index * n, and the epoch's metrics at zero."""
        if self.split_x is None:
            raise ValueError("set_epoch: no split attached (attach_split)")
        if order is not None:
            if order.dtype != torch.int64 or order.shape != self.order.shape:
                raise ValueError(f"set_epoch: order must be {tuple(self.order.shape)} int64")
            self.order.copy_(order)
        self.batch_base.copy_(self.rng_step)
        self.serial_base.fill_(int(epoch_index) * self.order.numel())
        self.metrics.zero_()

    def set_masks(self, masks: Sequence[Tensor]):
        """Injected classifier dropout masks, already scaled by 1/(1-p) (parity tests)."""
        for dst, m in zip(self.dmask, masks):
            dst.copy_(m.to(torch.float32), non_blocking=True)

    def draw_masks(self):
        """Production path: one Philox launch draws both keep-masks (scaled) and advances the AdamW state; the
        update advances the Philox counter (mg_rng_fill's adam_state rider / mg_adam_flat with state_ticked)."""
        ops.rng_fill(None, None, self.dmask[0], self.dmask[1] if len(self.dmask) > 1 else None, self.p_drop,
                     self.rng_seed, self.rng_step, tick_state=self.P.state, betas=self.betas)
        self.P.ticked = True

    # ---- the step ---------------------------------------------------------------------------------------
    def _sn_layers(self, with_grad: bool = False):
        out = []
        for nm in self.sn_names:
            ly = dict(w_orig=self.P.p[nm + ".weight"], w_eff=self.w_eff[nm], u=self.buf[nm + ".weight_u"],
                      v=self.buf[nm + ".weight_v"], sigma=self.sn_sigma[nm])
            if with_grad:
                ly["dw"] = self.P.g[nm + ".weight"]
            out.append(ly)
        return out

    def _w(self, name: str) -> Tensor:
        """The weight layer `name` computes with: w_orig / sigma when it is spectrally normalised."""
        return self.w_eff[name] if name in self.w_eff else self.P.p[name + ".weight"]

    def _tail_layers(self):
        """The classifier tail's [(weight it computes with, bias)], the head last (layers.tail_fwd / tail_bwd)."""
        return [(self._w(nm), self.P.p[nm + ".bias"]) for nm in self.names]

    def _tail_bwd(self, feat: Tensor, dfeat: Optional[Tensor], jobs: list):
        """dlogits back through the tail (d/d(pre-activation) = dropout mask * GELU'(cz)) to dfeat, the gradient of the
        tail's input `feat`; every layer's weight-gradient job is appended to `jobs`."""
        G = self.P.g
        grads = [(G[nm + ".weight"], G[nm + ".bias"]) for nm in self.names]
        tail_bwd(self.dlogits, feat, self._tail_layers(), self.cz, self.ca, self.dcz, self.dmask, dfeat, jobs, grads)

    def forward(self, train: bool = True):
        P, x = self.P.p, self.x
        if self.sn_names:          # power iteration (training mode) + effective weights of every normalised layer: one launch
            ops.spectral_norm_fwd(self._sn_layers(), train)
        jobs = []
        for i, (ci, co, _) in enumerate(self.chans):
            w = self._w(f"encoder.conv.{i}.net.0")
            if self.wino_f[i]:
                jobs.append((w, self.wino_wf[i], co, ci, ci * 3, 3, False))
            if self.wino_d[i] and train:
                jobs.append((w, self.wino_wd[i], ci, co, 3, ci * 3, True))
        if jobs:
            ops.wino3_weights_multi(jobs)
        for i in range(len(self.chans)):
            pre = f"encoder.conv.{i}.net."
            if self.wino_f[i]:
                ops.conv_wino3(x, self.wino_wf[i], self.z[i], bias=P[pre + "0.bias"])
            else:
                ops.conv1d_fwd(x, self._w(pre + "0"), self.z[i], 1, bias=P[pre + "0.bias"])
            if train:
                ops.bn_train_fwd(self.z[i], self.a[i], P[pre + "1.weight"], P[pre + "1.bias"], self.buf[pre + "1.running_mean"],
                                 self.buf[pre + "1.running_var"], self.bn_mean[i], self.bn_invstd[i], act=ACT_GELU)
            else:
                ops.bn_eval_fwd(self.z[i], self.a[i], P[pre + "1.weight"], P[pre + "1.bias"], self.buf[pre + "1.running_mean"],
                                self.buf[pre + "1.running_var"], act=ACT_GELU)
            x = self.a[i]
        ops.meanT_fwd(x, self.pool)
        ops.linear_fwd(self.pool, P["encoder.project.weight"], self.proj, bias=P["encoder.project.bias"])
        tail_fwd(self.proj, self._tail_layers(), self.cz, self.ca, self.logits, self.dmask if train else None)

    def backward(self):
        """Train-mode forward + cross-entropy + gradients of every parameter into self.P.grad."""
        P, G = self.P.p, self.P.g
        self.forward(train=True)
        ops.softmax_ce(self.logits, self.y, self.loss, self.dlogits, 1.0)
        jobs = []        # weight gradients: collected, launched together at the end (ops.wgrad_multi)
        self._tail_bwd(self.proj, self.dproj, jobs)
        jobs.append(ops.linear_wgrad(self.pool, self.dproj, G["encoder.project.weight"], db=G["encoder.project.bias"], defer=True))
        ops.linear_dgrad(self.dproj, P["encoder.project.weight"], self.dpool)
        last = len(self.chans) - 1
        ops.meanT_bwd(self.dpool, self.da[last])
        for i in range(last, -1, -1):
            pre = f"encoder.conv.{i}.net."
            ops.bn_train_bwd(self.da[i], self.a[i], self.z[i], self.dz[i], P[pre + "1.weight"], self.bn_mean[i],
                             self.bn_invstd[i], G[pre + "1.weight"], G[pre + "1.bias"], act=ACT_GELU, beta=P[pre + "1.bias"])
            xin = self.a[i - 1] if i > 0 else self.x
            jobs.append(ops.conv1d_wgrad(xin, self.dz[i], G[pre + "0.weight"], 1, db=G[pre + "0.bias"], defer=True))
            if i > 0 and self.wino_d[i]:
                ops.conv_wino3(self.dz[i], self.wino_wd[i], self.da[i - 1])
            elif i > 0:
                ops.conv1d_dgrad(self.dz[i], self._w(pre + "0"), self.da[i - 1], 1)
        ops.wgrad_multi(jobs)
        if self.sn_names:          # the launches above left d w_eff: through w_eff = w_orig / sigma to d w_orig
            ops.spectral_norm_bwd(self._sn_layers(with_grad=True))

    def backward_rng(self):
        self.draw_masks()
        self.backward()

    def step_rng(self):
        """Mask draw + forward/backward + AdamW as ONE capturable sequence (one graph launch per training step)."""
        self.backward_rng()
        self.update()

    def step_staged(self):
        """step_rng with its batch staged (and augmented) from the attached split by the device-side cursor, and the epoch's
        metrics accumulated, as ONE capturable sequence: a replay trains on the NEXT batch of the epoch's order.  The full
        engine takes batch number (step counter - base); a tail takes the last `B` positions of the order."""
        o = self._owner
        if o.split_x is None:
            raise ValueError("step_staged: no split attached (attach_split)")
        ops.stage_augment(o.split_x, o.split_y, self.x, self.y, self.B, o.order, o.order.numel(), self.rng_step, o.batch_base,
                          o.serial_base, o.aug, last=self is not o)
        self.backward_rng()
        self.update()
        ops.ed_metrics_acc(self.logits, self.y, self.loss, self.B, o.metrics)

    def update(self):
        fp = self.P
        ops.adam_flat(fp.data, fp.grad, fp.m, fp.v, fp.state, self.lr, *self.betas,
                      weight_decay=self.weight_decay if self.decoupled else 0.0,
                      ticked_rng_step=self.rng_step if fp.ticked else None)
        fp.ticked = False
        self.updates += 1

    def run(self, name: str, use_graph: bool = True):
        """hipGraph replay of a sub-step -- backward_rng, update, step_rng, step_staged, forward_eval -- (first call eager,
        second call captures).  What its Python does to host_state() is recorded at the capture and re-applied by each
        replay (ops.run_graphed); an update arriving behind the mask draw that advanced its state is a key of its own."""
        fn = getattr(self, name)
        if not use_graph:
            return fn()
        ops.run_graphed(self._graphs, name, fn, self)

    def host_state(self):
        """The host state the sub-steps change and a graph replay has to re-apply: (flags, counters)."""
        return (self.P.ticked,), (self.updates,)

    def set_host_state(self, flags, counters):
        (self.P.ticked,), (self.updates,) = flags, counters

    def forward_eval(self):
        self.forward(train=False)
