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
classifier tail uses (layers.tail_fwd / softmax_ce / layers.tail_bwd / wgrad_multi / rng_fill / adam_flat): the comparator of
the tests and of tools/ed_latent_bench.py.  The engine is built by EdEngine's constructor (its input side, _init_input, is the
batch of latents) and the public surface is EdEngine's, so train_ed's epoch loops and checkpoints work on either.  There is no augmentation in latent mode: the reference applies none (ed_dataset.py:322-323).
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Optional

import torch

from .. import ops
from .engine import EdEngine
from .layers import tail_fwd

Tensor = torch.Tensor

# The fused step is the default only once it has been measured no slower than the comparator in every alternation of
# tools/ed_latent_bench.py on the MI355X (DESIGN 9 f-2 holds the table, or says that there is none yet).
FUSED_DEFAULT = "0"


class EdLatentEngine(EdEngine):
    """One replica of the latent-mode emotion discriminator's training state on one GPU (input_mode == 'latent')."""
    input_mode = "latent"
    _mode_error = "EdLatentEngine: input_mode must be 'latent' (EdEngine pre-trains the 'notes' encoder)"

    def __init__(self, cfg: dict, device="cuda", batch_size: Optional[int] = None, max_notes: Optional[int] = None,
                 share: Optional["EdLatentEngine"] = None, fused: Optional[bool] = None):
        """max_notes is accepted for EdEngine's signature and unused.  share: see EdEngine.  fused: None = MELO_ED_LATENT_FUSED
        ('1' the two-launch step, '0' the per-layer comparator), which defaults to FUSED_DEFAULT."""
        self.fused = (os.environ.get("MELO_ED_LATENT_FUSED", FUSED_DEFAULT) != "0") if fused is None else bool(fused)
        if share is not None and share.fused != self.fused:
            raise ValueError("EdLatentEngine(share=...): the two engines must have the same model configuration")
        super().__init__(cfg, device, batch_size, None, share)
        self.loss_rows = torch.empty(self.B, device=self.dev)
        self._plain = ops.augment_spec("ed", self.rng_seed)          # everything off: the comparator's staging is a plain copy
        self.net = None
        if self.fused:      # the kernels' domain (layer count, widths, classes) is checked here: ValueError
            self.net = ops.MlpNet(self.B, [self._w(nm) for nm in self.names], [self.P.p[nm + ".bias"] for nm in self.names],
                                  self.cz, self.ca, self.dcz, self.dmask)
            self.w_off = [self.P.offsets[nm + ".weight"][0] for nm in self.names]
            self.b_off = [self.P.offsets[nm + ".bias"][0] for nm in self.names]

    def _init_input(self, max_notes):
        """The batch of latents; no encoder (EdEngine._init_input)."""
        self.D = int(self.cfg.get("latent_dim", 128))
        self.T = self.C = None
        self.x = torch.empty(self.B, self.D, device=self.dev)

    # ---- state in / out ---------------------------------------------------------------------------------
    def _tail_args(self) -> dict:
        return dict(fused=self.fused)

    def state_dict(self) -> "OrderedDict[str, Tensor]":
        """Keys and shapes of EmotionDiscriminator.state_dict() in latent mode (ed_model.py:72-95,123-130):
        classifier.net.{0,3,...}.{weight,bias} and classifier.head.{weight,bias}; under spectral norm weight_orig / _u / _v."""
        return self._sn_keys(self.P.state_dict())

    def _split_aug(self, aug):
        """aug must be None: latent mode has no augmentation (ed_dataset.py:322-323)."""
        if aug is not None:
            raise ValueError("attach_split: latent mode has no augmentation")
        return None

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
            self.updates += 1
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
        if self.sn_names:
            ops.spectral_norm_fwd(self._sn_layers(), train)
        tail_fwd(self.x, self._tail_layers(), self.cz, self.ca, self.logits, self.dmask if train else None)

    def backward(self):
        """Train-mode forward + cross-entropy + gradients of every parameter into self.P.grad (masks as they are in dmask)."""
        if self.fused:
            return self._fused_step(False, False, False, False, False)
        self.forward(train=True)
        ops.softmax_ce(self.logits, self.y, self.loss, self.dlogits, 1.0)
        jobs = []
        self._tail_bwd(self.x, None, jobs)
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
