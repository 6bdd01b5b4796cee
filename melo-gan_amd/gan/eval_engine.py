"""What the sampler (gan/generate.py) and the evaluator (gan/evaluate.py) share: one GanEngine of `batch` rows that only ever
runs in eval mode, the loading of its weights, and the cache (eval_pass.GraphCache) of the hipGraph of one batch, replayed
until its key changes."""
from __future__ import annotations

import os
from typing import Optional

from ..eval_pass import GraphCache
from . import config as C


class EvalEngine:
    """Abstract: a subclass sets `error` (GenerateError or EvaluateError: what every check here raises) and _check_config."""

    def __init__(self, cfg: dict, ed_cfg: Optional[dict], device, batch: int):
        from .engine import GanEngine
        from .generate import EMOTIONS
        if int(batch) < 1:
            raise self.error(f"batch = {batch}: must be >= 1")
        cfg = {"LR_G": 0.0, "LR_D": 0.0, **C.with_gan_defaults(cfg, require=False)}      # the rates are never used here
        self.cfg, self.B = cfg, int(batch)      # in front of _check_config, which may read them (and what the subclass set
        self._check_config(cfg, ed_cfg)         # before calling this constructor); nothing else of the base exists yet
        self.has_ed = ed_cfg is not None
        if not self.has_ed:     # the engine always holds a classifier: the smallest one (latent mode), never run
            ed_cfg = dict(input_mode="latent", latent_dim=int(cfg["LATENT_DIM"]), mlp_hidden=[256, 128], n_classes=len(EMOTIONS))
        self.eng = GanEngine(cfg, ed_cfg, device, self.B)
        self.eng.init_weights(int(cfg.get("SEED", 42)))     # defines every parameter, the critic's unused ones included
        self.graphs = GraphCache()      # the hipGraph of one batch, replayed until what it froze changes

    def _check_config(self, cfg: dict, ed_cfg: Optional[dict]):
        """The subclass's checks of the normalised GAN config and of the ED config (None: no classifier); its module's
        check_ed_config when one is given (evaluate's puts a path in front of the message)."""
        raise NotImplementedError

    def _read(self, ck):
        """A checkpoint dict or path (gan_final.pth, gan_epochNNNN.pth; this trainer's or the reference's) -> (dict, name)."""
        from .generate import load_checkpoint
        if isinstance(ck, (str, os.PathLike)):
            return load_checkpoint(str(ck), err=self.error), str(ck)
        return ck, "checkpoint"

    def load_generator(self, ck):
        """G (with its BatchNorm running statistics) and E_num from a checkpoint dict or path."""
        from .generate import check_generator_checkpoint
        from .train_gan import load_generator_state
        ck, path = self._read(ck)
        check_generator_checkpoint(ck, self.cfg, path, err=self.error)
        load_generator_state(self.eng, ck)
        self.eng.params_changed()

    def load_ed(self, path: str):
        """The frozen classifier (train_ed's ed_best.pth or a bare state_dict; spectral-norm keys folded)."""
        from .train_gan import load_ed_checkpoint
        if not self.has_ed:
            raise self.error(f"this {type(self).__name__} was built without an ED config")
        if not os.path.isfile(path):
            raise self.error(f"ED checkpoint {path} does not exist")
        load_ed_checkpoint(self.eng, path)
