"""What the sampler (gan/generate.py) and the evaluator (gan/evaluate.py) share: one GanEngine of `batch` rows that only ever
runs in eval mode, the loading of its weights, and the cache (eval_pass.GraphCache) of the hipGraph of one batch, replayed
until its key changes.  recalibrate_bn gives an engine that holds AVERAGED weights (EMA_DECAY, gan/ema.py) the BatchNorm running
statistics of those weights."""
from __future__ import annotations

import os
from typing import Optional

import torch

from .. import ops
from ..checkpoints import check_generator_checkpoint, ema_checkpoint, load_ed_checkpoint, load_generator_state, read_checkpoint
from ..eval_pass import GraphCache
from ..pieces import EMOTIONS
from . import config as C
from .engine import GanEngine


class EvalEngine:
    """Abstract: a subclass sets `error` (GenerateError or EvaluateError: what every check here raises) and _check_config."""

    def __init__(self, cfg: dict, ed_cfg: Optional[dict], device, batch: int):
        if int(batch) < 1:
            raise self.error(f"batch = {batch}: must be >= 1")
        cfg = {"LR_G": 0.0, "LR_D": 0.0, **C.with_gan_defaults(cfg, require=False)}      # the rates are never used here
        cfg["EMA_DECAY"] = 0.0                  # nothing is trained here: no shadow of this engine's own
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
        if isinstance(ck, (str, os.PathLike)):      # weights_only=None, torch's default: a GAN file holds tensors and numbers
            return read_checkpoint(str(ck), self.error, weights_only=None), str(ck)
        return ck, "checkpoint"

    def load_generator(self, ck, ema: bool = False) -> str:
        """G (with its BatchNorm running statistics) and E_num from a checkpoint dict or path.  ema: the averaged weights and
        their recalibrated statistics from a full checkpoint's `ema` block instead (a *_ema.pth file is an ordinary {G, E_num}
        file and needs no flag).  Returns which weights were loaded: "ema" or "raw"."""
        ck, path = self._read(ck)
        if ema:
            ck = ema_checkpoint(ck, path, self.error)
        check_generator_checkpoint(ck, self.cfg, path, err=self.error)
        load_generator_state(self.eng, ck)
        self.eng.params_changed()
        return "ema" if ema else "raw"

    def copy_ema_from(self, src):
        """The AVERAGED generator + encoder of a training engine (same config, EMA_DECAY > 0), device to device, cast to fp32 by
        torch; the BatchNorm buffers are the training engine's until recalibrate_bn replaces them.  Reads `src` only; ordered
        behind the caller's current stream."""
        e = self.eng
        if src.ema is None:
            raise self.error("copy_ema_from: the training engine keeps no average (EMA_DECAY = 0)")
        if e.GE.n != src.GE.n or list(e.GE.spec.items()) != list(src.GE.spec.items()):
            raise self.error("copy_ema_from: the engines were built from different configs")
        e.stream.wait_stream(torch.cuda.current_stream(e.dev))
        with torch.cuda.stream(e.stream):
            e.GE.data[:e.GE.n].copy_(src.ema)           # fp64 -> fp32, round to nearest
            for k in e.Gbuf:
                e.Gbuf[k].copy_(src.Gbuf[k])
            e.num_batches_tracked = src.num_batches_tracked
            e.params_changed()

    def load_ed(self, path: str):
        """The frozen classifier (train_ed's ed_best.pth or a bare state_dict; spectral-norm keys folded)."""
        if not self.has_ed:
            raise self.error(f"this {type(self).__name__} was built without an ED config")
        if not os.path.isfile(path):
            raise self.error(f"ED checkpoint {path} does not exist")
        load_ed_checkpoint(self.eng, path)


def recalibrate_bn(eval_engine: EvalEngine, dataset, seed: int) -> bool:
    """BatchNorm running statistics for the weights `eval_engine` holds -- the update_bn step of weight averaging: G's two
    BatchNorm layers carry the statistics of the RAW weights' activations, which are the wrong ones under averaged weights.

    Walks `dataset` (a resident GANDataset: the training split) in file order in k = n // B full batches (the trailing partial
    batch is dropped, as training's drop_last): E_num in eval mode (dropout off, as generation runs it), noise from
    mg_eval_noise keyed by (seed, row), G's forward with the train-mode BatchNorm launches, batch j at momentum 1 / (j + 1) --
    torch's momentum=None cumulative average -- so that the buffers end as the plain mean over the batches of the per-batch
    mean and unbiased variance.  Host code over existing kernels; writes this engine's buffers and activations only.
    n < B: the buffers stay as they are, a [WARN] is printed, returns False."""
    eng, B = eval_engine.eng, eval_engine.B
    n = len(dataset)
    k = n // B
    if k < 1:
        print(f"[WARN] recalibrate_bn: the split holds {n} rows, fewer than one batch of {B}: the BatchNorm statistics stay "
              "those of the raw weights")
        return False
    if (tuple(dataset.numeric.shape) != (n, eng.num_in) or tuple(dataset.latent.shape) != (n, eng.latent_dim) or
            not dataset.numeric.is_cuda):
        raise eval_engine.error("recalibrate_bn: the split's numeric features / latents do not match the config")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    cursors = torch.arange(k, dtype=torch.int64, device=eng.dev)
    base = torch.zeros(1, dtype=torch.int64, device=eng.dev)
    eng.stream.wait_stream(torch.cuda.current_stream(eng.dev))
    mom = eng.bn_mom
    try:
        with torch.cuda.stream(eng.stream):
            for j in range(k):
                eng.numeric.copy_(dataset.numeric[j * B:(j + 1) * B])
                if eng.latent_dim > 0:
                    eng.latent.copy_(dataset.latent[j * B:(j + 1) * B])
                ops.eval_noise(eng.noise, cursors[j:j + 1], base, n, seed)      # row r of batch j: key (seed, j B + r)
                eng.bn_mom = 1.0 / (j + 1)
                eng._e_fwd(False, "g", gin=True)
                eng._g_fwd(eng.notes, True, "g")
        torch.cuda.current_stream(eng.dev).wait_stream(eng.stream)
    finally:
        eng.bn_mom = mom
    eng.num_batches_tracked = k         # as update_bn leaves it: the batches of this pass
    return True
