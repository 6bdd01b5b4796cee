#!/usr/bin/env python3
"""Pre-training of the emotion discriminator -- the MI355X-native counterpart of
/root/reference/src/emotion_discriminator/train_ed.py (same YAML keys, same loop: train epoch, validation epoch,
ReduceLROnPlateau, best / periodic checkpoints {"epoch","model","optimizer","cfg"}, early stopping):

    python -m melo_gan_amd.emotion_discriminator.train_ed --config config/ed_config.yaml

Data: the row-aligned arrays the GAN trainer already uses, `<splits_dir>/<stem of {split}_split_csv>/{notes,emotion}.npy`
(kept resident in HBM); the reference's per-file manifest/.npz loader (ed_dataset.py) is out of scope.  Like the
reference's loaders (no drop_last, ed_dataset.py:542-558) an epoch ends with the trailing partial batch, run by a second
engine of that batch size over the same parameters (EdEngine.tail); metrics are sample-weighted (train_ed.py:75-82).
--synthetic N trains on N random rolls (smoke runs without the git-ignored dataset).  --eval-test: after training, the best
checkpoint is loaded into a fresh evaluator (emotion_discriminator.evaluate) and judged on the test split (the validation
split when there is none); the report goes to <checkpoint_dir>/ed_eval.json.  The training itself is the same with or
without the flag.

input_mode 'notes' trains the convolutional encoder (EdEngine); 'latent' (the reference's default) trains the MLP on the
(N, latent_dim) encoder latents that melo_gan_amd.ae.encode exports (EdLatentEngine: two launches per step).  The latents
are looked up in the reference's order (ed_dataset.py:69-90): `{split}_encoder_feats_path`, `encoder_feats_path`, then
`encoder_feats.npy` beside the split's emotion.npy.  Only a regular float array is read; the per-file mapping loaders are out
of scope.  Latent mode has no augmentation (ed_dataset.py:322-323): `augment: true` is accepted and does nothing.

Training epochs run the engine's staged step (EdEngine.step_staged): one graph replay per batch stages the batch from the
resident split by a device-side cursor, augments it in the same pass, trains on it and adds to the epoch's metrics.  The
reference's data-plane keys act on the train split only, as there (ed_dataset.py:499,505):
  augment, augment_cfg.{noise_std, dropout_prob, pitch_shift_prob}   ed_dataset.py:299-314, applied on the device
  use_weighted_sampler                                               ed_dataset.py:505-549: the epoch's order is drawn on the
                                                                     device with weight 1 / class count, with replacement
  preload                                                            needs nothing here: the split is resident in HBM
"""
import argparse
import os
from pathlib import Path

import numpy as np
import torch

from .. import ops
from ..gan import config as C
from ..gan.utils import label_indices, seed_everything
from .engine import EdEngine
from .latent_engine import make_engine


class Plateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau (rel threshold mode, cooldown 0, min_lr 0), train_ed.py:101-123."""

    def __init__(self, mode="min", factor=0.5, patience=5, threshold=1e-4):
        self.mode, self.factor, self.patience, self.threshold = mode, factor, patience, threshold
        self.best = float("inf") if mode == "min" else -float("inf")
        self.bad = 0

    def step(self, metric: float, lr: float) -> float:
        better = metric < self.best * (1 - self.threshold) if self.mode == "min" else metric > self.best * (1 + self.threshold)
        if better:
            self.best, self.bad = metric, 0
            return lr
        self.bad += 1
        if self.bad > self.patience:
            self.bad = 0
            return lr * self.factor
        return lr


def split_dir(cfg: dict, split: str) -> str:
    key = f"{split}_split_csv"
    if not cfg.get(key):
        raise ValueError(f"Missing split csv for '{split}' in config; expected key '{key}'.")
    return os.path.join(cfg.get("splits_dir", os.path.dirname(cfg[key]) or "data/splits"), Path(cfg[key]).stem)


def load_split(cfg: dict, split: str, device):
    d = split_dir(cfg, split)
    paths = [os.path.join(d, n) for n in ("notes.npy", "emotion.npy")]
    if not all(os.path.exists(p) for p in paths):
        raise FileNotFoundError(f"{paths}: export the split to notes.npy / emotion.npy (the per-file .npz loader of the "
                                "reference is not implemented)")
    notes = torch.from_numpy(np.ascontiguousarray(np.load(paths[0]), dtype=np.float32)).to(device)
    labels = label_indices(np.load(paths[1], allow_pickle=True), int(cfg.get("n_classes", 4)), f"{split} split labels").to(device)
    return notes, labels


def resolve_encoder_feats(cfg: dict, split: str) -> str:
    """ed_dataset.py:69-90: the split's own key, the global key, then encoder_feats.npy in the split's array directory."""
    for key in (f"{split}_encoder_feats_path", "encoder_feats_path"):
        if cfg.get(key):
            return cfg[key]
    return os.path.join(split_dir(cfg, split), "encoder_feats.npy")


def latent_rows(feats, labels, latent_dim: int, where: str = "encoder_feats"):
    """The (N, latent_dim) fp32 latents and their labels as the reference pairs them (ed_dataset.py:417-428): row i of the
    array belongs to row i of the split; an array shorter than the split drops the split's trailing rows."""
    feats = np.asarray(feats)
    if feats.dtype == object or feats.dtype.kind not in "fiu":
        raise ValueError(f"{where}: expected a regular float array (N, {latent_dim}), got dtype {feats.dtype}: the per-file "
                         "mapping form of encoder_feats is not implemented -- export the latents with melo_gan_amd.ae.encode")
    if feats.ndim != 2 or feats.shape[1] != latent_dim:
        raise ValueError(f"{where}: expected shape (N, latent_dim = {latent_dim}), got {tuple(feats.shape)}")
    n, m = feats.shape[0], len(labels)
    if n < m:
        print(f"[ed_dataset] encoder_feats ndarray shorter ({n}) than CSV ({m}): dropping last {m - n} rows.")
        labels = labels[:n]
    else:
        print(f"[ed_dataset] encoder_feats ndarray length OK ({n}) for CSV ({m}).")
        feats = feats[:m]
    return np.ascontiguousarray(feats, dtype=np.float32), labels


def load_latent_split(cfg: dict, split: str, device):
    path, lab_path = resolve_encoder_feats(cfg, split), os.path.join(split_dir(cfg, split), "emotion.npy")
    for p in (path, lab_path):
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p}: export the split's latents / labels to encoder_feats.npy (melo_gan_amd.ae.encode) and "
                                    "emotion.npy")
    feats, emotions = latent_rows(np.load(path, allow_pickle=True), np.load(lab_path, allow_pickle=True), int(cfg.get("latent_dim", 128)),
                                  path)
    labels = label_indices(emotions, int(cfg.get("n_classes", 4)), f"{split} split labels")      # of the rows that are left
    return torch.from_numpy(feats).to(device), labels.to(device)


def synthetic_latent_split(n, D, seed, device):
    """Learnable toy latents: x ~ N(0, 1), the class is the quadrant of (x0, x1) (x1 absent: of x0 alone)."""
    x = np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
    y = 2 * (x[:, 0] > 0).astype(np.int64) + ((x[:, 1] > 0).astype(np.int64) if D > 1 else 0)
    return torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)


def synthetic_split(n, T, Cn, seed, device):
    """Learnable toy labels: the class is the quadrant of (mean pitch, mean velocity) of a roll."""
    g = np.random.default_rng(seed)
    x = g.uniform(-1, 1, (n, T, Cn)).astype(np.float32)
    bias = g.uniform(-0.5, 0.5, (n, 1, 2)).astype(np.float32)
    x[:, :, :2] = np.clip(x[:, :, :2] * 0.5 + bias, -1, 1)
    y = (x[:, :, 0].mean(1) > 0).astype(np.int64) * 2 + (x[:, :, 1].mean(1) > 0).astype(np.int64)
    return torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)


def augment_from_cfg(cfg: dict):
    """The `augment` / `augment_cfg` keys (ed_dataset.py:299-314,499) as ops.augment_spec's struct, or None when `augment` is
    off.  Unknown keys inside augment_cfg and values out of range raise ValueError (no GPU needed)."""
    if not cfg.get("augment", False):
        return None
    acfg = cfg.get("augment_cfg") or {}
    if not isinstance(acfg, dict):
        raise ValueError(f"augment_cfg must be a mapping, got {type(acfg).__name__}")
    return ops.augment_spec("ed", int(cfg.get("seed", 42)), **acfg)


def sampler_weights(labels) -> torch.Tensor:
    """ed_dataset.py:531-536: one fp64 weight per row, 1 / (rows of its class)."""
    lab = torch.as_tensor(labels, dtype=torch.int64).cpu()
    return 1.0 / torch.bincount(lab).to(torch.float64)[lab]


def run_epoch_staged(eng: EdEngine, epoch_index: int, use_graph: bool, gen=None, cdf=None):
    """One training epoch over the split attached to `eng` (EdEngine.attach_split) by the staged step: the same batches, in
    the same order, from the same generator as run_epoch's host path when cdf is None; with cdf (ops.sampler_cdf) the order
    is the weighted sampler's and never visits the host.  epoch_index (from 0) keys the augmentation and the sampler."""
    n, B = eng.order.numel(), eng.B
    if cdf is None:
        eng.set_epoch(torch.randperm(n, generator=gen), epoch_index)
    else:
        ops.weighted_order(cdf, eng.order, eng.rng_seed, epoch_index)
        eng.set_epoch(None, epoch_index)
    for lo in range(0, n, B):
        rows = min(B, n - lo)
        (eng if rows == B else eng.tail(rows)).run("step_staged", use_graph)
    loss, a = (eng.metrics / n).tolist()
    return loss, a


def run_epoch(eng: EdEngine, x, y, train: bool, use_graph: bool, gen=None):
    """train_ed.py:51-82: sample-weighted mean loss and accuracy of one pass; one device->host read per epoch."""
    n, B = x.shape[0], eng.B
    if n == 0:
        raise ValueError("run_epoch: the split is empty")
    perm = torch.randperm(n, generator=gen).to(x.device) if train else torch.arange(n, device=x.device)
    acc = torch.zeros(2, device=x.device)
    for lo in range(0, n, B):
        rows = min(B, n - lo)
        e = eng if rows == B else eng.tail(rows)          # trailing partial batch: same parameters, smaller batch
        idx = perm[lo:lo + rows]
        e.set_batch(x.index_select(0, idx), y.index_select(0, idx))
        if train:
            e.run("step_rng", use_graph)
        else:
            e.run("forward_eval", use_graph)
            ops.softmax_ce(e.logits, e.y, e.loss, None, 1.0)
        acc[0:1] += e.loss * rows
        acc[1:2] += (e.logits.argmax(dim=1) == e.y).float().sum()
    loss, a = (acc / n).tolist()
    return loss, a


def save_checkpoint(eng: EdEngine, cfg: dict, epoch: int, is_best: bool):
    """train_ed.py:30-48: <checkpoint_dir>/<save_name> for the best model, ed_epochNNN.pth otherwise."""
    os.makedirs(cfg.get("checkpoint_dir", "data/models/ed"), exist_ok=True)
    name = cfg.get("save_name", "ed_best.pth") if is_best else f"ed_epoch{epoch:03d}.pth"
    path = os.path.join(cfg.get("checkpoint_dir", "data/models/ed"), name)
    fp = eng.P
    opt = {"state": {"step": float(fp.state[0].item()), "exp_avg": fp.m.cpu(), "exp_avg_sq": fp.v.cpu()},
           "param_groups": [{"lr": eng.lr, "betas": eng.betas, "eps": 1e-8, "weight_decay": eng.weight_decay}],
           "layout": {k: list(v) for k, v in fp.offsets.items()}}
    torch.save({"epoch": epoch, "model": eng.state_dict(), "optimizer": opt, "cfg": cfg}, path)
    return path


def eval_best(cfg: dict, synthetic: int, val, device) -> dict:
    """--eval-test: the best checkpoint in a fresh evaluator on the test split, else on `val` = (x, labels); writes and returns
    the report."""
    import json
    from .evaluate import EdEvaluator
    ckdir = cfg.get("checkpoint_dir", "data/models/ed")
    path = os.path.join(ckdir, cfg.get("save_name", "ed_best.pth"))
    (x, y), source = val, "val"
    if not synthetic and cfg.get("test_split_csv"):
        try:
            x, y = (load_latent_split if cfg.get("input_mode", "latent") == "latent" else load_split)(cfg, "test", device)
            source = "test"
        except FileNotFoundError:
            print("[eval-test] no test split arrays: evaluating the validation split")
    ev = EdEvaluator(cfg, device, int(cfg.get("batch_size", 64)))
    ev.load(path)
    rep = ev.evaluate(x.contiguous(), y.contiguous())
    rep.update(model=path, split=source)
    out = os.path.join(ckdir, "ed_eval.json")
    with open(out, "w") as f:
        json.dump(rep, f, indent=1, allow_nan=False)
    print(f"[eval-test] {source}: accuracy {rep['overall']['accuracy']}, macro_f1 {rep['overall']['macro_f1']}, "
          f"ece {rep['overall']['ece']}, best T {rep['temperature']['best_T']} -> {out}")
    return rep


def train(cfg: dict, synthetic: int = 0, use_graph: bool = True, eval_test: bool = False):
    mode = cfg.get("input_mode", "latent")
    if mode not in ("latent", "notes"):
        raise ValueError("melo_gan_amd.emotion_discriminator.train_ed: input_mode must be 'latent' or 'notes'")
    latent = mode == "latent"
    aug = None if latent else augment_from_cfg(cfg)      # ValueError on a bad augment_cfg, before the GPU is touched
    if latent and cfg.get("augment", False):
        print("[ed_dataset] augment: true has no effect with input_mode=latent (the reference augments notes only)")
    if not torch.cuda.is_available():
        raise RuntimeError("melo_gan_amd has no CPU path: a MI355X (ROCm) device is required")
    seed_everything(cfg.get("seed", 42))
    device = torch.device("cuda", torch.cuda.current_device())
    T, Cn = int(cfg.get("max_notes", 512)), int(cfg.get("note_dim", 4))
    n_val = max(synthetic // 4, int(cfg.get("batch_size", 64)))
    if synthetic and latent:
        D = int(cfg.get("latent_dim", 128))
        xt, yt = synthetic_latent_split(synthetic, D, cfg.get("seed", 42), device)
        xv, yv = synthetic_latent_split(n_val, D, cfg.get("seed", 42) + 1, device)
    elif synthetic:
        xt, yt = synthetic_split(synthetic, T, Cn, cfg.get("seed", 42), device)
        xv, yv = synthetic_split(n_val, T, Cn, cfg.get("seed", 42) + 1, device)
    else:
        load = load_latent_split if latent else load_split
        (xt, yt), (xv, yv) = load(cfg, "train", device), load(cfg, "val", device)
    eng = make_engine(cfg, device, int(cfg.get("batch_size", 64)), T)
    eng.init_weights(cfg.get("seed", 42))
    if xt.shape[0] == 0:
        raise ValueError("train: the training split is empty")
    eng.attach_split(xt.contiguous(), yt.contiguous(), aug)
    cdf = None
    if cfg.get("use_weighted_sampler", False):
        cdf = ops.sampler_cdf(yt)
        counts = {c: k for c, k in enumerate(torch.bincount(yt.cpu()).tolist()) if k}
        print(f"[ed_dataset] Using WeightedRandomSampler: classes={counts}, samples={xt.shape[0]}")
    sch = cfg.get("scheduler") or {}
    plateau = None
    if str(sch.get("name", "")).lower() == "reducelronplateau":
        plateau = Plateau(sch.get("mode", "min"), sch.get("factor", 0.5), sch.get("patience", 5), sch.get("threshold", 1e-4))
    epochs, patience = cfg.get("num_epochs", 50), cfg.get("early_stopping_patience", 10)
    by_loss = cfg.get("metric_for_best", "val_loss") == "val_loss"
    best, best_epoch = (float("inf") if by_loss else 0.0), 0
    gen = torch.Generator().manual_seed(cfg.get("seed", 42))
    print("Starting Emotion Discriminator Training")
    print("Input mode:", mode, "| Device:", device, "| Epochs:", epochs, "| Best metric target:",
          cfg.get("metric_for_best", "val_loss"))
    with torch.cuda.stream(eng.stream):
        for epoch in range(1, epochs + 1):
            tl, ta = run_epoch_staged(eng, epoch - 1, use_graph, gen, cdf)
            vl, va = run_epoch(eng, xv, yv, False, use_graph)
            metric = vl if by_loss else va
            if plateau is not None:
                lr = plateau.step(metric, eng.lr)
                if lr != eng.lr:
                    eng.set_lr(lr)
            better = metric < best if by_loss else metric > best
            status = ""
            if better:
                best, best_epoch = metric, epoch
                save_checkpoint(eng, cfg, epoch, True)
                status = "New Best"
            print(f"[Epoch {epoch:03d}] Train-Loss={tl:.4f}, Train-Acc={ta:.3f} | Val-Loss={vl:.4f}, Val-Acc={va:.3f} {status}")
            if epoch - best_epoch >= patience:
                print(f"Early stopping triggered at epoch {epoch}. Best epoch was {best_epoch}.")
                break
            if epoch % cfg.get("save_freq", 5) == 0:
                save_checkpoint(eng, cfg, epoch, False)
    print("Training Completed. Best epoch:", best_epoch, "Best metric:", best)
    if eval_test and best_epoch:
        eval_best(cfg, synthetic, (xv, yv), device)
    return eng, best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default="config/ed_config.yaml")
    ap.add_argument("--synthetic", type=int, default=0, help="train on N synthetic rolls instead of the split arrays")
    ap.add_argument("--epochs", type=int, default=None, help="override num_epochs")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--eval-test", action="store_true", help="evaluate the best checkpoint on the test split afterwards")
    args = ap.parse_args(argv)
    cfg = C.load_config(args.config)
    if args.epochs is not None:
        cfg["num_epochs"] = args.epochs
    train(cfg, args.synthetic, not args.no_graph, args.eval_test)


if __name__ == "__main__":
    main()
