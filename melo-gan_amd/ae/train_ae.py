#!/usr/bin/env python3
"""VAE trainer -- counterpart of /root/reference/src/ae/train_ae.py (same --config flag and ae_config.yaml keys:
MAX_NOTES, LATENT_DIM, BATCH_SIZE, LR, WEIGHT_DECAY, EPOCHS, KLD_WARMUP_EPOCHS, BETA, EARLY_STOP_PATIENCE,
CHECKPOINT_DIR, LOG_DIR; same checkpoints: ae_best.pth {'epoch','model_state'}, ae_final.pth = bare state_dict).

    python -m melo_gan_amd.ae.train_ae --config config/ae_config.yaml [--synthetic N]

Per batch (train_ae.py:110-122): forward, MSE + beta*KLD, backward, clip_grad_norm_(1.0), AdamW -- all inside
VaeEngine.  Per epoch (train_ae.py:101-107,126-199): KL warm-up beta, validation with beta=1, ReduceLROnPlateau
(factor 0.5, patience 5, min_lr 1e-6), best-checkpoint, early stopping.  Data: row-aligned
<SPLITS_DIR>/{train,val}/notes.npy arrays kept in HBM (the reference's per-file .npz loader is host I/O and out of
scope).  AUGMENT.{tempo_jitter, pitch_shift, note_dropout, velocity_jitter, timing_jitter} (ae/dataset.py:11-38,89-104,
training split only): when any is non-zero the training batch is gathered AND augmented by one launch on the device
(ops.stage_augment, program 'ae'); with all of them zero (the committed config) the gather is index_select.  Per epoch the first
(up to) 6 validation rolls are reconstructed in eval mode and written as <RECON_DIR>/ep<E>_val<NNN>_{in,out}.mid
(train_ae.py:94,173-188; RECON_FREQ, RECON_DIR) through melo_gan_amd.midi.  --eval-every N (default 0: off): every N epochs the
held-out pass of ae/evaluate.py runs over the validation split on the training engine's weights and logs val/active_units,
val/pitch_accuracy, val/onset_recall and, when <SPLITS_DIR>/val/emotion.npy exists, val/fisher_ratio.
"""
import argparse
import os

import numpy as np
import torch

from .. import ops
from ..midi import save_recon_midi
from ..gan.config import load_config
from ..gan.train_gan import _scalar_writer
from ..gan.utils import label_indices
from .engine import VaeEngine


def _load_split(cfg, name, device):
    p = os.path.join(cfg.get("SPLITS_DIR", "data/splits"), name, "notes.npy")
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} not found (export the split's normalised notes to one array, or use --synthetic)")
    return torch.from_numpy(np.load(p).astype(np.float32)).to(device)


def augment_from_cfg(cfg, seed: int = 0):
    """The AUGMENT block as ops.augment_spec's struct, or None when it is absent or all zero.  Unknown keys and values out
    of range raise ValueError (no GPU needed)."""
    acfg = cfg.get("AUGMENT") or {}
    if not isinstance(acfg, dict):
        raise ValueError(f"AUGMENT must be a mapping, got {type(acfg).__name__}")
    aug = ops.augment_spec("ae", seed, **acfg)
    return aug if any(acfg.get(k, 0) != 0 for k in ops.AUG_AE_KEYS) else None


def _val_labels(cfg, n, device):
    """The validation split's class indices for --eval-every, or None without <SPLITS_DIR>/val/emotion.npy."""
    p = os.path.join(cfg.get("SPLITS_DIR", "data/splits"), "val", "emotion.npy")
    if not os.path.exists(p):
        return None
    idx = label_indices(np.load(p, allow_pickle=True), None)       # unchecked here: the evaluator refuses what lies outside
    if len(idx) != n:
        raise ValueError(f"{p} holds {len(idx)} entries, the validation split {n} rows")
    return idx.to(device)


def train(cfg, synthetic: int = 0, eval_every: int = 0):
    aug = augment_from_cfg(cfg, int(cfg.get("SEED", 0)))
    if not torch.cuda.is_available():
        raise RuntimeError("melo_gan_amd has no CPU path: a MI355X (ROCm) device is required")
    dev = torch.device("cuda", torch.cuda.current_device())
    model_dir, log_dir = cfg.get("CHECKPOINT_DIR", "models/ae"), cfg.get("LOG_DIR", "experiments/ae")
    os.makedirs(model_dir, exist_ok=True)
    B, T = cfg["BATCH_SIZE"], cfg["MAX_NOTES"]
    if synthetic:
        g = torch.Generator().manual_seed(0)
        train_x = (torch.rand(synthetic, T, 4, generator=g) * 2 - 1).to(dev)
        val_x = (torch.rand(max(B, synthetic // 4), T, 4, generator=g) * 2 - 1).to(dev)
    else:
        train_x, val_x = _load_split(cfg, "train", dev), _load_split(cfg, "val", dev)
    print(f"Train files: {len(train_x)}   Val files: {len(val_x)}")
    eng = VaeEngine(cfg, dev, B)
    eng.init_weights(0)
    writer = _scalar_writer(log_dir)
    evaluator = val_y = None
    if eval_every > 0:          # reads the training engine's parameters and buffers; writes nothing of it
        from .evaluate import VaeEvaluator
        evaluator = VaeEvaluator(cfg, dev, B, share=eng)
        val_y = None if synthetic else _val_labels(cfg, len(val_x), dev)
    best_val, no_improve, patience = float("inf"), 0, cfg.get("EARLY_STOP_PATIENCE", 10)
    warm, final_beta = cfg.get("KLD_WARMUP_EPOCHS", 25), float(cfg.get("BETA", 1.0))
    sched_bad, sched_best = 0, float("inf")
    gen = torch.Generator().manual_seed(0)
    eps = torch.empty(B, eng.latent, device=dev)
    acc = torch.zeros(3, device=dev)
    if aug is not None:        # the augmented gather's cursor: batch number, and the serial of the epoch's first sample
        batch_no, zero, serial0 = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(3))
        xb = torch.empty(B, T, 4, device=dev)
    with torch.cuda.stream(eng.stream):
        for epoch in range(1, cfg["EPOCHS"] + 1):
            beta = final_beta if epoch >= warm else min(final_beta, (epoch / warm) * final_beta)
            perm = torch.randperm(len(train_x), generator=gen).to(dev)
            acc.zero_()
            nb = len(train_x) // B
            for i in range(nb):
                if aug is None:
                    eng.step(train_x.index_select(0, perm[i * B:(i + 1) * B]), eps.normal_(), beta)
                else:
                    batch_no.fill_(i)
                    serial0.fill_((epoch - 1) * len(train_x))
                    ops.stage_augment(train_x, None, xb, None, B, perm, len(train_x), batch_no, zero, serial0, aug)
                    eng.step(xb, eps.normal_(), beta)
                acc += eng.loss
            tr = (acc / max(1, nb)).tolist()
            acc.zero_()
            vb = 0
            # validation: eval-mode BN, beta = 1; drop_last=False (train_ae.py:67), every batch counts once (:153-155)
            for i in range(0, len(val_x), B):
                e = eng.tail(min(B, len(val_x) - i))
                e.x.copy_(val_x[i:i + e.B])
                e.eps.copy_(eps[:e.B].normal_())
                e.forward(train=False)
                ops.vae_loss(e.recon, e.x, e.mu, e.lv, 1.0, e.loss)
                acc += e.loss
                vb += 1
            if vb == 0:
                raise ValueError("the validation split is empty")
            va = (acc / vb).tolist()
            # ReduceLROnPlateau(factor 0.5, patience 5, min_lr 1e-6), train_ae.py:80
            if va[0] < sched_best * (1 - 1e-4):
                sched_best, sched_bad = va[0], 0
            else:
                sched_bad += 1
                if sched_bad > 5:
                    eng.lr, sched_bad = max(eng.lr * 0.5, 1e-6), 0
            print(f"[Epoch {epoch}] Train: {tr[0]:.6f} (Recon: {tr[1]:.6f}, KLD: {tr[2]:.6f}) | "
                  f"Val: {va[0]:.6f} (Recon: {va[1]:.6f}, KLD: {va[2]:.6f})")
            for tag, v in (("loss/train_total", tr[0]), ("loss/train_recon", tr[1]), ("loss/train_kld", tr[2]),
                           ("loss/val_total", va[0]), ("loss/val_recon", va[1]), ("loss/val_kld", va[2]),
                           ("lr", eng.lr), ("beta", beta)):
                writer.add_scalar(tag, v, epoch)
            if evaluator is not None and epoch % eval_every == 0:
                o = evaluator.evaluate(val_x, val_y)["overall"]
                for tag in ("active_units", "pitch_accuracy", "onset_recall"):
                    if o[tag] is not None:
                        writer.add_scalar("val/" + tag, o[tag], epoch)
                if val_y is not None and o["fisher_ratio_mean"] is not None:
                    writer.add_scalar("val/fisher_ratio", o["fisher_ratio_mean"], epoch)
            # reconstructions of the first (up to) 6 validation rolls, eval mode, batch 1 (train_ae.py:94,173-188)
            if epoch % cfg.get("RECON_FREQ", 1) == 0:
                recon_dir = cfg.get("RECON_DIR", os.path.join(log_dir, "reconstructions"))
                e1 = eng.tail(1)
                for j in range(min(6, len(val_x))):
                    e1.x.copy_(val_x[j:j + 1])
                    e1.eps.copy_(eps[:1].normal_())
                    e1.forward(train=False)
                    save_recon_midi(val_x[j].cpu().numpy(), e1.recon[0].cpu().numpy(), recon_dir, f"ep{epoch}_val{j:03d}")
            if va[0] < best_val:
                best_val, no_improve = va[0], 0
                torch.save({"epoch": epoch, "model_state": eng.state_dict()}, os.path.join(model_dir, "ae_best.pth"))
                print("Saved new best model ->", os.path.join(model_dir, "ae_best.pth"))
            else:
                no_improve += 1
            if no_improve >= patience:
                print("No improvement for", patience, "epochs. Early stopping.")
                break
    writer.close()
    print("Training complete. Best val:", best_val)
    torch.save(eng.state_dict(), os.path.join(model_dir, "ae_final.pth"))
    return eng


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, default="config/ae_config.yaml", help="Path to config yaml")
    parser.add_argument("--synthetic", type=int, default=0)
    parser.add_argument("--epochs", type=int, default=None)
    parser.add_argument("--eval-every", type=int, default=0, help="held-out VAE metrics of the validation split every N epochs")
    args = parser.parse_args(argv)
    cfg = load_config(args.config)
    if args.epochs is not None:
        cfg["EPOCHS"] = args.epochs
    train(cfg, args.synthetic, args.eval_every)


if __name__ == "__main__":
    main()
