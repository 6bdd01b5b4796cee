#!/usr/bin/env python3
"""WGAN-GP trainer with numeric-feature conditioning and a frozen emotion discriminator -- the
MI355X-native counterpart of /root/reference/src/gan/train_gan.py (same CLI, same YAML keys and
defaults, same checkpoint layout):

    python -m melo_gan_amd.gan.train_gan --config config/gan_config.yaml \
        --ed_config config/ed_config.yaml --ed_ckpt data/models/ed/ed_best.pth

Differences that do not change results: the epoch's batches come from an HBM-resident copy of the split
(no DataLoader workers), every D-step / G-step is a replayed hipGraph over libmelogan_hip, and the three
per-epoch scalars are accumulated on the device and read back once per epoch (the reference calls .item()
three times per batch, train_gan.py:205,250-251).  Extra flags (--synthetic, --epochs, --no-graph) exist
for smoke runs without the (git-ignored) dataset.  --eval-every N (not in the reference, which never looks at held-out data
while it trains) evaluates the current weights on VAL_SPLIT every N epochs (gan/evaluate.py) and logs Val/W_dist,
Val/ED_Acc_Fake, Val/ED_CE_Fake and Val/ED_Acc_Real; it changes nothing the training step reads.  EMA_DECAY d in (0, 1) (gan/ema.py; off by
default) keeps an exponential moving average of G and E_num behind every generator update: full checkpoints gain an `ema` key,
gan_final_ema.pth holds the averaged generator as an ordinary {G, E_num} file, and --eval-every also logs ValEMA/*.

Data parallel (not in the reference, which is single-GPU): launched under torch.distributed.run
(`--nnodes=1 --nproc-per-node N --master-addr 127.0.0.1`) every rank holds a replica, takes every N-th batch of the
epoch's (identically shuffled) order and averages gradients through melo_gan_amd.gan.dp.DataParallel (RCCL over
xGMI); rank 0 logs and checkpoints.
"""
import argparse
import json
import os
import time

import torch

from ..checkpoints import ema_block, load_ed_checkpoint, resume_checkpoint, save_checkpoint, save_ema_final
from . import config as C
from .dataset import GANDataset
from .dp import DataParallel
from .engine import GanEngine
from .utils import seed_everything


def _scalar_writer(log_dir):
    os.makedirs(log_dir, exist_ok=True)
    try:                                    # same tags as the reference when tensorboard is installed
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter(log_dir=log_dir)
    except Exception:
        class _Jsonl:
            def __init__(self, d):
                self.f = open(os.path.join(d, "scalars.jsonl"), "a")

            def add_scalar(self, tag, value, step):
                self.f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step), "wall_time": time.time()}) + "\n")
                self.f.flush()

            def close(self):
                self.f.close()
        return _Jsonl(log_dir)


def train(cfg: dict, ed_cfg: dict, ed_ckpt: str, synthetic: int = 0, use_graph: bool = True, resume: str = None,
          eval_every: int = 0):
    """eval_every = N > 0: after every N-th epoch rank 0 evaluates the current weights on VAL_SPLIT (with `synthetic`: on a
    second synthetic split drawn with SEED + 1) in an Evaluator of its own (gan/evaluate.py) and writes the Val/* scalars.
    The pass reads the training engine's weights and nothing else: a run with it ends in the same checkpoints, bit for bit."""
    cfg = C.with_gan_defaults(cfg, require=not synthetic)
    seed_everything(cfg.get("SEED", 42))
    if not torch.cuda.is_available():
        raise RuntimeError("melo_gan_amd has no CPU path: a MI355X (ROCm) device is required")
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if os.environ.get("MELO_SHARE_GPU") == "1":     # rehearsal on a single-GPU box: ranks share the device
            local_rank %= torch.cuda.device_count()
        torch.cuda.set_device(local_rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(os.environ.get("MELO_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    device = torch.device("cuda", torch.cuda.current_device())
    log = print if rank == 0 else (lambda *a, **k: None)
    log(f"Using main device: {device}" + (f" ({world} data-parallel ranks)" if world > 1 else ""))
    B = cfg.get("BATCH_SIZE", 32)
    if synthetic:
        ds = GANDataset.synthetic(synthetic, cfg["MAX_NOTES"], cfg["NOTE_DIM"], cfg["LATENT_DIM"], cfg.get("SEED", 42), device)
    else:
        ds = GANDataset.from_split(cfg, cfg["TRAIN_SPLIT"], cfg.get("ENCODER_FEATS_TRAIN"), device)
    log(f"Train set size: {len(ds)}")
    # ED_DTYPE: bf16 = the secondary configuration (frozen emotion discriminator stored in bf16); the
    # reference has no such key and the default is its fp32 arithmetic
    eng = GanEngine(cfg, ed_cfg, device, B, ed_dtype=str(cfg.get("ED_DTYPE", "fp32")))
    eng.init_weights(cfg.get("SEED", 42))
    load_ed_checkpoint(eng, ed_ckpt)
    start_epoch = resume_checkpoint(eng, resume) if resume else 0
    if resume:
        log(f"[INFO] Resumed from {resume} (epoch {start_epoch})")
    dp = DataParallel(eng, world, dist)
    dp.broadcast_params()
    eng.seed(cfg.get("SEED", 42) + rank)            # rank-offset Philox key: every shard draws its own noise
    ema_on = eng.ema is not None
    if ema_on and world > 1 and not resume:
        eng.ema_reset()             # the shadow of the broadcast parameters: every rank keeps its own, and they stay identical
    if ema_on:
        log(f"[INFO] Averaging the generator: EMA_DECAY {eng.ema_decay}, ramp {'on' if eng.ema_ramp else 'off'}, from "
            f"generator step {int(eng.ema_offset)}")
    writer = _scalar_writer(cfg.get("LOG_DIR", "experiments/gan/logs")) if rank == 0 else None
    os.makedirs(cfg.get("CHECKPOINT_DIR", "experiments/gan/checkpoints"), exist_ok=True)
    os.makedirs(cfg.get("SAMPLE_DIR", "experiments/gan/samples"), exist_ok=True)
    critic_iters = cfg.get("CRITIC_ITERS", 5)
    sums = torch.zeros(3, device=device)        # sum loss_d, sum g_adv, sum g_emo (device-side accumulation)
    shuffle_gen = torch.Generator().manual_seed(cfg.get("SEED", 42))
    if resume:
        # continue the two random streams where the checkpointed run left them, so that the resumed epochs are the ones an
        # uninterrupted run would have trained: the Philox step counter (advanced once per batch, by the critic's update) and
        # the shuffle generator (one permutation per epoch)
        eng.rng_step.fill_(int(eng.D.state[0].item()))
        for _ in range(start_epoch):
            torch.randperm(len(ds), generator=shuffle_gen)
    evaluator = val_ds = None
    if ema_on and rank == 0:        # holds the averaged weights while their BatchNorm statistics are recomputed (save, ValEMA)
        from .evaluate import Evaluator
        evaluator = Evaluator(cfg, ed_cfg, device, B)
    if eval_every > 0 and rank == 0:
        from .evaluate import Evaluator
        if synthetic:
            val_ds = GANDataset.synthetic(synthetic, cfg["MAX_NOTES"], cfg["NOTE_DIM"], cfg["LATENT_DIM"], cfg.get("SEED", 42) + 1,
                                          device)
        else:
            val_ds = GANDataset.from_split(cfg, cfg["VAL_SPLIT"], cfg.get("ENCODER_FEATS_VAL"), device, resident=True)
        log(f"Validation set size: {len(val_ds)} (evaluated every {eval_every} epoch(s))")
        evaluator = evaluator or Evaluator(cfg, ed_cfg, device, B)
    log("Starting WGAN-GP Training with Emotion Guidance...")

    def val_scalars(rep):
        return {"W_dist": rep["critic"]["w_dist"], "ED_Acc_Fake": rep["ed_fake"]["accuracy"], "ED_CE_Fake": rep["ed_fake"]["ce"],
                "ED_Acc_Real": rep["ed_real"]["accuracy"] if rep["ed_real"] else None}

    def averaged():
        """The evaluator holding the averaged weights with their own BatchNorm statistics (over the training split)."""
        from .eval_engine import recalibrate_bn
        evaluator.copy_ema_from(eng)
        recalibrate_bn(evaluator, ds, cfg.get("SEED", 42))
        return evaluator

    def epoch_batches():
        """Per batch of this rank's share of the epoch: stage it (or, for a bound resident split, nothing: the step's first
        launch gathers batch k of the epoch's order on the device) and yield its index."""
        if ds.resident:
            for k in range(ds.start_epoch(eng, shuffle_gen)):
                yield k
            return
        # every rank walks the same shuffled order and takes the batches rank, rank + world, ...; a trailing
        # incomplete round is dropped so that all ranks issue the same collectives
        usable = len(ds) // B - (len(ds) // B) % world
        for gi, batch in enumerate(ds.batches(B, shuffle_gen)):
            if gi >= usable:
                break
            if gi % world != rank:
                continue
            batch.stage(eng)           # one gather launch from the streamed rolls into the engine's buffers
            yield gi // world

    with torch.cuda.stream(eng.stream):
        if ds.resident:
            ds.bind(eng, B, rank, world)
        for epoch in range(start_epoch + 1, cfg["EPOCHS"] + 1):
            sums.zero_()
            steps = 0
            for batch_idx in epoch_batches():
                g_step = (batch_idx + 1) % critic_iters == 0
                dp.step(use_graph, g_step)
                sums[0:1] += eng.loss_d_out[0:1]
                if g_step:
                    sums[1:2] += eng.adv
                    sums[2:3] += eng.emo
                steps += 1
            s = sums.tolist()                                    # the epoch's only device->host sync
            g_steps = max(1, steps // critic_iters)
            steps = max(1, steps)
            log(f"Epoch {epoch}/{cfg['EPOCHS']} | D_loss: {s[0] / steps:.4f} | G_adv: {s[1] / g_steps:.4f} | "
                  f"G_emo: {s[2] / g_steps:.4f}")
            if rank != 0:
                continue
            writer.add_scalar("Loss/Critic", s[0] / steps, epoch)
            writer.add_scalar("Loss/Generator_Adv", s[1] / g_steps, epoch)
            writer.add_scalar("Loss/Generator_Emo", s[2] / g_steps, epoch)
            if val_ds is not None and epoch % eval_every == 0:
                evaluator.copy_from(eng)        # device-to-device, behind this stream's work; the engine is only read
                rep = evaluator.evaluate(val_ds, cfg.get("SEED", 42))
                val = {"Val/" + t: v for t, v in val_scalars(rep).items()}
                for tag, v in val.items():
                    if v is not None:
                        writer.add_scalar(tag, v, epoch)
                log(f"Epoch {epoch}/{cfg['EPOCHS']} | validation ({rep['n']} rows) | " +
                    " | ".join(f"{t[4:]}: {v:.4f}" for t, v in val.items() if v is not None))
                if ema_on:      # the same pass, seed and critic under the averaged generator: a paired second line
                    rep = averaged().evaluate(val_ds, cfg.get("SEED", 42))
                    val = {"ValEMA/" + t: v for t, v in val_scalars(rep).items()}
                    for tag, v in val.items():
                        if v is not None:
                            writer.add_scalar(tag, v, epoch)
                    log(f"Epoch {epoch}/{cfg['EPOCHS']} | validation, averaged weights | " +
                        " | ".join(f"{t[7:]}: {v:.4f}" for t, v in val.items() if v is not None))
            if epoch % cfg.get("SAVE_FREQ", 5) == 0:
                save_checkpoint(eng, os.path.join(cfg["CHECKPOINT_DIR"], f"gan_epoch{epoch:04d}.pth"), epoch, full=True,
                                ema=ema_block(eng, averaged()) if ema_on else None)
        if rank == 0 and ema_on:
            save_ema_final(ema_block(eng, averaged()), os.path.join(cfg["CHECKPOINT_DIR"], "gan_final_ema.pth"))
    if rank == 0:
        save_checkpoint(eng, os.path.join(cfg["CHECKPOINT_DIR"], "gan_final.pth"), full=False)
        writer.close()
    if world > 1:
        dist.barrier(async_op=True).wait()
        dist.destroy_process_group()
    log("Training Complete.")
    return eng


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, default="config/gan_config.yaml", help="Path to the main GAN config")
    parser.add_argument("--ed_config", type=str, default="config/ed_config.yaml", help="Path to the ED config")
    parser.add_argument("--ed_ckpt", type=str, default="data/models/ed/ed_best.pth")
    parser.add_argument("--synthetic", type=int, default=0, help="train on N synthetic rolls instead of TRAIN_SPLIT")
    parser.add_argument("--epochs", type=int, default=None, help="override EPOCHS")
    parser.add_argument("--no-graph", action="store_true")
    parser.add_argument("--resume", type=str, default=None, help="gan_epochNNNN.pth to continue from (G, D, E_num, opt_G, opt_D)")
    parser.add_argument("--eval-every", type=int, default=0,
                        help="evaluate on VAL_SPLIT every N epochs (gan/evaluate.py; 0 = off)")
    args = parser.parse_args(argv)
    cfg = C.load_config(args.config)
    ed_cfg = C.load_config(args.ed_config)
    if args.epochs is not None:
        cfg["EPOCHS"] = args.epochs
    train(cfg, ed_cfg, args.ed_ckpt, args.synthetic, not args.no_graph, args.resume, args.eval_every)


if __name__ == "__main__":
    main()
