"""The .pth files training leaves on disk -- the GAN's, the VAE's, the emotion classifier's -- read, checked and written in one
place: the only module that calls torch.load.  It knows shapes from params.py and engines by the attributes it touches, and
imports no engine, trainer or tool.  Every check raises the caller's error class with the caller's text."""
from __future__ import annotations

import math
import os
from collections import OrderedDict

import torch

from .params import discriminator_spec, emotion_disc_spec, feature_encoder_spec, generator_spec


def read_checkpoint(path: str, err, what: str = "checkpoint", weights_only=None):
    """torch.load(path) on the host; a missing or unreadable file raises err.  weights_only goes to torch.load as it is: every
    call site passes it and says why."""
    if not os.path.isfile(path):
        raise err(f"{what} {path} does not exist")
    try:
        return torch.load(path, map_location="cpu", weights_only=weights_only)
    except Exception as e:      # noqa: BLE001 -- any unreadable file is the same user error
        raise err(f"cannot read {what} {path}: {e}") from e


def state_mismatches(sd, shapes):
    """A state_dict against {key: shape}: (the keys it lacks, [(key, its shape, the wanted shape)] of those it holds with
    another shape), both in the order of `shapes`.  What to do about either is the caller's policy."""
    missing = [k for k in shapes if k not in sd]
    bad = [(k, tuple(sd[k].shape), tuple(s)) for k, s in shapes.items() if k in sd and tuple(sd[k].shape) != tuple(s)]
    return missing, bad


# ---- GAN ------------------------------------------------------------------------------------------------------------
def check_generator_checkpoint(ck, cfg: dict, path: str = "checkpoint", err=ValueError):
    """A dict with 'G' (with its BatchNorm running statistics) and 'E_num' whose tensors have the shapes the config implies."""
    if not isinstance(ck, dict) or "G" not in ck or "E_num" not in ck:
        have = sorted(ck) if isinstance(ck, dict) else type(ck).__name__
        raise err(f"{path}: not a generator checkpoint (needs 'G' and 'E_num'; has {have})")
    gspec = generator_spec(int(cfg["NOISE_DIM"]), int(cfg["LATENT_DIM"]), cfg.get("INTEGRATION_MODE", "conditioning"), 512,
                           int(cfg["MAX_NOTES"]), int(cfg["NOTE_DIM"]), int(cfg.get("ENCODER_OUT_DIM", 128)))
    for bn, ch in (("decoder.deconv.1", 128), ("decoder.deconv.4", 64)):
        gspec[bn + ".running_mean"] = gspec[bn + ".running_var"] = (ch,)
    espec = feature_encoder_spec(int(cfg.get("NUMERIC_INPUT_DIM", 6)), tuple(cfg.get("ENCODER_HIDDEN", [256, 128])),
                                 int(cfg.get("ENCODER_OUT_DIM", 128)))
    _check_part(ck, "G", gspec, path, err)
    _check_part(ck, "E_num", espec, path, err)


def check_critic_checkpoint(ck: dict, cfg: dict, path: str = "checkpoint", err=ValueError) -> bool:
    """Whether the checkpoint holds a critic ('D'); one it holds must have the config's shapes."""
    if "D" in ck:
        _check_part(ck, "D", discriminator_spec(int(cfg["NOTE_DIM"]), 256, int(cfg.get("ENCODER_OUT_DIM", 128))), path, err)
    return "D" in ck


def _check_part(ck: dict, part: str, spec, path: str, err):
    missing, bad = state_mismatches(ck[part], spec)
    if missing:
        raise err(f"{path}: {part} lacks {missing[0]}")
    if bad:
        raise err("{}: {}.{} has shape {}, the GAN config implies {}".format(path, part, *bad[0]))


def ema_checkpoint(ck, path: str, err) -> dict:
    """{'G', 'E_num'} of a full checkpoint's `ema` block (save_checkpoint), for check_generator_checkpoint and
    load_generator_state; raises err, naming the file, when the checkpoint has none."""
    blk = ck.get("ema") if isinstance(ck, dict) else None
    if not isinstance(blk, dict) or "G" not in blk or "E_num" not in blk:
        have = sorted(ck) if isinstance(ck, dict) else type(ck).__name__
        raise err(f"{path}: no averaged weights in this checkpoint (--ema reads the 'ema' block of a full gan_epochNNNN.pth "
                  f"written with EMA_DECAY > 0; has {have}).  A *_ema.pth file loads without the flag")
    return {"G": blk["G"], "E_num": blk["E_num"]}


def load_generator_state(eng, ck: dict):
    """G (with its BatchNorm running statistics) and E_num of a checkpoint dict -- gan_final.pth or gan_epochNNNN.pth, of
    this trainer or the reference's.  The caller runs eng.params_changed() once everything is loaded."""
    eng.GE.load({**{"G." + k: v for k, v in ck["G"].items()}, **{"E." + k: v for k, v in ck["E_num"].items()}})
    for k in eng.Gbuf:
        eng.Gbuf[k].copy_(ck["G"][k].float())


def save_checkpoint(eng, path: str, epoch=None, full=True, ema=None):
    """train_gan.py:267-282: {'epoch','G','D','E_num','opt_G','opt_D'} every SAVE_FREQ epochs; final {'G','E_num'}.  ema: the
    block of ema_block() -- one more key, 'ema', of a full checkpoint (the reference's loaders index by key and ignore it)."""
    sd = eng.state_dicts()
    if not full:
        torch.save({"G": sd["G"], "E_num": sd["E_num"]}, path)
        return
    betas = tuple(eng.betas)
    ck = {"epoch": epoch, "G": sd["G"], "D": sd["D"], "E_num": sd["E_num"],
          "opt_G": adam_state_dict(eng.GE, eng.lr_g, betas), "opt_D": adam_state_dict(eng.D, eng.lr_d, betas)}
    if ema is not None:
        ck["ema"] = ema
    torch.save(ck, path)


def ema_block(eng, calib) -> dict:
    """The `ema` key of a full checkpoint: decay, ramp, offset; 'G' under G's state-dict keys -- the parameters float64 from the
    shadow, the BatchNorm buffers float32 from `calib` (an EvalEngine that holds the averaged weights, after recalibrate_bn),
    num_batches_tracked int64 -- and 'E_num', float64."""
    sd = eng.ema_state_dicts()
    G = OrderedDict()
    for k, v in sd["G"].items():
        G[k] = v
        if k in ("decoder.deconv.1.bias", "decoder.deconv.4.bias"):     # BN buffers follow weight/bias
            base = k[:-len("bias")]
            G[base + "running_mean"] = calib.eng.Gbuf[base + "running_mean"].cpu().clone()
            G[base + "running_var"] = calib.eng.Gbuf[base + "running_var"].cpu().clone()
            G[base + "num_batches_tracked"] = torch.tensor(calib.eng.num_batches_tracked, dtype=torch.int64)
    return {"decay": float(eng.ema_decay), "ramp": bool(eng.ema_ramp), "offset": float(eng.ema_offset), "G": G, "E_num": sd["E_num"]}


def save_ema_final(block: dict, path: str):
    """gan_final_ema.pth: gan_final.pth's keys with the averaged parameters rounded to float32 and the recalibrated buffers --
    an ordinary generator checkpoint (the reference's app.py loads it as it is)."""
    f32 = lambda sd: OrderedDict((k, v.float() if v.is_floating_point() else v) for k, v in sd.items())  # noqa: E731
    torch.save({"G": f32(block["G"]), "E_num": f32(block["E_num"])}, path)


def adam_state_dict(fp, lr: float, betas, eps: float = 1e-8, weight_decay: float = 0.0) -> dict:
    """The flat optimiser state as `torch.optim.Adam.state_dict()` of the reference's optimisers (train_gan.py:136-145:
    opt_G over list(G.parameters()) + list(E_num.parameters()), opt_D over D.parameters()): parameter i of the optimiser is
    entry i of the flat buffer's spec (module definition order, the generator's tensors before the numeric encoder's), with
    its own `step`, `exp_avg`, `exp_avg_sq`.  `optimizer.load_state_dict()` of a reference trainer accepts it as is."""
    step = float(fp.state[0].item())
    state = {}
    for i, k in enumerate(fp.spec):
        off, n = fp.offsets[k]
        state[i] = {"step": torch.tensor(step, dtype=torch.float32),
                    "exp_avg": fp.m[off:off + n].view(fp.spec[k]).detach().cpu().clone(),
                    "exp_avg_sq": fp.v[off:off + n].view(fp.spec[k]).detach().cpu().clone()}
    group = {"lr": float(lr), "betas": tuple(float(b) for b in betas), "eps": eps, "weight_decay": weight_decay, "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "params": list(range(len(fp.spec)))}
    return {"state": state, "param_groups": [group]}


def load_adam_state_dict(fp, sd: dict):
    """Inverse of adam_state_dict (resume): fills the flat moment buffers, the step counter and the running beta powers
    the update kernel keeps beside it (state = [step, beta1^step, beta2^step, -])."""
    state = sd["state"]
    if not state:                       # an optimiser that never stepped: fresh moments
        fp.m.zero_(); fp.v.zero_(); fp.state.zero_()
        return
    if len(state) != len(fp.spec):
        raise ValueError(f"optimizer state_dict has {len(state)} parameter entries, this optimiser has {len(fp.spec)}")
    steps = set()
    for i, k in enumerate(fp.spec):
        if i not in state:
            raise ValueError(f"optimizer state_dict lacks entry {i} ({k})")
        st = state[i]
        for part in ("exp_avg", "exp_avg_sq"):
            if tuple(st[part].shape) != tuple(fp.spec[k]):
                raise ValueError(f"optimizer state_dict entry {i} ({k}).{part}: shape {tuple(st[part].shape)} != {tuple(fp.spec[k])}")
        steps.add(float(st["step"]))
    if len(steps) != 1:
        raise ValueError(f"optimizer state_dict: per-parameter step counts differ ({sorted(steps)}); the flat optimiser keeps one")
    for i, k in enumerate(fp.spec):
        off, n = fp.offsets[k]
        fp.m[off:off + n].copy_(state[i]["exp_avg"].reshape(-1).to(fp.m.device))
        fp.v[off:off + n].copy_(state[i]["exp_avg_sq"].reshape(-1).to(fp.v.device))
    step = steps.pop()
    b1, b2 = sd["param_groups"][0]["betas"]
    fp.state[0], fp.state[1], fp.state[2] = step, float(b1) ** step, float(b2) ** step


def _replay_beta_powers(fp, betas):
    """The running beta powers exactly as the update kernels hold them after fp.state[0] steps: a product in fp64, one factor
    per step, of the betas rounded to fp32 (they are float launch arguments).  load_adam_state_dict's closed form differs from
    it in the last bits (beta2 = 0.9 is not an fp32 number), enough to move single weights of a resumed run by an ulp."""
    step = int(fp.state[0].item())
    if step < 1:
        return
    b1, b2 = (torch.tensor(float(b), dtype=torch.float32).item() for b in betas)
    p1 = p2 = 1.0
    for _ in range(step):
        p1 *= b1
        p2 *= b2
    fp.state[1], fp.state[2] = p1, p2


def resume_checkpoint(eng, path: str) -> int:
    """Continue from a gan_epochNNNN.pth written by save_checkpoint (or by the reference trainer, train_gan.py:267-276):
    G (with its BatchNorm buffers), D, E_num, both optimisers.  Returns the epoch the checkpoint was written after."""
    # weights_only=None, torch's default: tensors, containers and numbers are all a gan_epochNNNN.pth holds
    ck = read_checkpoint(path, RuntimeError, weights_only=None)
    for key in ("G", "D", "E_num", "opt_G", "opt_D"):
        if key not in ck:
            raise KeyError(f"{path}: not a full training checkpoint (no '{key}')")
    load_generator_state(eng, ck)
    eng.D.load(ck["D"])
    nbt = [v for k, v in ck["G"].items() if k.endswith("num_batches_tracked")]
    if nbt:
        eng.num_batches_tracked = int(nbt[0])
    load_adam_state_dict(eng.GE, ck["opt_G"])
    load_adam_state_dict(eng.D, ck["opt_D"])
    for fp in (eng.GE, eng.D):
        _replay_beta_powers(fp, eng.betas)
    eng.params_changed()
    blk = ck.get("ema")
    if eng.ema is None:
        if blk is not None:
            print(f"[WARN] {path} holds averaged weights ('ema') but EMA_DECAY is 0: the block is ignored and averaging stays off")
    elif blk is None:
        eng.ema_reset()         # averaging starts here: the shadow is the resumed weights, the ramp counts from this step
    else:
        if float(blk["decay"]) != eng.ema_decay or bool(blk["ramp"]) != eng.ema_ramp:
            print(f"[WARN] {path}: averaged with EMA_DECAY {blk['decay']} / EMA_RAMP {blk['ramp']}, continuing with "
                  f"{eng.ema_decay} / {eng.ema_ramp}")
        flat = {**{"G." + k: v for k, v in blk["G"].items()}, **{"E." + k: v for k, v in blk["E_num"].items()}}
        bad = state_mismatches(flat, eng.GE.spec)[1]
        if bad:
            raise ValueError("{}: ema.{}: shape {} != {}".format(path, *bad[0]))
        shadow = torch.zeros(eng.GE.n, dtype=torch.float64)
        for k, (o, n) in eng.GE.offsets.items():
            shadow[o:o + n] = flat[k].reshape(-1).to(torch.float64)
        eng.ema_reset(shadow, float(blk["offset"]))     # its BatchNorm buffers are recomputed at the next save, never resumed
    return int(ck.get("epoch") or 0)


# ---- emotion classifier ---------------------------------------------------------------------------------------------
def read_ed_state(path: str, err, weights_only) -> dict:
    """The state_dict of train_ed's ed_best.pth / ed_epochNNN.pth ({"model": state_dict, ...}) or of a bare state_dict file (the
    reference's EmotionDiscriminator.state_dict(), weight_orig / _u / _v under spectral norm)."""
    ck = read_checkpoint(path, err, weights_only=weights_only)
    sd = ck["model"] if isinstance(ck, dict) and isinstance(ck.get("model"), dict) else ck
    if not isinstance(sd, dict):
        raise err(f"{path}: neither a train_ed checkpoint nor a state_dict")
    return sd


def ed_state_shapes(cfg: dict, sn_names=()) -> "OrderedDict[str, tuple]":
    """Keys and shapes of EmotionDiscriminator.state_dict() under an ED config, without num_batches_tracked; a layer of sn_names
    holds torch.nn.utils.spectral_norm's weight_orig, weight_u (out,), weight_v (the rest, flat) in place of its weight."""
    spec, bufs, _ = emotion_disc_spec(cfg)
    shapes = OrderedDict({**spec, **bufs})
    for nm in sn_names:
        w = tuple(shapes.pop(nm + ".weight"))
        shapes[nm + ".weight_orig"], shapes[nm + ".weight_u"] = w, (w[0],)
        shapes[nm + ".weight_v"] = (math.prod(w[1:]),)
    return shapes


def spectral_norm_weight(sd: dict, key: str):
    """sd[key], or -- for a layer the reference wrapped in nn.utils.spectral_norm (`use_spectral_norm`, ed_model.py:29-32,
    79-82: state_dict keys `<key>_orig`, `<key>_u`, `<key>_v`) -- the weight that wrapper uses in eval mode:
    weight_orig / sigma with sigma = u^T W v over W = weight_orig flattened to (out, -1), no power iteration.  The GAN step
    only ever runs the emotion discriminator frozen and in eval mode, so folding sigma in at load time is exact."""
    if key in sd:
        return sd[key]
    if key + "_orig" in sd and key + "_u" in sd and key + "_v" in sd:
        w = sd[key + "_orig"].double()
        sigma = torch.dot(sd[key + "_u"].double(), w.flatten(1).mv(sd[key + "_v"].double()))
        return (w / sigma).float()
    return None


def load_ed_checkpoint(eng, path: str):
    """train_gan.py:121-128: load_state_dict(strict=False); missing file => random ED with a warning."""
    if not os.path.exists(path):
        print(f"[WARN] ED checkpoint not found at {path}. ED will be random!")
        return False
    print(f"[INFO] Loading pre-trained Emotion Discriminator from {path}")
    # weights_only=None, torch's default, as this trainer always read it: an ed_best.pth's cfg and optimizer are plain containers
    sd = read_ed_state(path, RuntimeError, weights_only=None)
    # strict=False semantics: a key the checkpoint lacks keeps its initial value (reported, not silent -- a spectral-norm
    # triple with one part missing counts as missing); a key of the wrong shape raises, as load_state_dict does
    have = {k: spectral_norm_weight(sd, k) for k in eng.ED.spec}
    have = {k: w for k, w in have.items() if w is not None}
    have.update((k, sd[k]) for k in eng.EDbuf if k in sd)
    missing, bad = state_mismatches(have, {**eng.ED.spec, **{k: v.shape for k, v in eng.EDbuf.items()}})
    if bad:
        raise RuntimeError("Error(s) in loading state_dict for EmotionDiscriminator: size mismatch for " +
                           "; ".join(f"{k}: checkpoint {got} vs model {want}" for k, got, want in bad))
    for k, w in have.items():
        (eng.ED.p if k in eng.ED.spec else eng.EDbuf)[k].copy_(w.float())
    if missing:
        print(f"[WARN] ED checkpoint {path} lacks {len(missing)} key(s), left at their initial values: {', '.join(missing)}")
    eng.fold_ed()          # derived scale / shift / re-laid weights: eagerly, outside any graph
    return True


# ---- VAE ------------------------------------------------------------------------------------------------------------
def load_vae_checkpoint(eng, path: str, err):
    """The weights and BatchNorm buffers of train_ae's ae_best.pth ({'epoch', 'model_state'}, encode.py:118-119) or ae_final.pth
    (a bare state_dict) into a VaeEngine: read once, every key and shape checked against the engine's spec and buffers first."""
    # weights_only=False, as every reader of this file always passed: an ae_best.pth of the reference trainer is unpickled whole
    ck = read_checkpoint(path, err, weights_only=False)
    sd = ck["model_state"] if isinstance(ck, dict) and "model_state" in ck else ck
    if not isinstance(sd, dict):
        raise err(f"{path}: neither a train_ae checkpoint nor a state_dict")
    missing, bad = state_mismatches(sd, {**eng.P.spec, **{k: v.shape for k, v in eng.buf.items()}})
    if missing:
        raise err(f"{path}: no '{missing[0]}': not a checkpoint of this VAE")
    if bad:
        k, got, want = bad[0]
        raise err(f"{path}: '{k}' has shape {got}, the config (MAX_NOTES {eng.T}, LATENT_DIM {eng.latent}) implies {want}")
    eng.load_state({k: sd[k] for k in eng.P.spec}, {k: sd[k] for k in eng.buf})
