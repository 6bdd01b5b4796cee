#!/usr/bin/env python3
"""
Generates tests/golden/ed_latent_*.npz by RUNNING THE REFERENCE'S OWN EmotionDiscriminator in `input_mode: latent`
(imported at generation time only, like tests/golden/make_golden.py; only these small data fixtures are committed).

    python tests/golden/make_golden_ed_latent.py

SURVEY f-2 in latent mode: three pre-training steps (train_ed.py:51-82) of the MLP classifier (ed_model.py:72-95) on
(B, latent_dim) latents -- train mode with live dropout (p = 0.2; the keep-masks nn.Dropout drew are captured and stored),
CrossEntropyLoss, AdamW(lr 2e-4, betas (0.5, 0.999), wd 0.01).  Weights are not stored: both sides fill them from
oracle.fill_params(spec, 9.0) with the matrices multiplied by `scale` (logits of O(1), per-class gradients of different
sizes).  Before a fixture is written the free-running oracle is held against it (|d loss| < 5e-6, logits rtol 2e-3 /
atol 2e-5): a recipe the oracle drifts from (Adam amplifying rounding on near-zero gradients) is not a usable fixture.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import DropCapture, EmotionDiscriminator, O, checksum, load_into      # noqa: E402

CASES = [   # name, B, latent_dim, mlp_hidden, matrix scale
    ("ed_latent_d64_b8", 8, 64, [256, 128], 16.0),
    ("ed_latent_d8_b5", 5, 8, [256, 128], 8.0),
    ("ed_latent_d32_h3_b7", 7, 32, [96, 48, 24], 16.0),
]


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member timestamp: regenerating a fixture reproduces the file byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


def latent_cfg(D, hidden):
    return dict(O.default_ed_cfg(4), input_mode="latent", latent_dim=D, mlp_hidden=list(hidden), dropout=0.2)


def initial_params(cfg, scale):
    spec, _ = O.emotion_disc_spec(cfg)
    P = O.fill_params(spec, 9.0, O.norm_affine_names(spec))
    for v in P.values():
        if v.dim() >= 2:
            v.mul_(scale)
    return spec, P


def ed_latent_case(name, B, D, hidden, scale, n_steps=3):
    cfg = latent_cfg(D, hidden)
    ED = EmotionDiscriminator(cfg)
    spec, P = initial_params(cfg, scale)
    load_into(ED, P)
    opt = torch.optim.AdamW(ED.parameters(), lr=2e-4, betas=(0.5, 0.999), weight_decay=0.01)
    crit = nn.CrossEntropyLoss()
    g = torch.Generator().manual_seed(11)
    out = dict(B=B, D=D, hidden=np.asarray(hidden, dtype=np.int64), scale=np.float64(scale), n_steps=n_steps)
    cap = DropCapture(ED)
    ED.train()
    for it in range(n_steps):
        x = torch.randn(B, D, generator=g)
        y = torch.randint(0, 4, (B,), generator=g)
        opt.zero_grad()
        torch.manual_seed(3000 + it)
        logits = ED(x)
        for j, m in enumerate(cap.pop()):
            out[f"s{it}.dm{j}"] = m.numpy().astype(np.uint8)
        loss = crit(logits, y)
        loss.backward()
        opt.step()
        out[f"s{it}.x"], out[f"s{it}.y"] = x.numpy().copy(), y.numpy().copy()
        out[f"s{it}.loss"] = np.float64(loss.item())
        out[f"s{it}.logits"] = logits.detach().numpy().copy()
        if it == 0:
            out["s0.grad.head_w"] = ED.classifier.head.weight.grad.numpy().copy()
            out["s0.grad.net0_w"] = ED.classifier.net[0].weight.grad.numpy().copy()
    sd = ED.state_dict()
    for k, v in sd.items():
        out[f"end.{k}"] = checksum(v.float())
    out["end.head_w"] = sd["classifier.head.weight"].numpy().copy()
    ED.eval()
    cap.pop()
    with torch.no_grad():
        out["end.eval_logits"] = ED(torch.from_numpy(out["s0.x"])).numpy().copy()

    # the facts the tests lean on, checked before anything is written: the oracle, running free, reproduces the reference
    _, Po = initial_params(cfg, scale)
    oo = O.AdamState(Po, 2e-4, (0.5, 0.999), 1e-8, weight_decay=0.01, decoupled=True)
    for it in range(n_steps):
        dm = [torch.from_numpy(out[f"s{it}.dm{j}"]).float() / 0.8 for j in range(len(hidden))]
        r = O.ed_step(Po, {}, oo, torch.from_numpy(out[f"s{it}.x"]), torch.from_numpy(out[f"s{it}.y"]), cfg, dm)
        assert abs(r["loss"].item() - out[f"s{it}.loss"]) < 5e-6, (name, it, r["loss"].item(), out[f"s{it}.loss"])
        np.testing.assert_allclose(r["logits"].numpy(), out[f"s{it}.logits"], rtol=2e-3, atol=2e-5)
    path = os.path.join(HERE, name + ".npz")
    save_npz(path, out)
    assert os.path.getsize(path) < 128 * 1024          # the step-0 gradient of net.0.weight is the bulk of it
    print(name, "loss", [out[f"s{i}.loss"] for i in range(n_steps)], "max |logit|",
          [float(np.abs(out[f"s{i}.logits"]).max()) for i in range(n_steps)], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for case in CASES:
        ed_latent_case(*case)
