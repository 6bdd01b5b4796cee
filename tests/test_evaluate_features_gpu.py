"""GPU: the evaluator's feature-space metrics (Evaluator(features=True), --feature-metrics / --memorisation): the stashed
encoder features against a torch restatement of the oracle's encoder, every number of the report's feature_space block against
an fp64 host computation from the stashed features themselves (which isolates the pair kernels and the grouping), replay,
opt-in, batch-size independence, the nearest-training-row check and the CLI.

Bounds (tests/test_pair_metrics_gpu.py derives them): |delta d2| <= (2 D + 8) u (|a|^2 + |b|^2 + r2) at the row-norm maxima for
distances and margins -- a margin computed against the device's own radii carries the radii's error too, which the
membership rule's factor 2 covers -- and 2 * 3 u sum (|g| / D + 1)^2 |a||b| for a kernel sum.  A row takes part in a
membership count only when its fp64 margin is clear of 0 by more than twice the bound; at most 2 % of rows may be unclear."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd.gan import evaluate as EV  # noqa: E402
from melo_gan_amd.gan import feature_metrics as FM  # noqa: E402
from melo_gan_amd.gan.dataset import GANDataset  # noqa: E402
from oracle import melo_oracle as O  # noqa: E402
from test_evaluate_gpu import gen_state, save_state, make_split, oracle_pass  # noqa: E402,F401

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
K, N_ROWS, BATCH, KNN = 4, 22, 8, 3
U = 2.0 ** -24
SETUPS = [(32, 4), (64, 128)]


# ---------------------------------------------------------------------------------------------------------------------
# the encoder half of O.emotion_disc_fwd, restated (oracle/ cannot grow a second entry point)
# ---------------------------------------------------------------------------------------------------------------------
def encoder_features(S, ed_cfg, x):
    P, Bf = S.PED, S.BED
    with torch.no_grad():
        h = x.permute(0, 2, 1)
        for i in range(ed_cfg.get("notes_blocks", 4)):
            k = 5 if i == 0 else 3
            h = F.conv1d(h, P[f"encoder.conv.{i}.net.0.weight"], P[f"encoder.conv.{i}.net.0.bias"], 1, k // 2)
            h = F.batch_norm(h, Bf[f"encoder.conv.{i}.net.1.running_mean"], Bf[f"encoder.conv.{i}.net.1.running_var"],
                             P[f"encoder.conv.{i}.net.1.weight"], P[f"encoder.conv.{i}.net.1.bias"], False, O.BN_MOMENTUM, O.BN_EPS)
            h = F.gelu(h)
        return F.linear(h.mean(dim=2), P["encoder.project.weight"], P["encoder.project.bias"])


def pin_restatement(S, ed_cfg, x):
    """The restated features pushed through the oracle's classifier half give the oracle's logits, bit for bit."""
    feats = encoder_features(S, ed_cfg, x)
    with torch.no_grad():
        via = O.emotion_disc_fwd(S.PED, S.BED, feats, dict(ed_cfg, input_mode="latent"), train=False)
        whole = O.emotion_disc_fwd(S.PED, S.BED, x, ed_cfg, train=False)
    assert torch.equal(via, whole)
    return feats


# ---------------------------------------------------------------------------------------------------------------------
# the block from a pair of stashes, in fp64 on the host, with the bounds beside every number
# ---------------------------------------------------------------------------------------------------------------------
def kernel_sum(A, B, same):
    g = A @ B.T
    D = A.shape[1]
    w = np.ones_like(g)
    if same:
        np.fill_diagonal(w, 0.0)
    norms = np.sqrt((A * A).sum(1))[:, None] * np.sqrt((B * B).sum(1))[None, :]
    return float((w * (g / D + 1.0) ** 3).sum()), 2 * 3 * U * float((w * (np.abs(g) / D + 1.0) ** 2 * norms).sum())


def kid64(R, Fk):
    """(KID, bound) or (None, None)."""
    m, n = len(R), len(Fk)
    if m < 2 or n < 2:
        return None, None
    (xx, bxx), (yy, byy), (xy, bxy) = kernel_sum(R, R, True), kernel_sum(Fk, Fk, True), kernel_sum(R, Fk, False)
    return FM.kid_from_sums(xx, m, yy, n, xy), bxx / (m * (m - 1)) + byy / (n * (n - 1)) + 2 * bxy / (m * n)


def d2_64(A, B, exclude_self=False):
    d2 = np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T), 0.0)
    if exclude_self:
        np.fill_diagonal(d2, np.inf)
    return d2


def d2_bound(A, B, r2=0.0):
    return (2 * A.shape[1] + 8) * U * ((A * A).sum(1).max() + (B * B).sum(1).max() + float(np.max(r2)))


def inside64(X, Y, k):
    """Rows of X in Y's k-NN manifold: (rows clearly inside, rows unclear) or None when Y holds at most k rows."""
    if len(Y) <= k:
        return None
    r2 = np.sort(d2_64(Y, Y, exclude_self=True), axis=1)[:, k - 1]
    margin = (d2_64(X, Y) - r2[None, :]).min(1)
    clear = np.abs(margin) > 2 * d2_bound(X, Y, r2)
    return int(((margin <= 0) & clear).sum()), int((~clear).sum())


def check_share(got, ref, n, what):
    if ref is None:
        assert got is None, what
        return 0
    inside, unclear = ref
    print(f"{what}: {got} of {n} rows; fp64: {inside} clearly inside, {unclear} unclear")
    assert unclear <= 0.02 * n, what
    assert got is not None and inside - 1e-9 <= got * n <= inside + unclear + 1e-9, what
    return unclear


def check_kid(got, R, Fk, what):
    ref, bound = kid64(R, Fk)
    if ref is None:
        assert got is None, what
        return 0.0
    print(f"{what}: {got:.9g} (fp64 {ref:.9g}), |err| {abs(got - ref):.3g}, bound {bound:.3g}")
    assert got is not None and abs(got - ref) <= bound, what
    return bound


def check_block(block, R, Fk, labels, k):
    """Every number of the block against fp64 from the same features; returns {path: bound or unclear rows} for the
    batch-size comparison."""
    R, Fk, labels = R.double().numpy(), Fk.double().numpy(), labels.numpy()
    n = len(labels)
    slack = {}
    assert (block["dim"], block["k"]) == (R.shape[1], k)
    slack["kid"] = check_kid(block["kid"], R, Fk, "kid")
    slack["precision"] = check_share(block["precision"], inside64(Fk, R, k), n, "precision")
    slack["recall"] = check_share(block["recall"], inside64(R, Fk, k), n, "recall")
    assert list(block["per_emotion"]) == list(EV.EMOTIONS) == list(block["kid_matrix"])
    for e, name in enumerate(EV.EMOTIONS):
        Re, Fe = R[labels == e], Fk[labels == e]
        pe = block["per_emotion"][name]
        assert pe["n"] == len(Re)
        slack[f"{name}.precision"] = check_share(pe["precision"], inside64(Fe, Re, k), len(Re), f"{name}: precision")
        slack[f"{name}.recall"] = check_share(pe["recall"], inside64(Re, Fe, k), len(Re), f"{name}: recall")
        for f, other in enumerate(EV.EMOTIONS):
            slack[f"kid.{name}.{other}"] = check_kid(block["kid_matrix"][name][other], Re, Fk[labels == f], f"kid real {name} / fake {other}")
        assert pe["kid"] == block["kid_matrix"][name][name]
    return slack


ED_SCALE, PROJECT_SCALE = 8.0, 1.0 / 512.0


def spread_state(T, C):
    """gen_state with the classifier's four encoder convolutions x8 and its projection (weight and bias) x1/512.  The closed-form
    classifier maps every roll to nearly the same feature vector -- squared distances of 1e-10 between vectors of norm 1.4, far
    below what fp32 resolves of |a|^2 + |b|^2 - 2 a . b, so that no membership would be clear of the bound -- as gen_state
    itself scales the generator and the critic so that their metrics are not rounding noise.  The convolutions' x8 spreads
    the features (the real rolls' lie 1e-3 .. 1e2 of their squared norm apart); the projection's x1/512, which moves every
    distance and every bound alike, brings the elements of the larger side -- the generated rolls', whose generator gen_state
    scales up -- back to a few tenths.  The real side's are then small (RMS element 0.024 at T = 32 / C = 4 and 6e-4 at
    T = 64 / C = 128, against 0.086 for the unscaled classifier), where the absolute term of the stash's tolerance would
    decide alone: stash_close therefore scales both sides of such a comparison up to the unscaled classifier's size first."""
    S, cfg, ed_cfg = gen_state(T, C, "warm_start", "notes")
    for k in S.PED:
        if k.startswith("encoder.conv.") and k.endswith("net.0.weight"):
            S.PED[k] = S.PED[k] * ED_SCALE
        elif k.startswith("encoder.project."):
            S.PED[k] = S.PED[k] * PROJECT_SCALE
    return S, cfg, ed_cfg


UNSCALED_RMS = 0.086        # RMS feature element of gen_state's classifier as it comes (row norm 1.376 over 256 elements)


def stash_close(got, want, what):
    """rtol 1e-4, atol 2e-6 -- the bounds tests/test_evaluate_gpu.py holds logits_real to -- on a stash against the restated
    encoder.  Both sides are first multiplied by c >= 1 that brings the reference's RMS element to the unscaled classifier's,
    so that the projection's x1/512 does not let the absolute term swallow small features; never looser than the plain
    comparison."""
    got, want = got.cpu().double().numpy(), want.double().numpy()
    rms = float(np.sqrt((want * want).mean()))
    c = max(1.0, UNSCALED_RMS / rms)
    err = np.abs(got - want) * c
    print(f"{what}: RMS element {rms:.3g}, compared at x{c:.3g}; max |err| {err.max():.3g}, max of |err| / (2e-6 + 1e-4 |ref|) "
          f"{(err / (2e-6 + 1e-4 * np.abs(want) * c)).max():.3g}")
    np.testing.assert_allclose(got * c, want * c, rtol=1e-4, atol=2e-6, err_msg=what)


def own_rolls(ev, ds_parts):
    """The engine's own generated rolls of every split row.  eng.fake_d holds one batch; the noise of a row depends on (seed,
    row) alone and a batch's launches on nothing outside the batch, so the last batch of a pass over the first 8, the first
    16 and all 22 rows is batch 0, 1 and 2 of the full pass."""
    rolls = []
    for part, m in ds_parts:
        ev.evaluate(part, seed=3)
        rolls.append(ev.eng.fake_d[:m].cpu())
    return torch.cat(rolls)


def prefix(real, numeric, labels, cfg, n):
    return GANDataset(real[:n].numpy(), labels[:n].numpy(), numeric[:n].numpy(), None, cfg["LATENT_DIM"], "cuda")


def replayed_real_block(ev, labels, n):
    """The generated stash overwritten with the real rows moved on by one: every row lies in the other set's manifold as a
    copy, while the per-emotion slices hold copies of other emotions' rows -- their shares may lie anywhere."""
    ev.feat_fake[:n].copy_(ev.feat_real[:n].roll(1, 0))
    torch.cuda.synchronize()
    block = ev.feature_space(labels, n)
    check_block(block, ev.feat_real[:n].cpu(), ev.feat_fake[:n].cpu(), labels, ev.knn_k)
    assert block["precision"] == 1.0 and block["recall"] == 1.0
    return block


def build(tmp_path, T, C, batch=BATCH, features=True, knn_k=KNN):
    S, cfg, ed_cfg = spread_state(T, C)
    ck, ed = save_state(S, str(tmp_path))
    ev = EV.Evaluator(cfg, ed_cfg, "cuda", batch, features=features, knn_k=knn_k)
    ev.load_generator(ck)
    ev.load_critic(ck)
    ev.load_ed(ed)
    return S, cfg, ed_cfg, ev


# ---------------------------------------------------------------------------------------------------------------------
# stash, report block, replay, opt-in
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", SETUPS)
def test_stash_and_report_block(tmp_path, T, C):
    S, cfg, ed_cfg, ev = build(tmp_path, T, C)
    ds, real, numeric, latent, labels = make_split(T, C, cfg)
    feats = pin_restatement(S, ed_cfg, real)
    rolls = own_rolls(ev, [(prefix(real, numeric, labels, cfg, BATCH), BATCH), (prefix(real, numeric, labels, cfg, 2 * BATCH), BATCH),
                           (ds, N_ROWS - 2 * BATCH)])
    assert tuple(rolls.shape) == (N_ROWS, T, C)
    rep = ev.evaluate(ds, seed=3)
    assert torch.equal(ev.eng.fake_d[:N_ROWS - 2 * BATCH].cpu(), rolls[2 * BATCH:])
    json.loads(json.dumps(rep, allow_nan=False))
    # the real side's features in split row order; the padded tail of the last batch lies behind them
    assert tuple(ev.feat_real.shape) == (3 * BATCH, ed_cfg["notes_hidden"]) == tuple(ev.feat_fake.shape)
    stash_close(ev.feat_real[:N_ROWS], feats, "feat_real")
    # the generated side's, all 22 rows: the classifier's encoder on the engine's own rolls of every batch
    stash_close(ev.feat_fake[:N_ROWS], encoder_features(S, ed_cfg, rolls), "feat_fake")
    assert torch.unique(ev.feat_fake[:N_ROWS].cpu(), dim=0).shape[0] == N_ROWS
    # every number of the block from the stashed features themselves
    block = rep["feature_space"]
    assert "nn_train" not in block
    check_block(block, ev.feat_real[:N_ROWS].cpu(), ev.feat_fake[:N_ROWS].cpu(), labels, KNN)
    assert all(v["precision"] is not None and v["kid"] is not None for v in block["per_emotion"].values())
    assert "feature space" in EV.format_table(rep)
    # a second pass replays the graph: the same report, to the bit
    assert ev.evaluate(ds, seed=3) == rep
    # opt-in: without the flag the report is today's
    _, _, _, plain = build(tmp_path, T, C, features=False)
    rep0 = plain.evaluate(ds, seed=3)
    assert "feature_space" not in rep0 and plain.feat_real is None
    assert rep0 == {k: v for k, v in rep.items() if k != "feature_space"}
    # memberships that are not all on one side
    shares = [v[q] for v in replayed_real_block(ev, labels, N_ROWS)["per_emotion"].values() for q in ("precision", "recall")]
    assert all(s is not None and s > 0.0 for s in shares)


def test_small_and_missing_emotions_are_none(tmp_path):
    T, C = 32, 4
    S, cfg, ed_cfg, ev = build(tmp_path, T, C)
    real, numeric, latent, _ = O.synthetic_batch(N_ROWS, T, C, cfg["LATENT_DIM"], 6, 7)
    labels = torch.tensor([0, 1] * 10 + [2, 2])          # emotion 2: two rows; emotion 3: none
    ds = GANDataset(real.numpy(), labels.numpy(), numeric.numpy(), None, cfg["LATENT_DIM"], "cuda")
    rep = ev.evaluate(ds, seed=3)
    json.loads(json.dumps(rep, allow_nan=False))
    block = rep["feature_space"]
    check_block(block, ev.feat_real[:N_ROWS].cpu(), ev.feat_fake[:N_ROWS].cpu(), labels, KNN)
    two, none = block["per_emotion"][EV.EMOTIONS[2]], block["per_emotion"][EV.EMOTIONS[3]]
    assert two["n"] == 2 and two["precision"] is None and two["recall"] is None and two["kid"] is not None      # 2 rows: KID only
    assert none == {"n": 0, "kid": None, "precision": None, "recall": None}
    for name in EV.EMOTIONS:
        assert block["kid_matrix"][name][EV.EMOTIONS[3]] is None and block["kid_matrix"][EV.EMOTIONS[3]][name] is None
    assert block["per_emotion"][EV.EMOTIONS[0]]["precision"] is not None and block["precision"] is not None
    block = replayed_real_block(ev, labels, N_ROWS)
    assert block["per_emotion"][EV.EMOTIONS[2]]["precision"] is None and block["per_emotion"][EV.EMOTIONS[1]]["recall"] > 0


def test_feature_block_does_not_depend_on_the_batch_size(tmp_path):
    T, C = 32, 4
    blocks, slacks = {}, {}
    for batch in (8, 5):
        S, cfg, ed_cfg, ev = build(tmp_path, T, C, batch=batch)
        ds, real, numeric, latent, labels = make_split(T, C, cfg)
        blocks[batch] = ev.evaluate(ds, seed=5)["feature_space"]
        slacks[batch] = check_block(blocks[batch], ev.feat_real[:N_ROWS].cpu(), ev.feat_fake[:N_ROWS].cpu(), labels, KNN)
    a, b, sa, sb = blocks[8], blocks[5], slacks[8], slacks[5]

    def same(x, y, path, rows):
        assert (x is None) == (y is None), path
        if x is None:
            return
        if path.startswith("kid"):                       # floats: within the sum of the two runs' bounds against fp64
            assert abs(x - y) <= sa[path] + sb[path], (path, x, y)
        else:                                            # counts: equal apart from the rows the 2 % rule leaves out
            assert abs(x - y) * rows <= sa[path] + sb[path] + 1e-9, (path, x, y)

    same(a["kid"], b["kid"], "kid", N_ROWS)
    for q in ("precision", "recall"):
        same(a[q], b[q], q, N_ROWS)
    for name in EV.EMOTIONS:
        pa, pb = a["per_emotion"][name], b["per_emotion"][name]
        assert pa["n"] == pb["n"]
        for q in ("precision", "recall"):
            same(pa[q], pb[q], f"{name}.{q}", pa["n"])
        for other in EV.EMOTIONS:
            same(a["kid_matrix"][name][other], b["kid_matrix"][name][other], f"kid.{name}.{other}", 0)


# ---------------------------------------------------------------------------------------------------------------------
# the nearest-training-row check
# ---------------------------------------------------------------------------------------------------------------------
def test_memorisation(tmp_path):
    T, C, n_train = 32, 4, 37
    S, cfg, ed_cfg, ev = build(tmp_path, T, C)
    ds, real, numeric, latent, labels = make_split(T, C, cfg)
    treal, tnum, _, _ = O.synthetic_batch(n_train, T, C, cfg["LATENT_DIM"], 6, 19)
    train = GANDataset(treal.numpy(), (torch.arange(n_train) % K).numpy(), tnum.numpy(), None, cfg["LATENT_DIM"], "cuda")
    rep = ev.evaluate(ds, seed=3, train_dataset=train)
    json.loads(json.dumps(rep, allow_nan=False))
    # the training stash: the encoder on the training rolls, in row order over 5 batches of 8
    tfeat = encoder_features(S, ed_cfg, treal)
    stash_close(ev.feat_train[:n_train], tfeat, "feat_train")
    # the summary from fp64 distances between the stashes
    Rf, Ff, Tf = (t[:m].cpu().double().numpy() for t, m in ((ev.feat_real, N_ROWS), (ev.feat_fake, N_ROWS), (ev.feat_train, n_train)))
    nn = rep["feature_space"]["nn_train"]
    for side, X in (("fake", Ff), ("real", Rf)):
        d2, bound = d2_64(X, Tf).min(1), d2_bound(X, Tf)
        print(f"nn_train {side}: {nn[side]}, fp64 median {np.median(d2):.6g} p05 {np.quantile(d2, 0.05):.6g}, bound {bound:.3g}")
        assert abs(nn[side]["median"] - np.median(d2)) <= bound and abs(nn[side]["p05"] - np.quantile(d2, 0.05)) <= bound
    assert nn["real"]["median"] > 0 and 0.0 <= nn["fake_below_real_p05"] <= 1.0
    # the rest of the block is what it is without the training split
    rest = {k: v for k, v in rep["feature_space"].items() if k != "nn_train"}
    assert rest == ev.evaluate(ds, seed=3)["feature_space"]
    # a "generator" that replays the training set: its stash holds copies of training features
    ev.feat_fake[:N_ROWS].copy_(ev.feat_train[:N_ROWS])
    torch.cuda.synchronize()
    replay = ev.feature_space(labels, N_ROWS, ev.feat_train[:n_train])["nn_train"]
    assert replay["fake"]["median"] == 0 and replay["fake"]["p05"] == 0 and replay["fake_below_real_p05"] == 1.0
    assert replay["real"] == nn["real"]
    with pytest.raises(EV.EvaluateError, match="features=True"):
        build(tmp_path, T, C, features=False)[3].evaluate(ds, seed=3, train_dataset=train)


# ---------------------------------------------------------------------------------------------------------------------
# the CLI end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_feature_metrics_and_memorisation(tmp_path):
    S, _, ed_cfg = spread_state(32, 4)
    ck, ed = save_state(S, str(tmp_path))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    cfg.update(MAX_NOTES=32, LOG_DIR=str(tmp_path / "log"))
    cp, ep = tmp_path / "gan.yaml", tmp_path / "ed.yaml"
    cp.write_text(yaml.safe_dump(cfg))
    ep.write_text(yaml.safe_dump(ed_cfg))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, "-m", "melo_gan_amd.gan.evaluate", "--config", str(cp), "--ckpt",
                        ck, "--ed_config", str(ep), "--ed_ckpt", ed, "--synthetic", "40", "--batch", "16", "--seed", "7",
                        "--feature-metrics", "--memorisation"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=450)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rep = json.load(open(tmp_path / "log" / "eval.json"))
    fs = rep["feature_space"]
    assert rep["n"] == 40 and (fs["dim"], fs["k"]) == (ed_cfg["notes_hidden"], 3)
    assert sum(v["n"] for v in fs["per_emotion"].values()) == 40
    assert isinstance(fs["kid"], float) and 0.0 <= fs["precision"] <= 1.0 and 0.0 <= fs["recall"] <= 1.0
    assert fs["nn_train"]["real"]["median"] > 0 and fs["nn_train"]["fake"]["median"] > 0
    assert "feature space (dim" in r.stdout and "nearest training row" in r.stdout and "kid" in r.stdout
