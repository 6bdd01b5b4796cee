"""GPU: held-out evaluation (melo_gan_amd.gan.evaluate) -- the metrics kernel mg_eval_acc against torch in fp64, the
Evaluator against the oracle over a padded pass, its independence of the batch size, the trainer left undisturbed by
--eval-every, and the CLI end to end.  Fixtures are built in tmp_path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402
from melo_gan_amd.gan import evaluate as EV  # noqa: E402
from melo_gan_amd.gan.dataset import GANDataset  # noqa: E402
from oracle import melo_oracle as O  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
K = 4


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against torch
# ---------------------------------------------------------------------------------------------------------------------
def kernel_inputs(B, T, C, call, g):
    real = torch.randn(B, T, C, generator=g)
    fake = torch.randn(B, T, C, generator=g) * 3 + 0.5
    labels = (torch.arange(B) + call) % K
    if B >= 5:
        labels[call + 1::7] = -1                                         # padding rows
    elif call == 1:
        labels[:] = -1                                                   # B = 1: the second call is all padding
    d_real, d_fake = torch.randn(B, generator=g), torch.randn(B, generator=g) * 2
    lf, lr = torch.randn(B, K, generator=g) * 3, torch.randn(B, K, generator=g) * 3
    if B >= 5 and call == 1:
        lf[3, 2] = float("nan")                                          # row 3 is counted (label 0 in call 1): NaN is the maximum
    return real, fake, labels, d_real, d_fake, lf, lr


def torch_reference(calls, C):
    """The accumulator's contents by torch, sums in fp64 with the sum of |terms| beside each (the tolerance's scale)."""
    ref = {"n": torch.zeros(K, dtype=torch.int64), "conf": torch.zeros(2, K, K, dtype=torch.int64),
           "d": torch.zeros(2, dtype=torch.float64), "d_abs": torch.zeros(2, dtype=torch.float64),
           "cls": torch.zeros(2, 2, K, dtype=torch.float64), "cls_abs": torch.zeros(2, 2, K, dtype=torch.float64),
           "sum": torch.zeros(2, K, C, dtype=torch.float64), "sum_abs": torch.zeros(2, K, C, dtype=torch.float64),
           "sq": torch.zeros(2, K, C, dtype=torch.float64),
           "min": torch.full((2, K, C), float("inf")), "max": torch.full((2, K, C), float("-inf"))}
    for real, fake, labels, d_real, d_fake, lf, lr in calls:
        ok = labels >= 0
        ref["n"] += torch.bincount(labels[ok], minlength=K)
        for s, d in enumerate((d_real, d_fake)):
            ref["d"][s] += d[ok].double().sum()
            ref["d_abs"][s] += d[ok].double().abs().sum()
        for s, lg in enumerate((lf, lr)):
            pred = torch.argmax(lg.cuda(), dim=1).cpu()                  # first index wins, NaN counts as the maximum
            z = lg.double()
            ce = torch.logsumexp(z, 1) - z[torch.arange(len(z)), labels.clamp(min=0)]
            p = torch.softmax(z, 1)[torch.arange(len(z)), labels.clamp(min=0)]
            for k in range(K):
                m = labels == k
                ref["conf"][s, k] += torch.bincount(pred[m], minlength=K)
                for q, v in enumerate((ce, p)):
                    ref["cls"][s, q, k] += v[m].sum()
                    ref["cls_abs"][s, q, k] += v[m].abs().sum()
        for s, x in enumerate((real, fake)):
            for k in range(K):
                xs = x[labels == k].double().reshape(-1, C)
                if xs.numel() == 0:
                    continue
                ref["sum"][s, k] += xs.sum(0)
                ref["sum_abs"][s, k] += xs.abs().sum(0)
                ref["sq"][s, k] += (xs * xs).sum(0)
                ref["min"][s, k] = torch.minimum(ref["min"][s, k], xs.amin(0).float())
                ref["max"][s, k] = torch.maximum(ref["max"][s, k], xs.amax(0).float())
    return ref


def close64(got, ref, scale, what):
    """Every fp64 sum within 1e-12 * sum |terms| of torch's fp64 sum (test_emotion_score_matches_torch's bound); a sum torch
    finds NaN (the planted NaN logit) must be NaN here too."""
    got, ref, scale = got.flatten(), ref.flatten(), scale.flatten()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), (what, got, ref)
    err = (got - ref).abs()[~nan]
    bound = 1e-12 * scale[~nan].clamp(min=1e-30)
    print(f"{what}: max |err| / (1e-12 sum|terms|) = {float((err / bound).max()) if err.numel() else 0.0:.3g}")
    assert (err <= bound).all(), (what, float((err / bound).max()))


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("T,C", [(32, 4), (512, 4), (256, 128), (20, 4)])
def test_eval_acc_matches_torch(T, C, B):
    g = torch.Generator().manual_seed(1000 * T + 10 * C + B)
    calls = [kernel_inputs(B, T, C, call, g) for call in (0, 1)]
    dev = [tuple(t.cuda() for t in c) for c in calls]

    def run(acc):
        for real, fake, labels, d_real, d_fake, lf, lr in dev:          # two calls into one accumulator: it adds
            ops.eval_acc(real, fake, labels, d_real, d_fake, lf, lr, acc)

    # the first call alone holds no NaN: every sum, the classifier's of every class included, against a finite reference
    first = ops.eval_acc_new(K, C, "cuda")
    ops.eval_acc(*dev[0], first)
    torch.cuda.synchronize()
    v, ref = ops.eval_acc_views(first.cpu(), K, C), torch_reference(calls[:1], C)
    assert torch.isfinite(ref["cls"]).all()
    assert torch.equal(v["n"], ref["n"]) and torch.equal(v["conf_fake"], ref["conf"][0]) and torch.equal(v["conf_real"], ref["conf"][1])
    close64(v["d_sum"], ref["d"], ref["d_abs"], "first call: critic sums")
    close64(v["cls"], ref["cls"], ref["cls_abs"], "first call: CE / p_target sums")
    close64(v["nsum"], ref["sum"], ref["sum_abs"], "first call: sum x")
    close64(v["nsq"], ref["sq"], ref["sq"], "first call: sum x^2")
    acc = ops.eval_acc_new(K, C, "cuda")
    run(acc)
    torch.cuda.synchronize()
    host = acc.cpu()
    v = ops.eval_acc_views(host, K, C)
    ref = torch_reference(calls, C)
    assert torch.equal(v["n"], ref["n"])
    assert torch.equal(v["conf_fake"], ref["conf"][0]) and torch.equal(v["conf_real"], ref["conf"][1])
    if B == 64:
        assert (ref["conf"] > 0).all()                                   # random logits: every cell of both matrices is hit
    if B >= 5:
        assert ref["conf"][0, 0, 2] >= 1 and torch.isnan(ref["cls"][0, 0, 0])      # the NaN row: predicted 2, poisons its CE sum
    assert torch.equal(v["nmin"], ref["min"]) and torch.equal(v["nmax"], ref["max"])
    close64(v["d_sum"], ref["d"], ref["d_abs"], "critic sums")
    close64(v["cls"], ref["cls"], ref["cls_abs"], "CE / p_target sums")
    close64(v["nsum"], ref["sum"], ref["sum_abs"], "sum x")
    close64(v["nsq"], ref["sq"], ref["sq"], "sum x^2")
    # two runs: the same bits
    acc2 = ops.eval_acc_new(K, C, "cuda")
    run(acc2)
    torch.cuda.synchronize()
    assert torch.equal(acc2.cpu(), host)
    # eager and graph replay: the same bits
    acc3 = ops.eval_acc_new(K, C, "cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run(ops.eval_acc_new(K, C, "cuda"))                               # this stream's workspace exists before the capture
        torch.cuda.synchronize()
        gr = ops.Graph()
        gr.begin()
        try:
            run(acc3)
        finally:
            gr.end()
        gr.launch()
    torch.cuda.synchronize()
    assert torch.equal(acc3.cpu(), host)
    # reset: back to the empty accumulator
    ops.eval_acc_reset(acc3, K, C)
    torch.cuda.synchronize()
    assert torch.equal(acc3.cpu(), ops.eval_acc_new(K, C, "cuda").cpu())
    e = ops.eval_acc_views(acc3.cpu(), K, C)
    assert (e["n"] == 0).all() and (e["nsum"] == 0).all() and (e["nmin"] == float("inf")).all() and (e["nmax"] == float("-inf")).all()


def test_eval_acc_optional_sides_and_tick():
    """Without critic scores / classifier logits those sums stay untouched; tick advances the batch counter by one per call."""
    g = torch.Generator().manual_seed(3)
    real, fake, labels, d_real, d_fake, lf, lr = (t.cuda() for t in kernel_inputs(5, 20, 4, 0, g))
    acc, tick = ops.eval_acc_new(K, 4, "cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="n_classes"):
        ops.eval_acc(real, fake, labels, None, None, None, None, acc)
    ops.eval_acc(real, fake, labels, None, None, None, None, acc, tick=tick, n_classes=K)
    ops.eval_acc(real, fake, labels, None, None, lf, None, acc, tick=tick)
    torch.cuda.synchronize()
    v = ops.eval_acc_views(acc.cpu(), K, 4)
    assert int(tick) == 2 and int(v["n"].sum()) == 2 * int((labels >= 0).sum())
    assert (v["d_sum"] == 0).all() and (v["conf_real"] == 0).all() and (v["cls"][1] == 0).all()
    assert int(v["conf_fake"].sum()) == int((labels >= 0).sum())


def test_eval_noise_depends_on_seed_and_split_row_alone():
    n, nd = 22, 128

    def draw(batch, seed):
        ctr, base = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        out = []
        for b in range((n + batch - 1) // batch):
            buf = torch.full((batch, nd), float("nan"), device="cuda")
            ctr.fill_(b + 5)
            base.fill_(5)
            ops.eval_noise(buf, ctr, base, n, seed)
            out.append(buf.cpu())
        return torch.cat(out)

    a, b, c = draw(8, 3), draw(5, 3), draw(22, 3)
    assert torch.equal(a[:n], b[:n]) and torch.equal(a[:n], c)         # bit-equal per split row, whatever the batch
    assert (a[n:] == 0).all() and (b[n:] == 0).all()                    # the padded tail is written with zeros
    assert torch.unique(a[:n], dim=0).shape[0] == n
    other = draw(8, 4)
    assert (other[:n] != a[:n]).float().mean() > 0.99
    big = torch.empty(4096, 128, device="cuda")
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.eval_noise(big, z, z, 4096, 1234)
    x = big.double().flatten().cpu()
    assert abs(float(x.mean())) <= 5.0 / x.numel() ** 0.5 and abs(float(x.std()) - 1.0) <= 5.0 / (2.0 * x.numel()) ** 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 2. the Evaluator against the oracle
# ---------------------------------------------------------------------------------------------------------------------
N_ROWS, BATCH = 22, 8


def gen_state(T, C, mode, ed_mode, d_scale=8.0):
    """tests/test_generate_gpu.py's closed-form weights (generator x4, last deconvolution x400, non-trivial BatchNorm running
    statistics), and the critic's matrices x8 so that w_dist is not rounding noise."""
    cfg, ed_cfg = O.default_gan_cfg(BATCH, T, C), O.default_ed_cfg(C)
    cfg["INTEGRATION_MODE"], ed_cfg["input_mode"] = mode, ed_mode
    S = O.build_gan_state(cfg, ed_cfg, "closed_form")
    for k in S.PG:
        if k.endswith("weight") and S.PG[k].dim() > 1:
            S.PG[k].mul_(4.0 * (400.0 if k == "decoder.deconv.6.weight" else 1.0))
    gen1 = os.path.join(ROOT, "tests", "golden", f"gen1_c{C}_t{T}.npz")
    if os.path.exists(gen1):
        S.PG["decoder.deconv.6.bias"].copy_(torch.from_numpy(np.load(gen1)["bias6"]))
    S.BG.update(O.fill_buffers(O.generator_buffers(), 70.0))
    for k in S.PD:
        if S.PD[k].dim() > 1:
            S.PD[k] = S.PD[k] * d_scale
    return S, cfg, ed_cfg


def save_state(S, d):
    ck, ed = os.path.join(d, "gan_epoch0001.pth"), os.path.join(d, "ed_best.pth")
    torch.save({"epoch": 1, "G": {**S.PG, **S.BG}, "D": S.PD, "E_num": S.PE}, ck)
    torch.save({"model": {**S.PED, **S.BED}}, ed)
    return ck, ed


def oracle_pass(S, cfg, ed_cfg, real, numeric, latent, noise, dtype):
    c = lambda P: type(P)((k, v.to(dtype)) for k, v in P.items())  # noqa: E731
    PE, PG, BG, PD, PED, BED = (c(P) for P in (S.PE, S.PG, S.BG, S.PD, S.PED, S.BED))
    real, numeric, latent, noise = (t.to(dtype) for t in (real, numeric, latent, noise))
    with torch.no_grad():
        emb = O.feature_encoder_fwd(PE, numeric, None)
        fake, lat = O.generator_fwd(PG, BG, noise, latent, emb, cfg["INTEGRATION_MODE"], cfg["MAX_NOTES"], train=False)
        out = {"emb": emb, "fake": fake, "lat": lat, "d_real": O.discriminator_fwd(PD, real, emb),
               "d_fake": O.discriminator_fwd(PD, fake, emb)}
        notes_mode = ed_cfg["input_mode"] == "notes"
        out["logits_fake"] = O.emotion_disc_fwd(PED, BED, fake if notes_mode else lat, ed_cfg, train=False)
        out["logits_real"] = O.emotion_disc_fwd(PED, BED, real, ed_cfg, train=False) if notes_mode else None
    return out


def reduce64(o, real, labels):
    """The report's float metrics from one oracle pass, reduced with torch in fp64."""
    n = len(labels)
    r = {"mean_real": o["d_real"].double().mean(), "mean_fake": o["d_fake"].double().mean()}
    r["w_dist"] = r["mean_real"] - r["mean_fake"]
    for side in ("fake", "real"):
        lg = o["logits_" + side]
        if lg is None:
            continue
        z = lg.double()
        ce = torch.logsumexp(z, 1) - z[torch.arange(n), labels]
        p = torch.softmax(z, 1)[torch.arange(n), labels]
        r[f"ce_{side}"], r[f"p_{side}"] = ce.mean(), p.mean()
        r[f"ce_{side}_k"] = torch.stack([ce[labels == k].mean() for k in range(K)])
        r[f"p_{side}_k"] = torch.stack([p[labels == k].mean() for k in range(K)])
    for side, x in (("real", real), ("fake", o["fake"])):
        x = x.double()
        r[f"mean_{side}_kc"] = torch.stack([x[labels == k].mean((0, 1)) for k in range(K)])
        r[f"std_{side}_kc"] = torch.stack([x[labels == k].flatten(0, 1).std(0, unbiased=False) for k in range(K)])
        r[f"min_{side}_kc"] = torch.stack([x[labels == k].amin((0, 1)) for k in range(K)])
        r[f"max_{side}_kc"] = torch.stack([x[labels == k].amax((0, 1)) for k in range(K)])
    return r


def report_values(rep):
    """The same quantities out of a report."""
    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    r = {k: t(rep["critic"][k]) for k in ("mean_real", "mean_fake", "w_dist")}
    for side in ("fake", "real"):
        e = rep["ed_" + side]
        if e is None:
            continue
        r[f"ce_{side}"], r[f"p_{side}"] = t(e["ce"]), t(e["mean_p_target"])
        r[f"ce_{side}_k"] = t([e["per_emotion"][nm]["ce"] for nm in EV.EMOTIONS])
        r[f"p_{side}_k"] = t([e["per_emotion"][nm]["mean_p_target"] for nm in EV.EMOTIONS])
    for side in ("real", "fake"):
        for q in ("mean", "std", "min", "max"):
            r[f"{q}_{side}_kc"] = t([[ch[q] for ch in rep["notes"][side][nm]["channels"]] for nm in EV.EMOTIONS])
    return r


def rel_err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def through_generator_ok(got, ref32, ref64, what, slack=8.0, floor=2e-6):
    """tests/test_engine_gpu.py's grad_ok(slack=8, floor=2e-6), the rule it applies to d_fake: the error against the oracle run
    in fp64 is at most 8x the fp32 oracle's own error against fp64, plus the floor."""
    e_mine, e_ref = rel_err(got, ref64), rel_err(ref32, ref64)
    print(f"{what}: error vs fp64 oracle {e_mine:.3g}, fp32 oracle's own {e_ref:.3g}, bound {slack * e_ref + floor:.3g}")
    assert e_mine <= slack * e_ref + floor, (what, e_mine, e_ref)


def check_report(rep, o32, o64, real, labels, notes_mode):
    """Case 2's checks of a report against the oracle passes in fp32 and fp64."""
    n = len(labels)
    got, r32, r64 = report_values(rep), reduce64(o32, real, labels), reduce64(o64, real, labels)
    assert rep["n"] == n
    counts = torch.bincount(labels, minlength=K)
    # real side: exact inputs
    print(f"mean_real {float(got['mean_real']):.6g} (oracle {float(r32['mean_real']):.6g})  w_dist {float(got['w_dist']):.6g} "
          f"(oracle fp64 {float(r64['w_dist']):.6g})")
    np.testing.assert_allclose(float(got["mean_real"]), float(r32["mean_real"]), rtol=1e-4, atol=2e-6)
    for q in ("mean", "std"):
        np.testing.assert_allclose(got[f"{q}_real_kc"].numpy(), r64[f"{q}_real_kc"].numpy(), rtol=1e-9, atol=1e-12)
    for q in ("min", "max"):
        assert torch.equal(got[f"{q}_real_kc"], r64[f"{q}_real_kc"])
        np.testing.assert_allclose(got[f"{q}_fake_kc"].numpy(), r32[f"{q}_fake_kc"].numpy(), rtol=1e-3, atol=1e-4)
    # means that pass through the generator
    names = ["mean_fake", "w_dist", "mean_fake_kc", "std_fake_kc", "ce_fake", "p_fake", "ce_fake_k", "p_fake_k"]
    for k in names:
        through_generator_ok(got[k], r32[k], r64[k], k)
    if notes_mode:
        for k in ("ce_real", "p_real", "ce_real_k", "p_real_k"):
            np.testing.assert_allclose(got[k].numpy(), r32[k].numpy(), rtol=1e-4, atol=2e-6)
    else:
        assert rep["ed_real"] is None
    # confusion: rows whose reference top-2 logit margin exceeds 1e-4 (the sampler test's rule); at most 10 % left out
    for side in ("fake", "real") if notes_mode else ("fake",):
        ref = o32["logits_" + side]
        top2 = torch.topk(ref, 2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 1e-4
        print(f"confusion {side}: {int(clear.sum())} of {n} rows clear, smallest margin {float((top2[:, 0] - top2[:, 1]).min()):.3g}")
        assert int((~clear).sum()) <= n // 10
        conf = torch.tensor(rep["ed_" + side]["confusion"])
        pred = torch.argmax(ref, 1)
        floor_ = torch.zeros(K, K, dtype=torch.int64)
        for i in torch.nonzero(clear).flatten().tolist():
            floor_[labels[i], pred[i]] += 1
        assert torch.equal(conf.sum(1), counts) and (conf >= floor_).all(), (conf, floor_)
        if clear.all():
            assert torch.equal(conf, floor_)
        acc = rep["ed_" + side]["accuracy"]
        assert abs(acc - float(torch.diagonal(conf).sum()) / n) <= 1e-12
        for k, nm in enumerate(EV.EMOTIONS):
            assert rep["ed_" + side]["per_emotion"][nm]["n"] == int(counts[k])
    for side in ("real", "fake"):
        assert [rep["notes"][side][nm]["n_rows"] for nm in EV.EMOTIONS] == counts.tolist()


def make_split(T, C, cfg, seed=7):
    real, numeric, latent, _ = O.synthetic_batch(N_ROWS, T, C, cfg["LATENT_DIM"], 6, seed)
    labels = torch.arange(N_ROWS) % K
    ds = GANDataset(real.numpy(), labels.numpy(), numeric.numpy(), None, cfg["LATENT_DIM"], "cuda")
    return ds, real, numeric, latent, labels


@pytest.mark.parametrize("T,C,mode,ed_mode", [(32, 4, "warm_start", "notes"), (64, 128, "warm_start", "notes"),
                                              (16, 4, "conditioning", "latent")])
def test_evaluator_matches_the_oracle(tmp_path, T, C, mode, ed_mode):
    S, cfg, ed_cfg = gen_state(T, C, mode, ed_mode)
    ck, ed = save_state(S, str(tmp_path))
    ds, real, numeric, latent, labels = make_split(T, C, cfg)
    noise = torch.randn(N_ROWS, cfg["NOISE_DIM"], generator=torch.Generator().manual_seed(11))
    ev = EV.Evaluator(cfg, ed_cfg, "cuda", BATCH)
    ev.load_generator(ck)
    assert ev.load_critic(ck) is True
    ev.load_ed(ed)
    noise_d = noise.cuda()
    rep = ev.evaluate(ds, seed=3, noise=noise_d)                        # 22 rows in batches of 8: a padded tail of 2
    json.loads(json.dumps(rep, allow_nan=False))
    assert (rep["n"], rep["seed"], rep["batch"]) == (N_ROWS, 3, BATCH)
    o32 = oracle_pass(S, cfg, ed_cfg, real, numeric, latent, noise, torch.float32)
    o64 = oracle_pass(S, cfg, ed_cfg, real, numeric, latent, noise, torch.float64)
    # per-sample quantities of the last batch (split rows 16..21 in engine rows 0..5), read from the engine
    eng, last = ev.eng, slice(2 * BATCH, N_ROWS)
    m = N_ROWS - 2 * BATCH
    assert eng.emot_idx.cpu().tolist() == labels[last].tolist() + [-1] * (BATCH - m)
    np.testing.assert_allclose(eng.fake_d[:m].cpu().numpy(), o32["fake"][last].numpy(), rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(eng.s[:m].cpu().numpy(), o32["d_real"][last].numpy(), rtol=1e-4, atol=2e-6)
    notes_mode = ed_mode == "notes"
    with torch.no_grad():       # the classifier on the engine's own rolls (or latent), as the sampler test does
        x = eng.fake_d[:m].cpu() if notes_mode else eng.lat[:m].cpu()
        ref = O.emotion_disc_fwd(S.PED, S.BED, x, ed_cfg, train=False)
    np.testing.assert_allclose(eng.logits[:m].cpu().numpy(), ref.numpy(), rtol=1e-4, atol=2e-6)
    if notes_mode:
        np.testing.assert_allclose(ev.logits_real[:m].cpu().numpy(), o32["logits_real"][last].numpy(), rtol=1e-4, atol=2e-6)
    check_report(rep, o32, o64, real, labels, notes_mode)
    # a second pass replays the cached graph from a reset accumulator: the same report, to the bit
    assert ev.evaluate(ds, seed=3, noise=noise_d) == rep
    # gan_final.pth holds no critic: null critic metrics, not an error
    final = os.path.join(str(tmp_path), "gan_final.pth")
    torch.save({"G": {**S.PG, **S.BG}, "E_num": S.PE}, final)
    ev2 = EV.Evaluator(cfg, ed_cfg, "cuda", BATCH)
    ev2.load_generator(final)
    assert ev2.load_critic(final) is False
    ev2.load_ed(ed)
    rep2 = ev2.evaluate(ds, seed=3, noise=noise_d)
    assert rep2["critic"] is None and rep2["ed_fake"] == rep["ed_fake"] and rep2["notes"] == rep["notes"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. batch-size independence
# ---------------------------------------------------------------------------------------------------------------------
def test_report_does_not_depend_on_the_batch_size(tmp_path):
    T, C = 32, 4
    S, cfg, ed_cfg = gen_state(T, C, "warm_start", "notes")
    ck, ed = save_state(S, str(tmp_path))
    ds, real, numeric, latent, labels = make_split(T, C, cfg)
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    drawn = ops.eval_noise(torch.empty(N_ROWS, cfg["NOISE_DIM"], device="cuda"), z, z, N_ROWS, 5).cpu()
    o32 = oracle_pass(S, cfg, ed_cfg, real, numeric, latent, drawn, torch.float32)
    o64 = oracle_pass(S, cfg, ed_cfg, real, numeric, latent, drawn, torch.float64)
    reps = {}
    for batch in (8, 5):
        ev = EV.Evaluator(cfg, ed_cfg, "cuda", batch)
        ev.load_generator(ck)
        ev.load_critic(ck)
        ev.load_ed(ed)
        reps[batch] = ev.evaluate(ds, seed=5)                           # noise drawn on the device
        nb = (N_ROWS + batch - 1) // batch
        m = N_ROWS - (nb - 1) * batch                                   # the last batch's rows: bit-equal to the direct draw
        assert torch.equal(ev.eng.noise[:m].cpu(), drawn[(nb - 1) * batch:]), batch
        assert (ev.eng.noise[m:] == 0).all()
        check_report(reps[batch], o32, o64, real, labels, True)         # each run within case 2's bounds of the oracle
    a, b = reps[8], reps[5]
    assert a["n"] == b["n"] == N_ROWS
    for side in ("ed_fake", "ed_real"):
        assert a[side]["confusion"] == b[side]["confusion"]
        assert [a[side]["per_emotion"][nm]["n"] for nm in EV.EMOTIONS] == [b[side]["per_emotion"][nm]["n"] for nm in EV.EMOTIONS]
    va, vb = report_values(a), report_values(b)
    r32, r64 = reduce64(o32, real, labels), reduce64(o64, real, labels)
    # the two runs against each other, every float metric by the bound case 2 holds it to
    for k in va:
        e = rel_err(va[k], vb[k])
        print(f"{k}: batch 8 vs batch 5 {e:.3g}")
        if k in ("min_real_kc", "max_real_kc"):
            assert torch.equal(va[k], vb[k]), k
        elif k in ("min_fake_kc", "max_fake_kc"):
            np.testing.assert_allclose(va[k].numpy(), vb[k].numpy(), rtol=1e-3, atol=1e-4, err_msg=k)
        elif k in ("mean_real_kc", "std_real_kc"):
            np.testing.assert_allclose(va[k].numpy(), vb[k].numpy(), rtol=1e-9, atol=1e-12, err_msg=k)
        elif k == "mean_real" or k.endswith(("_real", "_real_k")):
            np.testing.assert_allclose(va[k].numpy(), vb[k].numpy(), rtol=1e-4, atol=2e-6, err_msg=k)
        else:           # through the generator: grad_ok(slack=8, floor=2e-6) with the other run in the fp64 oracle's place
            e_ref = rel_err(r32[k], r64[k])
            assert e <= 8.0 * e_ref + 2e-6, (k, e, e_ref)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the trainer is not disturbed
# ---------------------------------------------------------------------------------------------------------------------
def read_scalars(log_dir):
    p = os.path.join(log_dir, "scalars.jsonl")
    if os.path.exists(p):
        out = {}
        for line in open(p):
            r = json.loads(line)
            out.setdefault(r["tag"], []).append((r["step"], r["value"]))
        return out
    from tensorboard.backend.event_processing.event_accumulator import EventAccumulator
    acc = EventAccumulator(log_dir)
    acc.Reload()
    return {t: [(e.step, e.value) for e in acc.Scalars(t)] for t in acc.Tags()["scalars"]}


def test_eval_every_leaves_training_bit_identical(tmp_path):
    from melo_gan_amd.gan import train_gan
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    ed = yaml.safe_load(open(os.path.join(ROOT, "config", "ed_config.yaml")))
    runs = {}
    for every in (1, 0):
        d = tmp_path / f"every{every}"
        c = dict(cfg, EPOCHS=2, BATCH_SIZE=4, MAX_NOTES=32, SAVE_FREQ=1, CRITIC_ITERS=2, CHECKPOINT_DIR=str(d / "ck"),
                 LOG_DIR=str(d / "log"), SAMPLE_DIR=str(d / "s"))
        train_gan.train(c, dict(ed), str(tmp_path / "none.pth"), synthetic=20, eval_every=every)
        runs[every] = d

    def same(a, b, path):
        assert type(a) is type(b), path
        if isinstance(a, dict):
            assert list(a) == list(b), path
            for k in a:
                same(a[k], b[k], f"{path}.{k}")
        elif isinstance(a, (list, tuple)):
            assert len(a) == len(b), path
            for i, (x, y) in enumerate(zip(a, b)):
                same(x, y, f"{path}[{i}]")
        elif isinstance(a, torch.Tensor):
            assert a.dtype == b.dtype and torch.equal(a, b), path
        else:
            assert a == b, path

    for name in ("gan_final.pth", "gan_epoch0001.pth", "gan_epoch0002.pth"):
        a = torch.load(runs[1] / "ck" / name, map_location="cpu")
        b = torch.load(runs[0] / "ck" / name, map_location="cpu")
        same(a, b, name)
    sc = read_scalars(str(runs[1] / "log"))
    for tag in ("Val/W_dist", "Val/ED_Acc_Fake", "Val/ED_CE_Fake", "Val/ED_Acc_Real"):
        assert [s for s, _ in sc[tag]] == [1, 2], (tag, sc.get(tag))
        assert all(np.isfinite(v) for _, v in sc[tag]), (tag, sc[tag])
    assert not any(t.startswith("Val/") for t in read_scalars(str(runs[0] / "log")))
    assert "Loss/Critic" in sc


# ---------------------------------------------------------------------------------------------------------------------
# 5. the CLI end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path):
    S, _, ed_cfg = gen_state(32, 4, "warm_start", "notes")
    ck, ed = save_state(S, str(tmp_path))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    cfg.update(MAX_NOTES=32, LOG_DIR=str(tmp_path / "log"))
    cp, ep = tmp_path / "gan.yaml", tmp_path / "ed.yaml"
    cp.write_text(yaml.safe_dump(cfg))
    ep.write_text(yaml.safe_dump(ed_cfg))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, "-m", "melo_gan_amd.gan.evaluate", "--config", str(cp), "--ckpt",
                        ck, "--ed_config", str(ep), "--ed_ckpt", ed, "--synthetic", "40", "--batch", "16", "--seed", "7"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=450)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rep = json.load(open(tmp_path / "log" / "eval.json"))
    assert rep["n"] == 40 and rep["seed"] == 7 and rep["batch"] == 16
    for side in ("ed_fake", "ed_real"):
        assert sum(rep[side]["per_emotion"][nm]["n"] for nm in EV.EMOTIONS) == 40
        assert sum(map(sum, rep[side]["confusion"])) == 40
    assert rep["critic"] is not None and abs(rep["critic"]["w_dist"] - (rep["critic"]["mean_real"] - rep["critic"]["mean_fake"])) < 1e-12
    assert sum(rep["notes"]["fake"][nm]["n_rows"] for nm in EV.EMOTIONS) == 40
    assert "w_dist" in r.stdout and all(nm in r.stdout for nm in EV.EMOTIONS)
