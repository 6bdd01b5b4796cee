"""GPU: blends and transitions between emotions (melo_gan_amd.gan.morph) -- the input kernel mg_gen_inputs_mix pinned to
mg_gen_inputs bit for bit, its blended base and its spherical interpolation against numpy, the two path reductions
(mg_path_d2, mg_path_probs) against their fp64 host restatement, the Morpher against the oracle and against its own stashed
rows, and the command end to end through the MIDI contract.  Fixtures are built in tmp_path."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import midi, ops  # noqa: E402
from melo_gan_amd.gan import generate as G  # noqa: E402
from melo_gan_amd.gan import morph as M  # noqa: E402
from melo_gan_amd.gan import morph_metrics as MM  # noqa: E402
from oracle import melo_oracle as O  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LAT = 64
U = 2.0 ** -24              # half an fp32 ulp, relative
WIDTHS = [(128, 6), (5, 3)]


def table_of(n_emotions, num_dim, seed=0):
    if (n_emotions, num_dim) == (4, 6):
        return torch.tensor(G.EMOTION_TABLE, dtype=torch.float32)
    return torch.randn(n_emotions, num_dim, generator=torch.Generator().manual_seed(seed))


def in_graph(launch):
    """launch() eagerly, then captured and replayed once."""
    launch()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        g = ops.Graph.capture(launch)
        g.launch()
        torch.cuda.synchronize()


def draw(keys, seed, noise_dim, table, jitter=G.JITTER):
    """mg_gen_inputs for a list of (emotion, sample) keys into NaN-filled buffers; returns host (noise, numeric)."""
    n = len(keys)
    kt = torch.tensor(keys, dtype=torch.int32).t().contiguous().cuda()
    noise, numeric, latent = (torch.full((n, w), float("nan"), device="cuda") for w in (noise_dim, table.shape[1], LAT))
    ops.gen_inputs(kt[0], kt[1], noise, numeric, table.cuda(), jitter, latent, seed)
    torch.cuda.synchronize()
    return noise.cpu(), numeric.cpu()


def mix(weights, key_a, key_b, t, seed, noise_dim, table, jitter=G.JITTER, graph=False):
    """mg_gen_inputs_mix into NaN-filled buffers; returns host (noise, numeric, latent)."""
    n = len(key_a)
    w = torch.as_tensor(np.asarray(weights, np.float32)).reshape(n, table.shape[0]).cuda()
    ka, kb = (torch.tensor(k, dtype=torch.int32).reshape(n, 2).cuda() for k in (key_a, key_b))
    tt = torch.tensor(t, dtype=torch.float32).cuda()
    noise, numeric, latent = (torch.full((n, d), float("nan"), device="cuda") for d in (noise_dim, table.shape[1], LAT))
    tb = table.cuda()
    launch = lambda: ops.gen_inputs_mix(w, ka, kb, tt, noise, numeric, tb, jitter, latent, seed)  # noqa: E731
    if graph:
        in_graph(launch)
    else:
        launch()
    torch.cuda.synchronize()
    return noise.cpu(), numeric.cpu(), latent.cpu()


def one_hot(emotions, n=4):
    w = np.zeros((len(emotions), n), np.float32)
    for r, e in enumerate(emotions):
        if 0 <= e < n:
            w[r, e] = 1.0
    return w


@pytest.mark.parametrize("noise_dim,num_dim", WIDTHS)
def test_mix_exact_rows_equal_gen_inputs_bit_for_bit(noise_dim, num_dim):
    table = table_of(4, num_dim)
    key_a = [(e, k) for k in (1, 2, 3) for e in range(4)]
    key_b = [((e + 1) % 4, k + 7) for e, k in key_a]
    nz_a, nm_a = draw(key_a, 11, noise_dim, table)
    # t = 0 with any key_b: key_a's rows; one-hot weights give the table's row
    nz, nm, lt = mix(one_hot([e for e, _ in key_a]), key_a, key_b, [0.0] * 12, 11, noise_dim, table)
    assert torch.equal(nz, nz_a) and torch.equal(nm, nm_a)
    assert torch.equal(lt, torch.zeros_like(lt))
    # t = 1: key_b's draw on key_a's base -- mg_gen_inputs under key_b with a table whose row e + 1 is row e
    nz_b, nm_b = draw(key_b, 11, noise_dim, torch.roll(table, 1, 0))
    nz, nm, _ = mix(one_hot([e for e, _ in key_a]), key_a, key_b, [1.0] * 12, 11, noise_dim, table)
    assert torch.equal(nz, nz_b) and torch.equal(nm, nm_b)
    assert not torch.equal(nz_a, nz_b)
    # key_a == key_b: key_a's row at every t
    nz, nm, _ = mix(one_hot([e for e, _ in key_a]), key_a, key_a, [0.3, 0.5, 1.0, 0.75] * 3, 11, noise_dim, table)
    assert torch.equal(nz, nz_a) and torch.equal(nm, nm_a)
    # padding rows (key_a's emotion outside the table) are zeros whatever else the row says
    pad_a = [(-1, 0), (4, 2), (1, 1)]
    nz, nm, lt = mix(np.full((3, 4), 0.25, np.float32), pad_a, [(0, 1)] * 3, [0.5, 0.0, 0.0], 11, noise_dim, table)
    assert torch.equal(nz[:2], torch.zeros(2, noise_dim)) and torch.equal(nm[:2], torch.zeros(2, num_dim))
    assert torch.isfinite(nz[2]).all() and nz[2].abs().sum() > 0 and torch.equal(lt, torch.zeros_like(lt))


def test_mix_rows_depend_on_their_descriptors_alone():
    table = table_of(4, 6)
    rng = np.random.default_rng(1)
    n = 64
    key_a = [(int(e), int(k)) for e, k in zip(rng.integers(0, 4, n), rng.integers(1, 9, n))]
    key_b = [(int(e), int(k)) for e, k in zip(rng.integers(0, 4, n), rng.integers(1, 9, n))]
    t = [float(v) for v in rng.choice([0.0, 0.25, 0.5, 0.8, 1.0], n)]
    w = rng.random((n, 4)).astype(np.float32)
    ref = mix(w, key_a, key_b, t, 5, 128, table)
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[1]).all()
    for chunk in (1, 3, 64):
        for order in (np.arange(n), rng.permutation(n)):
            for c0 in range(0, n, chunk):
                idx = order[c0:c0 + chunk]
                nz, nm, _ = mix(w[idx], [key_a[i] for i in idx], [key_b[i] for i in idx], [t[i] for i in idx], 5, 128, table)
                assert torch.equal(nz, ref[0][idx]) and torch.equal(nm, ref[1][idx]), (chunk, c0)
    rep = mix(w, key_a, key_b, t, 5, 128, table, graph=True)                        # replayed graph == eager launch
    assert torch.equal(rep[0], ref[0]) and torch.equal(rep[1], ref[1]) and torch.equal(rep[2], torch.zeros_like(rep[2]))
    other = mix(w, key_a, key_b, t, 6, 128, table)
    assert not torch.equal(other[0], ref[0])


def fma32(a, b, c):
    """The correctly rounded fp32 value of a * b + c (fp32 arrays), exactly: rational arithmetic, then the nearest of the
    fp32 neighbours of the fp64 quotient (ties to even)."""
    out = np.empty(a.shape, np.float32)
    for i in np.ndindex(a.shape):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = np.float32(float(exact))
        cand = [f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))]
        err = [abs(Fraction(float(x)) - exact) for x in cand]
        best = [x for x, e in zip(cand, err) if e == min(err)]
        out[i] = best[0] if len(best) == 1 else [x for x in best if not (x.view(np.uint32) & 1)][0]
    return out


@pytest.mark.parametrize("n_emotions", [4, 7])
@pytest.mark.parametrize("jitter", [0.25, G.JITTER])
def test_mix_blended_base_is_the_float32_chain(n_emotions, jitter):
    """base = sum_e w_e table[e] in class order with every product and sum rounded to fp32, then numeric = base + jitter * v with
    v obtained from mg_gen_inputs (zero table, jitter 1).  mg_gen_inputs evaluates `base + jitter * v` as ONE fused
    multiply-add (the test above pins the two kernels to each other at one-hot weights), so the last step of the chain is
    that fused operation, evaluated exactly here.  At jitter = 0.25 the product is exact and the fused step equals the plain
    float32 product and sum, which is asserted as well."""
    table = table_of(n_emotions, 6, seed=3)
    rng = np.random.default_rng(n_emotions)
    n = 24
    keys = [(int(e), int(k)) for e, k in zip(rng.integers(0, n_emotions, n), rng.integers(1, 5, n))]
    w = rng.random((n, n_emotions)).astype(np.float32)
    w /= w.sum(axis=1, keepdims=True)
    _, v = draw(keys, 9, 128, torch.zeros(n_emotions, 6), jitter=1.0)
    v, tb = v.numpy(), table.numpy()
    base = np.zeros((n, 6), np.float32)
    for e in range(n_emotions):
        base = base + (w[:, e:e + 1] * tb[e][None, :]).astype(np.float32)
        assert base.dtype == np.float32
    _, nm, _ = mix(w, keys, keys, [0.0] * n, 9, 128, table, jitter=jitter)
    j32 = np.full(v.shape, jitter, np.float32)
    assert np.array_equal(nm.numpy(), fma32(j32, v, base))
    if jitter == 0.25:
        assert np.array_equal(nm.numpy(), base + j32 * v)


@pytest.mark.parametrize("noise_dim,num_dim", WIDTHS)
def test_mix_slerp_against_numpy_fp64(noise_dim, num_dim):
    table = table_of(4, num_dim)
    zero = torch.zeros(4, num_dim)
    key_a = [(e, k) for e in range(4) for k in (1, 2)]
    key_b = [((e + 2) % 4, k + 3) for e, k in key_a]
    ts = [0.25, 0.5, 0.25, 0.5, 0.1, 0.9, 0.6, 0.5]
    jitter = G.JITTER
    (za, va), (zb, vb) = draw(key_a, 21, noise_dim, zero, jitter=1.0), draw(key_b, 21, noise_dim, zero, jitter=1.0)
    za, va, zb, vb = (x.double().numpy() for x in (za, va, zb, vb))
    w = one_hot([e for e, _ in key_a])
    nz, nm, _ = mix(w, key_a, key_b, ts, 21, noise_dim, table)
    nz, nm = nz.double().numpy(), nm.double().numpy()
    for r, t in enumerate(ts):
        t = float(np.float32(t))                    # the t the kernel reads
        a, b = np.linalg.norm(za[r]), np.linalg.norm(zb[r])
        c = float(np.clip(za[r] @ zb[r] / (a * b), -1.0, 1.0))
        theta = np.arccos(c)
        assert np.sin(theta) >= 2.0 ** -20
        ca, cb = np.sin((1 - t) * theta) / np.sin(theta), np.sin(t * theta) / np.sin(theta)
        ref = ca * za[r] + cb * zb[r]
        bound = 8 * U * (np.abs(ca * za[r]) + np.abs(cb * zb[r]))
        assert np.all(np.abs(nz[r] - ref) <= bound), (r, np.max(np.abs(nz[r] - ref) / bound))
        base = table[key_a[r][0]].double().numpy()
        ref_n = base + jitter * (ca * va[r] + cb * vb[r])
        bound_n = jitter * 8 * U * (np.abs(ca * va[r]) + np.abs(cb * vb[r])) + 2 * U * np.abs(nm[r])
        assert np.all(np.abs(nm[r] - ref_n) <= bound_n), (r, np.max(np.abs(nm[r] - ref_n) / bound_n))
        # the interpolated row's norm lies between the end points' norms.  That holds whenever cos(theta) >= 0, and for a
        # negative cosine as long as cb (a + b) >= 2 ca |cos| min(a, b) and the same with ca and cb swapped: two 128-wide
        # normal draws have |cos| of about 0.09, five-wide ones can have any.  Checked where the condition (a property of
        # the reference draws alone) holds, which the 128-wide rows must.
        holds = c >= 0 or (cb * (a + b) >= 2 * ca * abs(c) * min(a, b) and ca * (a + b) >= 2 * cb * abs(c) * min(a, b))
        assert holds or noise_dim < 128
        if t in (0.25, 0.5) and holds:
            assert min(a, b) - 1e-5 <= np.linalg.norm(nz[r]) <= max(a, b) + 1e-5, (r, a, b, np.linalg.norm(nz[r]))


def test_path_d2_against_numpy_fp64():
    gen = torch.Generator().manual_seed(0)
    for D in (1, 3, 4, 255, 256, 1027, 2048):
        for S1 in (1, 2, 9):
            for P in (1, 5):
                R = P * S1
                buf = torch.randn(R * D + 4, generator=gen).cuda()
                for shift in ((0, 1) if D % 4 == 0 else (0,)):          # shift 1: rows off the 16-byte grid, the element-wise path
                    x = buf[shift:shift + R * D].view(R, D)
                    if S1 == 9:
                        x[3].copy_(x[2])                                # twin rows
                    out = torch.full((P, S1), float("nan"), dtype=torch.float64, device="cuda")
                    ops.path_d2(x, P, S1, out)
                    got, ref = out.cpu().numpy(), MM.host_path_d2(x.cpu().numpy(), P, S1)
                    assert np.all(np.abs(got - ref) <= 1e-12 * ref), (D, S1, P, shift)
                    x3 = x.cpu().double().view(P, S1, D)
                    end = ((x3[:, S1 - 1] - x3[:, 0]) ** 2).sum(1).numpy()
                    assert np.all(np.abs(got[:, S1 - 1] - end) <= 1e-12 * end)
                    if S1 == 1:
                        assert np.all(got == 0.0)
                    if S1 == 9:
                        assert got[0, 2] == 0.0 and got[0, 1] > 0.0
    x = torch.randn(5 * 9, 1027, generator=gen).cuda()
    out = torch.zeros(5, 9, dtype=torch.float64, device="cuda")
    ops.path_d2(x, 5, 9, out)
    first = out.clone()
    out.fill_(float("nan"))
    in_graph(lambda: ops.path_d2(x, 5, 9, out))                         # a rerun and a replay leave the same bits
    assert torch.equal(first, out)


@pytest.mark.parametrize("K", [2, 4, 7, 32])
def test_path_probs_against_the_host(K):
    gen = torch.Generator().manual_seed(K)
    P, S1, Gn = 11, 5, 4
    logits = torch.randn(P * S1, K, generator=gen) * 4
    logits[3, 0] = logits[3, 1] = logits[3].max() + 1.0                 # a tie: the lowest index is the maximum taken out
    group = torch.tensor([0, 3, 3, -1, 0, 1, 3, 4, 0, 1, 3], dtype=torch.int32)      # group 2 is empty; -1 and 4 are skipped
    probs = torch.full((P * S1, K), float("nan"), dtype=torch.float64, device="cuda")
    acc = torch.full((Gn, S1, K + 1), float("nan"), dtype=torch.float64, device="cuda")
    lg, gr = logits.cuda(), group.cuda()
    ops.path_probs(lg, gr, S1, Gn, probs, acc)
    got_p, got_a = probs.cpu().numpy(), acc.cpu().numpy()
    ref_p, ref_a = MM.host_path_probs(logits.numpy(), group.numpy(), S1, Gn)
    assert np.all(np.abs(got_p - ref_p) <= 1e-14)
    assert np.all(np.abs(got_p.sum(1) - 1.0) <= 1e-14)
    assert np.array_equal(got_a[:, :, K], ref_a[:, :, K]) and np.all(got_a[2] == 0.0)
    assert got_a[:, 0, K].tolist() == [3.0, 2.0, 0.0, 4.0]
    assert np.all(np.abs(got_a[:, :, :K] - ref_a[:, :, :K]) <= 1e-12 * ref_a[:, :, :K])     # every term is positive
    first_p, first_a = probs.clone(), acc.clone()
    probs.fill_(float("nan"))
    acc.fill_(float("nan"))
    in_graph(lambda: ops.path_probs(lg, gr, S1, Gn, probs, acc))
    assert torch.equal(first_p, probs) and torch.equal(first_a, acc)


def gen_state(T, C, mode, ed_mode):
    """Closed-form weights as tests/test_generate_gpu.py::gen_state builds them."""
    cfg, ed_cfg = O.default_gan_cfg(8, T, C), O.default_ed_cfg(C)
    cfg["INTEGRATION_MODE"], ed_cfg["input_mode"] = mode, ed_mode
    S = O.build_gan_state(cfg, ed_cfg, "closed_form")
    for k in S.PG:
        if k.endswith("weight") and S.PG[k].dim() > 1:
            S.PG[k].mul_(4.0 * (400.0 if k == "decoder.deconv.6.weight" else 1.0))
    gen1 = os.path.join(ROOT, "tests", "golden", f"gen1_c{C}_t{T}.npz")
    if os.path.exists(gen1):
        S.PG["decoder.deconv.6.bias"].copy_(torch.from_numpy(np.load(gen1)["bias6"]))
    S.BG.update(O.fill_buffers(O.generator_buffers(), 70.0))
    return S, cfg, ed_cfg


def save_state(S, d):
    ck, ed = os.path.join(d, "gan_final.pth"), os.path.join(d, "ed_best.pth")
    torch.save({"G": {**S.PG, **S.BG}, "E_num": S.PE}, ck)
    torch.save({"model": {**S.PED, **S.BED}}, ed)
    return ck, ed


def close(a, b, rel=1e-9):
    """Two report values: None and fractions exactly, sums to the reductions' own agreement (the device's fixed trees and
    numpy's sums differ by rounding, 1e-12 relative; the report's square roots and quotients keep that)."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, dict):
        return set(a) == set(b) and all(close(a[k], b[k], rel) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(close(x, y, rel) for x, y in zip(a, b))
    return abs(a - b) <= rel * max(abs(a), abs(b))


@pytest.mark.parametrize("batch", [8, 64])
@pytest.mark.parametrize("T,C,mode,ed_mode", [(32, 4, "warm_start", "notes"), (16, 4, "conditioning", "latent")])
def test_morpher_matches_the_oracle_and_its_own_rows(tmp_path, T, C, mode, ed_mode, batch):
    S, cfg, ed_cfg = gen_state(T, C, mode, ed_mode)
    ck, ed = save_state(S, str(tmp_path))
    m = M.Morpher(cfg, ed_cfg, "cuda", batch)
    assert m.load_generator(ck) == "raw"
    m.load_ed(ed)
    steps, samples, a, b = 4, 2, 1, 0
    rows = M.pair_rows([(a, b)], steps, samples, "slerp")
    res = m.run(rows, seed=3)
    eng, R = m.eng, rows.P * rows.S1
    assert R == 10 and res.notes.shape == (R, T, C)
    # the engine's inputs (its last chunk) == the eager draw of those rows
    nz, nm, _ = mix(rows.weights, rows.key_a.tolist(), rows.key_b.tolist(), rows.t.tolist(), 3, cfg["NOISE_DIM"], table_of(4, 6))
    c0 = (R - 1) // batch * batch
    n = R - c0
    assert torch.equal(eng.noise[:n].cpu(), nz[c0:]) and torch.equal(eng.numeric[:n].cpu(), nm[c0:])
    assert torch.equal(eng.noise[n:].cpu(), torch.zeros(batch - n, cfg["NOISE_DIM"]))          # padding rows
    # step 0 is generate's sample (a, k), the last step its sample (b, k)
    gz, gm = draw([(a, 1), (b, 1)], 3, cfg["NOISE_DIM"], table_of(4, 6))
    assert torch.equal(nz[0], gz[0]) and torch.equal(nm[0], gm[0]) and torch.equal(nz[steps], gz[1]) and torch.equal(nm[steps], gm[1])
    with torch.no_grad():
        emb = O.feature_encoder_fwd(S.PE, nm, None)
        gen, lat = O.generator_fwd(S.PG, S.BG, nz, torch.zeros(R, cfg["LATENT_DIM"]), emb, mode, T, train=False)
    np.testing.assert_allclose(res.notes, gen.numpy(), rtol=1e-3, atol=1e-4)
    logits = m.stash["logits"].cpu()
    assert torch.equal(m.stash["rolls"].cpu().view(R, T, C), torch.from_numpy(res.notes))
    assert torch.equal(logits[c0:], eng.logits[:n].cpu())
    with torch.no_grad():
        if ed_mode == "notes":          # the classifier on the Morpher's own notes, every row
            ref = O.emotion_disc_fwd(S.PED, S.BED, torch.from_numpy(res.notes), ed_cfg, train=False)
            np.testing.assert_allclose(logits.numpy(), ref.numpy(), rtol=1e-4, atol=2e-6)
        else:                           # ... on its own latents, which the engine holds for its last chunk
            np.testing.assert_allclose(eng.lat[:n].cpu().numpy(), lat[c0:].numpy(), rtol=1e-4, atol=1e-6)
            ref = O.emotion_disc_fwd(S.PED, S.BED, eng.lat[:n].cpu(), ed_cfg, train=False)
            np.testing.assert_allclose(logits[c0:].numpy(), ref.numpy(), rtol=1e-4, atol=2e-6)
    # the report == morph_metrics applied to host_path_stats of the stashed rows
    feats = m.stash["feature"]
    assert (feats is None) == (ed_mode == "latent")
    host = MM.host_path_stats(logits.numpy(), rows.group, rows.S1, rows.G, None if feats is None else feats.cpu().numpy(),
                              m.stash["rolls"].cpu().numpy())
    assert np.all(np.abs(res.stats.probs - host.probs) <= 1e-14)
    w = [s / steps for s in range(steps + 1)]
    got = MM.pair_report(res.stats, 0, [0, 1], w, a, b)
    want = MM.pair_report(host, 0, [0, 1], w, a, b)
    assert close(got, want), (got, want)
    assert got["monotone_fraction"] == want["monotone_fraction"] and got["switch_fraction"] == want["switch_fraction"]
    assert (got["feature"] is None) == (ed_mode == "latent")
    assert got["roll"]["path_length"] > 0 and len(got["p_mean"]) == steps + 1 and len(got["p_mean"][0]) == 4
    # a blended point through the same engine: the heaviest emotion's key, t = 0
    blend = M.blend_rows([0.7, 0.0, 0.0, 0.3], 2)
    out = m.run(blend, seed=3)
    bz, bm, _ = mix(blend.weights, blend.key_a.tolist(), blend.key_b.tolist(), blend.t.tolist(), 3, cfg["NOISE_DIM"], table_of(4, 6))
    assert torch.equal(eng.noise[:2].cpu(), bz) and torch.equal(eng.numeric[:2].cpu(), bm) and torch.equal(bz, draw([(0, 1), (0, 2)], 3, 128, table_of(4, 6))[0])
    assert out.stats.acc[0, 0, 4] == 2.0 and np.all(out.stats.roll == 0.0)


def test_morpher_without_a_classifier_reports_the_rolls_alone(tmp_path):
    S, cfg, _ = gen_state(16, 4, "conditioning", "latent")
    ck, _ = save_state(S, str(tmp_path))
    m = M.Morpher(cfg, None, "cuda", 4)
    m.load_generator(ck)
    rows = M.pair_rows([(0, 3)], 2, 1, "fixed")
    res = m.run(rows, seed=1)
    assert res.stats.probs is None and res.stats.acc is None and res.stats.feature is None
    rep = MM.pair_report(res.stats, 0, [0], [0.0, 0.5, 1.0], 0, 3)
    assert rep["p_mean"] is None and rep["feature"] is None and rep["roll"]["path_length"] > 0
    assert close(rep["roll"], MM.distance_block(MM.host_path_d2(res.notes.reshape(3, -1), 1, 3), 2))


def test_blend_and_all_pairs_with_wav_in_process(tmp_path, capsys):
    """The command's other two modes at T = 16, in process: --weights with --wav, and --pairs all with --join and --wav."""
    import wave
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    cfg.update(MAX_NOTES=16)
    S = O.build_gan_state(O.default_gan_cfg(2, 16, 4), O.default_ed_cfg(4))
    S.PG["decoder.deconv.6.weight"].mul_(400.0)                         # rolls that sound
    ck = str(tmp_path / "gan_final.pth")
    torch.save({"G": {**S.PG, **S.BG}, "E_num": S.PE}, ck)
    cfg_path = tmp_path / "gan.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    base = ["--config", str(cfg_path), "--ckpt", ck, "--seed", "5", "--batch", "4", "--wav", "--wav-fs", "8000", "--voice", "sine"]
    out = tmp_path / "blend"
    assert M.main(base + ["--weights", "happy=0.7,calm=0.3", "--samples", "2", "--out", str(out)]) == 0
    assert sorted(os.listdir(out)) == ["blend_1.mid", "blend_1.wav", "blend_2.mid", "blend_2.wav", "morph.json"]
    rep = json.load(open(out / "morph.json"))
    assert rep["mode"] == "blend" and rep["blend"]["key_emotion"] == "happy" and rep["blend"]["p_mean"] is None
    assert abs(rep["blend"]["weights"]["happy"] - 0.7) <= 1e-12 and abs(rep["blend"]["weights"]["calm"] - 0.3) <= 1e-12
    assert rep["wav"] == {"fs": 8000, "voice": "sine", "peak_db": -1.0}
    scale, bpm = M.style_of([0.7, 0.0, 0.0, 0.3])
    assert (scale, bpm) == ("major", round(0.7 * 140 + 0.3 * 90))
    for f in rep["files"]:
        assert (f["bpm"], f["scale"], f["wav"]) == (bpm, scale, f["file"][:-4] + ".wav") and f["truncated"] is False
        (fmt, div), tempo, _ = midi.read_smf_notes(str(out / f["file"]))
        assert (fmt, div) == (1, 220) and tempo == round(6e7 / bpm)
        with wave.open(str(out / f["wav"])) as w:
            assert (w.getframerate(), w.getnchannels(), w.getsampwidth()) == (8000, 1, 2)
            assert abs(w.getnframes() / 8000 - f["seconds"]) <= 1e-9
    out = tmp_path / "pairs"
    assert M.main(base + ["--pairs", "all", "--steps", "1", "--samples", "1", "--join", "--join-notes", "4", "--out", str(out)]) == 0
    names = G.EMOTIONS
    pairs = [(names[a], names[b]) for a in range(4) for b in range(a + 1, 4)]
    mids = [f"morph_{a}_{b}_1_s{s:02d}.mid" for a, b in pairs for s in (0, 1)] + [f"morph_{a}_{b}_1.mid" for a, b in pairs]
    assert sorted(os.listdir(out)) == sorted(mids + [m[:-4] + ".wav" for m in mids] + ["morph.json"])
    rep = json.load(open(out / "morph.json"))
    assert [(p["from"], p["to"]) for p in rep["pairs"]] == pairs and rep["noise"] == "fixed"
    assert all(p["p_mean"] is None and p["feature"] is None and p["roll"]["ppl"] >= 0.0 for p in rep["pairs"])
    # a path of one step is its own chord
    assert all(p["roll"]["path_length"] == p["roll"]["endpoint_distance"] for p in rep["pairs"])
    capsys.readouterr()


def test_cli_end_to_end(tmp_path):
    S, _, ed_cfg = gen_state(512, 4, "warm_start", "notes")
    ck, ed = save_state(S, str(tmp_path))
    cfg_path = os.path.join(ROOT, "config", "gan_config.yaml")
    cfg = yaml.safe_load(open(cfg_path))
    assert (cfg["MAX_NOTES"], cfg["NOTE_DIM"], cfg["INTEGRATION_MODE"]) == (512, 4, "warm_start")
    ed_yaml = tmp_path / "ed.yaml"
    ed_yaml.write_text(yaml.safe_dump(ed_cfg))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "melo_gan_amd.gan.morph", "--config", cfg_path, "--ckpt", ck, "--from", "sad", "--to", "happy",
                        "--steps", "2", "--samples", "1", "--join", "--noise", "slerp", "--seed", "7", "--out", str(out),
                        "--ed_config", str(ed_yaml), "--ed_ckpt", ed], cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    steps = [f"morph_sad_happy_1_s{s:02d}.mid" for s in range(3)]
    assert sorted(f for f in os.listdir(out)) == sorted(steps + ["morph_sad_happy_1.mid", "morph.json"])
    # the same seed and batch in process
    m = M.Morpher(cfg, ed_cfg, "cuda", 64)
    m.load_generator(ck)
    m.load_ed(ed)
    rows = M.pair_rows([(1, 0)], 2, 1, "slerp")
    res = m.run(rows, seed=7)
    styles = [("minor", 70), ("major", 105), ("major", 140)]          # the tie at 0.5 goes to the lower class index: happy
    ref = str(tmp_path / "ref.mid")
    for s, name in enumerate(steps):
        scale, bpm = styles[s]
        assert M.style_of(rows.weights[s]) == (scale, bpm)
        midi.save_piano_roll_to_midi(res.notes[s], ref, bpm=bpm, scale=scale, root_key=0)
        assert (out / name).read_bytes() == open(ref, "rb").read(), name
    # --noise slerp: the end points' inputs are the Sampler's for (sad, 1) and (happy, 1)
    smp = G.Sampler(cfg, None, "cuda", 2)
    smp.load_generator(ck)
    got = smp.sample(["sad", "happy"], 1, seed=7)
    assert got.emotion == ["sad", "happy"] and got.k == [1, 1]
    for row, srow in ((0, 0), (2, 1)):
        assert torch.equal(m.eng.noise[row].cpu(), smp.eng.noise[srow].cpu())
        assert torch.equal(m.eng.numeric[row].cpu(), smp.eng.numeric[srow].cpu())
    # the joined piece: every step's first 64 rows' notes, each step offset by the running end time, written at 120 bpm
    notes, end = [], 0.0
    for s in range(3):
        scale, bpm = styles[s]
        own, _ = midi.notes_from_roll(res.notes[s][:64], bpm=bpm, scale=scale, root_key=0)
        notes += [(v, p, end + t0, end + t1) for v, p, t0, t1 in own]
        for row in res.notes[s][:64]:
            end += max(0.1, ((float(row[3]) + 1.0) / 2.0) * 4.0) * 60.0 / bpm
    assert len(notes) > 0
    midi.write_smf(ref, notes, 120.0, 0)
    assert (out / "morph_sad_happy_1.mid").read_bytes() == open(ref, "rb").read()
    (fmt, div), tempo, _ = midi.read_smf_notes(str(out / "morph_sad_happy_1.mid"))
    assert (fmt, div) == (1, 220) and tempo == 500000
    rep = json.load(open(out / "morph.json"))
    assert (rep["checkpoint"], rep["weights"], rep["seed"], rep["steps"], rep["samples"], rep["noise"]) == (ck, "raw", 7, 2, 1, "slerp")
    assert sorted(f["file"] for f in rep["files"]) == sorted(steps + ["morph_sad_happy_1.mid"])
    assert len(rep["pairs"]) == 1
    blk = rep["pairs"][0]
    assert (blk["from"], blk["to"], blk["w"]) == ("sad", "happy", [0.0, 0.5, 1.0])
    assert set(blk) == {"from", "to", "w", "p_mean", "crossover", "monotone_fraction", "switch_fraction", "feature", "roll"}
    for space in ("feature", "roll"):
        assert set(blk[space]) == {"path_length", "endpoint_distance", "straightness", "ppl"}
    assert len(blk["p_mean"]) == 3 and all(abs(sum(p) - 1.0) <= 1e-12 for p in blk["p_mean"])
    assert close({k: blk[k] for k in blk if k not in ("from", "to")}, MM.pair_report(res.stats, 0, [0], [0.0, 0.5, 1.0], 1, 0))
