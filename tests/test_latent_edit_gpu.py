"""GPU: edits in the VAE's latent space (melo_gan_amd.ae.edit) -- mg_latent_rows on its exact cases, its keys and normals and
against the fp64 host restatement fed the device's own normals, mg_latent_cycle against its restatement, the LatentEditor against
VaeEngine.forward, the decoder-only reference and the oracle's encoder, and the command end to end through the MIDI contract."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import midi, ops  # noqa: E402
from melo_gan_amd.ae import edit as ED  # noqa: E402
from melo_gan_amd.ae import latent_edit as LE  # noqa: E402
from oracle import melo_oracle as O  # noqa: E402

WIDTHS = [5, 64, 130, 1024]         # less than a wave, exactly a wave, more than a wave and no multiple of 4, the maximum
N_SRC, N_DIR = 3, 2
SEED = 17
FIELDS = ("kind", "src_a", "src_b", "t", "dir", "alpha", "sigma", "key")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def sources(Ld):
    g = torch.Generator().manual_seed(Ld)
    return (torch.randn(N_SRC, Ld, generator=g), 0.5 * torch.randn(N_SRC, Ld, generator=g), torch.randn(N_DIR, Ld, generator=g))


def table(rows):
    """Row descriptors from a list of dicts (missing fields: a prior row with sigma 0 under the key (0, 0)) as an LE.Rows."""
    R = len(rows)
    col = lambda name, default, dt: np.array([r.get(name, default) for r in rows], dt)  # noqa: E731
    return LE.Rows("test", col("kind", 1, np.int32), col("a", 0, np.int32), col("b", 0, np.int32), col("t", 0.0, np.float32),
                   col("dir", -1, np.int32), col("alpha", 0.0, np.float32), col("sigma", 0.0, np.float32),
                   np.array([r.get("key", (0, 0)) for r in rows], np.int32).reshape(R, 2), list(range(N_SRC)))


def in_graph(launch):
    """launch() eagerly, then captured and replayed once."""
    launch()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        g = ops.Graph.capture(launch)
        g.launch()
        torch.cuda.synchronize()


def device_rows(rows, Ld, src=None, seed=SEED, interp=0, graph=False):
    """mg_latent_rows into a NaN-filled buffer; returns the host z (R, Ld)."""
    mu, lv, dirs = (v.cuda() for v in (sources(Ld) if src is None else src))
    d = {n: torch.from_numpy(np.ascontiguousarray(getattr(rows, n))).cuda() for n in FIELDS}
    z = torch.full((rows.R, Ld), float("nan"), device="cuda")
    launch = lambda: ops.latent_rows(mu, lv, dirs, *(d[n] for n in FIELDS), z, interp, seed)  # noqa: E731
    if graph:
        in_graph(launch)
    else:
        launch()
    torch.cuda.synchronize()
    return z.cpu().numpy()


def normals(keys, Ld, seed=SEED):
    """The device's N(0,1) draws of these keys, read back from prior rows with sigma = 1."""
    return device_rows(table([dict(kind=1, sigma=1.0, key=k) for k in keys]), Ld, seed=seed)


@pytest.mark.parametrize("Ld", WIDTHS)
def test_rows_exact_cases(Ld):
    mu, lv, dirs = sources(Ld)
    for interp in (0, 1):
        rows = table([dict(kind=2, a=1, b=2, t=0.0), dict(kind=2, a=1, b=2, t=1.0), dict(kind=2, a=2, b=2, t=0.4),
                      dict(kind=2, a=0, b=1, t=0.0, dir=1, alpha=0.0), dict(kind=2, a=0, b=1, t=1.0, dir=-1, alpha=3.0),
                      dict(kind=0, a=99, b=-5, dir=77, alpha=2.0, sigma=1.0, t=0.5), dict(kind=0),
                      ])
        z = device_rows(rows, Ld, interp=interp)
        for r, want in enumerate((mu[1], mu[2], mu[2], mu[0], mu[1])):
            assert np.array_equal(bits(z[r]), bits(want.numpy())), (interp, r)
        assert not z[5].any() and not z[6].any() and not np.signbit(z[5:]).any()       # padding: zeros, whatever the row holds
    # a single row, and a prior row with sigma = 2 against the sigma = 1 row of its key
    one = device_rows(table([dict(kind=2, a=2, b=0, t=1.0)]), Ld)
    assert np.array_equal(bits(one[0]), bits(mu[0].numpy()))
    n1 = normals([(3, 4)], Ld)
    n2 = device_rows(table([dict(kind=1, sigma=2.0, key=(3, 4))]), Ld)
    assert np.isfinite(n1).all() and np.array_equal(bits(n2), bits(2.0 * n1))


@pytest.mark.parametrize("Ld", WIDTHS)
def test_rows_normals_depend_on_the_key_and_the_seed_alone(Ld):
    keys = [(5, 1), (5, 2), (-1, 1), (0, 1), (2 ** 31 - 1, 7), (5, 3), (1, 1)]
    ref = normals(keys, Ld)                                                 # a launch of 7 rows
    assert np.isfinite(ref).all()
    for i, k in enumerate(keys):
        assert np.array_equal(bits(normals([k], Ld)), bits(ref[i:i + 1])), k           # alone, in a launch of 1 row
    perm = [3, 0, 6, 2, 5, 1, 4]
    assert np.array_equal(bits(normals([keys[i] for i in perm], Ld)), bits(ref[perm]))
    # among other kinds of rows: a posterior row with sigma = 1 and logvar = 0 adds the same normals to mu
    mu, lv, dirs = sources(Ld)
    mixed = device_rows(table([dict(kind=0), dict(kind=2, a=1, b=1, sigma=1.0, key=keys[0]), dict(kind=1, sigma=1.0, key=keys[4])]), Ld,
                        src=(mu, torch.zeros_like(lv), dirs))
    assert np.array_equal(bits(mixed[2]), bits(ref[4]))
    want = (mu[1].double().numpy() + ref[0].astype(np.float64)).astype(np.float32)      # exp(0) = 1 exactly: one rounding
    assert np.array_equal(bits(mixed[1]), bits(want))
    # other keys and other seeds: other numbers
    for a, b in ((ref[0], ref[1]), (ref[0], ref[3]), (ref[0], ref[5]), (ref[2], ref[3])):
        assert np.mean(a != b) > 0.99
    other = normals(keys, Ld, seed=SEED + 1)
    assert np.mean(other != ref) > 0.99
    assert not np.array_equal(bits(normals(keys, Ld, seed=SEED + (1 << 32))), bits(ref))           # the seed's high word counts


@pytest.mark.parametrize("Ld", WIDTHS)
def test_rows_normals_statistics(Ld):
    keys = [(p, k) for p in (-1, 0, 9) for k in range(1, 22)]
    x = normals(keys, Ld).astype(np.float64).ravel()
    n = x.size
    assert abs(x.mean()) <= 5 / np.sqrt(n) and abs(x.std() - 1.0) <= 5 / np.sqrt(2 * n), (x.mean(), x.std(), n)


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("Ld", WIDTHS)
def test_rows_against_the_host_restatement(Ld, interp):
    src = sources(Ld)
    keys = [(1, 1), (1, 2), (2, 1), (-1, 3), (0, 5), (0, 6), (2, 2)]
    rows = table([dict(kind=2, a=0, b=1, t=0.25, sigma=1.0, key=keys[0]),
                  dict(kind=2, a=1, b=2, t=0.5, dir=1, alpha=0.75, sigma=0.5, key=keys[1]),
                  dict(kind=2, a=2, b=0, t=0.9, dir=0, alpha=-1.5, key=keys[2]),
                  dict(kind=1, dir=1, alpha=2.0, sigma=0.7, key=keys[3]),
                  dict(kind=2, a=0, b=0, t=0.3, sigma=2.0, key=keys[4]),
                  dict(kind=2, a=1, b=0, t=1.0, dir=0, alpha=0.5, sigma=1.0, key=keys[5]),
                  dict(kind=0, key=keys[6])])
    rows.interp = interp
    n = normals(keys, Ld)
    host, base, move, noise = LE.host_latent_rows(*(v.numpy() for v in src), rows, n, parts=True)
    dev = device_rows(rows, Ld, src=src, interp=interp)
    bound = 2.0 ** -23 * (np.abs(base) + np.abs(move) + np.abs(noise))
    err = np.abs(dev.astype(np.float64) - host.astype(np.float64))
    print(f"L {Ld} interp {interp}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}, rows that differ {int((err > 0).any(axis=1).sum())}")
    assert np.isfinite(dev).all() and np.all(err <= bound), np.max(err / np.maximum(bound, 1e-300))
    assert not dev[6].any()
    # the same rows in a launch of 1, and eager against a replayed graph: identical bits
    first = LE.Rows("test", *(getattr(rows, f)[1:2] for f in FIELDS), rows.sources, interp)
    assert np.array_equal(bits(device_rows(first, Ld, src=src, interp=interp)), bits(dev[1:2]))
    assert np.array_equal(bits(device_rows(rows, Ld, src=src, interp=interp, graph=True)), bits(dev))


def test_rows_slerp_of_parallel_sources_is_the_chord():
    Ld = 130
    mu, lv, dirs = sources(Ld)
    mu[1] = 2.0 * mu[0]
    mu[2] = 0.0
    rows = table([dict(kind=2, a=0, b=1, t=0.5), dict(kind=2, a=0, b=2, t=0.25)])
    z = device_rows(rows, Ld, src=(mu, lv, dirs), interp=1)
    assert np.array_equal(z[0], (1.5 * mu[0].double().numpy()).astype(np.float32))
    assert np.array_equal(z[1], (0.75 * mu[0].double().numpy()).astype(np.float32))


def test_rows_and_cycle_refuse_bad_arguments_before_any_launch():
    Ld = 8
    mu, lv, dirs = (v.cuda() for v in sources(Ld))
    rows = table([dict(kind=2, a=0, b=1, t=0.5)] * 3)
    d = {n: torch.from_numpy(np.ascontiguousarray(getattr(rows, n))).cuda() for n in FIELDS}
    z = torch.full((3, Ld), float("nan"), device="cuda")
    call = lambda **kw: ops.latent_rows(*(kw.get(k, v) for k, v in (("mu", mu), ("logvar", lv), ("dirs", dirs))),  # noqa: E731
                                        *(kw.get(n, d[n]) for n in FIELDS), kw.get("z", z), kw.get("interp", 0), 1)
    for kw in (dict(z=torch.zeros(3, 1025, device="cuda")), dict(z=z.double()), dict(kind=d["kind"][:2]), dict(t=d["t"].double()),
               dict(key=d["key"][:, :1].contiguous()), dict(mu=mu[:, :4].contiguous()), dict(logvar=lv[:2]), dict(dirs=dirs.cpu()),
               dict(interp=2), dict(dir=d["dir"].long())):
        with pytest.raises(ValueError):
            call(**kw)
    from melo_gan_amd import _lib
    lib = _lib.load()
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    raw = lambda mu_=mu, n_src=N_SRC, R=3, L_=Ld: lib.mg_latent_rows(  # noqa: E731
        p(mu_), p(lv), n_src, p(dirs), N_DIR, *(p(d[n]) for n in FIELDS), R, L_, 0, 1, p(z), None)
    assert raw(mu_=None) == -1 and raw(R=-1) == -1 and raw(L_=0) == -1 and raw(L_=1025) == -1 and raw(n_src=-1) == -1
    assert raw(R=0) == 0
    cyc = torch.full((3, 6), float("nan"), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        ops.latent_cycle(z, z[:2], mu, dirs, d["kind"], d["src_a"], d["dir"], cyc)
    with pytest.raises(ValueError):
        ops.latent_cycle(z, z, mu, dirs, d["kind"], d["src_a"], d["dir"], cyc.float())
    torch.cuda.synchronize()
    assert torch.isnan(z).all() and torch.isnan(cyc).all()                  # nothing was launched
    # a row that points outside its array reads nothing and comes back as NaN; its neighbours are untouched by it
    rows = table([dict(kind=2, a=0, b=0), dict(kind=2, a=N_SRC, b=0), dict(kind=2, a=0, b=0, dir=N_DIR, alpha=1.0), dict(kind=7)])
    out = device_rows(rows, Ld)
    assert np.isfinite(out[0]).all() and np.isnan(out[1:]).all()


# ---- mg_latent_cycle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ld", WIDTHS)
def test_cycle_against_the_host_restatement(Ld):
    mu, lv, dirs = sources(Ld)
    g = torch.Generator().manual_seed(Ld + 1)
    R = 7
    z = torch.randn(R, Ld, generator=g)
    mu2 = z + 0.1 * torch.randn(R, Ld, generator=g)
    z[5], mu2[5] = mu[2], mu[2]                                             # identical inputs
    kind = np.array([2, 1, 0, 2, 1, 2, 2], np.int32)
    a = np.array([0, 99, -3, 1, 0, 2, 2], np.int32)
    dr = np.array([0, 1, 55, -1, -1, 1, 0], np.int32)
    out = torch.full((R, 6), float("nan"), dtype=torch.float64, device="cuda")
    dev = [t.cuda() for t in (z, mu2, mu, dirs)] + [torch.from_numpy(v).cuda() for v in (kind, a, dr)]
    launch = lambda: ops.latent_cycle(*dev, out)  # noqa: E731
    launch()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    host = LE.host_latent_cycle(z.numpy(), mu2.numpy(), mu.numpy(), dirs.numpy(), kind, a, dr)
    Z, M2, M, D = (v.double().numpy() for v in (z, mu2, mu, dirs))
    for r in range(R):
        m = M[a[r]] if kind[r] == 2 else np.zeros(Ld)
        d = D[dr[r]] if dr[r] >= 0 and kind[r] != 0 else np.zeros(Ld)
        terms = [(Z[r] - m) ** 2, (M2[r] - Z[r]) ** 2, (M2[r] - m) ** 2, (M2[r] - m) * d, (Z[r] - m) * d, d * d]
        for w, t in enumerate(terms):
            tol = 0.0 if kind[r] == 0 else 1e-12 * np.abs(t).sum()
            assert abs(got[r, w] - host[r, w]) <= tol and abs(got[r, w] - (0.0 if kind[r] == 0 else t.sum())) <= tol, (r, w)
    assert not got[2].any() and not got[3, 3:].any() and not got[4, 3:].any()
    assert got[5, :3].tolist() == [0.0, 0.0, 0.0] and got[5, 3] == 0.0 and got[5, 4] == 0.0 and got[5, 5] > 0
    first = got.copy()
    out.fill_(float("nan"))
    in_graph(launch)                                                        # a rerun and a replayed graph: identical bits
    assert np.array_equal(bits(out.cpu().numpy()), bits(first))
    one = ops.latent_cycle(*(t[:1].contiguous() if i in (0, 1, 4, 5, 6) else t for i, t in enumerate(dev)))
    assert np.array_equal(bits(one.cpu().numpy()), bits(first[:1]))


# ---- LatentEditor --------------------------------------------------------------------------------------------------------
LAT, N_NOTES = 8, 6


def vae_model(T):
    spec, bufs = O.vae_spec(T, LAT)
    P = O.fill_params(spec, 6.0, O.norm_affine_names(spec))
    Bf = {k: (torch.rand(s, generator=torch.Generator().manual_seed(1)) + 0.5 if k.endswith("running_var")
              else torch.randn(s, generator=torch.Generator().manual_seed(2)) * 0.1) for k, s in bufs.items()}
    return P, Bf


def cfg_of(T, B=4):
    return dict(MAX_NOTES=T, LATENT_DIM=LAT, BATCH_SIZE=B, LR=1e-4, WEIGHT_DECAY=1e-5)


def nine_rows():
    """9 output rows over 6 sources: rows 0-3 are sources 0-3 untouched, the rest noisy variations."""
    rows = LE.vary_rows([0, 1, 2, 3, 4, 5, 4, 5, 0], 1, 1.0, n_split=N_NOTES)
    rows.sigma[:4] = 0.0
    rows.key[:, 1] = np.arange(9)
    return rows


@pytest.mark.parametrize("T", [16, 20])
def test_editor_against_forward_the_decoder_reference_and_the_oracle(T):
    from melo_gan_amd.ae.engine import VaeEngine
    from vae_decode_ref import vae_decode
    P, Bf = vae_model(T)
    notes = torch.rand(N_NOTES, T, 4, generator=torch.Generator().manual_seed(7)) * 2 - 1
    rows = nine_rows()
    ed = ED.LatentEditor(cfg_of(T), "cuda", 4)                              # 9 + 6 rows at batch 4: a padded tail chunk
    ed.eng.load_state(P, Bf)
    res = ed.run(notes.cuda(), rows, SEED)
    assert res.R == 9 and res.z.shape == (15, LAT) and res.recon.shape == (15, T, 4) and res.cycle.shape == (15, 6)
    for a in (res.z, res.recon, res.mu2, res.cycle):
        assert np.isfinite(a).all()
    # identity rows reproduce forward(train=False) at eps = 0 for the same sources in the same batch slots
    fwd = VaeEngine(cfg_of(T), "cuda", 4)
    fwd.load_state(P, Bf)
    with torch.cuda.stream(fwd.stream):
        fwd.x.copy_(notes[:4].cuda())
        fwd.eps.zero_()
        fwd.forward(train=False)
    torch.cuda.synchronize()
    assert np.array_equal(bits(res.z[:4]), bits(fwd.mu.cpu().numpy())) and np.array_equal(bits(res.z[:4]), bits(fwd.zl.cpu().numpy()))
    assert np.array_equal(bits(res.recon[:4]), bits(fwd.recon.cpu().numpy()))
    assert np.array_equal(bits(res.z[9:13]), bits(res.z[:4]))               # the run's own identity rows of the sources
    # the device's z through the decoder-only reference, and the oracle's encoder on the device's recon
    np.testing.assert_allclose(res.recon, vae_decode(P, Bf, torch.from_numpy(res.z), T).numpy(), rtol=1e-3, atol=1e-5)
    _, _, mu_ref, _ = O.vae_fwd(P, Bf, torch.from_numpy(res.recon), torch.zeros(15, LAT), T, train=False)
    np.testing.assert_allclose(res.mu2, mu_ref.numpy(), rtol=2e-3, atol=2e-5)
    # the noisy rows moved, along their own normals; the cycle words are those of the arrays the run returns
    assert (np.abs(res.z[4:9] - res.z[[13, 14, 13, 14, 9]]) > 0).mean() > 0.99
    kind = np.full(15, 2, np.int32)
    src = np.concatenate([rows.src_a, np.arange(6, dtype=np.int32)])
    host = LE.host_latent_cycle(res.z, res.mu2, res.z[9:], None, kind, src, np.full(15, -1, np.int32))
    np.testing.assert_allclose(res.cycle, host, rtol=1e-12, atol=0.0)
    assert not res.cycle[:4, 0].any() and not res.cycle[9:, 0].any() and (res.cycle[4:9, 0] > 0).all()
    # a second run replays the graph: identical bits
    n_graphs = len(ed.graphs)
    again = ed.run(notes.cuda(), rows, SEED)
    assert len(ed.graphs) == n_graphs == 1
    for a, b in ((res.z, again.z), (res.recon, again.recon), (res.mu2, again.mu2), (res.cycle, again.cycle)):
        assert np.array_equal(bits(a), bits(b))
    # batch 9: the same z bits; its recon is compared through the reference only
    ed9 = ED.LatentEditor(cfg_of(T), "cuda", 9)
    ed9.eng.load_state(P, Bf)
    res9 = ed9.run(notes.cuda(), rows, SEED)
    assert np.array_equal(bits(res9.z), bits(res.z))
    np.testing.assert_allclose(res9.recon, vae_decode(P, Bf, torch.from_numpy(res9.z), T).numpy(), rtol=1e-3, atol=1e-5)
    other = ed.run(notes.cuda(), rows, SEED + 1)
    assert np.array_equal(bits(other.z[:4]), bits(res.z[:4])) and (other.z[4:9] != res.z[4:9]).mean() > 0.99


def test_editor_same_z_bits_at_another_batch():
    """z = mu + sigma * s * n depends on the batch only through the encoder's mu and logvar, which may round differently per batch
    size; with the encoded sources equal (prior rows have none) the chunking must not show at all."""
    T = 16
    P, Bf = vae_model(T)
    rows = LE.prior_rows(9, 0.8)
    out = []
    for B in (4, 9):
        ed = ED.LatentEditor(cfg_of(T), "cuda", B)
        ed.eng.load_state(P, Bf)
        out.append(ed.run(None, rows, SEED))
    assert np.array_equal(bits(out[0].z), bits(out[1].z)) and out[0].z.shape == (9, LAT)
    n = device_rows(table([dict(kind=1, sigma=1.0, key=tuple(k)) for k in rows.key.tolist()]), LAT)
    assert np.array_equal(out[0].z, (np.float64(np.float32(0.8)) * n.astype(np.float64)).astype(np.float32))


def test_editor_shift_requests_exactly_the_strength_asked_for():
    T = 16
    P, Bf = vae_model(T)
    notes = torch.rand(N_NOTES, T, 4, generator=torch.Generator().manual_seed(7)) * 2 - 1
    means = np.stack([np.linspace(-1.0, 1.0, LAT), np.linspace(0.5, -2.0, LAT)])        # two hand-placed class means
    diff = means[None, :, :] - means[:, None, :]
    strengths = [0.5, 1.0, 1.5]
    rows = LE.shift_rows([1, 4], [0, 0], 1, strengths, 2, n_split=N_NOTES)
    ed = ED.LatentEditor(cfg_of(T), "cuda", 4)
    ed.eng.load_state(P, Bf)
    res = ed.run(notes.cuda(), rows, SEED, centroids=diff)
    rep = LE.report(rows, res.cycle[:res.R])
    json.dumps(rep, allow_nan=False)
    print("max |mu|", float(np.abs(res.z[res.R:]).max()), "requested", [r["requested"] for r in rep["rows"]])
    for r, row in enumerate(rep["rows"]):
        assert abs(row["requested"] - strengths[r % 3]) <= 1e-6, (r, row["requested"])
        assert row["realised"] is not None and row["latent_step"] > 0
    d = diff[0, 1].astype(np.float32).astype(np.float64)
    for r in range(res.R):
        want = (res.z[res.R + rows.src_a[r]].astype(np.float64) + np.float64(rows.alpha[r]) * d).astype(np.float32)
        assert np.array_equal(bits(res.z[r]), bits(want))
    with pytest.raises(ED.AeEditError, match="centroids"):
        ed.run(notes.cuda(), rows, SEED)
    bad = diff.copy()
    bad[0, 1] = np.nan
    with pytest.raises(ED.AeEditError, match="no mean"):
        ed.run(notes.cuda(), rows, SEED, centroids=bad)
    with pytest.raises(ED.AeEditError, match="outside the split"):
        ed.run(notes[:3].cuda(), rows, SEED, centroids=diff)


@pytest.mark.parametrize("mode", ["notes", "latent"])
def test_editor_classifier_scores_against_its_own_logits(mode):
    from melo_gan_amd.emotion_discriminator.evaluate import EdEvaluator
    T = 32
    P, Bf = vae_model(T)
    notes = torch.rand(N_NOTES, T, 4, generator=torch.Generator().manual_seed(7)) * 2 - 1
    means = np.random.default_rng(0).standard_normal((4, LAT))
    rows = LE.shift_rows([0, 3, 5], [0, 1, 2], 3, [1.0, 2.0], 4, n_split=N_NOTES)
    ed_cfg = dict(O.default_ed_cfg(4), dropout=0.2, max_notes=T, batch_size=4, seed=3)
    if mode == "latent":
        ed_cfg.update(input_mode="latent", latent_dim=LAT)
    else:
        ed_cfg.update(input_mode="notes")
    cls = EdEvaluator(ed_cfg, "cuda", 4)
    cls.eng.init_weights(3)
    ed = ED.LatentEditor(cfg_of(T), "cuda", 4)
    ed.eng.load_state(P, Bf)
    res = ed.run(notes.cuda(), rows, SEED, centroids=means[None, :, :] - means[:, None, :], ed=cls)
    R = res.R

    def softmax_of(x):
        e, out = cls.eng, []
        for c0 in range(0, len(x), 4):
            e.x.zero_()
            chunk = torch.from_numpy(np.ascontiguousarray(x[c0:c0 + 4])).cuda()
            e.x[:len(chunk)].copy_(chunk.view((len(chunk),) + tuple(e.x.shape[1:])))
            e.forward(train=False)
            torch.cuda.synchronize()
            out.append(e.logits[:len(chunk)].double().cpu())
        return torch.softmax(torch.cat(out), 1).numpy()

    after = softmax_of(res.z if mode == "latent" else res.recon)
    want = {"after": after[:R], "before": after[R + rows.src_a]}
    if mode == "latent":
        want["cycled"] = softmax_of(res.mu2)[:R]
    assert set(res.scores) == set(want)
    for when, p in want.items():
        s = res.scores[when]
        np.testing.assert_allclose(s["p_target"], p[np.arange(R), rows.target], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(s["p_source"], p[np.arange(R), rows.source_label], rtol=1e-5, atol=1e-7)
        top2 = np.sort(p, axis=1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 1e-6
        assert np.array_equal(s["pred"][clear], np.argmax(p, axis=1)[clear])
    rep = LE.report(rows, res.cycle[:R], None, res.scores, ED.EMOTIONS)
    json.dumps(rep, allow_nan=False)
    assert all({"before", "after"} <= set(r) for r in rep["rows"]) and rep["summary"]["per_strength"][0]["became_target"] is not None
    wrong = dict(ed_cfg, max_notes=T + 8, latent_dim=LAT + 1)
    with pytest.raises(ED.AeEditError, match="classifier reads"):
        ed.run(notes.cuda(), rows, SEED, centroids=means[None, :, :] - means[:, None, :], ed=EdEvaluator(wrong, "cuda", 4))


# ---- the command end to end --------------------------------------------------------------------------------------------
def strict_json(path):
    def refuse(name):
        raise ValueError(f"{name} in {path}")
    return json.load(open(path), parse_constant=refuse)


@pytest.mark.parametrize("mode, argv, n_files", [
    ("prior", ["--prior", "4", "--temperature", "0.7"], 4),
    ("vary", ["--vary", "3,10", "--samples", "2", "--sigma", "0.5"], 4),
    ("path", ["--from", "2", "--to", "7", "--steps", "3", "--interp", "slerp", "--join"], 5),
    ("shift", ["--shift", "1,6", "--to", "calm", "--strength", "0.5,1"], 4),
])
def test_command_end_to_end(tmp_path, mode, argv, n_files):
    cfg = tmp_path / "ae.yaml"
    cfg.write_text(f"MAX_NOTES: 16\nLATENT_DIM: {LAT}\nBATCH_SIZE: 4\nLOG_DIR: {tmp_path / 'log'}\n")
    out = tmp_path / "out"
    base = ["--config", str(cfg), "--synthetic", "12", "--batch", "4", "--seed", "3"]
    assert ED.main(base + argv + ["--out", str(out)]) == 0
    rep = strict_json(out / "edit.json")
    assert rep["mode"] == mode and len(rep["files"]) == n_files and rep["summary"]["rows"] == len(rep["rows"])
    assert sorted(os.listdir(out)) == sorted([f["file"] for f in rep["files"]] + ["edit.json"])
    for f in rep["files"]:
        hdr, tempo, parsed = midi.read_smf_notes(str(out / f["file"]))
        assert hdr[0] == 1 and tempo > 0 and isinstance(parsed, list)
    for row in rep["rows"]:
        assert row["file"] in os.listdir(out) and row["cycle_error"] is not None and row["latent_step"] is not None
        assert ("notes" in row and row["notes"] is not None) == (mode != "prior")
    if mode == "shift":
        assert rep["files"][0]["scale"] == "major" and rep["files"][0]["bpm"] == 90.0         # generate.STYLE["calm"]
        assert [b["strength"] for b in rep["summary"]["per_strength"]] == [0.5, 1.0] and rep["centroids"]["counts"]["calm"] == 3
        for row in rep["rows"]:
            assert abs(row["requested"] - row["alpha"]) <= 1e-6 and row["target"] == "calm"
    if mode == "path":
        assert rep["rows"][0]["latent_step"] == 0.0 and rep["rows"][0]["notes"]["onset_changed"] == 0.0
        assert rep["files"][-1] == {"file": "path_r2_r7.mid", "joined": True, "join_notes": 16}
    # --no-files writes the report alone, with the same numbers
    bare = tmp_path / "bare"
    assert ED.main(base + [a for a in argv if a != "--join"] + ["--out", str(bare), "--no-files"]) == 0
    assert os.listdir(bare) == ["edit.json"]
    rep2 = strict_json(bare / "edit.json")
    assert rep2["files"] == [] and rep2["summary"] == rep["summary"]
    if mode == "vary":                  # a bad ROWS index
        assert ED.main(base + ["--vary", "3,12", "--samples", "2", "--out", str(tmp_path / "bad")]) == 2
        assert not os.path.exists(tmp_path / "bad")


def test_command_with_a_classifier_and_wav(tmp_path):
    import yaml
    from melo_gan_amd.emotion_discriminator.evaluate import EdEvaluator
    cfg = tmp_path / "ae.yaml"
    cfg.write_text(f"MAX_NOTES: 16\nLATENT_DIM: {LAT}\nBATCH_SIZE: 4\nLOG_DIR: {tmp_path / 'log'}\n")
    ed_cfg = dict(O.default_ed_cfg(4), input_mode="latent", latent_dim=LAT, dropout=0.2, batch_size=4, seed=3)
    (tmp_path / "ed.yaml").write_text(yaml.safe_dump(ed_cfg))
    cls = EdEvaluator(ed_cfg, "cuda", 4)
    cls.eng.init_weights(3)
    torch.save({"model": {k: v.cpu() for k, v in cls.eng.state_dict().items()}}, str(tmp_path / "ed_best.pth"))
    out = tmp_path / "out"
    argv = ["--config", str(cfg), "--synthetic", "12", "--batch", "4", "--shift", "0,5", "--to", "sad", "--strength", "1", "--out", str(out),
            "--ed_config", str(tmp_path / "ed.yaml"), "--ed_ckpt", str(tmp_path / "ed_best.pth"), "--wav", "--wav-fs", "8000"]
    assert ED.main(argv) == 0
    rep = strict_json(out / "edit.json")
    assert rep["classifier_input"] == "latent" and rep["wav"]["fs"] == 8000 and len(rep["files"]) == 2
    for f in rep["files"]:
        assert os.path.getsize(out / f["wav"]) > 44 and f["seconds"] > 0 and os.path.isfile(out / f["file"])
    for row in rep["rows"]:
        assert {"before", "after", "cycled"} <= set(row) and 0.0 <= row["after"]["p_target"] <= 1.0
        assert row["after"]["prediction"] in ED.EMOTIONS and row["target"] == "sad"
    blk = rep["summary"]["per_strength"][0]
    assert blk["strength"] == 1.0 and blk["rows"] == 2 and blk["became_target"] in (0.0, 0.5, 1.0)
    # a classifier that does not fit the VAE is refused
    (tmp_path / "ed9.yaml").write_text(yaml.safe_dump(dict(ed_cfg, latent_dim=LAT + 1)))
    assert ED.main(argv[:argv.index("--ed_config")] + ["--ed_config", str(tmp_path / "ed9.yaml"), "--ed_ckpt", str(tmp_path / "ed_best.pth")]) == 2


# ---- a real checkpoint file through the VAE's three loaders -------------------------------------------------------------
def test_one_checkpoint_file_loads_alike_through_editor_evaluator_and_encode(tmp_path):
    """MAX_NOTES 16, LATENT_DIM 8, batch 2: the smallest VAE the engine takes with two samples in a BatchNorm batch.  One
    file written from VaeEngine.state_dict(); parameters and buffers bit for bit behind each loader."""
    from melo_gan_amd.ae import encode
    from melo_gan_amd.ae.engine import VaeEngine
    from melo_gan_amd.ae.evaluate import VaeEvaluator
    cfg = dict(MAX_NOTES=16, LATENT_DIM=8, BATCH_SIZE=2)
    src = VaeEngine(cfg, "cuda", 2)
    src.init_weights(5)
    for i, v in enumerate(src.buf.values()):
        v.add_(0.125 * (i + 1))
    src.num_batches_tracked = 4
    want = src.state_dict()
    assert all(int(v) == 4 for k, v in want.items() if k.endswith("num_batches_tracked"))
    ckpt = str(tmp_path / "ae_best.pth")
    torch.save({"epoch": 1, "model_state": want}, ckpt)
    editor, evaluator, plain = ED.LatentEditor(cfg, "cuda", 2), VaeEvaluator(cfg, "cuda", 2), VaeEngine(cfg, "cuda", 2)
    editor.load(ckpt)
    evaluator.load(ckpt)
    encode.load_model(plain, ckpt)
    for name, eng in (("edit", editor.eng), ("evaluate", evaluator.eng), ("encode", plain)):
        for k in src.P.spec:
            assert torch.equal(eng.P.p[k].cpu(), want[k]), (name, k)
        for k in src.buf:
            assert torch.equal(eng.buf[k].cpu(), want[k]), (name, k)
