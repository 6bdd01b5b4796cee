"""Writes tests/golden/tsne_blobs192.npz from tests/tsne_ref.py (numpy only, fp64; about half a minute):

    python tests/golden/make_golden_tsne.py

The fixture is tsne_ref.blobs(48, 64, seed 0): four Gaussian blobs of 48 rows, D = 64, the shape of the validation split, embedded
with the defaults (perplexity 30, 1000 iterations, PCA initialisation rounded to fp32 as the device receives it).
  state_its, state_Y, state_update, state_gains   the state BEFORE iterations 0, 1, 100, 251 and 600 of that run (the
                                                  teacher-forced single-step test starts the device from each)
  kls, kl_lo, kl_hi                               the final KL of five runs whose Y0 is the fixture's moved by one fp32 ulp per
                                                  component, up or down at random (seeds 0..4), and their min and max: how far
                                                  a perturbation the size of fp32 rounding moves the end of a 1000-iteration run
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tsne_ref as R  # noqa: E402

N_PER, D, SEED, PERPLEXITY, ITERS = 48, 64, 0, 30.0, 1000
STATE_ITS = (0, 1, 100, 251, 600)


def fixture():
    X, labels = R.blobs(N_PER, D, SEED)
    P, _ = R.affinities(X, PERPLEXITY)
    Y0 = R.pca_init(X).astype(np.float32)
    return X, labels, P, Y0


def perturbed(Y0, k):
    up = np.random.default_rng(k).integers(0, 2, Y0.shape).astype(bool)
    return np.where(up, np.nextafter(Y0, np.float32(np.inf)), np.nextafter(Y0, np.float32(-np.inf))).astype(np.float32)


def main():
    X, labels, P, Y0 = fixture()
    Y, r, states = R.run(P, Y0.astype(np.float64), ITERS, keep=STATE_ITS)
    print("unperturbed: KL", r["kl"], "purity", R.knn_purity(Y, labels))
    kls = []
    for k in range(5):
        Yk, rk, _ = R.run(P, perturbed(Y0, k).astype(np.float64), ITERS)
        kls.append(rk["kl"])
        print("perturbation", k, "KL", rk["kl"], "purity", R.knn_purity(Yk, labels))
    out = os.path.join(HERE, "tsne_blobs192.npz")
    np.savez(out, state_its=np.array(STATE_ITS), state_Y=np.stack([states[i][0] for i in STATE_ITS]),
             state_update=np.stack([states[i][1] for i in STATE_ITS]), state_gains=np.stack([states[i][2] for i in STATE_ITS]),
             kls=np.array(kls), kl_lo=min(kls), kl_hi=max(kls), kl_unperturbed=r["kl"])
    print("wrote", out, "lo", min(kls), "hi", max(kls))


if __name__ == "__main__":
    main()
