"""numpy-only restatement of the exact t-SNE that csrc/tsne.hip and melo_gan_amd/gan/tsne.py compute, in fp64, with a float32
mode of the same code (dtype=np.float32: every array and every operation in float32) whose deviation from the fp64 mode is the
tests' yardstick for what fp32 rounding alone costs.

    affinities(X, perplexity)         -> P (N, N), beta (N)
    step(P, Y, update, gains, ...)    -> one iteration of scikit-learn's _gradient_descent: new state, grad, Z, KL
    run(P, Y0, iters, ...)            -> the fixed-length schedule: exaggeration and momentum 0.5 for the first
                                         `exaggeration_iters` iterations, then plain P and momentum 0.8 with update and gains
                                         reset (scikit-learn calls _gradient_descent once per phase); no early stop, no recentring
"""
import numpy as np

MAX_DOUBLINGS, BISECTIONS = 100, 64


def sq_dists(X, dtype=np.float64):
    X = np.asarray(X, dtype=dtype)
    n = (X * X).sum(1)
    d = np.maximum(n[:, None] + n[None, :] - dtype(2) * (X @ X.T), dtype(0))
    np.fill_diagonal(d, 0)
    return d


def _entropy(d, off, beta):
    """Row entropies of p_j|i ~ exp(-beta_i d_ij), j != i; also the rows' sums."""
    p = np.exp(-beta[:, None] * d)
    p[~off] = 0
    s0 = p.sum(1)
    s1 = (d * p).sum(1)
    return np.log(s0) + beta * s1 / s0, p, s0


def conditional(d2, perplexity, dtype=np.float64):
    """P_cond (rows sum to 1, zero diagonal) and beta: bracket by doubling from 1, then bisect BISECTIONS steps."""
    d2 = np.asarray(d2, dtype=dtype)
    N = d2.shape[0]
    off = ~np.eye(N, dtype=bool)
    d = d2 - np.where(off, d2, np.inf).min(1)[:, None]
    d[~off] = 0
    target = dtype(np.log(np.float64(perplexity)))
    lo, hi = np.zeros(N, dtype), np.ones(N, dtype)
    active = np.ones(N, bool)
    for _ in range(MAX_DOUBLINGS):
        H, _, _ = _entropy(d, off, hi)
        active &= H > target
        if not active.any():
            break
        lo = np.where(active, hi, lo)
        hi = np.where(active, hi * dtype(2), hi)
    for _ in range(BISECTIONS):
        mid = dtype(0.5) * (lo + hi)
        H, _, _ = _entropy(d, off, mid)
        up = H > target
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    beta = dtype(0.5) * (lo + hi)
    _, p, s0 = _entropy(d, off, beta)
    return p / s0[:, None], beta


def affinities(X, perplexity, dtype=np.float64):
    C, beta = conditional(sq_dists(X, dtype), perplexity, dtype)
    return (C + C.T) / dtype(2 * C.shape[0]), beta


def row_entropy(C):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(C > 0, C * np.log(C), 0).sum(1)


def forces(P, Y, exaggeration=1.0, dtype=np.float64):
    """grad = 4 (ee attr - rep / Z), Z, and KL = sum p log p - sum p log w + log Z of the plain P."""
    P, Y = np.asarray(P, dtype), np.asarray(Y, dtype)
    diff = Y[:, None, :] - Y[None, :, :]
    w = dtype(1) / (dtype(1) + (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]))
    np.fill_diagonal(w, 0)
    Z = w.sum()
    attr = ((P * w)[:, :, None] * diff).sum(1)
    rep = ((w * w)[:, :, None] * diff).sum(1)
    grad = dtype(4) * (dtype(exaggeration) * attr - rep / Z)
    m = P > 0
    kl = (P[m] * (np.log(P[m]) - np.log(w[m]))).sum() + np.log(Z)
    return grad, Z, kl


def step(P, Y, update, gains, exaggeration, momentum, lr, dtype=np.float64):
    Y, update, gains = (np.asarray(a, dtype) for a in (Y, update, gains))
    grad, Z, kl = forces(P, Y, exaggeration, dtype)
    inc = update * grad < 0
    gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
    update = dtype(momentum) * update - dtype(lr) * gains * grad
    return {"Y": Y + update, "update": update, "gains": gains, "grad": grad, "Z": Z, "kl": kl,
            "grad_norm": np.sqrt((grad.astype(np.float64) ** 2).sum())}


def auto_lr(N, exaggeration=12.0):
    return max(N / exaggeration / 4.0, 50.0)


def schedule(it, exaggeration=12.0, exaggeration_iters=250):
    """(exaggeration, momentum) of iteration `it`."""
    return (exaggeration, 0.5) if it < exaggeration_iters else (1.0, 0.8)


def run(P, Y0, iters, exaggeration=12.0, exaggeration_iters=250, lr=None, dtype=np.float64, keep=(), watch=None):
    """The whole descent.  keep: iterations whose state BEFORE the step is recorded as (Y, update, gains); watch(it, result):
    called after every step.  Returns (Y, last step's result, {it: state})."""
    N = P.shape[0]
    lr = auto_lr(N, exaggeration) if lr is None else lr
    Y = np.asarray(Y0, dtype).copy()
    update, gains = np.zeros_like(Y), np.ones_like(Y)
    states, r = {}, None
    for it in range(iters):
        if it == exaggeration_iters:
            update, gains = np.zeros_like(Y), np.ones_like(Y)
        if it in keep:
            states[it] = (Y.copy(), update.copy(), gains.copy())
        ee, mom = schedule(it, exaggeration, exaggeration_iters)
        r = step(P, Y, update, gains, ee, mom, lr, dtype)
        Y, update, gains = r["Y"], r["update"], r["gains"]
        if watch is not None:
            watch(it, r)
    return Y, r, states


def pca_init(X):
    """scikit-learn's init="pca": the first two principal components (signs fixed so that each component's largest-|.|
    loading is positive), scaled so that the first has standard deviation 1e-4."""
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(0)
    U, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    sign = np.sign(Vt[np.arange(Vt.shape[0]), np.abs(Vt).argmax(1)])
    sign[sign == 0] = 1
    Y = (U * S * sign)[:, :2]
    if Y.shape[1] < 2:
        Y = np.concatenate([Y, np.zeros((Y.shape[0], 2 - Y.shape[1]))], 1)
    return Y / np.std(Y[:, 0]) * 1e-4


def blobs(n_per, D, seed, k=4, spread=1.5):
    """k Gaussian blobs of n_per rows each: unit covariance, centres drawn from N(0, spread^2 I).  Returns X (fp32), labels."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, D)) * spread
    X = np.concatenate([c + rng.standard_normal((n_per, D)) for c in centres])
    return X.astype(np.float32), np.repeat(np.arange(k), n_per)


def knn_purity(Y, labels, k=5):
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, 1)[:, :k]
    return float((labels[nn] == labels[:, None]).mean())
