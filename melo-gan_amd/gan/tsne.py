#!/usr/bin/env python3
"""Exact t-SNE of VAE latents (or any feature set) on the device -- "is your VAE clustering emotions?", the question of the
reference's tsne.py, which hands (N, D) encoder features and a split's `emotion` column to scikit-learn and matplotlib:

    python -m melo_gan_amd.gan.tsne --config config/gan_config.yaml [--split train|val|PATH.csv] [--feats PATH] \
        [--perplexity 30] [--iters 1000] [--init pca|random] [--seed 42] [--out DIR]

writes DIR/<split>_tsne.npy (the (N, 2) embedding), DIR/<split>_tsne.svg (a scatter plot, one colour per emotion, a legend of
the classes present) and DIR/<split>_tsne.json (N, D, the parameters, the final KL and the KL trace).

`Tsne` is scikit-learn's TSNE(method="exact") with its defaults -- perplexity 30, 1000 iterations, early exaggeration 12 over
the first 250, learning rate max(N / 12 / 4, 50), momentum 0.5 then 0.8, gains, PCA initialisation of standard deviation 1e-4 --
under two decisions: the iteration count is fixed (no early stop: a run is reproducible and the host never reads back
mid-run) and, as in scikit-learn, the embedding is not recentred.  The affinities (mg_tsne_affinities) and every iteration
(mg_tsne_step: two launches) run on the device; the iterations are captured into one hipGraph of `trace_every` iterations
per phase and replayed, the last iteration of each replay leaving KL and |grad| in a device trace that the host reads once,
at the end.  The PCA of the initialisation runs on the host in numpy fp64, on the (N, D) array.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
from pathlib import Path
from xml.sax.saxutils import escape

import numpy as np

from ..pieces import require_device

EMOTIONS = ("happy", "sad", "angry", "calm")        # gan/utils.py emotion_to_index; anything else is "other"
OTHER = "other"
COLOURS = {"happy": "#e6a817", "sad": "#3b6fb6", "angry": "#c0392b", "calm": "#2e9e6b", OTHER: "#7f7f7f"}
LABEL_COL, FILE_COL = "emotion", "npz_path"
MIN_ROWS, MAX_ROWS = 4, 16384


class TsneError(ValueError):
    """A bad input, found on the host before any GPU use."""


# ---------------------------------------------------------------------------------------------------------------------
# host pieces (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def emotion_name(label) -> str:
    """A CSV label through the project's emotion map (case and blanks ignored, as the reference script); else "other"."""
    s = str(label).lower().strip()
    return s if s in EMOTIONS else OTHER


def load_latents(csv_path: str, feats_path: str):
    """The (N, D) fp32 features of a split and their emotion names, aligned by the reference's rules (tsne.py:22-123):
    a row-aligned (N, D) array is matched by row order and the longer of CSV and array is truncated; an object array holding a
    {npz_path or its basename: vector} map is matched by key and CSV rows without a key are dropped."""
    if not os.path.isfile(csv_path):
        raise TsneError(f"split CSV {csv_path} does not exist")
    if not os.path.isfile(feats_path):
        raise TsneError(f"features {feats_path} do not exist")
    with open(csv_path, newline="") as f:
        rows = list(csv.DictReader(f))
    if rows and LABEL_COL not in rows[0]:
        raise TsneError(f"{csv_path}: no {LABEL_COL!r} column")
    try:
        data = np.load(feats_path, allow_pickle=True)
    except Exception as e:      # noqa: BLE001 -- any unreadable file is the same user error
        raise TsneError(f"cannot read features {feats_path}: {e}") from e
    if data.dtype == np.object_:
        if rows and FILE_COL not in rows[0]:
            raise TsneError(f"{csv_path}: no {FILE_COL!r} column to match a feature map by")
        try:
            table = dict(data.tolist())
        except Exception as e:      # noqa: BLE001
            raise TsneError(f"{feats_path}: an object array that is not a key -> vector map: {e}") from e
        vecs, labels = [], []
        for r in rows:
            key = r.get(FILE_COL)
            if key is None or key == "":
                continue
            v = table.get(str(key))
            if v is None:
                v = table.get(os.path.basename(str(key)))
            if v is None:
                continue
            vecs.append(np.asarray(v, dtype=np.float32).reshape(-1))
            labels.append(emotion_name(r[LABEL_COL]))
        if not vecs:
            raise TsneError(f"no key of {feats_path} matches a {FILE_COL} of {csv_path}")
        if len({v.shape for v in vecs}) != 1:
            raise TsneError(f"{feats_path}: the map's vectors differ in length")
        X = np.stack(vecs)
    else:
        X = np.asarray(data, dtype=np.float32)
        if X.ndim < 2:
            raise TsneError(f"{feats_path}: features of shape {X.shape}, (N, D) expected")
        X = X.reshape(X.shape[0], -1)
        n = min(len(rows), X.shape[0])
        X, labels = X[:n], [emotion_name(r[LABEL_COL]) for r in rows[:n]]
    if len(labels) == 0:
        raise TsneError(f"{csv_path} and {feats_path} share no row")
    return np.ascontiguousarray(X, dtype=np.float32), labels


def pca_init(X) -> np.ndarray:
    """scikit-learn's init="pca" in numpy fp64: the first two principal components (each component's sign such that its
    largest-|.| loading is positive), scaled so that the first has standard deviation 1e-4."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(0)
    U, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    sign = np.sign(Vt[np.arange(Vt.shape[0]), np.abs(Vt).argmax(1)])
    sign[sign == 0] = 1.0
    Y = (U * S * sign)[:, :2]
    if Y.shape[1] < 2:          # D == 1
        Y = np.concatenate([Y, np.zeros((Y.shape[0], 2 - Y.shape[1]))], 1)
    sd = np.std(Y[:, 0])
    if not sd > 0:
        raise TsneError("init='pca': the rows are all equal")
    return Y / sd * 1e-4


MARKERS = ("circle", "cross")


def _marker(kind: str, x: float, y: float, colour: str) -> str:
    if kind == "cross":
        return (f'<path class="pt" d="M{x - 3:.2f} {y - 3:.2f}L{x + 3:.2f} {y + 3:.2f}M{x - 3:.2f} {y + 3:.2f}L{x + 3:.2f} {y - 3:.2f}" '
                f'stroke="{colour}" stroke-width="1.4" fill="none"/>')
    return f'<circle class="pt" cx="{x:.2f}" cy="{y:.2f}" r="3" fill="{colour}" fill-opacity="0.75"/>'


def write_svg(path: str, Y, labels, title: str = "t-SNE", groups=None, group_names=("real", "generated")) -> None:
    """A scatter plot of Y (N, 2) as a standalone SVG: one colour per emotion name in `labels`, a legend of the classes that
    occur; groups (N ints in {0, 1}, optional) chooses the marker shape (circle / cross) and adds the shapes to the legend."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[1] != 2 or len(labels) != Y.shape[0]:
        raise TsneError(f"write_svg: Y {Y.shape} and {len(labels)} labels")
    if not np.isfinite(Y).all():
        raise TsneError("write_svg: the embedding is not finite")
    W, H, pad, legend_w = 900.0, 640.0, 40.0, 130.0
    lo, hi = Y.min(0), Y.max(0)
    span = np.where(hi > lo, hi - lo, 1.0)
    px = pad + (Y[:, 0] - lo[0]) / span[0] * (W - 2 * pad - legend_w)
    py = H - pad - (Y[:, 1] - lo[1]) / span[1] * (H - 2 * pad - 20)
    groups = np.zeros(len(labels), dtype=int) if groups is None else np.asarray(groups, dtype=int)
    out = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{W:.0f}" height="{H:.0f}" viewBox="0 0 {W:.0f} {H:.0f}">',
           f'<rect width="{W:.0f}" height="{H:.0f}" fill="#ffffff"/>',
           f'<text x="{pad:.0f}" y="24" font-family="sans-serif" font-size="16">{escape(title)}</text>', '<g id="points">']
    for x, y, name, g in zip(px, py, labels, groups):
        out.append(_marker(MARKERS[int(g) % 2], x, y, COLOURS.get(name, COLOURS[OTHER])))
    out.append('</g>')
    out.append('<g id="legend" font-family="sans-serif" font-size="13">')
    lx, ly = W - legend_w, pad + 10
    for name in [e for e in EMOTIONS + (OTHER,) if e in set(labels)]:
        out.append(f'<g class="legend-class">{_marker("circle", lx, ly, COLOURS[name])}'
                   f'<text x="{lx + 10:.0f}" y="{ly + 4:.0f}">{escape(name)}</text></g>')
        ly += 20
    if len(set(groups.tolist())) > 1 or groups.any():
        ly += 8
        for g in sorted(set(groups.tolist())):
            out.append(f'<g class="legend-group">{_marker(MARKERS[g % 2], lx, ly, "#333333")}'
                       f'<text x="{lx + 10:.0f}" y="{ly + 4:.0f}">{escape(group_names[g % 2])}</text></g>')
            ly += 20
    out.append('</g></svg>')
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


# ---------------------------------------------------------------------------------------------------------------------
# the embedding
# ---------------------------------------------------------------------------------------------------------------------
class Tsne:
    """Exact t-SNE on the device with scikit-learn's defaults; fit_transform(X) -> (N, 2) numpy fp32.  After a fit:
    kl_trace / grad_trace (KL and |grad|_2 at iterations trace_iters, i.e. every trace_every-th and the last), kl_ (the last
    iteration's KL, of the plain P), lr_ and n_iter_.  X may be a numpy array or a device tensor; `embed` is the same on a
    device tensor without the final device -> host copy of Y."""

    def __init__(self, perplexity: float = 30.0, iters: int = 1000, exaggeration: float = 12.0, exaggeration_iters: int = 250,
                 lr="auto", init="pca", seed: int = 42, trace_every: int = 50, graphs: bool = True):
        if int(iters) < 1 or int(exaggeration_iters) < 0 or int(trace_every) < 1:
            raise TsneError("Tsne: iters >= 1, exaggeration_iters >= 0 and trace_every >= 1 expected")
        if not float(exaggeration) > 0 or not float(perplexity) >= 1:
            raise TsneError("Tsne: exaggeration > 0 and perplexity >= 1 expected")
        if not (lr == "auto" or float(lr) > 0):
            raise TsneError(f"Tsne: lr = {lr!r}: 'auto' or a positive number")
        if isinstance(init, str) and init not in ("pca", "random"):
            raise TsneError(f"Tsne: init = {init!r}: 'pca', 'random' or an (N, 2) array")
        self.perplexity, self.iters, self.exaggeration = float(perplexity), int(iters), float(exaggeration)
        self.exaggeration_iters, self.lr, self.init, self.seed = min(int(exaggeration_iters), int(iters)), lr, init, int(seed)
        self.trace_every, self.graphs = int(trace_every), bool(graphs)
        self.kl_trace = self.grad_trace = self.trace_iters = self.kl_ = self.lr_ = self.n_iter_ = None

    def check(self, n: int, d: int):
        if not MIN_ROWS <= n <= MAX_ROWS:
            raise TsneError(f"Tsne: {n} rows: {MIN_ROWS}..{MAX_ROWS} (the affinity matrix is dense)")
        if d < 1:
            raise TsneError("Tsne: the rows hold no feature")
        if not self.perplexity < n - 1:
            raise TsneError(f"Tsne: perplexity {self.perplexity} needs more than {int(self.perplexity) + 1} rows, got {n}")
        if not isinstance(self.init, str) and tuple(np.shape(self.init)) != (n, 2):
            raise TsneError(f"Tsne: init of shape {tuple(np.shape(self.init))}, ({n}, 2) expected")

    def trace_schedule(self):
        """The iterations that leave a trace record: every trace_every-th and the last."""
        its = [it for it in range(self.iters) if (it + 1) % self.trace_every == 0]
        if not its or its[-1] != self.iters - 1:
            its.append(self.iters - 1)
        return its

    def _initial(self, X, n, dev):
        import torch
        from .. import ops
        if isinstance(self.init, str) and self.init == "random":      # N(0, 1e-4^2) keyed by (seed, row)
            Y = torch.empty(n, 2, device=dev)
            zero = torch.zeros(1, dtype=torch.int64, device=dev)
            ops.eval_noise(Y, zero, zero, n, self.seed)
            return Y.mul_(1e-4)
        if isinstance(self.init, str):
            Y0 = pca_init(X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else X)
        else:
            Y0 = np.asarray(self.init, dtype=np.float64)
            if not np.isfinite(Y0).all():
                raise TsneError("Tsne: init is not finite")
        return torch.from_numpy(np.ascontiguousarray(Y0, dtype=np.float32)).to(dev)

    def embed(self, X):
        """X (N, D): numpy or a device fp32 tensor -> the embedding as a device tensor (N, 2)."""
        import torch
        from .. import ops
        if isinstance(X, torch.Tensor):
            if X.dim() != 2:
                raise TsneError(f"Tsne: X of shape {tuple(X.shape)}, (N, D) expected")
            self.check(X.shape[0], X.shape[1])
            if not X.is_cuda:
                raise TsneError("Tsne: a tensor X must be on the device")
            Xd = X.detach().to(torch.float32).contiguous()
        else:
            Xh = np.asarray(X, dtype=np.float32)
            if Xh.ndim != 2:
                raise TsneError(f"Tsne: X of shape {Xh.shape}, (N, D) expected")
            self.check(Xh.shape[0], Xh.shape[1])
            if not np.isfinite(Xh).all():
                raise TsneError("Tsne: X is not finite")
            require_device()
            Xd = torch.from_numpy(np.ascontiguousarray(Xh)).cuda()
        n, dev = Xd.shape[0], Xd.device
        lr = max(n / self.exaggeration / 4.0, 50.0) if self.lr == "auto" else float(self.lr)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            Y = self._initial(X, n, dev)
            work = ops.tsne_workspace(n, dev)
            P = ops.tsne_affinities(Xd, self.perplexity, work=work)
            update, gains = torch.zeros(n, 2, device=dev), torch.ones(n, 2, device=dev)
            sched = self.trace_schedule()
            trace = torch.zeros(len(sched), 4, dtype=torch.float64, device=dev)
            cursor = torch.zeros(1, dtype=torch.int64, device=dev)
            te, graphs = self.trace_every, {}

            def one(it, traced):
                ee, mom = (self.exaggeration, 0.5) if it < self.exaggeration_iters else (1.0, 0.8)
                ops.tsne_step(P, Y, update, gains, ee, mom, lr, trace=trace if traced else None,
                              cursor=cursor if traced else None, work=work)

            def block(it0):
                for k in range(te):
                    one(it0 + k, k == te - 1)

            it = 0
            while it < self.iters:
                if it == self.exaggeration_iters and it > 0:      # scikit-learn runs _gradient_descent once per phase
                    update.zero_()
                    gains.fill_(1.0)
                phase = it < self.exaggeration_iters
                end = self.exaggeration_iters if phase else self.iters
                if self.graphs and it % te == 0 and it + te <= end and te > 1:      # a whole block inside one phase: replay
                    g = graphs.get(phase)
                    if g is None:                   # te iterations of this phase, the last one traced; capturing runs nothing
                        g = graphs[phase] = ops.Graph.capture(lambda: block(it), execs=1)
                    g.launch()
                    it += te
                else:
                    one(it, it in sched)
                    it += 1
            host = trace.cpu()              # the run's only device -> host read
            for g in graphs.values():
                g.release()
        torch.cuda.current_stream(dev).wait_stream(stream)
        rec = host.numpy()
        self.trace_iters = list(sched)
        self.kl_trace, self.grad_trace = rec[:, 0].copy(), rec[:, 1].copy()
        self.kl_, self.lr_, self.n_iter_ = float(rec[-1, 0]), lr, self.iters
        return Y

    def fit_transform(self, X) -> np.ndarray:
        return self.embed(X).cpu().numpy()

    def params(self) -> dict:
        return {"perplexity": self.perplexity, "iters": self.iters, "exaggeration": self.exaggeration,
                "exaggeration_iters": self.exaggeration_iters, "lr": self.lr_ if self.lr_ is not None else self.lr,
                "init": self.init if isinstance(self.init, str) else "array", "seed": self.seed, "trace_every": self.trace_every}


# ---------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m melo_gan_amd.gan.tsne",
                                 description="Exact t-SNE of a split's encoder features, coloured by emotion.")
    ap.add_argument("--config", type=str, default="config/gan_config.yaml", help="Path to the main GAN config")
    ap.add_argument("--split", type=str, default="val", help="train, val or the path of a split CSV")
    ap.add_argument("--feats", type=str, default=None, help="encoder features of the split (default ENCODER_FEATS_TRAIN / _VAL)")
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--init", type=str, default="pca", choices=("pca", "random"))
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", type=str, default=None, help="output directory (default LOG_DIR)")
    return ap.parse_args(argv)


def plan(args):
    """Every check of what comes from outside, on the host; returns (X, labels, stem, out dir, Tsne)."""
    from . import config as C
    if not os.path.isfile(args.config):
        raise TsneError(f"config {args.config} does not exist")
    cfg = C.load_config(args.config)
    if not isinstance(cfg, dict):
        raise TsneError(f"config {args.config} is not a YAML mapping")
    keys = {"train": ("TRAIN_SPLIT", "ENCODER_FEATS_TRAIN"), "val": ("VAL_SPLIT", "ENCODER_FEATS_VAL")}
    if args.split in keys:
        ck, fk = keys[args.split]
        split_csv, feats, stem = cfg.get(ck), args.feats or cfg.get(fk), args.split
        if not split_csv:
            raise TsneError(f"config {args.config} lacks {ck}")
    else:
        split_csv, feats, stem = args.split, args.feats, Path(args.split).stem
    if not feats:
        raise TsneError("no features: give --feats (the config names them only for --split train / val)")
    X, labels = load_latents(split_csv, feats)
    if not np.isfinite(X).all():
        raise TsneError(f"{feats}: the features are not finite")
    try:
        ts = Tsne(perplexity=args.perplexity, iters=args.iters, init=args.init, seed=args.seed)
        ts.check(*X.shape)
    except TsneError as e:
        raise TsneError(f"{e} ({split_csv}, {feats})") from e
    out = args.out or cfg.get("LOG_DIR", "experiments/gan/logs")
    return X, labels, stem, out, ts


def main(argv=None) -> int:
    args = parse_args(argv)
    try:
        X, labels, stem, out, ts = plan(args)
    except TsneError as e:
        print(f"tsne: error: {e}", file=sys.stderr)
        return 2
    Y = ts.fit_transform(X)
    os.makedirs(out, exist_ok=True)
    base = os.path.join(out, f"{stem}_tsne")
    np.save(base + ".npy", Y)
    write_svg(base + ".svg", Y, labels, title=f"t-SNE of the {stem} latents ({X.shape[0]} x {X.shape[1]})")
    with open(base + ".json", "w") as f:
        json.dump({"n": int(X.shape[0]), "d": int(X.shape[1]), "params": ts.params(), "kl": ts.kl_,
                   "trace_iters": ts.trace_iters, "kl_trace": ts.kl_trace.tolist(), "grad_trace": ts.grad_trace.tolist(),
                   "classes": {c: labels.count(c) for c in EMOTIONS + (OTHER,) if c in labels}}, f, indent=1)
    print(f"t-SNE of {X.shape[0]} rows x {X.shape[1]}: KL {ts.kl_:.4f} after {ts.iters} iterations")
    print(f"wrote {base}.npy, .svg, .json")
    return 0


if __name__ == "__main__":
    sys.exit(main())
