"""CPU: the morpher's host side (melo_gan_amd.gan.morph, gan.morph_metrics) -- the report's arithmetic on planted curves and
paths, the argument checks of the three new entry points and of their wrappers, the command's host checks, and the offsets of
a joined piece against a sum made by hand."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import melo_gan_amd  # noqa: F401
from melo_gan_amd.gan import morph as M
from melo_gan_amd.gan import morph_metrics as MM

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_morph_metrics_imports_no_gpu_code():
    import ast
    tree = ast.parse(open(os.path.join(ROOT, "melo-gan_amd", "gan", "morph_metrics.py")).read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add("." * node.level + (node.module or ""))
    assert mods <= {"__future__", "dataclasses", "typing", "numpy"}, mods


def test_crossover_on_planted_curves():
    w = [0.0, 0.25, 0.5, 0.75, 1.0]
    p_from = [0.7 - 0.5 * x for x in w]
    p_to = [0.3 + 0.5 * x for x in w]              # the difference is x - 0.4: zero at 0.4, between steps 1 and 2
    assert abs(MM.crossover(w, p_from, p_to) - 0.4) <= 1e-12
    assert MM.crossover(w, [0.2] * 5, [0.2, 0.1, 0.1, 0.1, 0.1]) == 0.0            # already equal at step 0
    assert MM.crossover(w, [0.1] * 5, [0.5] * 5) == 0.0
    assert MM.crossover(w, [0.6] * 5, [0.1, 0.2, 0.3, 0.4, 0.5]) is None           # never crosses
    # a crossing exactly at a step: the interpolation lands on it
    assert abs(MM.crossover(w, [0.5] * 5, [0.0, 0.25, 0.5, 0.75, 1.0]) - 0.5) <= 1e-12


def planted_probs():
    """Two paths of five steps over four classes, from class 1 to class 0: path 0 rises monotonically and switches, path 1
    dips at step 2 and ends undecided for class 2."""
    p_to = np.array([[0.1, 0.3, 0.5, 0.7, 0.9], [0.1, 0.4, 0.3, 0.35, 0.4]])
    probs = np.zeros((2, 5, 4))
    probs[:, :, 0] = p_to
    probs[0, :, 1] = 1.0 - p_to[0]
    probs[1, :, 1] = [0.9, 0.6, 0.5, 0.2, 0.1]
    probs[1, :, 2] = 1.0 - probs[1, :, 0] - probs[1, :, 1]
    return probs


def test_curve_block_fractions_and_means():
    probs = planted_probs()
    acc = np.concatenate([probs.sum(axis=0), np.full((5, 1), 2.0)], axis=1)
    w = [0.0, 0.25, 0.5, 0.75, 1.0]
    blk = MM.curve_block(probs, acc, w, i_from=1, i_to=0)
    assert blk["monotone_fraction"] == 0.5
    assert blk["switch_fraction"] == 0.5           # path 1 ends at class 2 (0.5 against 0.4 and 0.1)
    np.testing.assert_allclose(np.array(blk["p_mean"]), probs.mean(axis=0), rtol=0, atol=1e-15)
    # mean curves: to = (.1, .35, .4, .525, .65), from = (.9, .65, .5, .25, .1): the difference -.1 at step 2, +.275 at step 3
    assert abs(blk["crossover"] - (0.5 + 0.25 * 0.1 / 0.375)) <= 1e-12


def test_distance_block_straightness_and_ppl():
    steps = 4
    a, b = np.array([1.0, -2.0, 0.5]), np.array([3.0, 1.0, -1.5])
    line = np.stack([a + (b - a) * s / steps for s in range(steps + 1)])           # uniform, collinear
    bent = line.copy()
    bent[2] += np.array([0.0, 0.0, 2.0])
    still = np.repeat(a[None], steps + 1, axis=0)
    x = np.concatenate([line, bent, still]).astype(np.float32)
    d2 = MM.host_path_d2(x, 3, steps + 1)
    assert d2.shape == (3, steps + 1) and np.all(d2[2] == 0.0)
    end2 = float(((b - a) ** 2).sum())
    assert abs(d2[0, steps] - end2) <= 1e-12 * end2 and abs(d2[1, steps] - end2) <= 1e-12 * end2
    blk = MM.distance_block(d2[:1], steps)
    assert abs(blk["straightness"] - 1.0) <= 1e-12
    assert abs(blk["ppl"] - end2) <= 1e-12 * end2                                   # uniform path: ppl = endpoint distance squared
    assert abs(blk["path_length"] - end2 ** 0.5) <= 1e-12 and abs(blk["endpoint_distance"] - end2 ** 0.5) <= 1e-12
    assert MM.distance_block(d2[1:2], steps)["straightness"] < 0.9
    assert MM.distance_block(d2[2:], steps)["straightness"] is None                 # no path of positive length
    both = MM.distance_block(d2[[0, 2]], steps)                                     # averaged over the positive ones only
    assert abs(both["straightness"] - 1.0) <= 1e-12 and abs(both["path_length"] - 0.5 * end2 ** 0.5) <= 1e-12
    one = MM.host_path_d2(x[:1], 1, 1)                                              # S1 = 1: the endpoint entry is 0
    assert one.shape == (1, 1) and one[0, 0] == 0.0


def test_host_path_probs_groups_and_counts():
    rng = np.random.default_rng(0)
    P, S1, K, G = 5, 3, 4, 3
    logits = rng.normal(size=(P * S1, K)).astype(np.float32) * 3
    group = np.array([0, 2, -1, 0, 2], np.int32)                                   # group 1 is empty, path 2 is skipped
    probs, acc = MM.host_path_probs(logits, group, S1, G)
    ref = torch.softmax(torch.from_numpy(logits).double(), 1).numpy()
    np.testing.assert_allclose(probs, ref, rtol=0, atol=1e-15)
    assert np.all(acc[1] == 0.0) and np.all(acc[0, :, K] == 2.0) and np.all(acc[2, :, K] == 2.0)
    p3 = probs.reshape(P, S1, K)
    np.testing.assert_allclose(acc[0, :, :K], p3[0] + p3[3], rtol=0, atol=1e-15)


def test_pair_report_blocks():
    probs = planted_probs()
    acc = np.concatenate([probs.sum(axis=0), np.full((5, 1), 2.0)], axis=1)[None]
    roll = np.ones((2, 5))
    rep = MM.pair_report(MM.PathStats(probs, acc, None, roll), 0, [0, 1], [0.0, 0.25, 0.5, 0.75, 1.0], 1, 0)
    assert rep["feature"] is None and rep["roll"]["ppl"] == 16.0 and rep["roll"]["path_length"] == 4.0
    assert set(rep) == {"w", "p_mean", "crossover", "monotone_fraction", "switch_fraction", "feature", "roll"}
    none = MM.pair_report(MM.PathStats(None, None, None, roll), 0, [0, 1], [0.0, 0.25, 0.5, 0.75, 1.0], 1, 0)
    assert none["p_mean"] is None and none["crossover"] is None and none["roll"]["straightness"] == 0.25


def test_entry_points_reject_bad_arguments_before_any_launch():
    from melo_gan_amd import _lib
    lib = _lib.load()
    q = 256                     # non-null dummy addresses: nothing here launches
    mix = lambda rows=4, nd=128, md=6, ne=4, lat=q, ld=64, w=q: lib.mg_gen_inputs_mix(  # noqa: E731
        w, q, q, q, rows, q, nd, q, md, q, ne, 0.15, lat, ld, 1, None)
    assert mix(w=None) == -1 and b"null" in lib.mg_last_error()
    for kw in (dict(rows=0), dict(nd=0), dict(md=0), dict(ne=0), dict(ne=33), dict(ld=-1), dict(lat=None)):
        assert mix(**kw) == -1 and b"mg_gen_inputs_mix" in lib.mg_last_error(), kw
    assert lib.mg_path_d2(None, 1, 1, 1, q, None) == -1 and b"null" in lib.mg_last_error()
    for P, S1, D in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (1 << 20, 1 << 12, 4)):
        assert lib.mg_path_d2(q, P, S1, D, q, None) == -1 and b"mg_path_d2" in lib.mg_last_error(), (P, S1, D)
    assert lib.mg_path_d2(q + 2, 2, 2, 4, q, None) == -1                            # a misaligned x
    assert lib.mg_path_probs(q, None, 2, 2, 4, 1, q, q, None) == -1 and b"null" in lib.mg_last_error()
    for P, S1, K, G in ((0, 2, 4, 1), (2, 0, 4, 1), (2, 2, 1, 1), (2, 2, 33, 1), (2, 2, 4, 0)):
        assert lib.mg_path_probs(q, q, P, S1, K, G, q, q, None) == -1 and b"mg_path_probs" in lib.mg_last_error(), (P, S1, K, G)


def test_ops_refuse_cpu_tensors_and_wrong_shapes():
    from melo_gan_amd import ops
    z = torch.zeros
    i2 = z(4, 2, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.gen_inputs_mix(z(4, 4), i2, i2, z(4), z(4, 128), z(4, 6), z(4, 6), 0.15, None, 1)
    with pytest.raises(ValueError):
        ops.path_d2(z(6, 8), 2, 3)
    with pytest.raises(ValueError):
        ops.path_probs(z(6, 4), z(2, dtype=torch.int32), 3, 1)


ARGS = ["--config", os.path.join(ROOT, "config", "gan_config.yaml")]


@pytest.mark.parametrize("argv,word", [
    ([], "exactly one"),
    (["--from", "happy"], "go together"),
    (["--from", "happy", "--to", "happy"], "two emotions"),
    (["--from", "happy", "--to", "glad"], "--to"),
    (["--pairs", "some"], "--pairs"),
    (["--pairs", "all", "--weights", "happy=1"], "exactly one"),
    (["--weights", "happy=-1,calm=2"], "--weights"),
    (["--weights", "happy=0"], "--weights"),
    (["--weights", "happy=1,happy=2"], "twice"),
    (["--weights", "glad=1"], "--weights"),
    (["--weights", "happy=x"], "not a number"),
    (["--weights", "happy=1", "--join"], "--join"),
    (["--pairs", "all", "--steps", "0"], "--steps"),
    (["--pairs", "all", "--samples", "0"], "--samples"),
    (["--pairs", "all", "--noise", "lerp"], "--noise"),
    (["--pairs", "all", "--batch", "0"], "--batch"),
    (["--pairs", "all", "--no-files", "--join"], "--no-files"),
    (["--pairs", "all", "--join", "--join-notes", "0"], "--join-notes"),
    (["--pairs", "all", "--ckpt", "/nonexistent/gan.pth"], "does not exist"),
    (["--pairs", "all", "--config", "/nonexistent/gan.yaml"], "does not exist"),
    (["--pairs", "all", "--ed_ckpt", "x.pth"], "--ed_config"),
])
def test_cli_host_checks_return_status_2(argv, word, capsys):
    assert M.main(ARGS + argv) == 2
    err = capsys.readouterr().err
    assert err.startswith("morph: error:") and word in err, err


def test_cli_exits_with_status_2():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "melo_gan_amd.gan.morph", *ARGS, "--from", "sad", "--to", "sad"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and r.stderr.strip().splitlines()[-1].startswith("morph: error:"), (r.stdout, r.stderr)


def test_rows_of_pairs_and_blends():
    rows = M.pair_rows([(1, 0), (2, 3)], steps=4, samples=2, noise="slerp")
    assert (rows.P, rows.S1, rows.G) == (4, 5, 2) and rows.group.tolist() == [0, 0, 1, 1]
    assert rows.paths == [(1, 0, 1), (1, 0, 2), (2, 3, 1), (2, 3, 2)]
    r = 1 * 5 + 3                                                                   # path (sad -> happy, k = 2), step 3
    assert rows.weights[r].tolist() == [0.75, 0.25, 0.0, 0.0] and rows.t[r] == 0.75
    assert rows.key_a[r].tolist() == [1, 2] and rows.key_b[r].tolist() == [0, 2]
    assert rows.weights[5].tolist() == [0.0, 1.0, 0.0, 0.0] and rows.weights[9].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert np.all(M.pair_rows([(1, 0)], 4, 1, "fixed").t == 0.0)
    b = M.blend_rows([0.7, 0.0, 0.0, 0.3], 3)
    assert (b.P, b.S1, b.G) == (3, 1, 1) and b.key_a.tolist() == [[0, 1], [0, 2], [0, 3]] and np.all(b.t == 0.0)
    assert M.parse_weights("happy=7, calm=3") == [0.7, 0.0, 0.0, 0.3]
    assert M.heaviest([0.5, 0.0, 0.5, 0.0]) == 0 and M.heaviest([0.1, 0.4, 0.1, 0.4]) == 1    # the lower index on a tie
    assert M.style_of([0.5, 0.5, 0.0, 0.0]) == ("major", 105) and M.style_of([0.0, 0.75, 0.25, 0.0]) == ("minor", round(0.75 * 70 + 40))


def test_join_offsets_against_a_sum_by_hand():
    # six rows; column 3 is the step: beats = max(0.1, (x + 1) / 2 * 4)
    step = [-1.0, -0.5, 0.0, 0.5, 1.0, -0.99]
    roll = np.zeros((6, 4), np.float32)
    roll[:, 3] = step
    beats = [0.1, 1.0, 2.0, 3.0, 4.0, 0.1]                                          # -0.99: 0.02 beats, below the floor
    for got, want in zip([max(0.1, ((float(np.float32(x)) + 1.0) / 2.0) * 4.0) for x in step], beats):
        assert abs(got - want) <= 1e-6
    off = MM.join_offsets([roll, roll, roll], [120, 60, 90], join_notes=4)
    first = 0.0
    for x in step[:4]:
        first += max(0.1, ((float(np.float32(x)) + 1.0) / 2.0) * 4.0) * 60.0 / 120
    second = first
    for x in step[:4]:
        second += max(0.1, ((float(np.float32(x)) + 1.0) / 2.0) * 4.0) * 60.0 / 60
    assert off == [0.0, first, second]
    assert abs(first - 6.1 * 0.5) <= 1e-6 and abs(second - (6.1 * 0.5 + 6.1)) <= 1e-6
    assert abs(MM.join_offsets([roll, roll], [120, 120], join_notes=64)[1] - 10.2 * 0.5) <= 1e-6        # all six rows
    # the joined note list: each step's notes at its offset
    roll[:, 1] = 0.5                                                                # every row sounds
    notes = M.joined_notes([roll, roll], [("major", 120), ("minor", 60)], 4)
    assert len(notes) == 8 and notes[0][2] == 0.0 and notes[4][2] == first
    from melo_gan_amd import midi
    own = midi.notes_from_roll(roll[:4], bpm=60, scale="minor", root_key=0)[0]
    assert [(v, p, s + first, e + first) for v, p, s, e in own] == notes[4:]
